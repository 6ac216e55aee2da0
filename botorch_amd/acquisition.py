"""Acquisition functions on the accelerated path (BoTorch-compatible API).

MC family: acquisition/monte_carlo.py:60-871 (SampleReducingMCAcquisitionFunction,
qExpectedImprovement, qNoisyExpectedImprovement, qProbabilityOfImprovement,
qSimpleRegret, qUpperConfidenceBound); multi-objective qEHVI:
acquisition/multi_objective/monte_carlo.py:146-322; analytic EI / PI / UCB:
acquisition/analytic.py.

For a SingleTaskGP with the identity objective and no constraints, ``forward``
runs the fused gfx950 path -- post_partials (K*x + R = K*x L^{-T} + R R^T on
the fp64 matrix cores) and qmc_finalize (q x q psd_safe_cholesky, Sobol
reparameterisation, q-max / sample-mean reduction) -- as one autograd node whose
backward is bo_qmc_backward + bo_post_backward.  Other objectives / models take
the generic route (device posterior -> sampler -> torch reduction).
"""
from __future__ import annotations

import copy
import math
import warnings
from typing import Callable, List, NamedTuple, Optional, Union

import torch
from torch import nn

from . import _lib, kernels
from .exceptions import (BotorchError, BotorchTensorDimensionError, BotorchWarning, NanError,
                         NotPSDError, UnsupportedError)
from .safe_math import (TAU_MAX, TAU_RELU, fatmax, log_improvement, logmeanexp, logplusexp,
                        smooth_amax)
from .objective import (ConstrainedMCObjective, GenericMCObjective, IdentityMCObjective,
                        LinearMCObjective, MCAcquisitionObjective, MCObjective,
                        compute_best_feasible_objective, compute_feasibility_indicator,
                        compute_smoothed_feasibility_indicator, repeat_to_match_aug_dim, _as_etas,
                        _linear_outcome_constraints)
from .models import prime_prediction_caches
from .posteriors import FUSED_QMAX
from .sampling import (ListSampler, MCSampler, ShapeOnlyPosterior, SobolQMCNormalSampler,
                       get_sampler)


# -- input handling (utils/transforms.py:146-336) -----------------------------
def t_batch_mode(X: torch.Tensor, expected_q: Optional[int] = None) -> torch.Tensor:
    if X.dim() == 2:
        X = X.unsqueeze(0)
    if expected_q is not None and X.shape[-2] != expected_q:
        raise AssertionError(f"Expected X to be `batch_shape x q={expected_q} x d`, but got X with shape {tuple(X.shape)}.")
    return X


def _cache_dim_ok(model, X: torch.Tensor) -> bool:
    """A MultiTaskGP's prediction cache is the task view of its one output task
    over the d non-task columns: X that carries the task column (d + 1 columns)
    keeps the generic route, which goes through ``model.posterior``."""
    return not model.__dict__.get("_is_multitask") or X.shape[-1] == model._d


class AcquisitionFunction(nn.Module):
    """acquisition/acquisition.py:33-74."""

    # whether the class's routes have been audited for a MultiTaskGP (its task view
    # carries no Cholesky factor and its caches are those of one output task)
    _admits_multitask = False

    def __init__(self, model):
        super().__init__()
        if getattr(model, "_is_multitask", False) and not self._admits_multitask:
            raise UnsupportedError(
                f"{type(self).__name__}: MultiTaskGP is not on the accelerated path of this "
                "acquisition function (admitted: qExpectedImprovement, qLogExpectedImprovement, "
                "qNoisyExpectedImprovement, qLogNoisyExpectedImprovement, qUpperConfidenceBound, "
                "ExpectedImprovement, LogExpectedImprovement, UpperConfidenceBound, "
                "PosteriorMean)")
        self.model = model
        self.X_pending = None

    def set_X_pending(self, X_pending: Optional[torch.Tensor] = None) -> None:
        if X_pending is not None:
            if X_pending.requires_grad:
                warnings.warn("Pending points require a gradient but the acquisition function"
                              " will not provide a gradient to these points.", BotorchWarning)
            self.X_pending = X_pending.detach().clone()
        else:
            self.X_pending = X_pending

    def _concat_pending(self, X: torch.Tensor) -> torch.Tensor:
        """utils/transforms.py:312-336."""
        if self.X_pending is not None:
            Xp = self.X_pending.to(X).expand(*X.shape[:-2], *self.X_pending.shape[-2:])
            X = torch.cat([X, Xp], dim=-2)
        return X


class MCAcquisitionFunction(AcquisitionFunction):
    """acquisition/acquisition.py:77-146 + SampleReducingMCAcquisitionFunction
    (acquisition/monte_carlo.py:155-330): samples -> objective -> per-sample
    utility -> constraint weighting -> q reduction -> sample reduction.

    Subclasses run a fused gfx950 kernel chain when the configuration allows
    (``_fused_eligible``) and otherwise this generic route, whose posterior,
    root decomposition and base samples are still the device kernels."""

    _default_sample_shape = torch.Size([512])
    _log = False

    def __init__(self, model, sampler: Optional[MCSampler] = None, objective=None,
                 posterior_transform=None, X_pending=None, constraints=None, eta=1e-3,
                 fat: bool = False):
        super().__init__(model)
        if constraints is not None and isinstance(objective, ConstrainedMCObjective):
            raise ValueError("ConstrainedMCObjective as well as constraints passed to constructor."
                             "Choose one or the other, preferably the latter.")
        if objective is None and model.num_outputs != 1 and posterior_transform is None:
            raise UnsupportedError("Must specify an objective or a posterior transform when "
                                   "using a multi-output model.")
        self.sampler = sampler
        self.objective = objective if objective is not None else IdentityMCObjective()
        self.posterior_transform = posterior_transform
        self._constraints = constraints
        self._eta = eta
        self._fat = fat
        self.set_X_pending(X_pending)

    @property
    def sample_shape(self) -> torch.Size:
        return self.sampler.sample_shape if self.sampler is not None else self._default_sample_shape

    def _ensure_sampler(self, posterior=None):
        if self.sampler is None:
            self.sampler = get_sampler(posterior, sample_shape=self._default_sample_shape)
        return self.sampler

    def get_posterior_samples(self, posterior):
        """acquisition/acquisition.py:109-146."""
        return self._ensure_sampler(posterior)(posterior)

    def _fused_eligible(self, X: torch.Tensor) -> bool:
        m = self.model
        return (hasattr(m, "prediction_cache") and type(self.objective) is IdentityMCObjective
                and self.posterior_transform is None and self._constraints is None
                and X.shape[-2] <= FUSED_QMAX and X.shape[-1] <= kernels.DP and X.is_cuda
                and len(self.sample_shape) == 1 and _cache_dim_ok(m, X))

    # -- generic route (monte_carlo.py:253-330) -----------------------------------------
    def _sample_forward(self, obj: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def _q_reduction(self, acqval: torch.Tensor) -> torch.Tensor:
        return acqval.amax(dim=-1)

    def _sample_reduction(self, acqval: torch.Tensor) -> torch.Tensor:
        return acqval.mean(dim=tuple(range(len(self.sample_shape))))

    def _apply_constraints(self, acqval: torch.Tensor, samples: torch.Tensor) -> torch.Tensor:
        """monte_carlo.py:305-330: weight (or, in log space, shift) the utility by
        the smoothed feasibility indicator."""
        if self._constraints is not None:
            if not self._log and (acqval < 0).any():
                raise ValueError("Constraint-weighting requires unconstrained "
                                 "acquisition values to be non-negative.")
            ind = compute_smoothed_feasibility_indicator(constraints=self._constraints,
                                                         samples=samples, eta=self._eta,
                                                         log=self._log, fat=self._fat)
            acqval = acqval.add(ind) if self._log else acqval.mul(ind)
        return acqval

    def _get_samples_and_objectives(self, X: torch.Tensor):
        posterior = self.model.posterior(X, posterior_transform=self.posterior_transform)
        samples = self.get_posterior_samples(posterior)
        return samples, self.objective(samples, X=X)

    def _generic_forward(self, X: torch.Tensor) -> torch.Tensor:
        samples, obj = self._get_samples_and_objectives(X)
        samples = repeat_to_match_aug_dim(target_tensor=samples, reference_tensor=obj)
        acqval = self._apply_constraints(self._sample_forward(obj), samples)
        return _ensemble_mean(self.model, self._sample_reduction(self._q_reduction(acqval)))


def _fused_mc(X3: torch.Tensor, acqf, mode: int, best_f: float, best_f_s, Z: torch.Tensor,
              tau: Optional[float] = None):
    """qEI / qLogEI / qSR / qPI / qUCB value of B t-batches on the gfx950 fused
    path through bo::qmc_acq (one torch.ops call; its registered backward gives
    dX).  The jitter-ladder status is read at the end of the backward when a
    gradient follows, else one call later (kernels.raise_not_psd_deferred).
    The modes' parameters ride in the existing slots (include/botorch_amd.h):
    qPI's ``tau`` in tau_relu, qUCB's beta' in ``best_f`` and the base samples'
    mean in ``best_f_s``."""
    from . import ops  # torch.ops.bo registration, QmcAcqGrad
    model = acqf.model
    cache = model.prediction_cache()
    ymean, ystd = model.outcome_stats()
    need_grad = torch.is_grad_enabled() and X3.requires_grad
    lp = getattr(acqf, "_log_params", None)
    fat, tau_relu, tau_max = lp if lp is not None else (True, 1.0, 1.0)
    if tau is not None:
        tau_relu = tau
    dev = X3.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if X3.dtype != torch.float64:  # the model computes in fp64; the value returns in X's dtype
        return _fused_mc(X3.to(torch.float64), acqf, mode, best_f, best_f_s, Z, tau).to(X3.dtype)
    cap = kernels._CAPTURE_STATUS.get(idx) if idx in kernels._CAPTURE else None
    if not need_grad and not kernels.SYNC_LADDER and (idx not in kernels._CAPTURE or cap):
        # eager forward-only: ONE native call issues the whole chain and defers
        # the ladder status (the previous call's is returned and acted on here);
        # under a graph capture the same call, its status folded into the
        # graph's pinned words by the finalisation kernel itself
        acq, prev = _lib.torch_ops().qmc_acq_eager(
            X3.contiguous(), cache.Xt_scaled, cache.U, cache.beta, cache.lengthscale,
            Z, best_f_s, int(cache.kind), int(mode), int(cache.n), float(cache.outputscale),
            float(cache.constant), float(ymean), float(ystd), float(best_f), bool(fat),
            float(tau_relu), float(tau_max), kernels.kxt_cap(dev),
            kernels.quad_ainv(cache, X3.shape[0], X3.shape[1]), cache.alpha,
            cap[0] if cap else None, cap[1] if cap else None)
        if cap:
            kernels.record_capture_status(idx, None, type(acqf).__name__)
        else:
            kernels.ladder_prev_outcome(prev, idx, type(acqf).__name__)
        return acq
    if need_grad:  # the registered op's semantics without its autograd wrapper
        acq, jit, info = ops.QmcAcqGrad.apply(
            X3, cache.Xt, cache.Xt_scaled, cache.U, cache.Linv, cache.beta, cache.alpha,
            cache.lengthscale, Z, best_f_s, int(cache.kind), int(mode), float(cache.outputscale),
            float(cache.constant), float(ymean), float(ystd), float(best_f), bool(fat),
            float(tau_relu), float(tau_max))
    else:
        outs = torch.ops.bo.qmc_acq(
            X3, cache.Xt, cache.Xt_scaled, cache.U, cache.Linv, cache.beta, cache.alpha,
            cache.lengthscale, Z, best_f_s, int(cache.kind), int(mode), float(cache.outputscale),
            float(cache.constant), float(ymean), float(ystd), float(best_f), bool(fat),
            float(tau_relu), float(tau_max), False,
            kernels.quad_ainv(cache, X3.shape[0], X3.shape[1]))
        acq, jit, info = outs[0], outs[6], outs[7]
    # deferred either way: with a gradient the status is read at the end of the
    # registered backward (ops._acq_bwd), once the backward's launches are
    # queued behind the forward -- so the evaluation that produced a failed
    # root raises NotPSDError (as gen.py's closure sees the reference's) but
    # the device does not drain between the forward and the backward
    kernels.raise_not_psd_deferred(info, jit, type(acqf).__name__)
    return acq

def _host_scalar(module, name: str) -> float:
    """float(module.<name>) read once per value: a best_f on the device (the
    usual ``best_f=train_Y.max()``) would otherwise be a device-to-host read,
    i.e. a stream drain, in every forward.  The cache holds the tensor itself
    (so a replacement can never reuse its identity) and its version counter:
    a new tensor or an in-place change is read again."""
    t = getattr(module, name)
    cache = module.__dict__.setdefault("_host_scalars", {})
    hit = cache.get(name)
    if hit is None or hit[0] is not t or hit[1] != t._version:
        hit = (t, t._version, float(t))
        cache[name] = hit
    return hit[2]


def _ensemble_mean(model, acq: torch.Tensor) -> torch.Tensor:
    """Average over the MCMC batch of ensemble models (utils/transforms.py:289-293)."""
    return acq.mean(dim=-1) if getattr(model, "_is_ensemble", False) else acq


class qExpectedImprovement(MCAcquisitionFunction):
    """MC batch EI (acquisition/monte_carlo.py:332-414):
    qEI(X) = E[max_j max(Y_j - best_f, 0)], optionally weighted by smoothed
    outcome constraints (``constraints``, ``eta``)."""

    _admits_multitask = True

    def __init__(self, model, best_f: Union[float, torch.Tensor], sampler=None, objective=None,
                 posterior_transform=None, X_pending=None, constraints=None, eta=1e-3):
        super().__init__(model, sampler, objective, posterior_transform, X_pending,
                         constraints=constraints, eta=eta)
        self.register_buffer("best_f", torch.as_tensor(best_f, dtype=torch.float64))

    def _sample_forward(self, obj: torch.Tensor) -> torch.Tensor:
        """monte_carlo.py:405-414."""
        return (obj - self.best_f.unsqueeze(-1).to(obj)).clamp_min(0)

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = self._concat_pending(t_batch_mode(X))
        batch = X.shape[:-2]
        q, d = X.shape[-2], X.shape[-1]
        X3 = X.reshape(-1, q, d)
        if self._fused_eligible(X) and self.best_f.numel() == 1:
            sampler = self._ensure_sampler()
            Z = sampler.base_samples_2d(q, X.device)
            acq = _fused_mc(X3, self, _lib.QMC_QEI, _host_scalar(self, "best_f"), None, Z)
            return acq.reshape(batch)
        if (getattr(self.model, "_is_fully_bayesian", False) and X.is_cuda and not self._log
                and type(self.objective) is IdentityMCObjective and self.posterior_transform is None
                and self._constraints is None and len(self.sample_shape) == 1
                and self.best_f.numel() == 1 and q <= FUSED_QMAX):
            sampler = self._ensure_sampler()
            Z = sampler.base_samples_2d(q, X.device)
            return _SaasQEI.apply(X3, self, _host_scalar(self, "best_f"), Z).reshape(batch)
        if self._constraints is not None:  # outcome constraints: the weighted fused route
            acq = _weighted_qei_forward(self, X)
            if acq is not None:
                return acq
        return self._generic_forward(X)


class _SaasQEI(torch.autograd.Function):
    """qEI over the MCMC ensemble of a SAAS model (models/fully_bayesian.py:509-546,
    averaged over MCMC_DIM as utils/transforms.py:289-293), any d <= 128, with
    all M members batched into each launch.

    Forward: K*x of every member (one bo_covar_batched, Matern-5/2 x outputscale),
    R = K*x L_m^{-T} and the means (batched MFMA GEMMs over M), the R R^T blocks
    (batched over M x B), K** (one bo_covar_batched over M x B), the jittered
    q x q roots (bo_chol_small over M x B), reparameterised samples (one batched
    GEMM) and the qEI reduction (bo_mc_reduce over M x B), averaged over M.
    Backward: bo_qmc_backward over M x B -> d mu, d Sigma; d K*x = d mu alpha^T
    - G W (W = R L^{-1}, batched GEMMs); bo_kernel_grad per member for K*x and K**."""

    @staticmethod
    def forward(ctx, X3, acqf, best_f, Z):
        model = acqf.model
        B, q, d = X3.shape
        dev = X3.device
        X2 = X3.detach().reshape(B * q, d).contiguous()
        need_grad = ctx.needs_input_grad[0]
        ym, ys = model.outcome_stats()
        ens = model.ensemble_cache()
        M, n = ens["U"].shape[0], ens["n"]
        f64 = dict(dtype=torch.float64, device=dev)
        Bq = B * q
        Kx = torch.empty(M, Bq, n, **f64)
        kernels.covar_batched(ens["kind"], X2, (0, 0), Bq, ens["Xt"], (0, 0), n, d, ens["ls"],
                              (d, 0), ens["os"], (1, 0), Kx, (Bq * n, 0), n, M, 1)
        R = kernels.gemm(Kx, ens["U"], flags=_lib.GEMM_B_UPPER)              # M x Bq x n
        mean = kernels.gemm(Kx, ens["alpha"].unsqueeze(-1)).reshape(M, B, q)
        RR = kernels.gemm(R.view(M * B, q, n), R.view(M * B, q, n), transB=True)  # MB x q x q
        Kxx = torch.empty(M * B, q, q, **f64)
        kernels.covar_batched(ens["kind"], X2, (0, q * d), q, X2, (0, q * d), q, d, ens["ls"],
                              (d, 0), ens["os"], (1, 0), Kxx, (B * q * q, q * q), q, M, B)
        cov = (Kxx - RR) * (ys * ys)
        mean = ym + ys * (mean + ens["const"].view(M, 1, 1))
        L = kernels.chol_jitter(cov)                                          # MB x q x q
        f = kernels.sample_mvn(mean.reshape(M * B, q), L, Z)                  # S x MB x q
        acq = kernels.mc_reduce(f, best_f).view(M, B).mean(dim=0)
        if need_grad:
            ctx.ens, ctx.X2, ctx.Z, ctx.best_f, ctx.shape, ctx.ys = ens, X2, Z, best_f, (B, q, d), ys
            ctx.R, ctx.mean, ctx.L = R, mean.reshape(M * B, q), L
        return acq

    @staticmethod
    def backward(ctx, dacq):
        B, q, d = ctx.shape
        ens, ys = ctx.ens, ctx.ys
        M, n = ens["U"].shape[0], ens["n"]
        da = (dacq / M).repeat(M).contiguous()                                # MB
        dmean, dcov = kernels.qmc_backward(_lib.QMC_QEI, ctx.mean, ctx.L, ctx.Z, da, ctx.best_f)
        dmu = (ys * dmean).reshape(M, B * q)                                  # standardized
        G = ((ys * ys) * (dcov + dcov.mT)).contiguous()                       # MB x q x q
        W = kernels.gemm(ctx.R, ens["U"], transB=True, flags=_lib.GEMM_B_LOWER)  # M x Bq x n
        dK = (dmu.unsqueeze(-1) * ens["alpha"].unsqueeze(1)).contiguous()    # M x Bq x n
        kernels.gemm(G, W.view(M * B, q, n), alpha=-1.0, beta=1.0, C=dK.view(M * B, q, n))
        Gm = G.view(M, B * q, q)
        dX = None
        for mi in range(M):
            ls = ens["ls"][mi]
            os_ = ens["os_host"][mi]
            dX = kernels.kernel_grad(ctx.X2, ens["Xt"], dK[mi], ls, ens["kind"], os_, dX=dX)
            dX = kernels.kernel_grad(ctx.X2, ctx.X2, Gm[mi].contiguous(), ls, ens["kind"], os_,
                                     group=q, dX=dX)
        return dX.reshape(B, q, d), None, None, None


class _PlainMaxMCAcquisitionFunction(MCAcquisitionFunction):
    """The sample-reducing acquisitions without a relu (qSR, qPI, qUCB): qEI's
    forward shape -- the fused kernels under ``_fused_eligible`` (mode
    ``_fused_mode`` with the parameters of ``_fused_params``), else the generic
    route through ``_sample_forward``."""

    _fused_mode: int

    def _fused_ok(self, X: torch.Tensor) -> bool:
        return self._fused_eligible(X)

    def _fused_params(self, q: int, device):
        """(best_f slot, best_f_s slot, tau) as host floats / a device tensor."""
        return 0.0, None, None

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = self._concat_pending(t_batch_mode(X))
        if self._fused_ok(X):
            batch, q = X.shape[:-2], X.shape[-2]
            Z = self._ensure_sampler().base_samples_2d(q, X.device)
            best_f, best_f_s, tau = self._fused_params(q, X.device)
            acq = _fused_mc(X.reshape(-1, q, X.shape[-1]), self, self._fused_mode, best_f, best_f_s,
                            Z, tau)
            return acq.reshape(batch)
        return self._generic_forward(X)


class qProbabilityOfImprovement(_PlainMaxMCAcquisitionFunction):
    """MC batch PI (acquisition/monte_carlo.py:648-731): the indicator of
    improvement smoothed by a sigmoid at temperature ``tau``,
    qPI(X) = E[max_j sigmoid((Y_j - best_f) / tau)]."""

    _fused_mode = _lib.QMC_QPI

    def __init__(self, model, best_f: Union[float, torch.Tensor], sampler=None, objective=None,
                 posterior_transform=None, X_pending=None, tau: float = 1e-3, constraints=None,
                 eta=1e-3):
        super().__init__(model, sampler, objective, posterior_transform, X_pending,
                         constraints=constraints, eta=eta)
        self.register_buffer("best_f", torch.as_tensor(best_f, dtype=torch.float64).unsqueeze(-1))
        self.register_buffer("tau", torch.as_tensor(tau, dtype=torch.float64))

    def _sample_forward(self, obj: torch.Tensor) -> torch.Tensor:
        """monte_carlo.py:721-731."""
        return torch.sigmoid((obj - self.best_f.to(obj)) / self.tau.to(obj))

    def _fused_ok(self, X: torch.Tensor) -> bool:
        return self._fused_eligible(X) and self.best_f.numel() == 1

    def _fused_params(self, q: int, device):
        return _host_scalar(self, "best_f"), None, _host_scalar(self, "tau")


class qSimpleRegret(_PlainMaxMCAcquisitionFunction):
    """MC batch simple regret (acquisition/monte_carlo.py:734-798):
    qSR(X) = E[max_j Y_j].  Values may be negative, so there is no
    ``constraints`` argument (use a ConstrainedMCObjective)."""

    _fused_mode = _lib.QMC_QSR

    def __init__(self, model, sampler=None, objective=None, posterior_transform=None,
                 X_pending=None):
        super().__init__(model, sampler, objective, posterior_transform, X_pending)

    def _sample_forward(self, obj: torch.Tensor) -> torch.Tensor:
        """monte_carlo.py:789-798."""
        return obj


class qUpperConfidenceBound(_PlainMaxMCAcquisitionFunction):
    """MC batch UCB (acquisition/monte_carlo.py:801-871, [Wilson2017reparam]
    appendix A): qUCB(X) = E[max_j (mu_j + beta' |Y_j - mu_j|)] with
    beta' = sqrt(beta pi / 2) and mu the mean of the samples (not of the
    posterior), as the reference computes it."""

    _admits_multitask = True

    _fused_mode = _lib.QMC_QUCB

    def __init__(self, model, beta: float, sampler=None, objective=None, posterior_transform=None,
                 X_pending=None):
        super().__init__(model, sampler, objective, posterior_transform, X_pending)
        self.beta_prime = math.sqrt(beta * math.pi / 2)

    def _sample_forward(self, obj: torch.Tensor) -> torch.Tensor:
        """monte_carlo.py:861-871."""
        mean = obj.mean(dim=0)
        return mean + self.beta_prime * (obj - mean).abs()

    def _fused_params(self, q: int, device):
        # mean_s f = mu' + L_q zbar: the base samples' mean, kept with them
        return self.beta_prime, self._ensure_sampler().base_sample_mean_2d(q, device), None


# -- analytic ------------------------------------------------------------------------
_INV_SQRT_2PI = 1 / math.sqrt(2 * math.pi)  # utils/probability/utils.py:27-29
_NEG_INV_SQRT_2 = -(1 / math.sqrt(2))


def _ndtr(x):
    """Standard normal CDF (utils/probability/utils.py:133-136)."""
    return 0.5 * torch.erfc(_NEG_INV_SQRT_2 * x)


def _phi(x):
    """Standard normal PDF (utils/probability/utils.py:139-142)."""
    return _INV_SQRT_2PI * (-0.5 * x.square()).exp()


class AnalyticAcquisitionFunction(AcquisitionFunction):
    def __init__(self, model, posterior_transform=None):
        super().__init__(model)
        self.posterior_transform = posterior_transform

    def set_X_pending(self, X_pending=None) -> None:
        """acquisition/analytic.py:78-82."""
        raise UnsupportedError("Analytic acquisition functions do not account for X_pending yet.")

    def _mean_and_sigma(self, X, compute_sigma=True, min_var=1e-12):
        """acquisition/analytic.py:84-108."""
        posterior = self.model.posterior(X, posterior_transform=self.posterior_transform)
        mean = posterior.mean.squeeze(-2).squeeze(-1)
        if not compute_sigma:
            return mean, None
        sigma = posterior.variance.clamp_min(min_var).sqrt().view(mean.shape)
        return mean, sigma


class ExpectedImprovement(AnalyticAcquisitionFunction):
    """acquisition/analytic.py:298-354: sigma (phi(u) + u Phi(u)), u = (mu - best_f)/sigma."""

    _admits_multitask = True

    def __init__(self, model, best_f, posterior_transform=None, maximize=True):
        super().__init__(model, posterior_transform)
        self.register_buffer("best_f", torch.as_tensor(best_f, dtype=torch.float64))
        self.maximize = maximize

    def forward(self, X):
        X = t_batch_mode(X, expected_q=1)
        mean, sigma = self._mean_and_sigma(X)
        u = (mean - self.best_f.to(mean)) / sigma
        if not self.maximize:
            u = -u
        return sigma * (_phi(u) + u * _ndtr(u))


class ProbabilityOfImprovement(AnalyticAcquisitionFunction):
    """acquisition/analytic.py (PI): Phi((mu - best_f)/sigma)."""

    def __init__(self, model, best_f, posterior_transform=None, maximize=True):
        super().__init__(model, posterior_transform)
        self.register_buffer("best_f", torch.as_tensor(best_f, dtype=torch.float64))
        self.maximize = maximize

    def forward(self, X):
        X = t_batch_mode(X, expected_q=1)
        mean, sigma = self._mean_and_sigma(X)
        u = (mean - self.best_f.to(mean)) / sigma
        return _ndtr(u if self.maximize else -u)


class UpperConfidenceBound(AnalyticAcquisitionFunction):
    """acquisition/analytic.py (UCB): mu + sqrt(beta) sigma."""

    _admits_multitask = True

    def __init__(self, model, beta, posterior_transform=None, maximize=True):
        super().__init__(model, posterior_transform)
        self.register_buffer("beta", torch.as_tensor(beta, dtype=torch.float64))
        self.maximize = maximize

    def forward(self, X):
        X = t_batch_mode(X, expected_q=1)
        mean, sigma = self._mean_and_sigma(X)
        return (mean if self.maximize else -mean) + self.beta.to(mean).sqrt() * sigma


class PosteriorMean(AnalyticAcquisitionFunction):
    """acquisition/analytic.py (PosteriorMean): mu, or -mu with ``maximize=False``."""

    _admits_multitask = True

    def __init__(self, model, posterior_transform=None, maximize=True):
        super().__init__(model, posterior_transform)
        self.maximize = maximize

    def forward(self, X):
        X = t_batch_mode(X, expected_q=1)
        mean, _ = self._mean_and_sigma(X, compute_sigma=False)
        return mean if self.maximize else -mean


# -- analytic, log forms and outcome constraints: one fused chain on the moments ------------
def _exact_members(model) -> Optional[list]:
    """The single-output exact GPs behind ``model`` -- itself, the outputs of a
    multi-output SingleTaskGP, or a ModelListGP's members -- or None where the
    model is anything else (the generic route then)."""
    from .models import ModelListGP, SingleTaskGP
    if isinstance(model, ModelListGP) or (isinstance(model, SingleTaskGP)
                                          and model._is_multi_output):
        members = list(model.models)
    else:
        members = [model]
    if all(isinstance(mm, SingleTaskGP) and not mm._is_multi_output for mm in members):
        return members
    if getattr(model, "_is_multitask", False) and model.num_outputs == 1:
        return members  # its prediction cache is the one output task's view
    return None


class _MomentChainAcquisition(AnalyticAcquisitionFunction):
    """The analytic q = 1 acquisitions that are a chain on the posterior mean
    and variance (LogEI, LogPI, the posterior standard deviation and the
    constrained (Log)EI).  ``forward`` takes one of two routes:

    fused: the moments of the members the value reads, from
    ``posteriors.posterior_moments`` (differentiable), stacked ``Mt x R`` into
    ``bo::analytic`` -- one launch forward, one backward, instead of the 40 to 60
    small launches of the torch chain each way;

    generic: the reference's formula with the ``safe_math`` functions on
    ``model.posterior`` (any model, any device, posterior transforms).

    ``_route``: None (by ``_fused_applies``), "fused" or "generic" (tests, tools)."""

    _an_mode: int = -1

    def __init__(self, model, posterior_transform=None, check_outputs: bool = True):
        super().__init__(model, posterior_transform)
        if check_outputs and posterior_transform is None and model.num_outputs != 1:
            raise UnsupportedError("Must specify a posterior transform when using a "
                                   "multi-output model.")
        self._route = None

    # what the kernel reads: the members' indices in the model (the objective
    # first) and the constraint table over their positions
    def _an_members(self) -> List[int]:
        return [0]

    def _an_constraints(self) -> list:
        return []

    def _fused_applies(self, X3: torch.Tensor) -> bool:
        if not X3.is_cuda or self.posterior_transform is not None:
            return False
        members = _exact_members(self.model)
        if members is None:
            return False
        idx = self._an_members()
        return (len(idx) <= kernels.AN_MT_MAX and len(self._an_constraints()) <= kernels.AN_CMAX
                and max(idx) < len(members) and _cache_dim_ok(self.model, X3))

    def _best_f_rows(self, batch: torch.Size, like: torch.Tensor) -> Optional[torch.Tensor]:
        best_f = getattr(self, "best_f", None)
        if best_f is None:
            return None
        best_f = best_f.to(like)
        if best_f.numel() == 1:
            return best_f.reshape(1)
        return torch.broadcast_to(best_f, batch).reshape(-1)

    def _fused(self, X3: torch.Tensor, batch: torch.Size) -> torch.Tensor:
        from . import ops  # noqa: F401  (torch.ops.bo registration)
        from .posteriors import posterior_moments
        members = _exact_members(self.model)
        if members is None:
            raise UnsupportedError(f"{type(self).__name__}: the fused route needs an exact GP "
                                   "(SingleTaskGP or a ModelListGP of them)")
        picked = [members[i] for i in self._an_members()]
        for mm in picked:
            if mm.training:
                mm.eval()
        prime_prediction_caches(picked)
        means, variances = [], []
        for mm in picked:
            mean, cov = posterior_moments(mm, X3)
            means.append(mean.reshape(-1))
            variances.append(cov.reshape(-1))
        mean, var = torch.stack(means), torch.stack(variances)
        cons = self._an_constraints()
        return torch.ops.bo.analytic(
            mean, var, self._best_f_rows(batch, mean), self._an_mode, 0,
            1.0 if self.maximize else -1.0, 0.0, kernels.AN_MIN_VAR, [c[0] for c in cons],
            [c[1] for c in cons], [c[2] for c in cons], [c[3] for c in cons])

    def _generic(self, X: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError  # pragma: no cover

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = t_batch_mode(X, expected_q=1)
        if X.dtype != torch.float64:  # the model computes in fp64; the value returns in X's dtype
            return self.forward(X.to(torch.float64)).to(X.dtype)
        batch = X.shape[:-2]
        X3 = X.reshape(-1, 1, X.shape[-1])
        fused = self._fused_applies(X3) if self._route is None else self._route == "fused"
        if fused:
            return self._fused(X3, batch).reshape(batch)
        return self._generic(X)


def _scaled_improvement(mean, sigma, best_f, maximize: bool):
    """acquisition/analytic.py:960-965."""
    u = (mean - best_f) / sigma
    return u if maximize else -u


class LogExpectedImprovement(_MomentChainAcquisition):
    """acquisition/analytic.py:356-416: log EI(x) = log_ei(u) + log sigma with
    u = (mu - best_f) / sigma; finite, with a usable gradient, where EI itself
    underflows to 0."""

    _admits_multitask = True

    _log: bool = True
    _an_mode = kernels.AN_LOG_EI

    def __init__(self, model, best_f, posterior_transform=None, maximize: bool = True):
        super().__init__(model, posterior_transform)
        self.register_buffer("best_f", torch.as_tensor(best_f, dtype=torch.float64))
        self.maximize = maximize

    def _generic(self, X):
        from .safe_math import log_ei_helper
        mean, sigma = self._mean_and_sigma(X)
        u = _scaled_improvement(mean, sigma, self.best_f.to(mean), self.maximize)
        return log_ei_helper(u) + sigma.log()


class LogProbabilityOfImprovement(_MomentChainAcquisition):
    """acquisition/analytic.py:111-170: log Phi((mu - best_f) / sigma)."""

    _log: bool = True
    _an_mode = kernels.AN_LOG_PI

    def __init__(self, model, best_f, posterior_transform=None, maximize: bool = True):
        super().__init__(model, posterior_transform)
        self.register_buffer("best_f", torch.as_tensor(best_f, dtype=torch.float64))
        self.maximize = maximize

    def _generic(self, X):
        from .safe_math import log_Phi
        mean, sigma = self._mean_and_sigma(X)
        return log_Phi(_scaled_improvement(mean, sigma, self.best_f.to(mean), self.maximize))


class PosteriorStandardDeviation(_MomentChainAcquisition):
    """acquisition/analytic.py:890-954: sigma, or -sigma with ``maximize=False``."""

    _an_mode = kernels.AN_STD

    def __init__(self, model, posterior_transform=None, maximize: bool = True):
        super().__init__(model, posterior_transform)
        self.maximize = maximize

    def _generic(self, X):
        _, std = self._mean_and_sigma(X)
        return std if self.maximize else -std


class ScalarizedPosteriorMean(AnalyticAcquisitionFunction):
    """acquisition/analytic.py:849-887: the posterior mean of the q points
    weighted by ``weights`` (q).  A weighted sum of means: torch only."""

    def __init__(self, model, weights: torch.Tensor, posterior_transform=None):
        super().__init__(model, posterior_transform)
        if posterior_transform is None and model.num_outputs != 1:
            raise UnsupportedError("Must specify a posterior transform when using a "
                                   "multi-output model.")
        self.register_buffer("weights", weights)

    def forward(self, X):
        X = t_batch_mode(X)
        mean, _ = self._mean_and_sigma(X, compute_sigma=False)
        return mean @ self.weights.to(mean)


def _preprocess_constraint_bounds(acqf, constraints) -> None:
    """acquisition/analytic.py:1137-1179: the constraints ``{i: (lower, upper)}``
    (None: unbounded) sorted into lower, upper and two-sided groups, as buffers."""
    con_lower, con_lower_inds = [], []
    con_upper, con_upper_inds = [], []
    con_both, con_both_inds = [], []
    con_indices = list(constraints.keys())
    if len(con_indices) == 0:
        raise ValueError("There must be at least one constraint.")
    if acqf.objective_index in con_indices:
        raise ValueError("Output corresponding to objective should not be a constraint.")
    for k in con_indices:
        if constraints[k][0] is not None and constraints[k][1] is not None:
            if constraints[k][1] <= constraints[k][0]:
                raise ValueError("Upper bound is less than the lower bound.")
            con_both_inds.append(k)
            con_both.append([constraints[k][0], constraints[k][1]])
        elif constraints[k][0] is not None:
            con_lower_inds.append(k)
            con_lower.append(constraints[k][0])
        elif constraints[k][1] is not None:
            con_upper_inds.append(k)
            con_upper.append(constraints[k][1])
    for name, indices in [("con_lower_inds", con_lower_inds), ("con_upper_inds", con_upper_inds),
                          ("con_both_inds", con_both_inds), ("con_both", con_both),
                          ("con_lower", con_lower), ("con_upper", con_upper)]:
        # (the bounds in fp64: as the default dtype they would reach the formula rounded to fp32)
        dtype = torch.long if name.endswith("_inds") else torch.float64
        acqf.register_buffer(name, torch.as_tensor(indices, dtype=dtype))
    # the same table on the host, in the groups' order, for the fused route:
    # (output, lower, upper, kind)
    acqf._con_table = (
        [(k, float(v), 0.0, kernels.AN_CON_LOWER) for k, v in zip(con_lower_inds, con_lower)]
        + [(k, 0.0, float(v), kernels.AN_CON_UPPER) for k, v in zip(con_upper_inds, con_upper)]
        + [(k, float(lo), float(hi), kernels.AN_CON_BOTH)
           for k, (lo, hi) in zip(con_both_inds, con_both)])


def _compute_log_prob_feas(acqf, means: torch.Tensor, sigmas: torch.Tensor) -> torch.Tensor:
    """acquisition/analytic.py:1182-1220: the log probability that every
    constrained output lies within its bounds, the outputs independent."""
    from .safe_math import log_Phi, log_prob_normal_in
    acqf.to(device=means.device)
    log_prob = torch.zeros_like(means[..., 0])
    if len(acqf.con_lower_inds) > 0:
        i = acqf.con_lower_inds
        dist_l = (acqf.con_lower - means[..., i]) / sigmas[..., i]
        log_prob = log_prob + log_Phi(-dist_l).sum(dim=-1)  # 1 - Phi(x) = Phi(-x)
    if len(acqf.con_upper_inds) > 0:
        i = acqf.con_upper_inds
        dist_u = (acqf.con_upper - means[..., i]) / sigmas[..., i]
        log_prob = log_prob + log_Phi(dist_u).sum(dim=-1)
    if len(acqf.con_both_inds) > 0:
        i = acqf.con_both_inds
        con_lower, con_upper = acqf.con_both[:, 0], acqf.con_both[:, 1]
        dist_l = (con_lower - means[..., i]) / sigmas[..., i]
        dist_u = (con_upper - means[..., i]) / sigmas[..., i]
        log_prob = log_prob + log_prob_normal_in(a=dist_l, b=dist_u).sum(dim=-1)
    return log_prob


class LogConstrainedExpectedImprovement(_MomentChainAcquisition):
    """acquisition/analytic.py:419-495: log EI of output ``objective_index`` plus
    the log probability that the constrained outputs are feasible, over a
    multi-output SingleTaskGP or a ModelListGP (independent outputs)."""

    _log: bool = True
    _an_mode = kernels.AN_LOG_EI

    def __init__(self, model, best_f, objective_index: int, constraints: dict,
                 maximize: bool = True):
        super().__init__(model, None, check_outputs=False)
        self.maximize = maximize
        self.objective_index = objective_index
        self.constraints = constraints
        self.register_buffer("best_f", torch.as_tensor(best_f, dtype=torch.float64))
        _preprocess_constraint_bounds(self, constraints=constraints)

    def _an_members(self) -> List[int]:
        return [self.objective_index] + [c[0] for c in self._con_table]

    def _an_constraints(self) -> list:
        return [(pos + 1, lo, hi, kind) for pos, (_, lo, hi, kind) in enumerate(self._con_table)]

    def _objective_terms(self, X):
        means, sigmas = self._mean_and_sigma(X)
        ind = self.objective_index
        mean_obj, sigma_obj = means[..., ind], sigmas[..., ind]
        u = _scaled_improvement(mean_obj, sigma_obj, self.best_f.to(mean_obj), self.maximize)
        return u, sigma_obj, _compute_log_prob_feas(self, means=means, sigmas=sigmas)

    def _generic(self, X):
        from .safe_math import log_ei_helper
        u, sigma_obj, log_prob_feas = self._objective_terms(X)
        return log_ei_helper(u) + sigma_obj.log() + log_prob_feas


class ConstrainedExpectedImprovement(LogConstrainedExpectedImprovement):
    """acquisition/analytic.py:498-574: EI of the objective output times the
    probability of feasibility.  LogConstrainedExpectedImprovement has the
    better numerics (this one is exactly 0 where either factor underflows)."""

    _log: bool = False
    _an_mode = kernels.AN_EI

    def _generic(self, X):
        from .safe_math import ei_helper
        u, sigma_obj, log_prob_feas = self._objective_terms(X)
        return (sigma_obj * ei_helper(u)).mul(log_prob_feas.exp())


# -- pathwise Thompson sampling -----------------------------------------------------------
BATCH_SIZE_CHANGE_ERROR = """The batch size of PathwiseThompsonSampling should \
not change during a forward pass - was {}, now {}. Please re-initialize the \
acquisition if you want to change the batch size."""


class PathwiseThompsonSampling(AcquisitionFunction):
    """acquisition/thompson_sampling.py:22-87: single-outcome Thompson sampling
    as an acquisition function.  The q points of a t-batch are evaluated on q
    posterior function draws (point i on draw i; pathwise.get_matheron_path_model,
    the fused kernel's mapped mode) and the values summed, so maximising it
    yields q Thompson samples.  The draws are made at the first call and kept
    until :meth:`redraw`."""

    def __init__(self, model, posterior_transform=None):
        if getattr(model, "_is_fully_bayesian", False):
            raise NotImplementedError(
                "PathwiseThompsonSampling is not supported for fully Bayesian models")
        super().__init__(model)
        self.batch_size: Optional[int] = None
        self.samples = None

    def redraw(self) -> None:
        from .pathwise import get_matheron_path_model
        self.samples = get_matheron_path_model(model=self.model,
                                               sample_shape=torch.Size([self.batch_size]))

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = t_batch_mode(X)
        batch_size = X.shape[-2]
        if self.batch_size is None:
            self.batch_size = batch_size
            self.redraw()
        elif self.batch_size != batch_size:
            raise ValueError(BATCH_SIZE_CHANGE_ERROR.format(self.batch_size, batch_size))
        # batch_shape x q x 1 x d on the q draws -> batch_shape x q x 1 x m
        values = self.samples(X.unsqueeze(-2)).squeeze(-2)
        return values.sum(-2).squeeze(-1)


# -- one-shot knowledge gradient --------------------------------------------------------
class OneShotAcquisitionFunction:
    """acquisition/acquisition.py:149-177: an acquisition function optimised
    jointly over the candidates and the solutions of its inner problems."""

    def get_augmented_q_batch_size(self, q: int) -> int:
        raise NotImplementedError

    def extract_candidates(self, X_full: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError


def _split_fantasy_points(X: torch.Tensor, n_f: int):
    """acquisition/knowledge_gradient.py:559-586, without the permutation to a
    fantasy batch: (X_actual b x q x d, X_fantasies b x n_f x d)."""
    if n_f > X.size(-2):
        raise ValueError(f"n_f ({n_f}) must be less than the q-batch dimension of X ({X.size(-2)})")
    return X[..., : X.size(-2) - n_f, :], X[..., X.size(-2) - n_f:, :]


class qKnowledgeGradient(MCAcquisitionFunction, OneShotAcquisitionFunction):
    """One-shot batch knowledge gradient (acquisition/knowledge_gradient.py:53-305)
    of a single-output exact GP with the posterior mean as inner value
    (``objective=None``): X is b x (q + N_f) x d, the q candidates followed by
    the N_f solutions x'_i of the fantasy models' inner problems.

    The reference draws Y_i = mu(X) + L z_i under observation noise (L the root
    of A = Sigma(X, X) + s2 I, z_i the fantasy sampler's base samples),
    conditions the model on (X, Y_i) and takes the fantasy model's posterior
    mean at x'_i.  That mean is, in the current model's joint posterior,

        v_i = mu(x'_i) + Sigma(x'_i, X) L^{-T} z_i,   KG = mean_i v_i - current_value

    so no fantasy model is built.  For q (pending points included) up to
    kernels.KG_FUSED_QMAX and d <= kernels.DP the points are packed into tiles
    of at most 16 rows (kernels.kg_tile_plan), the fused posterior runs once
    over all tiles and bo::kg reduces them; otherwise the generic posterior
    kernels give the joint moments and the formula runs in torch.  Both are
    differentiable in all q + N_f points."""

    def __init__(self, model, num_fantasies: Optional[int] = 64, sampler=None, objective=None,
                 posterior_transform=None, inner_sampler=None, X_pending=None,
                 current_value=None):
        if sampler is None:
            if num_fantasies is None:
                raise ValueError("Must specify `num_fantasies` if no `sampler` is provided.")
            # base samples should be fixed for joint optimization over X, X_fantasies
            sampler = SobolQMCNormalSampler(sample_shape=torch.Size([num_fantasies]))
        elif num_fantasies is not None:
            if sampler.sample_shape != torch.Size([num_fantasies]):
                raise ValueError(f"The sampler shape must match num_fantasies={num_fantasies}.")
        else:
            num_fantasies = sampler.sample_shape[0]
        AcquisitionFunction.__init__(self, model)
        if objective is not None:
            raise UnsupportedError("qKnowledgeGradient: an `objective` (the MC inner expectation "
                                   "over an inner sampler) is not on the accelerated path; the "
                                   "inner value is the posterior mean")
        if getattr(model, "_is_ensemble", False):
            raise UnsupportedError("qKnowledgeGradient: fully Bayesian (ensemble) models are not "
                                   "on the accelerated path")
        if model.num_outputs != 1 or not hasattr(model, "prediction_cache"):
            raise UnsupportedError("qKnowledgeGradient: multi-output models and ModelListGP are "
                                   "not on the accelerated path (single-output SingleTaskGP only)")
        if posterior_transform is not None:
            w = getattr(posterior_transform, "weights", None)
            if not getattr(posterior_transform, "scalarize", False) or w is None or w.numel() != 1:
                raise UnsupportedError("qKnowledgeGradient: only a single-output "
                                       "ScalarizedPosteriorTransform is supported")
            self._affine = (float(w.reshape(-1)[0]), float(posterior_transform.offset))
        else:
            self._affine = None
        self.sampler = sampler
        self.objective = None
        self.posterior_transform = posterior_transform
        self.set_X_pending(X_pending)
        self.inner_sampler = inner_sampler
        self.num_fantasies = int(num_fantasies)
        self.current_value = current_value
        self._tile_index = {}

    def _noise(self) -> float:
        """sigma'^2 of the fantasy observations in outcome space, from host
        values: the likelihood's noise (fixed noise: its mean, models/model.py
        fantasize) times ystd^2."""
        ystd = self.model.outcome_stats()[1]
        return self.model.prediction_cache().noise * ystd * ystd

    def _fused(self, Xa: torch.Tensor, Xf: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
        from . import ops  # noqa: F401  (torch.ops.bo registration)
        from .posteriors import _fused_moments
        B, q_a, d = Xa.shape
        N_f = Xf.shape[1]
        T, slots = kernels.kg_tile_plan(q_a, N_f)
        key = (N_f, T, slots, Xa.device)
        idx = self._tile_index.get(key)
        if idx is None:  # fantasy of each slot; the spare slots repeat the last one
            idx = torch.arange(T * slots, device=Xa.device).clamp_max(N_f - 1).view(T, slots)
            self._tile_index[key] = idx
        tiles = torch.cat([Xa.unsqueeze(1).expand(B, T, q_a, d), Xf[:, idx]], dim=2)
        mean, cov = _fused_moments(tiles.reshape(B * T, q_a + slots, d), self.model)
        acq, _, _, _, jit, info = torch.ops.bo.kg(mean, cov, Z, self._noise(), q_a, slots)
        kernels.raise_not_psd_deferred(info, jit, type(self).__name__)
        return acq

    def _generic(self, Xa: torch.Tensor, Xf: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
        from .posteriors import _CholJitter, posterior_moments
        B, q_a, _ = Xa.shape
        mean, cov = posterior_moments(self.model, torch.cat([Xa, Xf], dim=-2))
        eye = torch.eye(q_a, dtype=cov.dtype, device=cov.device)
        L = _CholJitter.apply(cov[:, :q_a, :q_a] + self._noise() * eye)
        Wt = torch.linalg.solve_triangular(L.mT, Z.T.expand(B, q_a, Z.shape[0]), upper=True)
        values = mean[:, q_a:] + (cov[:, q_a:, :q_a] * Wt.mT).sum(dim=-1)
        return values.mean(dim=-1)

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = t_batch_mode(X)
        X_actual, X_fantasies = _split_fantasy_points(X, self.num_fantasies)
        if X.dtype != torch.float64:  # the model computes in fp64; the value returns in X's dtype
            return self.forward(X.to(torch.float64)).to(X.dtype)
        # X_pending joins the actual points only after the split
        X_actual = self._concat_pending(X_actual)
        batch = X.shape[:-2]
        q_a, d = X_actual.shape[-2], X.shape[-1]
        if q_a < 1:
            raise ValueError("qKnowledgeGradient: X holds no candidate besides the "
                             f"{self.num_fantasies} fantasy points")
        Xa = X_actual.reshape(-1, q_a, d)
        Xf = X_fantasies.reshape(-1, self.num_fantasies, d)
        Z = self.sampler.base_samples_2d(q_a, X.device)
        if q_a <= kernels.KG_FUSED_QMAX and d <= kernels.DP and X.is_cuda:
            acq = self._fused(Xa, Xf, Z)
        else:
            acq = self._generic(Xa, Xf, Z)
        if self._affine is not None:
            acq = self._affine[0] * acq + self._affine[1]
        if self.current_value is not None:
            acq = acq - torch.as_tensor(self.current_value).to(acq)
        return acq.reshape(batch)

    def evaluate(self, X: torch.Tensor, bounds: torch.Tensor, **kwargs):
        raise UnsupportedError("qKnowledgeGradient.evaluate (the separate optimisation of the "
                               "inner problem on fantasy models) is not on the accelerated path")

    def get_augmented_q_batch_size(self, q: int) -> int:
        return q + self.num_fantasies

    def extract_candidates(self, X_full: torch.Tensor) -> torch.Tensor:
        return X_full[..., : -self.num_fantasies, :]


# -- joint entropy search (lower bound) -------------------------------------------------
JES_ESTIMATION_TYPES = ["MC", "LB"]
JES_FULLY_BAYESIAN_ERROR_MSG = (
    "JES is not yet available with Fully Bayesian GPs. Track the issue, "
    "which regards conditioning on a number of optima on a collection "
    "of models, in detail at https://github.com/pytorch/botorch/issues/1680"
)
JES_S2_FLOOR, JES_PHI_FLOOR, JES_INNER_FLOOR = 1e-10, 1e-8, 1e-8


def _jes_chain(c, mu, var, g, sinv, wf, tau2, w: float):
    """H (...): the elementwise chain of the JES lower bound in torch, from
    c (... x P) and the rows' mu, var (...) -- what bo::jes computes on its
    accumulators (the generic route's formula)."""
    mu_j = mu.unsqueeze(-1) + c * g
    s2 = (var.unsqueeze(-1) - c * c * sinv).clamp_min(JES_S2_FLOOR)
    z = (wf - w * mu_j) / s2.sqrt()
    Phi = 0.5 * torch.erfc(-z / math.sqrt(2.0))
    r = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) / Phi.clamp_min(JES_PHI_FLOOR)
    vt = s2 * (1.0 - (z + r) * r).clamp_min(JES_INNER_FLOOR) + tau2
    return 0.5 * torch.log(vt).mean(dim=-1)


class qJointEntropySearch(AcquisitionFunction):
    """Joint entropy search (acquisition/joint_entropy_search.py:60-265) with the
    lower-bound estimate, for a single-output exact GP:

        acq(X) = logdet(Sigma(X) + tau2 I) / 2 - sum_i mean_j log(vt_ji) / 2

    where vt_ji is the (truncated) predictive variance at x_i of the model
    conditioned on the optimum (x*_j, f*_j).  No conditioned model is built:
    conditioning on one observation is a rank-one correction of the current
    posterior, so model j's moments at x_i follow from the current posterior at
    X, the posterior covariance c_ij of x_i with x*_j, and per-optimum constants
    fixed at construction (with V = A^{-1} k(Xt, x*), two GEMMs on the cached
    L^{-1}).  All of it is computed in the model's transformed outcome space;
    the Standardize constant cancels between the two entropy terms.

    ``optimal_inputs`` P x d and ``optimal_outputs`` P x 1 (outcome space), as
    :func:`pathwise.get_optimal_samples` returns them.  For d <=
    kernels.JES_DMAX the fused route forms c_ij on the matrix cores and runs
    the chain on the accumulator (``bo::jes``); the generic route takes c_ij
    from the joint posterior of the q + P points and applies the formula in
    torch.  ``maximize=False`` takes the optima as minima (the outputs and the
    conditioned means are both negated)."""

    def __init__(self, model, optimal_inputs: torch.Tensor, optimal_outputs: torch.Tensor,
                 condition_noiseless: bool = True, posterior_transform=None, X_pending=None,
                 estimation_type: str = "LB", maximize: bool = True, num_samples: int = 64):
        from .models import (MIN_INFERRED_NOISE_LEVEL, FixedNoiseGaussianLikelihood, ModelListGP,
                             SaasFullyBayesianSingleTaskGP, SingleTaskGP)
        super().__init__(model)
        if isinstance(model, SaasFullyBayesianSingleTaskGP):
            raise NotImplementedError(JES_FULLY_BAYESIAN_ERROR_MSG)
        if (isinstance(model, ModelListGP) or not isinstance(model, SingleTaskGP)
                or model.num_outputs != 1):
            raise UnsupportedError("qJointEntropySearch: multi-output models and ModelListGP are "
                                   "not on the accelerated path (single-output SingleTaskGP only)")
        if posterior_transform is not None:
            raise UnsupportedError("qJointEntropySearch: a `posterior_transform` is not on the "
                                   "accelerated path")
        if model.training:
            raise UnsupportedError("qJointEntropySearch needs a model in eval mode (model.eval()): "
                                   "the optima are conditioned on the trained model's prediction "
                                   "caches")
        if estimation_type == "MC":
            raise UnsupportedError("qJointEntropySearch: estimation_type='MC' is not on the "
                                   "accelerated path (the lower bound 'LB' is)")
        if estimation_type != "LB":
            raise ValueError(f"Estimation type {estimation_type} is not valid. "
                             f"Please specify any of {JES_ESTIMATION_TYPES}")
        d = model.train_inputs[0].shape[-1]
        if optimal_inputs.dim() != 2 or optimal_inputs.shape[-1] != d or optimal_inputs.shape[0] < 1:
            raise ValueError(f"qJointEntropySearch: optimal_inputs must be `num_optima x {d}`, got "
                             f"{tuple(optimal_inputs.shape)}")
        P = optimal_inputs.shape[0]
        if tuple(optimal_outputs.shape) != (P, 1):
            raise ValueError(f"qJointEntropySearch: optimal_outputs must be `{P} x 1`, got "
                             f"{tuple(optimal_outputs.shape)}")
        fixed = isinstance(model.likelihood, FixedNoiseGaussianLikelihood)
        if fixed and not condition_noiseless:
            raise RuntimeError("FixedNoiseGaussianLikelihood.fantasize requires a `noise` kwarg")
        self.posterior_transform = None
        self.condition_noiseless = bool(condition_noiseless)
        self.estimation_type = estimation_type
        self.maximize = bool(maximize)
        self.num_samples = P
        self.optimal_inputs = optimal_inputs.unsqueeze(-2)
        self.optimal_outputs = optimal_outputs.unsqueeze(-2)
        self._route = None  # None: by size; "fused" / "generic": forced (tests, tools)
        self._w = 1.0 if maximize else -1.0
        self._condition(model, optimal_inputs, optimal_outputs, fixed, MIN_INFERRED_NOISE_LEVEL)
        self.set_X_pending(X_pending)

    def _condition(self, model, optimal_inputs, optimal_outputs, fixed: bool, min_noise: float):
        """The per-optimum constants, once: m_j, v_j (the current posterior at
        x*_j), nu_j, s_j = v_j + nu_j, g_j = (f*_j - m_j) / s_j, tau2_j and
        V = A^{-1} k(Xt, x*) against the cached L^{-1}."""
        from .posteriors import posterior_moments
        with torch.no_grad():
            cache = model.prediction_cache()
            ymean, ystd = model.outcome_stats()
            n, dev = cache.n, cache.Xt.device
            Xo = optimal_inputs.detach().to(device=dev, dtype=torch.float64).contiguous()
            P, d = Xo.shape
            f = (optimal_outputs.detach().to(device=dev, dtype=torch.float64).reshape(-1)
                 - ymean) / ystd
            mean_o, cov_o = posterior_moments(model, Xo.unsqueeze(-2))
            m = (mean_o.reshape(-1) - ymean) / ystd
            v = cov_o.reshape(-1) / (ystd * ystd)
            tau2 = float(cache.noise)  # the level, or the mean of the fixed variances
            nu = min_noise if self.condition_noiseless else tau2
            s = v + nu
            self._tau2 = tau2
            self._Xo = Xo
            self._Xo_scaled = (Xo / cache.lengthscale).contiguous()
            self._Xt_scaled = (cache.Xt / cache.lengthscale).contiguous() if n else None
            self._g = ((f - m) / s).contiguous()
            self._sinv = (1.0 / s).contiguous()
            self._wf = (self._w * f).contiguous()
            self._tau2_j = torch.full((P,), (n * tau2 + nu) / (n + 1) if fixed else tau2,
                                      dtype=torch.float64, device=dev)
            self._V = None
            if n and d <= kernels.JES_DMAX:
                K = kernels.covar_matrix(Xo, cache.Xt, cache.lengthscale, cache.kind,
                                         cache.outputscale)
                E = K.t().contiguous()  # n x P
                ld = cache.Linv.shape[1]
                T = torch.empty(n, P, dtype=torch.float64, device=dev)
                Vt = torch.empty(n, P, dtype=torch.float64, device=dev)
                # the leading n x n block of the (padded) L^{-1}, read in place
                kernels.gemm_strided(n, P, n, cache.Linv, ld, 0, E, P, 0, T, P, 0, 1)
                kernels.gemm_strided(n, P, n, cache.Linv, ld, 0, T, P, 0, Vt, P, 0, 1, transA=True)
                self._V = Vt.t().contiguous()
            self._hyper = (cache.lengthscale, int(cache.kind), float(cache.outputscale))
            self._stats = (float(ymean), float(ystd))

    def _entropy(self, Sigma: torch.Tensor) -> torch.Tensor:
        """logdet(Sigma + tau2 I) / 2 = sum log diag chol, through the
        differentiable jitter-ladder Cholesky."""
        from .posteriors import _CholJitter
        q = Sigma.shape[-1]
        A = Sigma + self._tau2 * torch.eye(q, dtype=Sigma.dtype, device=Sigma.device)
        L = _CholJitter.apply(A) if torch.is_grad_enabled() and A.requires_grad \
            else kernels.chol_jitter(A)
        return L.diagonal(dim1=-2, dim2=-1).log().sum(dim=-1)

    def _fused(self, X3: torch.Tensor) -> torch.Tensor:
        from . import ops  # noqa: F401  (torch.ops.bo registration)
        from .posteriors import posterior_moments
        B, q, d = X3.shape
        ymean, ystd = self._stats
        mean, cov = posterior_moments(self.model, X3)
        mu, Sigma = (mean - ymean) / ystd, cov / (ystd * ystd)
        var = Sigma.diagonal(dim1=-2, dim2=-1)
        ls, kind, o = self._hyper
        H = torch.ops.bo.jes(X3.reshape(B * q, d), mu.reshape(B * q), var.reshape(B * q), ls,
                             self._Xt_scaled if self._V is not None else None, self._Xo_scaled,
                             self._V, self._g, self._sinv, self._wf, self._tau2_j, kind, o, self._w)
        return self._entropy(Sigma) - H.view(B, q).sum(dim=-1)

    def _generic(self, X3: torch.Tensor) -> torch.Tensor:
        from .posteriors import posterior_moments
        B, q, d = X3.shape
        ymean, ystd = self._stats
        P = self._Xo.shape[0]
        mean, cov = posterior_moments(self.model, torch.cat([X3, self._Xo.expand(B, P, d)], dim=-2))
        mu = (mean[:, :q] - ymean) / ystd
        Sigma = cov[:, :q, :q] / (ystd * ystd)
        c = cov[:, :q, q:] / (ystd * ystd)
        H = _jes_chain(c, mu, Sigma.diagonal(dim1=-2, dim2=-1), self._g, self._sinv, self._wf,
                       self._tau2_j, self._w)
        return self._entropy(Sigma) - H.sum(dim=-1)

    def conditioned_moments(self, X: torch.Tensor):
        """(mean, variance) in outcome space, each ``batch x q x P``, that the
        model conditioned on optimum j predicts at X with observation noise:
        mu_ji and s2_ji + tau2_j of the class docstring (unclamped), from the
        joint posterior of the q + P points and the constants of the
        construction.  What ``condition_on_observations(x*_j, f*_j, noise=nu)``
        followed by ``.posterior(X, observation_noise=True)`` gives, one
        optimum at a time."""
        from .posteriors import posterior_moments
        X = t_batch_mode(X).to(torch.float64)
        q, P = X.shape[-2], self._Xo.shape[0]
        ymean, ystd = self._stats
        Xo = self._Xo.expand(*X.shape[:-2], P, X.shape[-1])
        mean, cov = posterior_moments(self.model, torch.cat([X, Xo], dim=-2))
        mu = (mean[..., :q] - ymean) / ystd
        c = cov[..., :q, q:] / (ystd * ystd)
        var = cov[..., :q, :q].diagonal(dim1=-2, dim2=-1) / (ystd * ystd)
        mu_j = mu.unsqueeze(-1) + c * self._g
        vt = var.unsqueeze(-1) - c * c * self._sinv + self._tau2_j
        return ymean + ystd * mu_j, (ystd * ystd) * vt

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = t_batch_mode(X)
        if X.dtype != torch.float64:  # the model computes in fp64; the value returns in X's dtype
            return self.forward(X.to(torch.float64)).to(X.dtype)
        batch = X.shape[:-2]
        X = self._concat_pending(X)
        q, d = X.shape[-2], X.shape[-1]
        X3 = X.reshape(-1, q, d)
        fused = d <= kernels.JES_DMAX and X.is_cuda if self._route is None \
            else self._route == "fused"
        acq = self._fused(X3) if fused else self._generic(X3)
        return acq.reshape(batch)


# -- max-value entropy search: MES and GIBBON -------------------------------------------
MES_CLAMP_LB = 1e-8
MES_VDET_EPS = (1.0 + 1e-12) - 1.0  # lim - qf = qf MES_VDET_EPS on GIBBON's clamped branch


def _mes_Phi(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def _mes_chain(mu, var, fstar, z, tau2: float, w: float):
    """ig (R) of qMaxValueEntropy from the rows' posterior mean and variance (R
    each), the max values fstar (S_M) and the base samples z (S_m), as broadcast
    torch tensors R x S_M x S_m (max_value_entropy_search.py:427-515 without
    fantasies): what bo::mes computes in registers (the generic route's
    formula; DESIGN.md section 18 states it)."""
    m = (w * mu)[:, None, None]
    vM = var.clamp_min(MES_CLAMP_LB)[:, None, None]
    vm = (var + tau2)[:, None, None]
    zk, f = z[None, None, :], fstar[None, :, None]
    mean_new = m + (vM / vm) * vm.sqrt() * (w * zk)
    s2n = (vM - vM * vM / vm).clamp_min(MES_CLAMP_LB)
    Z = _mes_Phi((f - mean_new) / s2n.sqrt()).clamp_min(MES_CLAMP_LB) \
        / _mes_Phi((f - m) / vM.sqrt()).clamp_min(MES_CLAMP_LB)
    lp = -0.5 * zk * zk - 0.5 * torch.log(2.0 * math.pi * vm)
    h1 = -Z * Z.log() - Z * lp
    h0 = -lp
    H1bar, H0bar = h1.mean(dim=(1, 2)), h0.mean(dim=(1, 2))
    cov = ((h1 - H1bar[:, None, None]) * (h0 - H0bar[:, None, None])).mean(dim=(1, 2))
    beta = cov / (h0.var(dim=(1, 2)) * h1.var(dim=(1, 2))).sqrt()
    H0 = 0.5 * torch.log(2.0 * math.pi * math.e * vm.reshape(-1))
    return H0 - H1bar + beta * (H0bar - H0)


def _gibbon_chain(mu, var, fstar, tau2: float, w: float, A=None, Binv=None):
    """acq (R) of GIBBON in torch (max_value_entropy_search.py:563-664): the
    quality term and, with A (R x m) and Binv (m x m), the repulsion term in
    outcome space -- what bo::gibbon computes (the generic route's formula)."""
    vM = var.clamp_min(MES_CLAMP_LB)
    vm = (var + tau2).clamp_min(MES_CLAMP_LB)
    g = (fstar[None, :] - (w * mu)[:, None]) / vM.sqrt()[:, None]
    r = torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi) / _mes_Phi(g).clamp_min(MES_CLAMP_LB)
    inner = 1.0 - (vM / vm)[:, None] * r * (g + r)
    acq = -0.5 * inner.clamp_min(MES_CLAMP_LB).log().mean(dim=1)
    if A is not None and A.shape[-1] > 0:
        qf = ((A @ Binv) * A).sum(-1)
        lim = qf * (1.0 + 1e-12)
        # clamped: lim - qf without its cancellation; the gradient runs through qf
        vdet = torch.where(vm >= lim, vm - qf, qf * MES_VDET_EPS)
        acq = acq + 0.5 * (torch.log(vdet) - torch.log(vm))
    return acq


def _mv_moments(model, candidate_set: torch.Tensor, maximize: bool):
    """(w mu, sigma), N each: the candidate set's posterior in one
    posterior_moments call over N x 1 x d."""
    from .posteriors import posterior_moments
    mean, cov = posterior_moments(model, candidate_set.unsqueeze(-2))
    w = 1.0 if maximize else -1.0
    return w * mean.reshape(-1), cov.reshape(-1).clamp_min(1e-8).sqrt()


def _sample_max_value_Thompson(model, candidate_set: torch.Tensor, num_samples: int,
                               posterior_transform=None, maximize: bool = True) -> torch.Tensor:
    """max_value_entropy_search.py:924-956: the maxima of ``num_samples`` joint
    posterior draws over the candidate set, ``num_samples x 1``."""
    posterior = model.posterior(candidate_set, posterior_transform=posterior_transform)
    weight = 1.0 if maximize else -1.0
    samples = weight * posterior.rsample(torch.Size([num_samples])).squeeze(-1)
    return samples.max(dim=-1).values.unsqueeze(-1)


def _sample_max_value_Gumbel(model, candidate_set: torch.Tensor, num_samples: int,
                             posterior_transform=None, maximize: bool = True) -> torch.Tensor:
    """max_value_entropy_search.py:959-1022: the Gumbel approximation of the
    maximum over the candidate set under independence, ``num_samples x 1``.  The
    three quantiles it is fitted to come from one on-device bisection launch
    (bo::mv_quantiles) in place of brentq on host copies."""
    from . import ops  # noqa: F401  (torch.ops.bo registration)
    if posterior_transform is not None:
        raise UnsupportedError("max-value sampling: a `posterior_transform` is not on the "
                               "accelerated path")
    mu, sigma = _mv_moments(model, candidate_set, maximize)
    y, status = torch.ops.bo.mv_quantiles(mu, sigma, False, 0.0, 0.0)
    kernels.mv_quantiles_raise(status.tolist())
    q25, q50, q75 = y[0:1], y[1:2], y[2:3]
    b = (q25 - q75) / (math.log(math.log(4.0 / 3.0)) - math.log(math.log(4.0)))
    a = q50 + b * math.log(math.log(2.0))
    eps = torch.rand(num_samples, 1, device=mu.device, dtype=mu.dtype)
    return a - b * eps.log().mul(-1.0).log()


def _mv_validate(name: str, model, posterior_transform) -> None:
    """The supported configuration of the max-value family: a single-output
    SingleTaskGP in eval mode without posterior transform."""
    from .models import ModelListGP, SaasFullyBayesianSingleTaskGP, SingleTaskGP
    if isinstance(model, SaasFullyBayesianSingleTaskGP):
        raise UnsupportedError(f"{name}: SaasFullyBayesianSingleTaskGP is not on the accelerated "
                               "path (single-output SingleTaskGP only)")
    if (isinstance(model, ModelListGP) or not isinstance(model, SingleTaskGP)
            or model.num_outputs != 1):
        raise UnsupportedError(f"{name}: multi-output models and ModelListGP are not on the "
                               "accelerated path (single-output SingleTaskGP only)")
    if posterior_transform is not None:
        raise UnsupportedError(f"{name}: a `posterior_transform` is not on the accelerated path")
    if model.training:
        raise UnsupportedError(f"{name} needs a model in eval mode (model.eval()): the posterior "
                               "comes from the trained model's prediction caches")


class MaxValueBase(AcquisitionFunction):
    """max_value_entropy_search.py:60-191: the max-value entropy family for a
    single-output exact GP.  Subclasses set ``posterior_max_values`` (S_M x 1,
    in the w-signed outcome space) in ``_sample_max_values`` and compute the
    value of the rows of a ``R x 1 x d`` tensor in ``_fused`` / ``_generic``.
    Every t-batch is q = 1; everything is computed in outcome space."""

    def __init__(self, model, num_mv_samples: int, posterior_transform=None,
                 maximize: bool = True, X_pending=None):
        _mv_validate(type(self).__name__, model, posterior_transform)
        super().__init__(model)
        self.num_mv_samples = num_mv_samples
        self.posterior_transform = None
        self.maximize = bool(maximize)
        self.weight = 1.0 if maximize else -1.0
        self._route = None  # None: by size; "fused" / "generic": forced (tests, tools)
        _, ystd = model.outcome_stats()
        # what GPyTorchPosterior.from_model(..., observation_noise=True) adds
        self._tau2 = float(model.likelihood.noise.detach().mean()) * float(ystd) ** 2
        self.set_X_pending(X_pending)

    def set_X_pending(self, X_pending: Optional[torch.Tensor] = None) -> None:
        if X_pending is not None:
            X_pending = X_pending.detach().clone()
        self._sample_max_values(num_samples=self.num_mv_samples, X_pending=X_pending)
        self.X_pending = X_pending

    def _sample_max_values(self, num_samples: int, X_pending=None) -> None:
        raise NotImplementedError  # pragma: no cover

    def _fused(self, X3: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError  # pragma: no cover

    def _generic(self, X3: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError  # pragma: no cover

    def _fused_applies(self, X3: torch.Tensor) -> bool:
        return X3.is_cuda

    def _fstar(self) -> torch.Tensor:
        return self.posterior_max_values.reshape(-1).to(torch.float64)

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = t_batch_mode(X, expected_q=1)
        if X.dtype != torch.float64:  # the model computes in fp64; the value returns in X's dtype
            return self.forward(X.to(torch.float64)).to(X.dtype)
        batch = X.shape[:-2]
        X3 = X.reshape(-1, 1, X.shape[-1])
        fused = self._fused_applies(X3) if self._route is None else self._route == "fused"
        return (self._fused(X3) if fused else self._generic(X3)).reshape(batch)


class DiscreteMaxValueBase(MaxValueBase):
    """max_value_entropy_search.py:194-297: max values drawn on a discrete
    candidate set (with the training inputs, and the pending points, appended),
    by the Gumbel approximation or by discrete Thompson sampling."""

    def __init__(self, model, candidate_set: torch.Tensor, num_mv_samples: int = 10,
                 posterior_transform=None, use_gumbel: bool = True, maximize: bool = True,
                 X_pending=None, train_inputs=None):
        _mv_validate(type(self).__name__, model, posterior_transform)
        if train_inputs is None and hasattr(model, "train_inputs"):
            train_inputs = model.train_inputs[0]
        if train_inputs is not None:
            if train_inputs.ndim > 2:
                raise NotImplementedError("Batch GP models (e.g. fantasized models) "
                                          "are not yet supported by `MaxValueBase`")
            candidate_set = torch.cat([candidate_set, train_inputs.to(candidate_set)], dim=0)
        self.use_gumbel = use_gumbel
        self.candidate_set = candidate_set
        super().__init__(model=model, num_mv_samples=num_mv_samples,
                         posterior_transform=posterior_transform, maximize=maximize,
                         X_pending=X_pending)

    def _sample_max_values(self, num_samples: int, X_pending=None) -> None:
        sample = _sample_max_value_Gumbel if self.use_gumbel else _sample_max_value_Thompson
        candidate_set = self.candidate_set
        with torch.no_grad():
            if X_pending is not None:
                candidate_set = torch.cat([candidate_set, X_pending.to(candidate_set)], dim=0)
            self.posterior_max_values = sample(
                model=self.model, candidate_set=candidate_set, num_samples=self.num_mv_samples,
                posterior_transform=None, maximize=self.maximize).to(candidate_set.dtype)


MES_PENDING_MSG = (
    "qMaxValueEntropy with pending points needs batched fantasy models (`model.fantasize`), "
    "which are not on the accelerated path (DESIGN.md section 7); use "
    "qLowerBoundMaxValueEntropy (GIBBON) for batches with pending points")


class qMaxValueEntropy(DiscreteMaxValueBase):
    """Max-value entropy search (max_value_entropy_search.py:300-515) without
    pending points: the mutual information of the maximum and the noisy
    observation at x, with the regression-adjusted two-level estimate over
    ``num_mv_samples`` max values and ``num_y_samples`` Sobol base samples
    (drawn once at construction and shared by all t-batches).  The fused route
    (``bo::mes``) keeps the S_M x S_m pairs of a row in one wave's registers; the
    generic route is the same formula as broadcast torch tensors.
    ``num_fantasies`` is accepted and unused: pending points raise
    ``UnsupportedError``."""

    def __init__(self, model, candidate_set: torch.Tensor, num_fantasies: int = 16,
                 num_mv_samples: int = 10, num_y_samples: int = 128, posterior_transform=None,
                 use_gumbel: bool = True, maximize: bool = True, X_pending=None,
                 train_inputs=None):
        _mv_validate("qMaxValueEntropy", model, posterior_transform)
        if X_pending is not None:
            raise UnsupportedError(MES_PENDING_MSG)
        if num_y_samples < 2:
            raise ValueError("qMaxValueEntropy: num_y_samples >= 2 (the regression adjustment "
                             f"divides by the sample variance; got {num_y_samples})")
        kernels.mes_check(num_mv_samples, num_y_samples)
        super().__init__(model=model, candidate_set=candidate_set, num_mv_samples=num_mv_samples,
                         posterior_transform=posterior_transform, use_gumbel=use_gumbel,
                         maximize=maximize, X_pending=None, train_inputs=train_inputs)
        self.num_fantasies = num_fantasies
        self.num_y_samples = num_y_samples
        # the seed comes from torch's global generator (sampling/base.py)
        seed = int(torch.randint(0, 1000000, (1,)).item())
        dev = model.train_inputs[0].device
        self.base_samples = kernels.sobol_normal(1, num_y_samples, seed, dev).reshape(-1)
        self._consts = kernels.mes_host_constants(self.base_samples)

    def set_X_pending(self, X_pending: Optional[torch.Tensor] = None) -> None:
        if X_pending is not None:
            raise UnsupportedError(MES_PENDING_MSG)
        super().set_X_pending(None)

    def _moments(self, X3: torch.Tensor):
        from .posteriors import posterior_moments
        mean, cov = posterior_moments(self.model, X3)
        return mean.reshape(-1), cov.reshape(-1)

    def _fused(self, X3: torch.Tensor) -> torch.Tensor:
        from . import ops  # noqa: F401  (torch.ops.bo registration)
        mu, var = self._moments(X3)
        return torch.ops.bo.mes(mu, var, self._fstar(), self.base_samples, *self._consts,
                                self._tau2, self.weight)

    def _generic(self, X3: torch.Tensor) -> torch.Tensor:
        mu, var = self._moments(X3)
        return _mes_chain(mu, var, self._fstar(), self.base_samples, self._tau2, self.weight)


class qLowerBoundMaxValueEntropy(DiscreteMaxValueBase):
    """GIBBON (max_value_entropy_search.py:518-664): the cheap lower bound of the
    information gain, with the repulsion term of the pending points that
    ``optimize_acqf(..., q > 1, sequential=True)`` sets.  With m pending points
    one posterior over ``R x (1 + m) x d`` gives mu, sigma^2 (row 0) and the
    cross-covariance A; B^{-1} is fixed at ``set_X_pending``.  The fused route
    (``bo::gibbon``) applies up to kernels.GIBBON_MMAX pending points."""

    def set_X_pending(self, X_pending: Optional[torch.Tensor] = None) -> None:
        super().set_X_pending(X_pending)
        self._Binv = None
        if self.X_pending is not None:
            from .posteriors import posterior_moments
            with torch.no_grad():
                Xp = self.X_pending.to(torch.float64)
                _, cov = posterior_moments(self.model, Xp.unsqueeze(0))
                m = Xp.shape[-2]
                B = cov[0] + self._tau2 * torch.eye(m, dtype=torch.float64, device=cov.device)
                self._Binv = torch.cholesky_inverse(kernels.chol_jitter(B))

    def _moments(self, X3: torch.Tensor):
        from .posteriors import posterior_moments
        if self.X_pending is None:
            mean, cov = posterior_moments(self.model, X3)
            return mean.reshape(-1), cov.reshape(-1), None
        Xp = self.X_pending.to(X3)
        mean, cov = posterior_moments(self.model,
                                      torch.cat([X3, Xp.expand(X3.shape[0], *Xp.shape)], dim=-2))
        return mean[:, 0], cov[:, 0, 0], cov[:, 0, 1:]

    def _fused_applies(self, X3: torch.Tensor) -> bool:
        m = 0 if self.X_pending is None else self.X_pending.shape[-2]
        return X3.is_cuda and m <= kernels.GIBBON_MMAX

    def _fused(self, X3: torch.Tensor) -> torch.Tensor:
        from . import ops  # noqa: F401  (torch.ops.bo registration)
        mu, var, A = self._moments(X3)
        return torch.ops.bo.gibbon(mu, var, A, self._Binv if A is not None else None,
                                   self._fstar(), self._tau2, self.weight)

    def _generic(self, X3: torch.Tensor) -> torch.Tensor:
        mu, var, A = self._moments(X3)
        return _gibbon_chain(mu, var, self._fstar(), self._tau2, self.weight, A, self._Binv)


# -- active learning: integrated posterior variance ---------------------------------------
NIPV_GENERIC_TRANSIENT = 1 << 24  # doubles of one array of a chunk of the generic route


def _nipv_value(Sigma, G, tau2: float, vbar: float, N: int, chol=None):
    """-(vbar - tr((Sigma + tau2 I)^{-1} G) / N) (...), from Sigma and G
    (... x q x q): the integrated posterior variance after observing the q
    points with noise tau2, negated (transformed outcome space).  ``chol``
    factors Sigma + tau2 I (default torch.linalg.cholesky); the trace is taken
    through two triangular solves, tr(L^{-1} G L^{-T})."""
    q = Sigma.shape[-1]
    M = Sigma + tau2 * torch.eye(q, dtype=Sigma.dtype, device=Sigma.device)
    L = torch.linalg.cholesky(M) if chol is None else chol(M)
    W = torch.linalg.solve_triangular(L, G, upper=False)
    W = torch.linalg.solve_triangular(L, W.mT, upper=False)
    return W.diagonal(dim1=-2, dim2=-1).sum(dim=-1) / N - vbar


class _NipvMember:
    """What qNegIntegratedPosteriorVariance keeps of one single-output member."""
    __slots__ = ("model", "Z_scaled", "Xt_scaled", "V", "vbar", "tau2", "hyper", "ystd", "w2")


class qNegIntegratedPosteriorVariance(AcquisitionFunction):
    """Negative integrated posterior variance (acquisition/active_learning.py:
    40-126) for exact GPs:

        acq(X) = -mean_z var(z | data, observations at X with noise tau2)

    over the N integration points ``mc_points`` (N x d).  The reference builds
    ``model.fantasize(X)`` per t-batch and evaluates its posterior at the
    integration points.  No fantasy model is built here: observing q points is
    a rank-q correction of the current posterior,

        acq(X) = -ystd^2 (vbar - tr((Sigma(X, X) + tau2 I)^{-1} G(X)) / N),
        G(X) = C C^T,  C = [cov(f(x_i), f(z) | data)]  (q x N),

    with vbar the current mean variance over the integration points (fixed at
    construction), tau2 the noise level (the mean of the fixed variances for a
    fixed-noise likelihood, as ``Model.fantasize`` passes it), everything in the
    model's transformed outcome space.  The fused route (X on the device, d <=
    kernels.NIPV_DMAX, q with pending points <= kernels.NIPV_QMAX) forms C on
    the matrix cores and contracts it to G without storing it (``bo::nipv_gram``);
    the generic route takes C from the joint posterior of X and chunks of the
    integration points and applies the same formula in torch.

    ``sampler`` is accepted and kept for the reference's signature; it is not
    used, because the posterior variance of an exact GP does not depend on the
    fantasised values.  A multi-output ``SingleTaskGP`` or a ``ModelListGP`` of
    single-output ``SingleTaskGP``s needs a ``ScalarizedPosteriorTransform``:
    the outputs are independent, so acq = sum_t w_t^2 acq_t (the offset drops
    out)."""

    def __init__(self, model, mc_points: torch.Tensor, sampler=None, posterior_transform=None,
                 X_pending=None):
        from .models import ModelListGP, SaasFullyBayesianSingleTaskGP, SingleTaskGP
        from .objective import ScalarizedPosteriorTransform
        super().__init__(model)
        if isinstance(model, SaasFullyBayesianSingleTaskGP):
            raise UnsupportedError("qNegIntegratedPosteriorVariance: SaasFullyBayesianSingleTaskGP "
                                   "is not supported (SingleTaskGP, or a ModelListGP of "
                                   "single-output SingleTaskGPs, is)")
        if isinstance(model, ModelListGP) or (isinstance(model, SingleTaskGP)
                                              and model.num_outputs > 1):
            members = list(model.models)
        elif isinstance(model, SingleTaskGP):
            members = [model]
        else:
            raise UnsupportedError(f"qNegIntegratedPosteriorVariance: {type(model).__name__} is not "
                                   "supported (SingleTaskGP, or a ModelListGP of single-output "
                                   "SingleTaskGPs, is)")
        for mm in members:
            if not isinstance(mm, SingleTaskGP) or isinstance(mm, SaasFullyBayesianSingleTaskGP) \
                    or mm.num_outputs != 1:
                raise UnsupportedError("qNegIntegratedPosteriorVariance: every member of a "
                                       "ModelListGP must be a single-output SingleTaskGP")
        if posterior_transform is None:
            if len(members) > 1:
                raise UnsupportedError("Must specify a posterior transform when using a "
                                       "multi-output model (a ScalarizedPosteriorTransform is "
                                       "supported).")
            weights = [1.0]
        elif isinstance(posterior_transform, ScalarizedPosteriorTransform):
            weights = [float(w) for w in posterior_transform.weights.detach().reshape(-1).tolist()]
            if len(weights) != len(members):
                raise ValueError(f"qNegIntegratedPosteriorVariance: {len(weights)} weights for a "
                                 f"model with {len(members)} outputs")
        else:
            raise UnsupportedError("qNegIntegratedPosteriorVariance: only a "
                                   "ScalarizedPosteriorTransform is supported as "
                                   "`posterior_transform`")
        if model.training or any(mm.training for mm in members):
            raise UnsupportedError("qNegIntegratedPosteriorVariance needs a model in eval mode "
                                   "(model.eval()): the integration points are conditioned on the "
                                   "trained model's prediction caches")
        d = members[0].train_inputs[0].shape[-1]
        if mc_points.dim() != 2 or mc_points.shape[-1] != d or mc_points.shape[0] < 1:
            raise UnsupportedError("qNegIntegratedPosteriorVariance: mc_points must be `N x "
                                   f"{d}` without batch dimensions, got {tuple(mc_points.shape)}")
        self.posterior_transform = posterior_transform
        self.sampler = sampler  # unused: the variance does not depend on the fantasies
        self.register_buffer("mc_points", mc_points)
        self._route = None  # None: by size; "fused" / "generic": forced (tests, tools)
        self._members = [self._condition(mm, mc_points, w) for mm, w in zip(members, weights)]
        self.set_X_pending(X_pending)

    @staticmethod
    def _condition(model, mc_points, w: float) -> _NipvMember:
        """One member's constants, once: the scaled integration points, V =
        A^{-1} o k(Xt, Z) against the cached L^{-1}, the current mean variance
        over Z, the noise level, the hyperparameters and the outcome scale."""
        from .posteriors import posterior_moments
        m = _NipvMember()
        with torch.no_grad():
            cache = model.prediction_cache()
            _, ystd = model.outcome_stats()
            n, dev = cache.n, cache.Xt.device
            Z = mc_points.detach().to(device=dev, dtype=torch.float64).contiguous()
            N, d = Z.shape
            _, cov = posterior_moments(model, Z.unsqueeze(-2))
            m.model = model
            m.vbar = float(cov.reshape(-1).mean()) / (ystd * ystd)
            m.tau2 = float(cache.noise)  # the level, or the mean of the fixed variances
            m.Z_scaled = (Z / cache.lengthscale).contiguous()
            m.Xt_scaled = (cache.Xt / cache.lengthscale).contiguous() if n else None
            m.V = None
            if n and d <= kernels.NIPV_DMAX:
                K = kernels.covar_matrix(Z, cache.Xt, cache.lengthscale, cache.kind,
                                         cache.outputscale)
                E = K.t().contiguous()  # n x N
                ld = cache.Linv.shape[1]
                T = torch.empty(n, N, dtype=torch.float64, device=dev)
                Vt = torch.empty(n, N, dtype=torch.float64, device=dev)
                # the leading n x n block of the (padded) L^{-1}, read in place
                kernels.gemm_strided(n, N, n, cache.Linv, ld, 0, E, N, 0, T, N, 0, 1)
                kernels.gemm_strided(n, N, n, cache.Linv, ld, 0, T, N, 0, Vt, N, 0, 1, transA=True)
                m.V = Vt.t().contiguous()
            m.hyper = (cache.lengthscale, int(cache.kind), float(cache.outputscale))
            m.ystd = float(ystd)
            m.w2 = float(w) * float(w)
        return m

    @staticmethod
    def _chol(M: torch.Tensor) -> torch.Tensor:
        from .posteriors import _CholJitter
        return _CholJitter.apply(M) if torch.is_grad_enabled() and M.requires_grad \
            else kernels.chol_jitter(M)

    def _fused(self, X3: torch.Tensor) -> torch.Tensor:
        from . import ops  # noqa: F401  (torch.ops.bo registration)
        from .posteriors import posterior_moments
        B, q, d = X3.shape
        N = self.mc_points.shape[0]
        X2 = X3.reshape(B * q, d)
        acq = None
        for m in self._members:
            _, cov = posterior_moments(m.model, X3)
            ls, kind, o = m.hyper
            G = torch.ops.bo.nipv_gram(X2, q, ls, m.Xt_scaled if m.V is not None else None,
                                       m.Z_scaled, m.V, kind, o, 0)
            a = _nipv_value(cov / (m.ystd * m.ystd), G, m.tau2, m.vbar, N, self._chol)
            a = (m.w2 * m.ystd * m.ystd) * a
            acq = a if acq is None else acq + a
        return acq

    def _generic(self, X3: torch.Tensor) -> torch.Tensor:
        from .posteriors import posterior_moments
        B, q, d = X3.shape
        Z = self.mc_points.to(device=X3.device, dtype=torch.float64)
        N = Z.shape[0]
        acq = None
        for m in self._members:
            s2 = m.ystd * m.ystd
            # chunks of the integration points: the B (q + nc) x n kernel rows and the
            # B x (q + nc)^2 covariance of one chunk stay within the transient bound
            n = m.model.train_inputs[0].shape[0]
            nc = max(16, min(NIPV_GENERIC_TRANSIENT // (B * max(n, 1)),
                             int(math.sqrt(NIPV_GENERIC_TRANSIENT / B))) - q)
            Sigma, G = None, 0.0
            for z0 in range(0, N, nc):
                Zc = Z[z0:z0 + nc]
                _, cov = posterior_moments(m.model,
                                           torch.cat([X3, Zc.expand(B, *Zc.shape)], dim=-2))
                if Sigma is None:
                    Sigma = cov[:, :q, :q] / s2
                C = cov[:, :q, q:] / s2
                G = G + C @ C.mT
            a = (m.w2 * s2) * _nipv_value(Sigma, G, m.tau2, m.vbar, N, self._chol)
            acq = a if acq is None else acq + a
        return acq

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = t_batch_mode(X)
        if X.dtype != torch.float64:  # the model computes in fp64; the value returns in X's dtype
            return self.forward(X.to(torch.float64)).to(X.dtype)
        batch = X.shape[:-2]
        X = self._concat_pending(X)
        q, d = X.shape[-2], X.shape[-1]
        X3 = X.reshape(-1, q, d)
        fused = (X.is_cuda and d <= kernels.NIPV_DMAX and q <= kernels.NIPV_QMAX) \
            if self._route is None else self._route == "fused"
        acq = self._fused(X3) if fused else self._generic(X3)
        return acq.reshape(batch)


# -- qNEI -------------------------------------------------------------------------------
def prune_inferior_points(model, X, objective=None, posterior_transform=None, constraints=None,
                          num_samples: int = 2048, max_frac: float = 1.0, sampler=None,
                          marginalize_dim=None):
    """acquisition/utils.py:245-349: keep the points with non-zero empirical
    probability of being the best (feasible) point under ``num_samples`` joint
    posterior samples.  The joint n x n posterior, its jittered Cholesky and the
    sample GEMM run on the device."""
    if marginalize_dim is None and getattr(model, "_is_ensemble", False):
        marginalize_dim = MCMC_DIM
    if X.ndim > 2:
        raise UnsupportedError("Batched inputs `X` are currently unsupported by prune_inferior_points")
    if X.size(-2) == 0:
        raise ValueError("X must have at least one point.")
    if max_frac <= 0 or max_frac > 1.0:
        raise ValueError(f"max_frac must take values in (0, 1], is {max_frac}")
    max_points = math.ceil(max_frac * X.size(-2))
    with torch.no_grad():
        posterior = model.posterior(X=X, posterior_transform=posterior_transform)
        if sampler is None:
            sampler = get_sampler(posterior, sample_shape=torch.Size([num_samples]))
        samples = sampler(posterior)
        if objective is None:
            objective = IdentityMCObjective()
        obj_vals = objective(samples, X=X)
    if obj_vals.ndim > 2:
        if obj_vals.ndim == 3 and marginalize_dim is not None:
            if marginalize_dim < 0:
                marginalize_dim = 1 + (marginalize_dim % obj_vals.ndim)
            obj_vals = obj_vals.mean(dim=marginalize_dim)
        else:
            raise UnsupportedError("Models with multiple batch dims are currently unsupported by"
                                   " prune_inferior_points.")
    infeas = ~compute_feasibility_indicator(constraints=constraints, samples=samples,
                                            marginalize_dim=marginalize_dim)
    if infeas.any():
        obj_vals[infeas] = obj_vals.min() - 1
    is_best = torch.argmax(obj_vals, dim=-1)
    idcs, counts = torch.unique(is_best, return_counts=True)
    if len(idcs) > max_points:
        counts, order_idcs = torch.sort(counts, descending=True)
        idcs = order_idcs[:max_points]  # reference quirk kept (utils.py:345-347)
    return X[idcs]


MCMC_DIM = -3  # models/fully_bayesian.py


def supports_cache_root(model, posterior_transform=None) -> bool:
    """acquisition/cached_cholesky.py:34-51, for the models built here: exact
    GPs (SingleTaskGP, the SAAS ensemble) with a linear (Standardize) outcome
    transform.  A ModelListGP is cached here only under a scalarising posterior
    transform (its joint root is then single-output); without one the full
    joint samples are drawn instead."""
    if hasattr(model, "models"):
        return posterior_transform is not None and all(supports_cache_root(m) for m in model.models)
    return hasattr(model, "prediction_cache") or getattr(model, "_is_fully_bayesian", False)


def sample_cached_cholesky(posterior, baseline_L: torch.Tensor, q: int, base_samples: torch.Tensor,
                           sample_shape: torch.Size, max_tries: int = 6) -> torch.Tensor:
    """utils/low_rank.py:85-173 for a single-output joint posterior over
    (X_baseline, X): the q new rows of the joint Cholesky from the cached
    baseline root (bl = K_qb L_bb^{-T}, br = psd_safe_cholesky(K_qq - bl bl^T)),
    then samples = mean_q + [bl, br] Z (Z the joint base samples).  Raises
    NanError on non-finite samples."""
    from .exceptions import NanError
    from .posteriors import _CholJitter
    mvn = posterior.distribution
    cov = mvn.covariance_matrix
    bottom = cov[..., -q:, :]
    bl, br = bottom.split([bottom.shape[-1] - q, q], dim=-1)
    bl_chol = torch.linalg.solve_triangular(baseline_L.to(bl), bl.transpose(-2, -1),
                                            upper=False).transpose(-2, -1)
    br_to_chol = br - bl_chol @ bl_chol.transpose(-2, -1)
    if torch.is_grad_enabled() and br_to_chol.requires_grad:
        br_chol = _CholJitter.apply(br_to_chol)
    else:
        br_chol = kernels.chol_jitter(br_to_chol, max_tries=max_tries)
    new_Lq = torch.cat([bl_chol, br_chol], dim=-1)                     # batch x q x (r + q)
    mean = mvn.mean[..., -q:]                                          # batch x q
    n_tot = new_Lq.shape[-1]
    Z = base_samples.reshape(*sample_shape, -1, n_tot)
    if Z.shape[len(sample_shape)] != 1:
        raise UnsupportedError("sample_cached_cholesky here takes base samples shared over t-batches")
    Z = Z.reshape(-1, n_tot).to(new_Lq)                               # S' x (r + q)
    f = torch.matmul(Z, new_Lq.reshape(-1, q, n_tot).mT)              # B' x S' x q
    f = f.permute(1, 0, 2) + mean.reshape(1, -1, q)
    res = f.reshape(*sample_shape, *mean.shape[:-1], q, 1)
    bad_nan, bad_inf = bool(torch.isnan(res).any()), bool(torch.isinf(res).any())
    if bad_nan or bad_inf:
        what = " and ".join(w for w, b in (("nans", bad_nan), ("infs", bad_inf)) if b)
        raise NanError(f"Samples contain {what}.")
    return res


class _CachedBaselineRoot:
    """Cached-root state of one exact-GP output over X_baseline
    (acquisition/cached_cholesky.py:94-120, utils/low_rank.py:85-173) and the
    fused-path pieces built on it.

    Construction: the baseline posterior (outcome space), its jittered
    Cholesky L_rr with inverse, the baseline samples mean_b + Z_base L_rr^T, and
    P_b = L_rr^{-1} K(X_b, X_tr) L^{-T} (r x np), Q_b = P_b U^T, the scaled
    baseline inputs.  forward(): T = L_rr^{-1} Sigma'(X_b, X) = s^2 (L_rr^{-1}
    K_bX - P_b R^T) (two MFMA GEMMs) and the sample term F = Z_base T.
    backward(): dT = Z_base^T dF - T G (G = dSigma + dSigma^T) pushed through
    both GEMMs to dK*x (E = -s^2 dT^T Q_b) and d K_bX (s^2 L_rr^{-T} dT)."""

    def __init__(self, model, X_baseline, Z_base, posterior_transform=None):
        r = X_baseline.shape[-2]
        self.Z_base = Z_base
        with torch.no_grad():
            post = model.posterior(X_baseline, posterior_transform=posterior_transform)
            mean_b = post.distribution.mean.reshape(1, r)
            cov_b = post.distribution.covariance_matrix.reshape(r, r)
            L_rr, Linv_rr, _ = kernels.cholesky_with_inverse(cov_b)
            base = kernels.sample_mvn(mean_b, L_rr.unsqueeze(0).contiguous(), Z_base)
            self.samples = base.reshape(Z_base.shape[0], r)
            self.L = L_rr.contiguous()
            self.Linv = Linv_rr.contiguous()
            self.fused_ready = False
            if (hasattr(model, "prediction_cache") and X_baseline.shape[-1] <= kernels.DP
                    and _cache_dim_ok(model, X_baseline)):
                cache = model.prediction_cache()
                Kb = kernels.covar_matrix(X_baseline.contiguous(), cache.Xt, cache.lengthscale,
                                          cache.kind, cache.outputscale)
                R_b = kernels.gemm(Kb, cache.U[: cache.n, : cache.n], flags=_lib.GEMM_B_UPPER)
                P_b = torch.zeros(r, cache.np, dtype=torch.float64, device=Kb.device)
                P_b[:, : cache.n] = kernels.gemm(self.Linv, R_b, flags=_lib.GEMM_A_LOWER)
                self.P_b = P_b
                # Q_b = P_b U^T = L_rr^{-1} K(X_b, X_tr) A^{-1}  (gradient of the
                # cross-covariance through R = K*x L^{-T})
                self.Q_b = kernels.gemm(P_b, cache.U, transB=True, flags=_lib.GEMM_B_LOWER)
                self.Xb_scaled = torch.zeros(r, kernels.DP, dtype=torch.float64, device=Kb.device)
                self.Xb_scaled[:, : cache.d] = X_baseline / cache.lengthscale
                self.fused_ready = True

    def forward(self, cache, pp, ystd, F_out=None):
        """T and F (F written into F_out when given: the stacked qEHVI input)."""
        s2 = ystd * ystd
        ones = self.__dict__.get("_ones")
        if ones is None or ones.device != pp.Xq.device:
            ones = self._ones = torch.ones(kernels.DP, dtype=torch.float64, device=pp.Xq.device)
        Kbx = kernels.covar_matrix(self.Xb_scaled, pp.Xq, ones, cache.kind, cache.outputscale)
        T = kernels.gemm(self.Linv, Kbx, alpha=s2, flags=_lib.GEMM_A_LOWER)
        if pp.Cx is not None:   # P_b R^T = Q_b K*x^T, fused into the posterior pass
            T.add_(pp.Cx, alpha=-s2)
        else:
            T = kernels.gemm(self.P_b, pp.Rt, alpha=-s2, beta=1.0, C=T)
        F = kernels.gemm(self.Z_base, T, C=F_out)
        return T, F

    def backward(self, cache, pp, W, dmean, dcov, dF, T, ystd, dX=None):
        s2 = ystd * ystd
        B, q, Qp, nrows = pp.B, pp.q, pp.Qp, pp.nrows_pad
        r = self.Linv.shape[0]
        dT = kernels.gemm(self.Z_base, dF, transA=True)            # r x nrows_pad
        G = (dcov + dcov.mT).contiguous()                          # B x q x q
        kernels.gemm_strided(r, q, q, T, nrows, Qp, G, q, q * q, dT, nrows, Qp, B,
                             alpha=-1.0, beta=1.0)                  # dT_b -= T_b G_b
        E = kernels.gemm(dT, self.Q_b, transA=True, alpha=-s2)     # nrows_pad x np
        dKbx = kernels.gemm(self.Linv, dT, transA=True, alpha=s2, flags=_lib.GEMM_A_UPPER)
        dX = kernels.post_backward(cache, pp, W, dmean, dcov, ystd, E=E, dX=dX)
        return kernels.post_backward(cache, pp, None, None, None, ystd, E=dKbx.mT.contiguous(),
                                     Xt_scaled=self.Xb_scaled, n=r, dX=dX)


class qNoisyExpectedImprovement(MCAcquisitionFunction):
    """MC batch noisy EI (acquisition/monte_carlo.py:417-645, cached_cholesky.py:
    63-186, utils/low_rank.py:85-173):
    qNEI(X) = E[max(max_j Y_j - max_i Y_base_i, 0)].

    ``cache_root=True`` (default): the baseline posterior, its jittered root
    L_rr and the baseline samples are computed once; ``base_sampler`` keeps the
    baseline base samples and every forward reuses them as the leading columns
    of the joint (r + q) draw (sampling/normal.py:68-131).  For a SingleTaskGP
    with the identity objective, q <= 16 and d <= 8 the forward is the fused
    chain (post_partials with the cross term, T = L_rr^{-1} Sigma'(X_b, X),
    F = Z_b T, qmc_finalize(QNEI)); otherwise the joint posterior over
    (X_baseline, X) goes through sample_cached_cholesky.  A NotPSD/NaN failure
    of either falls back to standard joint sampling with a BotorchWarning
    (cached_cholesky.py:141-165).  ``cache_root=False``: every forward samples
    the joint (r + q) posterior and takes the baseline best from those samples.
    """

    _admits_multitask = True

    _fused_mode = _lib.QMC_QNEI

    def __init__(self, model, X_baseline, sampler=None, objective=None, posterior_transform=None,
                 X_pending=None, prune_baseline=True, cache_root=True, constraints=None,
                 eta=1e-3, marginalize_dim=None):
        super().__init__(model, sampler, objective, posterior_transform, X_pending,
                         constraints=constraints, eta=eta)
        self._init_baseline(model, X_baseline, prune_baseline, cache_root, marginalize_dim)

    def _init_baseline(self, model, X_baseline, prune_baseline, cache_root, marginalize_dim):
        # outcome constraints on the fused route (per-member cached roots, _FusedSOFeas):
        # a single Sobol sampler; on a model list it must be given (without one the
        # generic route builds a ListSampler, which keeps that route)
        wplan = _weighted_so_plan(self) if cache_root else None
        if wplan is not None and not (
                X_baseline.ndim == 2 and X_baseline.shape[-1] <= kernels.DP and X_baseline.is_cuda
                and X_baseline.shape[-2] > 0 and len(self.sample_shape) == 1
                and (type(self.sampler) is SobolQMCNormalSampler
                     or (self.sampler is None and not hasattr(model, "models")))):
            wplan = None
        self._roots = None
        if cache_root and wplan is None and not supports_cache_root(model, self.posterior_transform):
            warnings.warn("`cache_root` is only supported here for exact GPs (or a ModelListGP "
                          f"under a scalarising posterior transform); got {type(model)}. "
                          "Setting `cache_root = False`.", RuntimeWarning)
            cache_root = False
        self._cache_root = cache_root
        if prune_baseline:
            X_baseline = prune_inferior_points(model, X_baseline, objective=self.objective,
                                               posterior_transform=self.posterior_transform,
                                               constraints=self._constraints,
                                               marginalize_dim=marginalize_dim)
        self.register_buffer("X_baseline", X_baseline)
        self.baseline_samples = None
        self.baseline_obj = None
        self.base_sampler = None
        self._root = None
        self._zq = None
        if not self._cache_root:
            return
        self.q_in = -1
        r = X_baseline.shape[-2]
        fusable = (hasattr(model, "prediction_cache") and type(self.objective) is IdentityMCObjective
                   and self.posterior_transform is None and self._constraints is None
                   and X_baseline.ndim == 2 and X_baseline.shape[-1] <= kernels.DP
                   and X_baseline.is_cuda and len(self.sample_shape) == 1
                   and _cache_dim_ok(model, X_baseline))
        with torch.no_grad():
            if wplan is not None:
                # qNEHVI's convention: member t's baseline base samples are the
                # columns i Mt + t of the (r Mt)-dimensional draw
                sampler = self._ensure_sampler()
                Mt = len(wplan.members)
                if Mt == 1:   # the sampler's own S x r draw, kept for the base sampler
                    sampler._construct_base_samples(ShapeOnlyPosterior(torch.Size(), r, X_baseline.device))
                    Zb = sampler.base_samples.reshape(-1, r, 1)
                else:
                    Zb = kernels.sobol_normal(r * Mt, sampler.sample_shape.numel(), sampler.seed,
                                              X_baseline.device).view(-1, r, Mt)
                self._roots = [_CachedBaselineRoot(mm, X_baseline, Zb[:, :, t].contiguous())
                               for t, mm in enumerate(wplan.members)]
                baseline_samples = torch.stack([rt.samples for rt in self._roots], dim=-1).reshape(
                    *self.sample_shape, r, Mt)
                baseline_L = self._roots[0].L if Mt == 1 else None
                self._zqm = {}
            elif fusable:
                # the sampler's own base samples over X_baseline (S x r), then the
                # device root + fused precomputations on them
                sampler = self._ensure_sampler()
                sampler._construct_base_samples(ShapeOnlyPosterior(torch.Size(), r, X_baseline.device))
                Z_base = sampler.base_samples.reshape(-1, r).contiguous()
                self._root = _CachedBaselineRoot(model, X_baseline, Z_base)
                baseline_samples = self._root.samples.reshape(*self.sample_shape, r, 1)
                baseline_L = self._root.L
            else:
                posterior = self.model.posterior(X_baseline, posterior_transform=self.posterior_transform)
                baseline_samples = self.get_posterior_samples(posterior)
                baseline_L = posterior.distribution.scale_tril
            baseline_obj = self.objective(baseline_samples, X=X_baseline)
        self.base_sampler = copy.deepcopy(self.sampler)
        self.baseline_samples = baseline_samples
        self.baseline_obj = baseline_obj
        self.register_buffer("_baseline_best_f", self._compute_best_feasible_objective(
            samples=baseline_samples, obj=baseline_obj).contiguous())
        self._baseline_L_t = baseline_L

    @property
    def _baseline_L(self) -> torch.Tensor:
        return self._baseline_L_t

    @_baseline_L.setter
    def _baseline_L(self, L: torch.Tensor) -> None:
        # a replaced root invalidates the fused precomputations built on the old one
        self._baseline_L_t = L
        self._root = None

    @property
    def _fused_ready(self) -> bool:
        return self._root is not None and self._root.fused_ready

    def _compute_best_feasible_objective(self, samples, obj):
        """monte_carlo.py:628-645."""
        return compute_best_feasible_objective(samples=samples, obj=obj,
                                               constraints=self._constraints, model=self.model,
                                               objective=self.objective,
                                               posterior_transform=self.posterior_transform,
                                               X_baseline=self.X_baseline)

    def compute_best_f(self, obj: torch.Tensor) -> torch.Tensor:
        """monte_carlo.py:540-563: the (cached or per-forward) best feasible
        baseline objective, viewed against obj without its q dimension."""
        if self._cache_root:
            val = self._baseline_best_f
        else:
            val = self._compute_best_feasible_objective(samples=self.baseline_samples,
                                                        obj=self.baseline_obj)
        n_sample_dims = len(self.sample_shape)
        view_shape = torch.Size([*val.shape[:n_sample_dims],
                                 *(1,) * (obj.ndim - val.ndim - 1),
                                 *val.shape[n_sample_dims:]])
        return val.view(view_shape).to(obj)

    def _sample_forward(self, obj: torch.Tensor) -> torch.Tensor:
        """monte_carlo.py:565-575."""
        return (obj - self.compute_best_f(obj).unsqueeze(-1)).clamp_min(0)

    # -- joint base samples (cached_cholesky.py:167-186) ----------------------------------
    def _set_sampler(self, q_in: int, posterior) -> None:
        if self.q_in != q_in and self.base_sampler is not None:
            self.sampler._update_base_samples(posterior=posterior, base_sampler=self.base_sampler)
            self.q_in = q_in
            self._zq = None

    def _base_samples_q(self, q: int, device) -> torch.Tensor:
        """The q new columns of the joint (r + q) base samples (S x q) for the
        fused path; the leading r columns are the cached baseline ones."""
        r = self.X_baseline.shape[-2]
        S = self.sample_shape.numel()
        bs = self.sampler.base_samples
        if self.q_in != q or bs is None or bs.numel() != S * (r + q):
            self.q_in = -1
            self._set_sampler(q, ShapeOnlyPosterior(torch.Size([1]), r + q, device))
            bs = self.sampler.base_samples
        key = (q, bs.data_ptr(), bs._version)
        if self._zq is None or self._zq[0] != key:
            self._zq = (key, bs.reshape(S, r + q)[:, r:].contiguous())
        return self._zq[1]

    def _get_f_X_samples(self, posterior, q_in: int) -> torch.Tensor:
        """cached_cholesky.py:122-165."""
        if self._cache_root and self._baseline_L is not None:
            try:
                return sample_cached_cholesky(posterior=posterior, baseline_L=self._baseline_L,
                                              q=q_in, base_samples=self.sampler.base_samples,
                                              sample_shape=self.sampler.sample_shape)
            except (NanError, NotPSDError):
                warnings.warn("Low-rank cholesky updates failed due NaNs or due to an "
                              "ill-conditioned covariance matrix. Falling back to standard "
                              "sampling.", BotorchWarning)
        samples = self.get_posterior_samples(posterior)
        return samples[..., -q_in:, :]

    def _joint_posterior(self, X: torch.Tensor):
        Xb = self.X_baseline
        X_full = torch.cat([Xb.expand(*X.shape[:-2], *Xb.shape[-2:]), X], dim=-2)
        return X_full, self.model.posterior(X_full, posterior_transform=self.posterior_transform)

    def _get_samples_and_objectives(self, X: torch.Tensor):
        """monte_carlo.py:577-626."""
        q = X.shape[-2]
        X_full, posterior = self._joint_posterior(X)
        if not self._cache_root:
            samples_full = self.get_posterior_samples(posterior)
            samples = samples_full[..., -q:, :]
            obj_full = self.objective(samples_full, X=X_full)
            self.baseline_obj, obj = obj_full[..., :-q], obj_full[..., -q:]
            self.baseline_samples = samples_full[..., :-q, :]
        else:
            self._set_sampler(q_in=q, posterior=posterior)
            samples = self._get_f_X_samples(posterior=posterior, q_in=q)
            obj = self.objective(samples, X=X_full[..., -q:, :])
        return samples, obj

    def _fallback_forward(self, X: torch.Tensor) -> torch.Tensor:
        """Standard joint sampling after a failed low-rank update of the fused path
        (cached_cholesky.py:147-165): the cached baseline best is kept."""
        q = X.shape[-2]
        X_full, posterior = self._joint_posterior(X)
        self._set_sampler(q_in=q, posterior=posterior)
        samples = self.get_posterior_samples(posterior)[..., -q:, :]
        obj = self.objective(samples, X=X)
        acqval = self._apply_constraints(self._sample_forward(obj), samples)
        return _ensemble_mean(self.model, self._sample_reduction(self._q_reduction(acqval)))

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = self._concat_pending(t_batch_mode(X))
        batch = X.shape[:-2]
        q, d = X.shape[-2], X.shape[-1]
        if self._fused_ready and self._fused_eligible(X):
            try:
                return _FusedQNEI.apply(X.reshape(-1, q, d), self).reshape(batch)
            except (NotPSDError, NanError):
                warnings.warn("Low-rank cholesky updates failed due NaNs or due to an "
                              "ill-conditioned covariance matrix. Falling back to standard "
                              "sampling.", BotorchWarning)
                return self._fallback_forward(X)
        if self._roots is not None and self._cache_root:
            plan = _weighted_so_route(self, X)
            if plan is not None:
                try:
                    acq = _FusedSOFeas.apply(X.reshape(-1, q, d).to(torch.float64), self, plan, None, None)
                    return acq.to(X.dtype).reshape(batch)
                except (NotPSDError, NanError):
                    warnings.warn("Low-rank cholesky updates failed due NaNs or due to an "
                                  "ill-conditioned covariance matrix. Falling back to standard "
                                  "sampling.", BotorchWarning)
                    return self._fallback_forward(X)
        return self._generic_forward(X)

    def _base_samples_members(self, q: int, Mt: int, device) -> torch.Tensor:
        """The q Mt new columns of the (r + q) Mt-dimensional Sobol draw (column
        p Mt + t for new point p, member t), behind the baseline's r Mt."""
        if q not in self._zqm:
            r = self.X_baseline.shape[-2]
            full = kernels.sobol_normal((r + q) * Mt, self.sampler.sample_shape.numel(),
                                        self.sampler.seed, device)
            self._zqm[q] = full[:, r * Mt:].contiguous()
        return self._zqm[q]


class _FusedQNEI(torch.autograd.Function):
    """qNEI value of B t-batches on the cached-root fused path, with its gradient.

    Forward: post_partials (+ R^T), T = L_rr^{-1} Sigma'(X_b, X) =
    s^2 (L_rr^{-1} K_bX - P_b R^T), F = Z_b T, qmc_finalize(QNEI) on
    Sigma_cond = Sigma' - T^T T.
    Backward (utils/low_rank.py:85-173 differentiated):
      qmc_backward -> d mu', d Sigma_cond, dF;   dT = Z_b^T dF - T (G_b), G_b = dS + dS^T
      d K*x += -s^2 dT^T Q_b   (Q_b = P_b U^T, through R = K*x L^{-T})
      d K_bX = s^2 L_rr^{-T} dT (through K(X_b, X))
    and post_backward reduces both through dk/dx."""

    @staticmethod
    def forward(ctx, X3, acqf):
        model = acqf.model
        cache = model.prediction_cache()
        ymean, ystd = model.outcome_stats()
        q = X3.shape[-2]
        need_grad = ctx.needs_input_grad[0]
        pp = kernels.post_partials(cache, X3.detach(), store_R=need_grad, cross=acqf._root.Q_b)
        T, F = acqf._root.forward(cache, pp, ystd)
        Zq = acqf._base_samples_q(q, X3.device)
        lp = getattr(acqf, "_log_params", None)
        out = kernels.qmc_finalize(cache, pp, acqf._fused_mode, ymean, ystd, Z=Zq,
                                   best_f_s=acqf._baseline_best_f, want_mean=need_grad,
                                   want_cov=False, want_L=need_grad, T=T, F=F, log_params=lp)
        kernels._raise_not_psd(out["info"], out["jitter"], type(acqf).__name__)
        if need_grad:
            ctx.acqf, ctx.cache, ctx.pp, ctx.ystd = acqf, cache, pp, ystd
            ctx.lp, ctx.acq = lp, out["acq"].detach().clone()
            ctx.T, ctx.F, ctx.Zq = T, F, Zq
            ctx.mean, ctx.L = out["mean"], out["L"]
            ctx.W = kernels.w_matrix(cache, pp)
        return out["acq"]

    @staticmethod
    def backward(ctx, dacq):
        acqf, cache, pp, ystd = ctx.acqf, ctx.cache, ctx.pp, ctx.ystd
        dmean, dcov, dF = kernels.qmc_backward(acqf._fused_mode, ctx.mean, ctx.L, ctx.Zq,
                                               dacq.contiguous(), best_f_s=acqf._baseline_best_f,
                                               F=ctx.F, acq_fwd=ctx.acq, log_params=ctx.lp)
        dX = acqf._root.backward(cache, pp, ctx.W, dmean, dcov, dF, ctx.T, ystd)
        return dX, None


# -- LogEI family ---------------------------------------------------------------------
def _check_tau(tau, name: str):
    """acquisition/logei.py:537-544."""
    if isinstance(tau, torch.Tensor) and tau.numel() != 1:
        raise ValueError(name + f" is not a scalar: {tau.numel() = }.")
    if not (tau > 0):
        raise ValueError(name + f" is non-positive: {tau = }.")
    return tau


class qLogExpectedImprovement(qExpectedImprovement):
    """MC batch log expected improvement (acquisition/logei.py:71-234):
    qLogEI(X) = logmeanexp_s q_reduce_j log_soft_clamp(Y_sj - best_f), with
    q_reduce = fatmax(tau_max) and log_soft_clamp = log_fatplus(tau_relu) when
    fat (default), else smooth_amax / log_softplus; constraints add the
    log-feasibility (fatmoid when fat).

    Fused path: bo_qmc_finalize in BO_QMC_QLOGEI mode (the same post_partials
    posterior and q x q root as qEI; only the per-sample reduction differs),
    backward through bo_qmc_backward's dense log-mode weights."""

    _log = True

    def __init__(self, model, best_f, sampler=None, objective=None, posterior_transform=None,
                 X_pending=None, constraints=None, eta=1e-3, fat: bool = True,
                 tau_max: float = TAU_MAX, tau_relu: float = TAU_RELU):
        super().__init__(model, best_f, sampler, objective, posterior_transform, X_pending,
                         constraints=constraints, eta=eta)
        self.tau_max = _check_tau(tau_max, "tau_max")
        self.tau_relu = _check_tau(tau_relu, "tau_relu")
        self._fat = fat
        self._log_params = (int(bool(fat)), float(tau_relu), float(tau_max))

    def _sample_forward(self, obj: torch.Tensor) -> torch.Tensor:
        """logei.py:219-234."""
        return log_improvement(obj, self.best_f, tau=self.tau_relu, fat=self._fat)

    def _q_reduction(self, acqval: torch.Tensor) -> torch.Tensor:
        return (fatmax if self._fat else smooth_amax)(acqval, dim=-1, tau=self.tau_max)

    def _sample_reduction(self, acqval: torch.Tensor) -> torch.Tensor:
        return logmeanexp(acqval, dim=tuple(range(len(self.sample_shape))))

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = self._concat_pending(t_batch_mode(X))
        batch = X.shape[:-2]
        q, d = X.shape[-2], X.shape[-1]
        if self._fused_eligible(X) and self.best_f.numel() == 1:
            sampler = self._ensure_sampler()
            Z = sampler.base_samples_2d(q, X.device)
            acq = _fused_mc(X.reshape(-1, q, d), self, _lib.QMC_QLOGEI,
                            _host_scalar(self, "best_f"), None, Z)
            return acq.reshape(batch)
        if self._constraints is not None:
            acq = _weighted_qei_forward(self, X)
            if acq is not None:
                return acq
        return self._generic_forward(X)


class qLogNoisyExpectedImprovement(qNoisyExpectedImprovement):
    """MC batch log noisy expected improvement (acquisition/logei.py:236-507):
    the qNEI samples (cached root or full joint, as qNoisyExpectedImprovement)
    under the LogEI reductions against the per-sample baseline best.  Unlike
    qNEI, ``prune_baseline`` defaults to False (logei.py:270).  Fused path:
    bo_qmc_finalize / bo_qmc_backward in BO_QMC_QLOGNEI mode."""

    _log = True
    _fused_mode = _lib.QMC_QLOGNEI

    def __init__(self, model, X_baseline, sampler=None, objective=None, posterior_transform=None,
                 X_pending=None, constraints=None, eta=1e-3, fat: bool = True,
                 prune_baseline: bool = False, cache_root: bool = True,
                 tau_max: float = TAU_MAX, tau_relu: float = TAU_RELU, marginalize_dim=None):
        MCAcquisitionFunction.__init__(self, model, sampler, objective, posterior_transform,
                                       X_pending, constraints=constraints, eta=eta, fat=fat)
        self.tau_max = _check_tau(tau_max, "tau_max")
        self.tau_relu = _check_tau(tau_relu, "tau_relu")
        self._log_params = (int(bool(fat)), float(tau_relu), float(tau_max))
        self._init_baseline(model, X_baseline, prune_baseline, cache_root, marginalize_dim)

    def _sample_forward(self, obj: torch.Tensor) -> torch.Tensor:
        """logei.py:347-362."""
        return log_improvement(obj, self.compute_best_f(obj), tau=self.tau_relu, fat=self._fat)

    def _q_reduction(self, acqval: torch.Tensor) -> torch.Tensor:
        return (fatmax if self._fat else smooth_amax)(acqval, dim=-1, tau=self.tau_max)

    def _sample_reduction(self, acqval: torch.Tensor) -> torch.Tensor:
        return logmeanexp(acqval, dim=tuple(range(len(self.sample_shape))))


# -- qEHVI ---------------------------------------------------------------------------
def _qehvi_members_eager(acqf, X3: torch.Tensor):
    """Forward-only qEHVI through ONE native call (bo::qehvi_members_eager:
    every member's rows, K*x^T, posterior partials, finalisation and the
    qEHVI launch, issued from C++).  The members' ladder outcomes are
    deferred as the eager qEI's (a ring of pinned slots: the previous calls'
    outcomes are acted on here, kernels.check_ladder_status waits for all);
    with BO_SYNC_LADDER=1, one stream sync and the members' outcomes raised /
    warned in member order.
    None where it does not apply (graph capture; members of unequal shape or
    kernel; more than 8 members): the caller takes _FusedHVI."""
    dev = X3.device
    idx = kernels._dev_index(dev)
    if idx in kernels._CAPTURE:
        return None
    models = acqf.model.models
    if len(models) > 8:
        return None
    keys = prime_prediction_caches(models)
    key = (tuple(keys), idx)
    args = acqf.__dict__.get("_native_args")
    if args is None or args[0] != key:
        caches = [mm.prediction_cache(key=k) for mm, k in zip(models, keys)]
        c0 = caches[0]
        if not all(c.n == c0.n and c.np == c0.np and c.d == c0.d and c.kind == c0.kind
                   and c.U.numel() for c in caches):
            return None
        stats = [mm.outcome_stats() for mm in models]
        args = (key, [c.Xt_scaled for c in caches], [c.U for c in caches],
                [c.beta for c in caches], [c.lengthscale for c in caches],
                [float(c.outputscale) for c in caches], [float(c.constant) for c in caches],
                [float(m_) for m_, _ in stats], [float(s_) for _, s_ in stats], int(c0.kind),
                int(c0.n))
        acqf.__dict__["_native_args"] = args
    q = X3.shape[-2]
    Z = acqf._ensure_sampler().base_samples_2d(q * len(models), dev)
    lo, hi = acqf._cells(dev)
    defer = not kernels.SYNC_LADDER
    acq, status = _lib.torch_ops().qehvi_members_eager(
        X3.contiguous(), *args[1:], Z, lo, hi, kernels.kxt_cap(dev), defer)
    if defer:
        # as the eager qEI: the previous calls' outcomes, this one's pending
        # (kernels.check_ladder_status / the optimisers' end-of-loop poll)
        kernels.ladder_prev_outcome(status, idx, "qEHVI posterior root")
    else:
        kernels._stream_sync(dev)
        kernels.raise_status_words(status.tolist(), "qEHVI posterior root")
    return acq


class _MemberPosterior(NamedTuple):
    """What _member_posterior leaves for the reduction kernel and the backward."""
    mean: torch.Tensor              # M x B x q
    L: torch.Tensor                 # M x B x q x q
    F: Optional[torch.Tensor]       # M x S x nrows_pad cached-root sample term (None without roots)
    Qp: int                         # row stride of a t-batch in F (0 without roots)
    saved: list                     # per member (cache, pp, ystd, T, W); empty without a gradient
    batched: bool                   # the cached-root terms went as GEMMs batched over the members
    info: object                    # the members' ladder outputs, indexed by member
    jitter: object
    root_acqf: object               # the acquisition function that owns the roots, or None


def _member_posterior(members, X3, need_grad: bool, ladder, root_acqf=None) -> _MemberPosterior:
    """The posterior stage shared by the fused ModelListGP acquisitions (qEHVI,
    qNEHVI, constrained qEI / qNEI and their log forms): every member's mean and
    jittered q x q root of the B t-batches, written straight into their slices
    of the stacked M x B x q (x q) inputs of the reduction launch (no stack
    copies), the ladder outcomes folded into ``ladder.words`` where it has any.

    Without ``root_acqf``: post_partials_members (one launch where the
    small-grid or member stream-K plan applies), the finalisation, W.

    With ``root_acqf`` (cached baseline roots, ``root_acqf._roots``): per
    member additionally T_t = L_rr,t^{-1} Sigma'_t(X_b, X) and F_t = Z_b,t T_t,
    and the root of Sigma'_t - T_t^T T_t.  Where the one-model plan splits k
    (C4) the cross term cannot ride in the posterior pass and R^T is stored
    anyway: then every member's partials + R^T in one launch, and the root
    terms as GEMMs batched over the members where _roots_batched allows;
    elsewhere per member (post_partials with the cross term, two GEMMs + one)."""
    M = len(members)
    B, q, _ = X3.shape
    Xd = X3.detach()
    roots = root_acqf._roots if root_acqf is not None else None
    keys = prime_prediction_caches(members)
    caches = [mm.prediction_cache(key=key) for mm, key in zip(members, keys)]
    c0 = caches[0]
    pps = None
    if roots is None:
        pps = kernels.post_partials_members(caches, Xd, store_R=need_grad)
    elif (1 < M <= 8 and kernels.split_plan(B, q, c0.n)[0] != 0
            and all(c.n == c0.n and c.np == c0.np and c.d == c0.d for c in caches)):
        pps = kernels.post_partials_members(caches, Xd, store_R=True)
    f64 = dict(dtype=torch.float64, device=X3.device)
    mean = torch.empty(M, B, q, **f64)
    L = torch.empty(M, B, q, q, **f64)
    stats = [mm.outcome_stats() for mm in members]
    Ts = F = Ws = None
    batched = roots is not None and pps is not None and _roots_batched(root_acqf, caches, pps, stats)
    if batched:
        # every member's T and F in three batched GEMMs over the members
        Ts, F = _roots_forward_batched(root_acqf, caches, pps, stats)
        if need_grad:
            Ws = kernels.w_matrix_members(caches, pps)
    elif roots is not None:
        given, pps, Ts, Ws = pps, [], [], []
        for t, (cache, rt) in enumerate(zip(caches, roots)):
            pp = given[t] if given is not None else kernels.post_partials(
                cache, Xd, store_R=need_grad, cross=rt.Q_b)
            pps.append(pp)
            if F is None:
                F = torch.empty(M, rt.Z_base.shape[0], pp.nrows_pad, **f64)
            Ts.append(rt.forward(cache, pp, stats[t][1], F_out=F[t])[0])
            if need_grad:
                Ws.append(kernels.w_matrix(cache, pp))
    if (M <= 8 and all(p_.Spart.shape == pps[0].Spart.shape for p_ in pps)
            and all(c.kind == c0.kind for c in caches)):
        # every member's finalisation in one launch
        info, jitter = kernels.qmc_finalize_members(caches, pps, stats, mean, L,
                                                    status=ladder.words, Ts=Ts, F=F)
    else:
        info, jitter = [], []
        for t, (cache, pp) in enumerate(zip(caches, pps)):
            out = kernels.qmc_finalize(cache, pp, _lib.QMC_CHOL, *stats[t], want_mean=True,
                                       want_cov=False, want_L=True, T=Ts[t] if Ts else None,
                                       F=F[t] if F is not None else None, mean_out=mean[t],
                                       L_out=L[t], status=ladder.words[t] if ladder.words else None)
            info.append(out["info"])
            jitter.append(out["jitter"])
    saved = []
    if need_grad:
        if roots is None:
            Ws = kernels.w_matrix_members(caches, pps)   # one launch where stream-K
        saved = [(caches[t], pps[t], stats[t][1], Ts[t] if Ts else None, Ws[t]) for t in range(M)]
    return _MemberPosterior(mean, L, F, pps[-1].Qp if roots is not None else 0, saved, batched,
                            info, jitter, root_acqf)


def _chol_backward_members(L, dL):
    """d Sigma of every member's t-batches (M x B x q x q) in one launch."""
    q = L.shape[-1]
    return kernels.chol_backward(L.reshape(-1, q, q), dL.reshape(-1, q, q)).reshape(L.shape)


def _member_posterior_backward(post: _MemberPosterior, dmean, dL, dF):
    """(d mean, d L, d F) of _member_posterior's outputs -> dX: bo_chol_backward
    (d Sigma_t), then the members' bo_post_backward passes -- with roots, behind
    the cached-root backward (dT = Z_b^T dF - T G) and with a second pass per
    member through K(X_b, X)."""
    if post.root_acqf is None:
        dcovs = _chol_backward_members(post.L, dL)
        jobs = [dict(cache=cache, pp=pp, W=W, dmean=dmean[t], dcov=dcovs[t], ystd=ystd)
                for t, (cache, pp, ystd, _, W) in enumerate(post.saved)]
    elif post.batched:
        jobs = _roots_backward_jobs(post, dmean, dL, dF)
    else:
        dX = None
        for t, (cache, pp, ystd, T, W) in enumerate(post.saved):
            dcov = kernels.chol_backward(post.L[t], dL[t])
            dX = post.root_acqf._roots[t].backward(cache, pp, W, dmean[t], dcov,
                                                   dF[t].contiguous(), T, ystd, dX=dX)
        return dX
    c0 = jobs[0]["cache"]
    if 1 < len(jobs) <= 16 and all(j["cache"].kind == c0.kind and j["cache"].d == c0.d
                                   for j in jobs):
        return kernels.post_backward_jobs(jobs)     # every pass in one launch
    dX = None
    for job in jobs:
        dX = kernels.post_backward(**job, dX=dX)
    return dX


class _FusedHVI(torch.autograd.Function):
    """qEHVI / qNEHVI (plain, feasibility-weighted or log-space) of B t-batches
    over a ModelListGP, with its gradient; ``noisy``: qNEHVI, the members'
    cached baseline roots and per-sample cells.

    Forward: _member_posterior, then one bo_qehvi / bo_qehvi_feas / bo_qlogehvi
    launch over (sample, hypercell) pairs with f = mean + L z (+ F).
    Backward: the kernel's backward (inclusion-exclusion derivative) -> d mu_t,
    d L_t (, d F_t), then _member_posterior_backward."""

    @staticmethod
    def forward(ctx, X3, acqf, noisy):
        members = acqf.model.models
        need_grad = ctx.needs_input_grad[0]
        q, dev = X3.shape[-2], X3.device
        # forward-only qNEHVI defers the ladder outcome (the eager qEI's ring:
        # no stream sync per call); forward-only qEHVI comes here only for the
        # log, weighted and capture cases and reads it behind the launch
        with kernels.member_ladder(dev, len(members), need_grad,
                                   ("qNEHVI" if noisy else "qEHVI") + " posterior root",
                                   defer_forward_only=noisy) as ladder:
            post = _member_posterior(members, X3, need_grad, ladder, acqf if noisy else None)
            mean, L, F, Qp = post[:4]
            if noisy:
                Z = acqf._base_samples_q(q, dev)
                lo, hi = acqf._cells
            else:
                Z = acqf._ensure_sampler().base_samples_2d(q * len(members), dev)
                lo, hi = acqf._cells(dev)
            # the kernel itself (as the backward below): this Function already is
            # the autograd node, the registered op's wrapper would only add host time
            feas = ctx.log = None
            if acqf._log:
                acq, ctx.log = _log_hvi_forward(acqf, mean, L, Z, lo, hi, F, Qp, need_grad)
            elif acqf._weighted:
                # outcome constraints: the weighted kernel on the objective members
                feas = _feas_weights(acqf, mean, L, Z, F, Qp, need_grad)
                acq = kernels.qehvi_feas(mean, L, Z, lo, hi, feas[0].detach(), acqf._out_idx, F=F,
                                         Qp=Qp)
            else:
                acq = kernels.qehvi(mean, L, Z, lo, hi, F=F, Qp=Qp)
            # the members' ladders checked once, behind the reduction launch (one
            # host read per forward instead of one per member, each of which
            # drained the queue: ~40 us of idle device between members at C4)
            ladder.finish(ctx, post.info, post.jitter)
        if need_grad:
            ctx.acqf, ctx.post, ctx.Z, ctx.cells, ctx.feas = acqf, post, Z, (lo, hi), feas
        return acq

    @staticmethod
    def backward(ctx, dacq):
        acqf, (mean, L, F, Qp), (lo, hi) = ctx.acqf, ctx.post[:4], ctx.cells
        dF = None
        if ctx.log is not None:
            dmean, dL, dF = _log_hvi_backward(acqf, ctx.log, mean, L, ctx.Z, lo, hi, dacq, F, Qp)
        elif ctx.feas is not None:
            dmean, dL, *dF, dfeas = kernels.qehvi_feas_backward(
                mean, L, ctx.Z, lo, hi, ctx.feas[0].detach(), acqf._out_idx, dacq, F=F, Qp=Qp)
            dF = dF[0] if dF else None              # returned with roots only
            _feas_backward(ctx.feas, dfeas, dmean, dL, dF)
        else:
            dmean, dL, *dF = kernels.qehvi_backward(mean, L, ctx.Z, lo, hi, dacq, F=F, Qp=Qp)
            dF = dF[0] if dF else None
        dX = _member_posterior_backward(ctx.post, dmean, dL, dF)
        _settle_ladder(ctx)
        return dX, None, None


def _settle_ladder(ctx) -> None:
    """The forward's deferred ladder outcome (kernels._LadderRing), read once
    the backward's launches are queued behind it."""
    lad = getattr(ctx, "ladder", None)
    if lad is not None:
        ctx.ladder = None
        lad[0].settle(lad[1])


class IdentityMCMultiOutputObjective(MCObjective):
    """acquisition/multi_objective/objective.py:65-101: the samples, or their
    ``outcomes`` columns (the objective members of a model list that also has
    constraint members; negative indices count from ``num_outcomes``)."""

    def __init__(self, outcomes: Optional[List[int]] = None, num_outcomes: Optional[int] = None):
        super().__init__()
        if outcomes is not None:
            outcomes = [int(i) for i in outcomes]
            if len(outcomes) < 2:
                raise BotorchTensorDimensionError("Must specify at least two outcomes for MOO.")
            if any(i < 0 for i in outcomes):
                if num_outcomes is None:
                    raise BotorchError("num_outcomes is required if any outcomes are less than 0.")
                if any(not -num_outcomes <= i < num_outcomes for i in outcomes):
                    raise ValueError(f"outcomes {outcomes} out of range for {num_outcomes} outcomes")
                outcomes = [i % num_outcomes for i in outcomes]
            self.register_buffer("outcomes", torch.tensor(outcomes, dtype=torch.long))

    def forward(self, samples, X=None):
        if hasattr(self, "outcomes"):
            return samples.index_select(-1, self.outcomes.to(device=samples.device))
        return samples


def _init_outcome_constraints(acqf, num_members: int, objective, constraints, eta, fat,
                              num_ref: int) -> None:
    """The constraint options of qEHVI / qNEHVI (monte_carlo.py:105-130),
    checked before any device work: sets ``constraints``, ``eta``, ``fat``, the
    objective members ``_out_idx`` and ``_weighted`` (whether forward takes the
    feasibility-weighted kernels: constraints, or an objective that selects
    outcomes)."""
    acqf.constraints = list(constraints) if constraints else None
    acqf.fat = fat
    acqf.eta = None
    if acqf.constraints is not None:
        if objective is not None and type(objective) is not IdentityMCMultiOutputObjective:
            raise UnsupportedError("outcome constraints with a non-identity multi-output objective "
                                   "are not on the accelerated path")
        acqf.eta = _as_etas(eta, len(acqf.constraints)).to(torch.float64)
    outcomes = (getattr(objective, "outcomes", None)
                if type(objective) is IdentityMCMultiOutputObjective else None)
    if outcomes is not None:
        out_idx = [int(i) for i in outcomes.tolist()]
        if any(not 0 <= i < num_members for i in out_idx) or len(set(out_idx)) != len(out_idx):
            raise ValueError(f"objective outcomes {out_idx} must be distinct members of the "
                             f"{num_members}-member model list")
    else:
        out_idx = list(range(num_members))
    acqf._out_idx = out_idx
    acqf._weighted = acqf.constraints is not None or outcomes is not None
    if acqf._weighted:
        if num_ref != len(out_idx):
            raise ValueError("The length of the reference point must match the number of outcomes. "
                             f"Got ref_point with {num_ref} elements, but expected {len(out_idx)}.")
        if not 2 <= len(out_idx) <= 4:
            raise UnsupportedError("the feasibility-weighted kernels support 2 to 4 objectives")


def _member_samples(mean, L, Z, F, Qp: int):
    """The samples f = mean + L z (+ F) of all members, S x B x q x Mt, in torch
    (mean Mt x B x q, L Mt x B x q x q, Z S x (q Mt) point-major / member-minor,
    F Mt x S x ldF with rows b Qp + p)."""
    Mt, B, q = mean.shape
    S = Z.shape[0]
    f = mean.permute(1, 2, 0).unsqueeze(0) + torch.einsum(
        "tbpj,sjt->sbpt", L.tril(), Z.reshape(S, q, Mt))
    if F is not None:
        f = f + F[:, :, : B * Qp].reshape(Mt, S, B, Qp)[..., :q].permute(1, 2, 3, 0)
    return f


def _feas_weights(acqf, mean, L, Z, F, Qp: int, need_grad: bool, log: bool = False):
    """The smoothed feasibility weights w (S x B x q) of the samples
    f = mean + L z (+ F) of ALL members (S x B x q x Mt; the constraint
    callables may read any output), as a differentiable function of detached
    leaf copies of mean, L (and F): -> (w, leaves).  Plain torch: the tensor is
    tiny next to the posterior.  Without constraints (an objective that only
    selects outcomes) every weight is 1."""
    if acqf.constraints is None:
        return torch.ones(Z.shape[0], *mean.shape[1:], dtype=torch.float64, device=mean.device), None
    leaves = [t.detach().requires_grad_(need_grad) for t in ((mean, L) if F is None else (mean, L, F))]
    with torch.enable_grad() if need_grad else torch.no_grad():
        f = _member_samples(*leaves[:2], Z, leaves[2] if F is not None else None, Qp)
        w = compute_smoothed_feasibility_indicator(acqf.constraints, f, acqf.eta.to(f),
                                                   log=log, fat=acqf.fat)
        # inside the grad mode above: a copy made outside it (w comes out
        # non-contiguous for one member) would drop the graph
        w = w.to(torch.float64).contiguous()
    return w, leaves


def _feas_backward(feas, dfeas, dmean, dL, dF) -> None:
    """The constraint path's cotangents added to the kernel's: one
    autograd.grad of w w.r.t. the leaves of _feas_weights, for all members."""
    w, leaves = feas
    if leaves is None or not w.requires_grad:
        return
    grads = torch.autograd.grad(w, leaves, dfeas, allow_unused=True)
    for out, g in zip((dmean, dL, dF), grads):
        if g is not None:
            out.add_(g)


class qExpectedHypervolumeImprovement(MCAcquisitionFunction):
    """MC qEHVI (acquisition/multi_objective/monte_carlo.py:146-322) over the
    hypercells of a non-dominated partitioning.

    Fused path (ModelListGP of SingleTaskGPs, identity objective): per output,
    the exact posterior of the B t-batches (post_partials + the per-t-batch
    jittered Cholesky, qmc_finalize in CHOL mode), then one bo_qehvi launch that
    draws the non-interleaved Sobol samples and evaluates the inclusion-exclusion
    hypervolume improvement over (sample, hypercell) pairs.

    Outcome constraints (monte_carlo.py:245-251, 303-309): the model list holds
    objective and constraint members, ``objective =
    IdentityMCMultiOutputObjective(outcomes=[...])`` picks the objectives, and
    every subset term is weighted by the smoothed feasibility of its points
    (``constraints``: callables on the S x B x q x Mt samples, <= 0 feasible;
    ``eta``, ``fat``): bo_qehvi_feas / bo_qehvi_feas_backward, the constraint
    path's gradient through torch autograd on the small sample tensor."""

    _default_sample_shape = torch.Size([128])
    _log = False  # the log-space subclasses (qLogEHVI, qLogNEHVI) take bo_qlogehvi

    def __init__(self, model, ref_point, partitioning, sampler=None, objective=None,
                 constraints=None, X_pending=None, eta=1e-3, fat=False):
        if len(ref_point) != partitioning.num_outcomes:
            raise ValueError(
                "The length of the reference point must match the number of outcomes. "
                f"Got ref_point with {len(ref_point)} elements, but expected "
                f"{partitioning.num_outcomes}.")
        AcquisitionFunction.__init__(self, model)
        _init_outcome_constraints(self, len(getattr(model, "models", None) or ()), objective,
                                  constraints, eta, fat, len(ref_point))
        self.sampler = sampler
        self.objective = objective if objective is not None else IdentityMCMultiOutputObjective()
        self.posterior_transform = None
        self.set_X_pending(X_pending)
        self.ref_point = torch.as_tensor(ref_point, dtype=torch.float64)
        lo, hi = partitioning.get_hypercell_bounds()
        self.cell_lower_bounds = lo.to(torch.float64)
        self.cell_upper_bounds = hi.to(torch.float64)
        self._dev_cells = {}

    def _cells(self, device):
        key = str(device)
        if key not in self._dev_cells:
            self._dev_cells[key] = (self.cell_lower_bounds.to(device).contiguous(),
                                    self.cell_upper_bounds.to(device).contiguous())
        return self._dev_cells[key]

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = self._concat_pending(t_batch_mode(X))
        batch = X.shape[:-2]
        q, d = X.shape[-2], X.shape[-1]
        X3 = X.reshape(-1, q, d)
        models = getattr(self.model, "models", None)
        if models is None or not all(hasattr(mm, "prediction_cache") for mm in models):
            raise UnsupportedError("qEHVI here runs on a ModelListGP of SingleTaskGPs")
        if not isinstance(self.objective, IdentityMCMultiOutputObjective):
            raise UnsupportedError("only the identity multi-output objective is accelerated")
        _check_log_q(self, q)
        if q > 12 or d > kernels.DP:
            raise UnsupportedError("fused qEHVI supports q <= 12 and d <= 8")
        acq = None
        if (not self._log and not self._weighted and not (torch.is_grad_enabled() and X3.requires_grad)
                and X3.dtype == torch.float64):
            acq = _qehvi_members_eager(self, X3)
        if acq is None:
            acq = _FusedHVI.apply(X3, self, False)
        return acq.reshape(batch)


# -- qNEHVI ------------------------------------------------------------------------------
def prune_inferior_points_multi_objective(model, X, ref_point, objective=None, constraints=None,
                                          num_samples: int = 2048, max_frac: float = 1.0,
                                          marginalize_dim=None, chunk: int = 64):
    """acquisition/multi_objective/utils.py:77-161: keep the points with a
    positive probability of being feasible, Pareto-optimal and better than
    ref_point under ``num_samples`` joint posterior samples (drawn on the
    device; Pareto masks in sample chunks).  ``constraints`` read the samples
    of all outputs, ``objective`` selects / maps the objectives' columns."""
    from .multi_objective import is_non_dominated
    if X.ndim > 2:
        raise UnsupportedError("Batched inputs `X` are currently unsupported by "
                               "prune_inferior_points_multi_objective")
    if max_frac <= 0 or max_frac > 1.0:
        raise ValueError(f"max_frac must take values in (0, 1], is {max_frac}")
    max_points = math.ceil(max_frac * X.size(-2))
    ref = torch.as_tensor(ref_point, dtype=torch.float64, device=X.device)
    models = getattr(model, "models", [model])
    n, m = X.shape[-2], len(models)
    with torch.no_grad():
        # joint samples of the independent outputs: Sobol dimension n m,
        # point-major / output-minor base samples (get_sampler on the MTMVN),
        # seeded as the reference's sampler seeds itself from the global
        # generator (sampling/base.py: torch.randint(0, 1000000, (1,)))
        if n * m <= 21201:
            seed = int(torch.randint(0, 1000000, (1,)).item())
            Z = kernels.sobol_normal(n * m, num_samples, seed, X.device).view(num_samples, n, m)
        else:
            Z = torch.randn(num_samples, n, m, dtype=torch.float64, device=X.device)
        cols = []
        for t, mm in enumerate(models):
            post = mm.posterior(X)
            mean = post.distribution.mean.reshape(1, n)
            L, _, _ = kernels.cholesky_with_inverse(post.distribution.covariance_matrix.reshape(n, n))
            cols.append(kernels.sample_mvn(mean, L.unsqueeze(0).contiguous(),
                                           Z[:, :, t].contiguous()).reshape(num_samples, n))
        samples = torch.stack(cols, dim=-1)  # S x n x m
        obj = samples if objective is None else objective(samples, X=X)
        if constraints:
            # infeasible samples never count as Pareto-optimal (utils.py:144-150)
            infeas = ~compute_feasibility_indicator(constraints, samples,
                                                    marginalize_dim=marginalize_dim)
            obj = obj.masked_fill(infeas.unsqueeze(-1), float("-inf"))
        hits = torch.zeros(n, dtype=torch.float64, device=X.device)
        # one device launch for all samples (bo_pareto_mask); host tensors chunked
        step = obj.shape[0] if obj.is_cuda else chunk
        for s0 in range(0, obj.shape[0], step):
            o = obj[s0:s0 + step]
            mask = is_non_dominated(o, deduplicate=False) & (o > ref).all(dim=-1)
            hits += mask.to(torch.float64).sum(dim=0)
    probs = hits / obj.shape[0]
    idcs = probs.nonzero().view(-1)
    if idcs.shape[0] > max_points:
        counts, order_idcs = torch.sort(probs, descending=True)
        idcs = order_idcs[:max_points]
    return X[idcs]


def _roots_backward_jobs(post: _MemberPosterior, dmean, dL, dF) -> list:
    """_CachedBaselineRoot.backward for all members at once (the forward's
    batched route): dT = Z_base^T dF and the dK*x / dK(X_b, X) GEMMs batched
    over the members (s^2 folded into the stacked operands), the per-t-batch
    dT -= T G -> the two post_backward passes per member (training, then
    baseline points) as post_backward_jobs' dicts."""
    acqf = post.root_acqf
    roots = acqf._roots
    key, Linv_s, _, Zb, _ = acqf.__dict__["_root_stack"]
    Qb_s = acqf.__dict__.get("_root_stack_qb")
    if Qb_s is None or Qb_s[0] != key:
        s2 = [float(sv) ** 2 for sv in key[0]]
        Qb_s = (key, torch.stack([rt.Q_b * (-s2[t]) for t, rt in enumerate(roots)]).contiguous())
        acqf.__dict__["_root_stack_qb"] = Qb_s
    Qb_s = Qb_s[1]
    dT = kernels.gemm(Zb, dF.contiguous(), transA=True)                 # M x r x N
    r = dT.shape[1]
    dcovs = _chol_backward_members(post.L, dL)
    for t, (cache, pp, ystd, T, W) in enumerate(post.saved):
        dcov = dcovs[t]
        G = (dcov + dcov.mT).contiguous()
        q, Qp, nrows, B = pp.q, pp.Qp, pp.nrows_pad, pp.B
        kernels.gemm_strided(r, q, q, T, nrows, Qp, G, q, q * q, dT[t], nrows, Qp, B,
                             alpha=-1.0, beta=1.0)                      # dT_b -= T_b G_b
    E = kernels.gemm(dT, Qb_s, transA=True)                             # M x N x np
    # (s^2 L_rr^-T dT)^T = dT^T (s^2 L_rr^-1): already in post_backward's layout
    dKbxT = kernels.gemm(dT, Linv_s, transA=True, flags=_lib.GEMM_B_LOWER)  # M x N x r
    jobs = []
    for t, (cache, pp, ystd, T, W) in enumerate(post.saved):
        jobs.append(dict(cache=cache, pp=pp, W=W, dmean=dmean[t], dcov=dcovs[t], ystd=ystd, E=E[t]))
        jobs.append(dict(cache=cache, pp=pp, W=None, dmean=None, dcov=None, ystd=ystd, E=dKbxT[t],
                         Xt_scaled=roots[t].Xb_scaled, n=r))
    return jobs


def _roots_batched(acqf, caches, pps, stats) -> bool:
    """Whether the members' cached-root terms can go as batched GEMMs: R^T
    stacked by the members' route, equal baseline sizes and sample counts."""
    roots = acqf._roots
    if any(p_.Rt is None or p_.Cx is not None for p_ in pps):
        return False
    r0, S0 = roots[0].Linv.shape[0], roots[0].Z_base.shape[0]
    if any(rt.Linv.shape[0] != r0 or rt.Z_base.shape[0] != S0 for rt in roots):
        return False
    base = pps[0].Rt
    step = base.numel()
    return all(p_.Rt.data_ptr() == base.data_ptr() + 8 * step * t and p_.Rt.is_contiguous()
               for t, p_ in enumerate(pps))


def _roots_forward_batched(acqf, caches, pps, stats):
    """_CachedBaselineRoot.forward for all members at once: T_t = s_t^2
    (L_rr,t^-1 K(X_b, X)_t - P_b,t R_t^T), F_t = Z_base,t T_t as three batched
    GEMMs over the members (the s_t^2 folded into stacked copies of L_rr^-1
    and P_b, rebuilt when the outcome scales change)."""
    roots = acqf._roots
    M = len(roots)
    p0 = pps[0]
    dev = p0.Xq.device
    # keyed by the roots too (their identity and baseline size), not only by
    # the outcome scales: _set_cell_bounds rebuilds the roots
    key = (tuple(float(s_[1]) for s_ in stats), str(dev),
           tuple((id(rt), rt.Linv.data_ptr(), rt.Linv.shape[0]) for rt in roots))
    stk = acqf.__dict__.get("_root_stack")
    if stk is None or stk[0] != key:
        s2 = [float(s_[1]) ** 2 for s_ in stats]
        stk = (key, torch.stack([rt.Linv * s2[t] for t, rt in enumerate(roots)]).contiguous(),
               torch.stack([rt.P_b * s2[t] for t, rt in enumerate(roots)]).contiguous(),
               torch.stack([rt.Z_base for rt in roots]).contiguous(),
               torch.ones(kernels.DP, dtype=torch.float64, device=dev))
        acqf.__dict__["_root_stack"] = stk
    _, Linv_s, Pb_s, Zb, ones = stk
    r = Linv_s.shape[1]
    Kbx = torch.empty(M, r, p0.nrows_pad, dtype=torch.float64, device=dev)
    for t, (rt, c, p_) in enumerate(zip(roots, caches, pps)):
        kernels.covar_matrix(rt.Xb_scaled, p_.Xq, ones, c.kind, c.outputscale, out=Kbx[t])
    T = kernels.gemm(Linv_s, Kbx, flags=_lib.GEMM_A_LOWER)
    Rt_all = p0.Rt.as_strided((M,) + tuple(p0.Rt.shape), (p0.Rt.numel(),) + tuple(p0.Rt.stride()))
    T = kernels.gemm(Pb_s, Rt_all, alpha=-1.0, beta=1.0, C=T)
    F = kernels.gemm(Zb, T)
    return [T[t] for t in range(M)], F


# -- outcome constraints on the single-objective classes ---------------------------------
class _WeightedSOPlan:
    """What the feasibility-weighted fused route of qEI / qLogEI / qNEI / qLogNEI
    needs from the acquisition function, fixed at construction: the members (a
    SingleTaskGP, or a ModelListGP's members), the objective weights ``c`` over
    them, and the constraints -- ``lin = (A, rhs)`` when every callable comes
    from get_outcome_constraint_transforms (then evaluated inside bo_qmc_feas),
    else None (the callables run in torch on the members' samples,
    _feas_weights).  ``constraints`` / ``eta`` / ``fat`` under the names
    _feas_weights reads; the etas are set at the first forward, where the
    generic route would check them."""

    def __init__(self, members, c, constraints, lin, fat):
        self.members, self.c, self.constraints, self.lin, self.fat = members, c, constraints, lin, fat
        self.eta = None
        self.etas = None

    def set_eta(self, eta) -> None:
        if self.etas is None:
            self.eta = _as_etas(eta, len(self.constraints)).to(torch.float64)
            self.etas = [float(v) for v in self.eta.tolist()]


def _weighted_so_plan(acqf) -> Optional[_WeightedSOPlan]:
    """The plan (built once), or None where the route does not apply: no
    constraints, a posterior transform, an ensemble, a model that is neither a
    SingleTaskGP under the identity objective nor a list of <= 8 of them under
    LinearMCObjective(weights over the members)."""
    plan = acqf.__dict__.get("_wso")
    if plan is None:
        plan = _make_weighted_so_plan(acqf) or False
        acqf.__dict__["_wso"] = plan
    return plan or None


def _make_weighted_so_plan(acqf) -> Optional[_WeightedSOPlan]:
    cons = acqf._constraints
    if cons is None or len(cons) == 0 or acqf.posterior_transform is not None:
        return None
    model = acqf.model
    models = getattr(model, "models", None)
    if models is None:
        if not hasattr(model, "prediction_cache") or type(acqf.objective) is not IdentityMCObjective:
            return None
        members, c = [model], [1.0]
    else:
        if (not 1 <= len(models) <= kernels.QMC_FEAS_MTMAX
                or not all(hasattr(mm, "prediction_cache") for mm in models)
                or type(acqf.objective) is not LinearMCObjective
                or acqf.objective.weights.numel() != len(models)):
            return None
        members, c = list(models), [float(v) for v in acqf.objective.weights.tolist()]
    if any(getattr(mm, "_is_ensemble", False) or getattr(mm, "_is_fully_bayesian", False)
           for mm in members):
        return None
    lin = _linear_outcome_constraints(cons)
    if lin is not None and (len(lin[0]) > kernels.QMC_FEAS_KMAX or len(lin[0][0]) != len(members)):
        lin = None
    return _WeightedSOPlan(members, c, list(cons), lin, acqf._fat)


def _weighted_so_route(acqf, X: torch.Tensor) -> Optional[_WeightedSOPlan]:
    """The plan where this call can take the fused route: X on the device,
    q <= 16 (pending points included), d <= 8, a one-dimensional sample shape,
    and no graph capture running (a capture takes the route it took before)."""
    plan = _weighted_so_plan(acqf)
    if (plan is None or not X.is_cuda or X.shape[-2] > kernels.QMC_FEAS_QMAX
            or X.shape[-1] > kernels.DP or len(acqf.sample_shape) != 1
            or kernels._dev_index(X.device) in kernels._CAPTURE):
        return None
    plan.set_eta(acqf._eta)
    plan.fat = acqf._fat
    return plan


def _weighted_so_base_samples(acqf, plan, q: int, device) -> Optional[torch.Tensor]:
    """Z (S x q Mt, column j Mt + t) of qEI / qLogEI: a single sampler's
    base_samples_2d(q Mt) (the qEHVI convention); a ListSampler of Mt samplers
    interleaved from each member's base_samples_2d(q) -- the samples the generic
    route draws -- and cached per q.  Without a sampler, the one the generic
    route would build.  None for any other sampler."""
    Mt = len(plan.members)
    if acqf.sampler is None:
        if hasattr(acqf.model, "models"):
            acqf.sampler = ListSampler(*[SobolQMCNormalSampler(sample_shape=acqf._default_sample_shape)
                                         for _ in range(Mt)])
        else:
            acqf._ensure_sampler()
    s = acqf.sampler
    if isinstance(s, ListSampler):
        if len(s.samplers) != Mt or not all(hasattr(x, "base_samples_2d") for x in s.samplers):
            return None
        parts = [x.base_samples_2d(q, device) for x in s.samplers]
        key = tuple((p.data_ptr(), p._version) for p in parts)
        cache = acqf.__dict__.setdefault("_zlist", {})
        hit = cache.get(q)
        if hit is None or hit[0] != key:
            hit = (key, torch.stack(parts, dim=-1).reshape(parts[0].shape[0], q * Mt).contiguous())
            cache[q] = hit
        return hit[1]
    if hasattr(s, "base_samples_2d"):
        return s.base_samples_2d(q * Mt, device)
    return None


def _weighted_qei_forward(acqf, X: torch.Tensor) -> Optional[torch.Tensor]:
    """qEI / qLogEI with outcome constraints on the fused route (X already in
    t-batch mode with the pending points), or None where it does not apply."""
    if acqf.best_f.numel() != 1:
        return None
    plan = _weighted_so_route(acqf, X)
    if plan is None:
        return None
    q, d = X.shape[-2], X.shape[-1]
    Z = _weighted_so_base_samples(acqf, plan, q, X.device)
    if Z is None:
        return None
    X3 = X.reshape(-1, q, d)
    acq = _FusedSOFeas.apply(X3.to(torch.float64), acqf, plan, Z, _host_scalar(acqf, "best_f"))
    return acq.to(X.dtype).reshape(X.shape[:-2])


def _so_feas_forward(acqf, plan, mean, L, Z, F, Qp: int, best_f: float, best_f_s, need_grad: bool):
    """bo_qmc_feas on the members' stacked means / roots: the linear
    constraints inside the kernel, any other callable through _feas_weights
    (log-weights in log mode) -> acq, the state the backward takes back."""
    lp = getattr(acqf, "_log_params", None) or (0, TAU_RELU, TAU_MAX)
    kw = dict(best_f=best_f, best_f_s=best_f_s, F=F, Qp=Qp, log=acqf._log, fat=plan.fat,
              tau_relu=lp[1], tau_max=lp[2])
    feas = None
    if plan.lin is not None:
        kw.update(A=plan.lin[0], rhs=plan.lin[1], eta=plan.etas)
    else:
        feas = _feas_weights(plan, mean, L, Z, F, Qp, need_grad, log=acqf._log)
        kw.update(feas=feas[0].detach())
    return kernels.qmc_feas(mean, L, Z, plan.c, **kw), (kw, feas)


def _so_feas_backward(plan, state, mean, L, Z, acq, dacq):
    """bo_qmc_feas_backward, plus the constraint callables' path -> dmean, dL, dF."""
    kw, feas = state
    dmean, dL, dF, dfeas = kernels.qmc_feas_backward(mean, L, Z, plan.c, dacq.contiguous(), acq=acq,
                                                     **kw)
    if feas is not None:
        _feas_backward(feas, dfeas, dmean, dL, dF)
    return dmean, dL, dF


class _FusedSOFeas(torch.autograd.Function):
    """Constrained qEI / qLogEI (``Z``, ``best_f`` given) or qNEI / qLogNEI
    (both None: the members' cached baseline roots, the per-sample baseline
    best) of B t-batches over the plan's members, with its gradient:
    _FusedHVI's chain with bo_qmc_feas as the reduction."""

    @staticmethod
    def forward(ctx, X3, acqf, plan, Z, best_f):
        need_grad = ctx.needs_input_grad[0]
        noisy = Z is None
        M = len(plan.members)
        with kernels.member_ladder(X3.device, M, need_grad, type(acqf).__name__ + " posterior root",
                                   defer_forward_only=noisy) as ladder:
            post = _member_posterior(plan.members, X3, need_grad, ladder, acqf if noisy else None)
            best_f_s = None
            if noisy:
                Z = acqf._base_samples_members(X3.shape[-2], M, X3.device)
                best_f, best_f_s = 0.0, acqf._baseline_best_f
            acq, state = _so_feas_forward(acqf, plan, post.mean, post.L, Z, post.F, post.Qp, best_f,
                                          best_f_s, need_grad)
            ladder.finish(ctx, post.info, post.jitter)
        if need_grad:
            ctx.plan, ctx.state, ctx.post, ctx.Z, ctx.acq = plan, state, post, Z, acq.detach().clone()
        return acq

    @staticmethod
    def backward(ctx, dacq):
        post = ctx.post
        dmean, dL, dF = _so_feas_backward(ctx.plan, ctx.state, post.mean, post.L, ctx.Z, ctx.acq, dacq)
        dX = _member_posterior_backward(post, dmean, dL, dF)
        _settle_ladder(ctx)
        return dX, None, None, None, None


class _QEHVIFromRoots(torch.autograd.Function):
    """The fused hypervolume-improvement kernel (bo_qehvi) on caller-made
    sample roots, f_s = mean + F_s + L z_s (mean m x B x q, L m x B x q x q,
    F m x S x B q), as a differentiable function of (mean, L, F)."""

    @staticmethod
    def forward(ctx, mean, L, F, Zq, lo, hi, q):
        acq = kernels.qehvi(mean, L, Zq, lo, hi, F=F, Qp=q)
        ctx.save_for_backward(mean, L, F, Zq, lo, hi)
        ctx.q = q
        return acq

    @staticmethod
    def backward(ctx, dacq):
        mean, L, F, Zq, lo, hi = ctx.saved_tensors
        dmean, dL, dF = kernels.qehvi_backward(mean, L, Zq, lo, hi, dacq.contiguous(), F=F,
                                               Qp=ctx.q)
        return dmean, dL, dF, None, None, None, None


class _QEHVIFeasFromRoots(torch.autograd.Function):
    """_QEHVIFromRoots with feasibility weights (bo_qehvi_feas): a
    differentiable function of (mean, L, F, w) over all Mt members; the caller
    forms w from the same (mean, L, F) in torch, so autograd adds the
    constraint path through dfeas."""

    @staticmethod
    def forward(ctx, mean, L, F, w, Zq, lo, hi, q, out_idx):
        acq = kernels.qehvi_feas(mean, L, Zq, lo, hi, w, out_idx, F=F, Qp=q)
        ctx.save_for_backward(mean, L, F, w, Zq, lo, hi)
        ctx.q, ctx.out_idx = q, out_idx
        return acq

    @staticmethod
    def backward(ctx, dacq):
        mean, L, F, w, Zq, lo, hi = ctx.saved_tensors
        dmean, dL, dF, dfeas = kernels.qehvi_feas_backward(mean, L, Zq, lo, hi, w, ctx.out_idx,
                                                           dacq.contiguous(), F=F, Qp=ctx.q)
        return dmean, dL, dF, dfeas, None, None, None, None, None


def _check_log_q(acqf, q: int) -> None:
    """The log-space kernels evaluate all 2^q - 1 subsets of every (sample,
    cell) pair: q <= 8, pending points included."""
    if acqf._log and q > kernels.QLOGEHVI_QMAX:
        raise UnsupportedError(f"{type(acqf).__name__} supports q <= {kernels.QLOGEHVI_QMAX} "
                               f"(pending points included), got q = {q}")


def _log_hvi_forward(acqf, mean, L, Z, lo, hi, F, Qp: int, need_grad: bool):
    """The log-space reduction of _FusedHVI (bo_qlogehvi) on
    the members' means and roots: -> (acq, state for _log_hvi_backward).  With
    outcome constraints the points' log feasibility (logei.py:162-169) is formed
    in torch from detached leaves, as _feas_weights does for the plain classes."""
    feas, logw = None, None
    if acqf.constraints is not None:
        feas = _feas_weights(acqf, mean, L, Z, F, Qp, need_grad, log=True)
        logw = feas[0].detach()
    acq, hvi = kernels.qlogehvi(mean, L, Z, lo, hi, acqf._out_idx, logw, F=F, Qp=Qp, fat=acqf.fat,
                                tau_relu=acqf.tau_relu, tau_max=acqf.tau_max)
    # the state keeps an alias of acq, not the Function's output itself (which
    # would tie the output to its own node)
    return acq, (acq.detach(), hvi, feas)


def _log_hvi_backward(acqf, state, mean, L, Z, lo, hi, dacq, F, Qp: int):
    """bo_qlogehvi_backward -> dmean, dL, dF (the constraint path's cotangents
    added through dlogw)."""
    acq, hvi, feas = state
    dmean, dL, dF, dlogw = kernels.qlogehvi_backward(
        mean, L, Z, lo, hi, acq, hvi, dacq, acqf._out_idx,
        feas[0].detach() if feas is not None else None, F=F, Qp=Qp, fat=acqf.fat,
        tau_relu=acqf.tau_relu, tau_max=acqf.tau_max)
    if feas is not None:
        _feas_backward(feas, dlogw, dmean, dL, dF)
    return dmean, dL, dF


class _QLogEHVIFromRoots(torch.autograd.Function):
    """_QEHVIFeasFromRoots in log space (bo_qlogehvi): a differentiable
    function of (mean, L, F, logw); logw may be None."""

    @staticmethod
    def forward(ctx, mean, L, F, logw, Zq, lo, hi, q, out_idx, fat, tau_relu, tau_max):
        acq, hvi = kernels.qlogehvi(mean, L, Zq, lo, hi, out_idx, logw, F=F, Qp=q, fat=fat,
                                    tau_relu=tau_relu, tau_max=tau_max)
        ctx.save_for_backward(mean, L, F, logw, Zq, lo, hi, acq, hvi)
        ctx.opts = (q, out_idx, fat, tau_relu, tau_max)
        return acq

    @staticmethod
    def backward(ctx, dacq):
        mean, L, F, logw, Zq, lo, hi, acq, hvi = ctx.saved_tensors
        q, out_idx, fat, tau_relu, tau_max = ctx.opts
        dmean, dL, dF, dlogw = kernels.qlogehvi_backward(
            mean, L, Zq, lo, hi, acq, hvi, dacq.contiguous(), out_idx, logw, F=F, Qp=q, fat=fat,
            tau_relu=tau_relu, tau_max=tau_max)
        return (dmean, dL, dF, dlogw) + (None,) * 8


class qNoisyExpectedHypervolumeImprovement(qExpectedHypervolumeImprovement):
    """MC q-noisy expected hypervolume improvement (acquisition/multi_objective/
    monte_carlo.py:325-468; NoisyExpectedHypervolumeMixin,
    utils/multi_objective/hypervolume.py:507-835) for a ModelListGP of
    SingleTaskGPs:

      qNEHVI(X) = mean_s HVI(f_s(X, X_pending) | Pareto front of f_s(X_baseline))
                  + prev_nehvi.

    Construction: the joint baseline samples (Sobol dimension r m), one box
    decomposition of the non-dominated region per sample (exact:
    FastNondominatedPartitioning; alpha > 0: the approximate binary
    partitioning of NondominatedPartitioning, m > 2; both in native host code,
    as the reference runs them on the CPU for m > 2), padded with empty cells to
    a common count (BoxDecompositionList), resident on the device as S x K x m.
    Forward / backward: _FusedHVI over the q new points and the pending
    points not yet in the baseline.

    cache_root=False: every forward samples the joint posterior of each
    t-batch with its own root (_joint_forward) instead of the cached baseline
    root and its low-rank update; the same quantity up to the jitter of the
    (r + q) root.

    Pending points (hypervolume.py:778-822): with cache_pending, more than
    max_iep new ones join the baseline and the decompositions are rebuilt
    (without incremental_nehvi, the hypervolume they add to every sample's
    front, mean_s (HV_s - HV0_s)+, is carried in prev_nehvi); up to max_iep, or
    all of them without cache_pending, are appended to every forward's q-batch
    (concatenate_pending_points).

    Outcome constraints (hypervolume.py:725-767): roots and base samples cover
    all Mt members; every sample's decomposition is built from its strictly
    feasible baseline points in objective space (pending points that join the
    baseline included), the new points are weighted softly as in qEHVI."""

    _default_sample_shape = torch.Size([128])

    def __init__(self, model, ref_point, X_baseline, sampler=None, objective=None,
                 constraints=None, X_pending=None, eta=1e-3, fat=False, prune_baseline=False,
                 alpha=0.0, cache_pending=True, max_iep=0, incremental_nehvi=True,
                 cache_root=True, marginalize_dim=None):
        if len(ref_point) < 2:
            raise ValueError("NoisyExpectedHypervolumeMixin supports m>=2 outcomes "
                             f"but ref_point has length {len(ref_point)}, which is smaller than 2.")
        if X_baseline.ndim > 2:
            raise UnsupportedError("NoisyExpectedHypervolumeMixin does not support batched "
                                   f"X_baseline. Expected 2 dims, got {X_baseline.ndim}.")
        models = getattr(model, "models", None)
        if models is None or not all(hasattr(mm, "prediction_cache") for mm in models):
            raise UnsupportedError("qNEHVI here runs on a ModelListGP of SingleTaskGPs")
        AcquisitionFunction.__init__(self, model)
        _init_outcome_constraints(self, len(models), objective, constraints, eta, fat,
                                  len(ref_point))
        if len(self._out_idx) != len(ref_point):
            raise ValueError("The length of the reference point must match the number of outcomes.")
        self.sampler = sampler
        self.objective = objective if objective is not None else IdentityMCMultiOutputObjective()
        if not isinstance(self.objective, IdentityMCMultiOutputObjective):
            raise UnsupportedError("only the identity multi-output objective is accelerated")
        self.posterior_transform = None
        self.ref_point = torch.as_tensor(ref_point, dtype=torch.float64, device=X_baseline.device)
        self.alpha = alpha
        self.cache_pending = bool(cache_pending)
        self._max_iep = int(max_iep)
        self.incremental_nehvi = bool(incremental_nehvi)
        self._cache_root = bool(cache_root)
        self.X_pending = None
        if prune_baseline:
            X_baseline = prune_inferior_points_multi_objective(
                model, X_baseline, self.ref_point,
                objective=self.objective if self._weighted else None,
                constraints=self.constraints, marginalize_dim=marginalize_dim)
        self._X_baseline = X_baseline
        self._X_baseline_and_pending = X_baseline
        self._partitioned = False
        # on the baseline's device, as the reference's tkwargs buffer
        # (hypervolume.py:619-622): a host scalar here made every forward's
        # ``+ prev_nehvi`` a pageable copy that drained the stream (C4
        # qNEHVI forward + backward: ~150 us of idle device per call)
        self.register_buffer("_prev_nehvi", torch.tensor(0.0, dtype=torch.float64,
                                                         device=X_baseline.device))
        if X_pending is not None:
            self.set_X_pending(X_pending)
        # hypervolume.py:643-644: the first decomposition, unless set_X_pending
        # already made it (more than max_iep pending points joined the
        # baseline).  Without cache_pending nothing joins, and the reference's
        # condition would skip the decomposition altogether (its first forward
        # then fails on the missing cell bounds): it is made here.
        if not self._partitioned:
            self._set_cell_bounds()

    @property
    def X_baseline(self) -> torch.Tensor:
        return self._X_baseline_and_pending

    def set_X_pending(self, X_pending=None) -> None:
        """hypervolume.py:778-822."""
        if X_pending is None:
            self.X_pending = None
            return
        if X_pending.requires_grad:
            warnings.warn("Pending points require a gradient but the acquisition function"
                          " will not provide a gradient to these points.", BotorchWarning)
        X_pending = X_pending.detach().clone()
        if not self.cache_pending:
            self.X_pending = X_pending
            return
        joined = torch.cat([self._X_baseline, X_pending], dim=-2)
        num_new = joined.shape[0] - self.X_baseline.shape[0]
        if num_new <= 0:
            return
        if num_new > self._max_iep:
            self._X_baseline_and_pending = joined
            self._set_cell_bounds()
            if not self.incremental_nehvi:
                self._prev_nehvi = (self._hypervolumes - self._initial_hvs).clamp_min(0.0).mean()
            self.X_pending = None
        else:
            self.X_pending = X_pending[-num_new:]

    def _set_cell_bounds(self) -> None:
        """hypervolume.py:680-776: baseline samples and one box decomposition per
        MC sample (native host threads), padded to a common cell count
        (box_decomposition_list.py:62-94), then resident on the device.  The
        first decomposition of a non-incremental qNEHVI records every sample's
        baseline hypervolume (_compute_initial_hvs, :654-678)."""
        Xb = self.X_baseline
        models = self.model.models
        r, m = Xb.shape[-2], len(models)
        if r == 0:
            raise UnsupportedError("qNEHVI here needs at least one baseline point")
        sampler = self._ensure_sampler()
        S = sampler.sample_shape.numel()
        Zb = kernels.sobol_normal(r * m, S, sampler.seed, Xb.device).view(S, r, m)
        self._roots = [_CachedBaselineRoot(mm, Xb, Zb[:, :, t].contiguous())
                       for t, mm in enumerate(models)]
        # the members' stacked root operands (_roots_forward_batched /
        # _roots_backward_batched) belong to the previous roots: a baseline
        # that grew by pending points has a different r
        self.__dict__.pop("_root_stack", None)
        self.__dict__.pop("_root_stack_qb", None)
        if not all(rt.fused_ready for rt in self._roots):
            raise UnsupportedError(f"qNEHVI here needs d <= {kernels.DP}")
        Y = torch.stack([rt.samples for rt in self._roots], dim=-1).cpu()  # S x r x m
        self.baseline_samples = Y
        if self._weighted:
            # hypervolume.py:725-767: every sample's decomposition is built from
            # its feasible baseline points (the hard, strict indicator of the
            # samples of all members) in objective space.  The host
            # decomposition keeps only the points strictly above the reference
            # point, so an infeasible row overwritten with the reference point
            # is dropped: exactly the cells of the filtered set.
            obj = Y[..., self._out_idx].clone()
            if self.constraints is not None:
                feas = compute_feasibility_indicator(self.constraints, Y)     # S x r
                obj[~feas] = self.ref_point.cpu()
            Y = obj
            m = Y.shape[-1]
        self._baseline_obj = Y
        if self.alpha > 0 and m > 2:  # NondominatedPartitioning(alpha); m = 2 is exact there
            lo, hi = kernels.nd_partition_host(Y, self.ref_point.cpu(), alpha=self.alpha)
        else:
            lo, hi = kernels.nd_partition_host(Y, self.ref_point.cpu())  # native, threaded
        self.cell_lower_bounds = lo.to(Xb.device)
        self.cell_upper_bounds = hi.to(Xb.device)
        self._cells = (self.cell_lower_bounds, self.cell_upper_bounds)
        self._zq = {}
        if not self._partitioned and not self.incremental_nehvi:
            # _compute_initial_hvs (:654-678): the feasible points' hypervolume
            self._initial_hvs = dominated_hypervolume(Y, self.ref_point.cpu()).to(self.ref_point)
        self._partitioned = True

    @property
    def _hypervolumes(self) -> torch.Tensor:
        """hypervolume.py:824-835: every sample's hypervolume over the current
        baseline, from its cells (non_dominated.py:445-457)."""
        return cells_hypervolume(self._baseline_obj, self.ref_point.cpu(),
                                 self.cell_lower_bounds.cpu(),
                                 self.cell_upper_bounds.cpu()).to(self.ref_point)

    def _base_samples_q(self, q: int, device) -> torch.Tensor:
        """The q m new columns of the (r+q) m-dim Sobol draw (sampling/normal.py:
        68-131): point-major, output-minor, i.e. column p m + t for new point p."""
        if q not in self._zq:
            r, m = self.X_baseline.shape[-2], len(self.model.models)
            S = self.sampler.sample_shape.numel()
            full = kernels.sobol_normal((r + q) * m, S, self.sampler.seed, device)
            self._zq[q] = full[:, r * m:].contiguous()
        return self._zq[q]

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = self._concat_pending(t_batch_mode(X))
        batch = X.shape[:-2]
        q, d = X.shape[-2], X.shape[-1]
        _check_log_q(self, q)
        if q > 12 or d > kernels.DP or not X.is_cuda:
            raise UnsupportedError(f"fused qNEHVI supports q <= 12 (pending points included) "
                                   f"and d <= {kernels.DP} on the device")
        X3 = X.reshape(-1, q, d)
        if self._cache_root:
            acq = _FusedHVI.apply(X3, self, True)
        else:
            acq = self._joint_forward(X3)
        if self._log:
            if self.incremental_nehvi:
                return acq.reshape(batch)
            # logei.py:471: the pending points' hypervolume joins in log space
            return logplusexp(acq.reshape(batch), self._prev_nehvi.to(acq).log())
        return acq.reshape(batch) + self._prev_nehvi.to(acq)

    def _joint_forward(self, X3: torch.Tensor) -> torch.Tensor:
        """cache_root=False (monte_carlo.py:444-468, cached_cholesky.py:161-165):
        every forward samples the joint posterior over [X_baseline; X] of each
        t-batch -- its own jittered (r + q) Cholesky -- with the cached
        baseline base samples in the leading r columns (the base sampler's)
        and the new point's columns after them, and keeps the new rows:
        f = mean_X + Z_b L[X, b]^T + L[X, X] z.  The hypervolume improvement
        over the per-sample cells is the fused kernel's; moments, the joint
        root and its gradient are the general differentiable kernels'."""
        B, q, d = X3.shape
        Xb = self.X_baseline.to(X3)
        r = Xb.shape[-2]
        Xf = torch.cat([Xb.expand(B, r, d), X3], dim=-2)
        means, Ls, Fs = [], [], []
        for t, mm in enumerate(self.model.models):
            post = mm.posterior(Xf)
            mean = post.distribution.mean.reshape(B, r + q)
            Lj = post.distribution.scale_tril.reshape(B, r + q, r + q)
            Zb = self._roots[t].Z_base.to(Lj)                              # S x r
            F = torch.matmul(Zb, Lj[:, r:, :r].mT).permute(1, 0, 2)       # S x B x q
            means.append(mean[:, r:])
            Ls.append(Lj[:, r:, r:])
            Fs.append(F.reshape(Zb.shape[0], B * q))
        Zq = self._base_samples_q(q, X3.device)
        lo, hi = self._cells
        mean, L, F = torch.stack(means), torch.stack(Ls), torch.stack(Fs)
        if not self._log and not self._weighted:
            return _QEHVIFromRoots.apply(mean, L, F, Zq, lo, hi, q)
        w = None  # the points' (log) feasibility weights, S x B x q
        if self.constraints is not None:
            f = _member_samples(mean, L, Zq, F, q)
            w = compute_smoothed_feasibility_indicator(
                self.constraints, f, self.eta.to(f), log=self._log,
                fat=self.fat).to(torch.float64).contiguous()
        if self._log:
            return _QLogEHVIFromRoots.apply(mean, L, F, w, Zq, lo, hi, q, tuple(self._out_idx),
                                            self.fat, self.tau_relu, self.tau_max)
        if w is None:
            w = torch.ones(Zq.shape[0], B, q, dtype=torch.float64, device=X3.device)
        return _QEHVIFeasFromRoots.apply(mean, L, F, w, Zq, lo, hi, q, tuple(self._out_idx))


class qLogExpectedHypervolumeImprovement(qExpectedHypervolumeImprovement):
    """MC qLogEHVI (acquisition/multi_objective/logei.py:48-317): the expected
    hypervolume improvement with every clamp and minimum replaced by a smooth,
    (with ``fat``) fat-tailed one, evaluated in log space, so the value stays
    finite and the gradient informative where plain qEHVI is exactly zero.

    Everything up to the reduction is qExpectedHypervolumeImprovement's (the
    members' posteriors and roots, pending points, outcome constraints with
    the log smoothed feasibility); the reduction is bo_qlogehvi /
    bo_qlogehvi_backward over all subsets of the q <= 8 points (pending points
    included).  The defaults are the reference's (logei.py:54-67)."""

    _log = True

    def __init__(self, model, ref_point, partitioning, sampler=None, objective=None,
                 constraints=None, X_pending=None, eta=1e-2, fat=True,
                 tau_relu: float = TAU_RELU, tau_max: float = TAU_MAX):
        tau_relu, tau_max = _check_tau(tau_relu, "tau_relu"), _check_tau(tau_max, "tau_max")
        super().__init__(model, ref_point, partitioning, sampler=sampler, objective=objective,
                         constraints=constraints, X_pending=X_pending, eta=eta, fat=fat)
        self.tau_relu, self.tau_max = tau_relu, tau_max


class qLogNoisyExpectedHypervolumeImprovement(qNoisyExpectedHypervolumeImprovement):
    """MC qLogNEHVI (acquisition/multi_objective/logei.py:320-471):
    qNoisyExpectedHypervolumeImprovement's cached baseline roots, per-sample box
    decompositions and pending-point handling, with qLogEHVI's log-space
    reduction (bo_qlogehvi over the per-sample cells, whose padding cells are
    skipped).  Without incremental_nehvi the pending points' hypervolume joins
    as logplusexp(value, log prev_nehvi) (:471).  The defaults are the
    reference's (:327-347)."""

    _log = True

    def __init__(self, model, ref_point, X_baseline, sampler=None, objective=None,
                 constraints=None, X_pending=None, eta=1e-3, prune_baseline=False, alpha=0.0,
                 cache_pending=True, max_iep=0, incremental_nehvi=True, cache_root=True,
                 tau_relu: float = TAU_RELU, tau_max: float = 1e-3, fat=True,
                 marginalize_dim=None):
        tau_relu, tau_max = _check_tau(tau_relu, "tau_relu"), _check_tau(tau_max, "tau_max")
        super().__init__(model, ref_point, X_baseline, sampler=sampler, objective=objective,
                         constraints=constraints, X_pending=X_pending, eta=eta, fat=fat,
                         prune_baseline=prune_baseline, alpha=alpha, cache_pending=cache_pending,
                         max_iep=max_iep, incremental_nehvi=incremental_nehvi,
                         cache_root=cache_root, marginalize_dim=marginalize_dim)
        self.tau_relu, self.tau_max = tau_relu, tau_max


def cells_hypervolume(Y: torch.Tensor, ref: torch.Tensor, lo: torch.Tensor,
                      hi: torch.Tensor) -> torch.Tensor:
    """FastNondominatedPartitioning.compute_hypervolume (box_decompositions/
    non_dominated.py:445-457) per sample: the box [ref, ideal] less the
    non-dominated cells clipped to it; ideal = the best value of every outcome
    over the points above ref (those of the Pareto front); 0 without one.
    Y: S x n x m, lo / hi: S x K x m (padded cells are empty)."""
    above = (Y > ref).all(dim=-1, keepdim=True)
    ideal = torch.where(above, Y, torch.full_like(Y, float("-inf"))).max(dim=-2, keepdim=True).values
    has = above.any(dim=-2).squeeze(-1)
    total = (ideal.squeeze(-2) - ref).clamp_min(0.0).prod(dim=-1)
    clip_lo, clip_hi = torch.minimum(lo, ideal), torch.minimum(hi, ideal)
    non_dom = (clip_hi - clip_lo).clamp_min(0.0).prod(dim=-1).sum(dim=-1)
    return torch.where(has, total - non_dom, torch.zeros_like(total))


def dominated_hypervolume(Y: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Every sample's dominated hypervolume (DominatedPartitioning.
    compute_hypervolume, box_decompositions/dominated.py:51-62, as
    _compute_initial_hvs uses it): through the exact non-dominated cells of the
    same points, whose complement in [ref, ideal] it is."""
    lo, hi = kernels.nd_partition_host(Y, ref)
    return cells_hypervolume(Y, ref, lo, hi)


# -- Bayesian active learning by disagreement (acquisition/bayesian_active_learning.py) ------
class FullyBayesianAcquisitionFunction(AcquisitionFunction):
    """bayesian_active_learning.py:34-49: the base of the acquisitions that need
    an MCMC ensemble."""

    def __init__(self, model):
        if not getattr(model, "_is_fully_bayesian", False):
            raise ValueError("Fully Bayesian acquisition functions require "
                             "a SaasFullyBayesianSingleTaskGP to run.")
        super().__init__(model)


def _bald_value(mean: torch.Tensor, L: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """out (B x M) = H_b - C_bm of bayesian_active_learning.py:96-126 in torch,
    on any device: mean (B x M x q) and L (B x M x q x q) the components of the
    mixture posterior (observation noise included), y (S x B x M x q) their
    samples.  The log-density of every sample under every component is the
    S x B x M x M tensor the fused kernel never stores.  The mixture density is
    taken as a log-sum-exp where the reference writes exp().mean().log(): the
    same number wherever that is finite."""
    M, q = mean.shape[-2], mean.shape[-1]
    eye = torch.eye(q, dtype=L.dtype, device=L.device).expand_as(L)
    Linv = torch.linalg.solve_triangular(L, eye, upper=False)
    r = y.unsqueeze(-2) - mean.unsqueeze(-3)                    # S x B x M (drawn) x M (evaluated) x q
    w = torch.einsum("bnij,sbmnj->sbmni", Linv, r)
    half_log_det = L.diagonal(dim1=-2, dim2=-1).log().sum(-1)   # B x M
    lp = (-0.5 * w.pow(2).sum(-1) - half_log_det.unsqueeze(-2)
          - 0.5 * q * math.log(2.0 * math.pi))                  # S x B x M x M
    H = -(torch.logsumexp(lp, dim=-1) - math.log(M)).mean(dim=(0, 2))
    C = -lp.diagonal(dim1=-2, dim2=-1).mean(dim=0)
    return H.unsqueeze(-1) - C


class _FusedBALD(torch.autograd.Function):
    """BALD over the MCMC ensemble of a SAAS model in batched launches: the
    ensemble moments as in _SaasQEI.forward, the members' noise on the diagonal
    (model space, before the outcome untransform), the jittered q x q roots
    (bo_chol_small over M x B) and bo_bald; averaged over M.  Backward:
    bo_bald_backward -> d mu, d L; bo_chol_backward -> d Sigma; then the d mu,
    d Sigma chain of _SaasQEI.backward."""

    @staticmethod
    def forward(ctx, X3, acqf, Z):
        model = acqf.model
        B, q, d = X3.shape
        dev = X3.device
        X2 = X3.detach().reshape(B * q, d).contiguous()
        ym, ys = model.outcome_stats()
        ens = model.ensemble_cache()
        M, n = ens["U"].shape[0], ens["n"]
        f64 = dict(dtype=torch.float64, device=dev)
        Bq = B * q
        Kx = torch.empty(M, Bq, n, **f64)
        kernels.covar_batched(ens["kind"], X2, (0, 0), Bq, ens["Xt"], (0, 0), n, d, ens["ls"],
                              (d, 0), ens["os"], (1, 0), Kx, (Bq * n, 0), n, M, 1)
        R = kernels.gemm(Kx, ens["U"], flags=_lib.GEMM_B_UPPER)              # M x Bq x n
        mean = kernels.gemm(Kx, ens["alpha"].unsqueeze(-1)).reshape(M, B, q)
        RR = kernels.gemm(R.view(M * B, q, n), R.view(M * B, q, n), transB=True)  # MB x q x q
        Kxx = torch.empty(M * B, q, q, **f64)
        kernels.covar_batched(ens["kind"], X2, (0, q * d), q, X2, (0, q * d), q, d, ens["ls"],
                              (d, 0), ens["os"], (1, 0), Kxx, (B * q * q, q * q), q, M, B)
        cov = Kxx - RR
        tau2 = torch.stack([mm.likelihood.noise.reshape(()) for mm in model._members]).to(**f64)
        cov.view(M, B, q, q).diagonal(dim1=-2, dim2=-1).add_(tau2.view(M, 1, 1))
        cov *= ys * ys
        mean = (ym + ys * (mean + ens["const"].view(M, 1, 1))).reshape(M * B, q)
        L = kernels.chol_jitter(cov)                                          # MB x q x q
        acq = kernels.bald(mean, L, Z, M).mean(dim=-1)
        if ctx.needs_input_grad[0]:
            ctx.ens, ctx.X2, ctx.Z, ctx.shape, ctx.ys = ens, X2, Z, (B, q, d), ys
            ctx.R, ctx.mean, ctx.L = R, mean, L
        return acq

    @staticmethod
    def backward(ctx, dacq):
        B, q, d = ctx.shape
        ens, ys = ctx.ens, ctx.ys
        M, n = ens["U"].shape[0], ens["n"]
        dout = (dacq / M).unsqueeze(-1).expand(B, M).contiguous()
        dmean, dL = kernels.bald_backward(dout, ctx.mean, ctx.L, ctx.Z, M)
        dcov = kernels.chol_backward(ctx.L, dL)                               # MB x q x q
        dmu = (ys * dmean).reshape(M, B * q)                                  # standardized
        G = ((ys * ys) * (dcov + dcov.mT)).contiguous()
        W = kernels.gemm(ctx.R, ens["U"], transB=True, flags=_lib.GEMM_B_LOWER)  # M x Bq x n
        dK = (dmu.unsqueeze(-1) * ens["alpha"].unsqueeze(1)).contiguous()    # M x Bq x n
        kernels.gemm(G, W.view(M * B, q, n), alpha=-1.0, beta=1.0, C=dK.view(M * B, q, n))
        Gm = G.view(M, B * q, q)
        dX = None
        for mi in range(M):
            ls = ens["ls"][mi]
            os_ = ens["os_host"][mi]
            dX = kernels.kernel_grad(ctx.X2, ens["Xt"], dK[mi], ls, ens["kind"], os_, dX=dX)
            dX = kernels.kernel_grad(ctx.X2, ctx.X2, Gm[mi].contiguous(), ls, ens["kind"], os_,
                                     group=q, dX=dX)
        return dX.reshape(B, q, d), None, None


class qBayesianActiveLearningByDisagreement(FullyBayesianAcquisitionFunction):
    """Batch BALD (bayesian_active_learning.py:52-126): the mutual information
    between the next q noisy observations and the model's hyperparameters, as
    the entropy of the Gaussian-mixture posterior of the MCMC ensemble minus the
    mean entropy of its components, by Monte Carlo over base samples shared by
    the components.  On the device, for q (pending points included) <= 16 and
    up to 64 ensemble members without a posterior transform, one fused launch
    evaluates every sample under every component in registers (bald.hip,
    DESIGN.md section 20); everything else takes ``_generic``, the same formula
    in torch."""

    _default_sample_shape = torch.Size([512])
    _GENERIC_CHUNK = 1 << 25  # doubles of one S x B x M x M x q intermediate per chunk

    def __init__(self, model, sampler: Optional[MCSampler] = None, posterior_transform=None,
                 X_pending=None):
        super().__init__(model)
        model.num_mcmc_samples  # (RuntimeError for a model that has not been fitted)
        if model.training:
            raise UnsupportedError("qBayesianActiveLearningByDisagreement needs a model in eval "
                                   "mode (model.eval())")
        self.sampler = sampler if sampler is not None else SobolQMCNormalSampler(
            self._default_sample_shape)
        self.posterior_transform = posterior_transform
        self.set_X_pending(X_pending)

    @property
    def sample_shape(self) -> torch.Size:
        return self.sampler.sample_shape

    def _fused_ok(self, X: torch.Tensor) -> bool:
        return (X.is_cuda and self.posterior_transform is None and X.shape[-2] <= FUSED_QMAX
                and X.shape[-1] <= 128 and self.model.num_mcmc_samples <= kernels.BALD_MMAX
                and len(self.sample_shape) == 1 and hasattr(self.sampler, "base_samples_2d")
                and self.sample_shape.numel() <= kernels.BALD_SMAX)

    def _generic(self, X: torch.Tensor) -> torch.Tensor:
        """The reference's formula in torch on the model's posterior, in chunks of
        t-batches that bound the S x B x M x M x q intermediates."""
        batch, q, d = X.shape[:-2], X.shape[-2], X.shape[-1]
        X3 = X.reshape(-1, q, d)
        if X3.shape[0] == 0:
            return X.new_empty(batch)
        M, S = self.model.num_mcmc_samples, self.sample_shape.numel()
        chunk = max(1, self._GENERIC_CHUNK // (M * M * S * q))
        ns = len(self.sample_shape)
        vals = []
        for Xc in X3.split(chunk):
            post = self.model.posterior(Xc, observation_noise=True,
                                        posterior_transform=self.posterior_transform)
            y = self.sampler(post).squeeze(-1)                # sample_shape x B x M x q
            mvn = post.distribution
            vals.append(_bald_value(mvn.loc, mvn.scale_tril, y.flatten(0, ns - 1)).mean(dim=-1))
        return torch.cat(vals).reshape(batch)

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = self._concat_pending(t_batch_mode(X))
        if not self._fused_ok(X):
            return self._generic(X)
        batch, q, d = X.shape[:-2], X.shape[-2], X.shape[-1]
        X3 = X.reshape(-1, q, d).to(torch.float64)
        if X3.shape[0] == 0:
            return X.new_empty(batch)
        Z = self.sampler.base_samples_2d(q, X.device)
        return _FusedBALD.apply(X3, self, Z).reshape(batch).to(X.dtype)


def _acq_device(acqf) -> Optional[torch.device]:
    """The device an acquisition's model lives on (its training inputs, or a
    ModelListGP member's), None when it has none."""
    model = getattr(acqf, "model", None)
    for m in [model] + list(getattr(model, "models", None) or []):
        ti = getattr(m, "train_inputs", None) if m is not None else None
        if ti:
            return ti[0].device
    return None


class FixedFeatureAcquisitionFunction(AcquisitionFunction):
    """acquisition/fixed_feature.py:54-200: the base acquisition over the full
    d-dim input, evaluated on X of dim d' = d - d_f with the ``columns`` filled
    from ``values``.  The optimisers use it to drop fixed features from the
    search space (generation/utils.py:102-196).  The fixed values live on the
    base acquisition's device from construction, and filling the columns is one
    concatenation and one index_select with a device index, so no host data
    moves per call and the fused forward of the base acquisition (and its
    HIP-graph capture) is unchanged."""

    def __init__(self, acq_function: AcquisitionFunction, d: int, columns: List[int], values):
        nn.Module.__init__(self)
        self.acq_func = acq_function
        self.d = d
        home = _acq_device(acq_function)
        if torch.is_tensor(values):
            vals = values.detach().clone()
        else:
            # python numbers are fp64 (fixed_feature.py:25-37); tensors keep shape
            single = all(torch.is_tensor(v) and v.dtype == torch.float32 for v in values)
            dtype = torch.float32 if single else torch.float64
            dev = next((v.device for v in values if torch.is_tensor(v) and v.is_cuda),
                       home or torch.device("cpu"))
            parts = []
            for v in values:
                t = torch.tensor([float(v)], dtype=dtype) if not torch.is_tensor(v) else (
                    v.detach().clone().reshape(1) if v.ndim == 0 else v.detach().clone())
                parts.append(t.to(dtype=dtype, device=dev))
            vals = torch.cat(torch.broadcast_tensors(*parts), dim=-1)
        if home is not None:
            vals = vals.to(home)
        self.register_buffer("values", vals)
        # column i of X_full: from X (free) or from the appended values (fixed)
        d_f = vals.shape[-1]
        cols = set(columns)
        free = iter(range(d - d_f))
        fixed = iter(range(d - d_f, d))
        self._selector = [next(fixed) if i in cols else next(free) for i in range(d)]
        self._placed = {}  # (device, dtype) -> (values, device index of the selector)

    @property
    def model(self):
        return self.acq_func.model

    @property
    def X_pending(self):
        try:
            return self.acq_func.X_pending
        except AttributeError:
            raise ValueError(f"Base acquisition function {type(self.acq_func).__name__} does not "
                             "have an `X_pending` attribute.")

    @X_pending.setter
    def X_pending(self, X_pending):
        if "acq_func" not in self._modules:  # AcquisitionFunction.__init__ is skipped
            return
        self.acq_func.X_pending = (self._construct_X_full(X_pending) if X_pending is not None
                                   else None)

    def set_X_pending(self, X_pending=None) -> None:
        self.acq_func.set_X_pending(self._construct_X_full(X_pending) if X_pending is not None
                                    else None)

    def _on(self, X: torch.Tensor):
        """The values and the column selector on X's device and dtype (placed
        once per device / dtype: a call under stream capture copies nothing)."""
        key = (X.device, X.dtype)
        hit = self._placed.get(key)
        v = self.values
        # rebuilt if values was replaced or updated in place (version counter,
        # storage): .to() may have made a copy that an in-place update misses
        src = (v, v._version, v.data_ptr())
        if hit is None or hit[2][0] is not v or hit[2][1:] != src[1:]:
            vals = v.to(device=X.device, dtype=X.dtype)
            sel = torch.tensor(self._selector, dtype=torch.long, device=X.device)
            hit = (vals, sel, src)
            self._placed[key] = hit
        return hit[0], hit[1]

    def _construct_X_full(self, X: torch.Tensor) -> torch.Tensor:
        d_prime, d_f = X.shape[-1], self.values.shape[-1]
        if d_prime + d_f != self.d:
            raise ValueError(f"Feature dimension d' ({d_prime}) of input must be "
                             f"d - d_f ({self.d - d_f}).")
        vals, sel = self._on(X)
        vals = vals.expand(*X.shape[:-1], d_f)
        return torch.cat([X, vals], dim=-1).index_select(-1, sel)

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return self.acq_func(self._construct_X_full(X))
