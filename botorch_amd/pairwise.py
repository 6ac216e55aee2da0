"""Preference learning: PairwiseGP with the Laplace approximation, its marginal log
likelihood and the expected utility of the best option (botorch/models/pairwise_gp.py,
models/likelihoods/pairwise.py, acquisition/preference.py).

The hot path (every closure call of the fit, every change of the hyperparameters) is one
``bo_pairwise_laplace`` launch (csrc/pairwise.hip) for device data
in the range of n where it was measured to win; :func:`pairwise_laplace_torch` has the same
contract in torch fp64 for CPU tensors and every other shape.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional

import torch
from torch import Tensor

from . import _lib, kernels
from .exceptions import NotPSDError, NumericalWarning, UnsupportedError
from .models import GammaPrior, MaternKernel, Model, RBFKernel, ScaleKernel, SmoothedBoxPrior

F64 = torch.float64
ZLIM = 3.0            # PairwiseProbitLikelihood._zlim
SIGMA_JITTER = 1e-8   # acquisition/preference.py
_SQRT2 = math.sqrt(2.0)
# The largest n at which the fused route is the default: the rows of
# profiles/pairwise/bench.json in which its slowest run beats the torch route's fastest
# (the Laplace launch wins at n = 64, 256, 512 and loses at 1024; the
# posterior's forward wins at 64 and 256 and loses at 512 and 1024, its forward + backward
# wins in every row).  Above, the torch route is the default; model._route forces either.
FUSED_LAPLACE_MAX_N = 512
FUSED_POSTERIOR_FORWARD_MAX_N = 256


# ---- the torch route ------------------------------------------------------------------------------
def _kbar(X1: Tensor, X2: Tensor, ls: Tensor, kind: int):
    """(kbar, dkbar/dr^2, r^2) of the unit-outputscale ARD kernel."""
    diff = X1.unsqueeze(-2) / ls - X2.unsqueeze(-3) / ls
    r2 = (diff * diff).sum(-1)
    if kind == _lib.RBF:
        k = torch.exp(-0.5 * r2)
        return k, -0.5 * k, r2
    s5r = math.sqrt(5.0) * torch.sqrt(r2.clamp_min(1e-30))
    e = torch.exp(-s5r)
    return (1.0 + s5r + (5.0 / 3.0) * r2) * e, -(5.0 / 6.0) * (1.0 + s5r) * e, r2


def _probit_terms(zr: Tensor):
    z = zr.clamp(-ZLIM, ZLIM)
    lp = torch.special.log_ndtr(z)
    h = torch.exp(-0.5 * z * z - 0.5 * math.log(2 * math.pi) - lp)
    return z, lp, h, 0.5 * h * (h + z)


def _laplace_row(X, comp, hy, kind, f_init, jitter, tol, maxfev, want_grad):
    n, d = X.shape
    dev = X.device
    zeros = dict(f=torch.zeros(n, dtype=F64, device=dev), alpha=torch.zeros(n, dtype=F64, device=dev),
                 psi=torch.tensor(-math.inf, dtype=F64, device=dev),
                 grad=torch.zeros(d + 1, dtype=F64, device=dev),
                 R=torch.zeros(n, n, dtype=F64, device=dev), iters=0)
    if not (torch.isfinite(hy).all() and (hy > 0).all() and torch.isfinite(X).all()
            and (f_init is None or torch.isfinite(f_init).all())):
        return dict(zeros, status=1)
    os_, ls = hy[0], hy[1:]
    kb, dkb, _ = _kbar(X, X, ls, kind)
    eye = torch.eye(n, dtype=F64, device=dev)
    L, info = torch.linalg.cholesky_ex(os_ * (kb + jitter * eye))
    if int(info) != 0:
        return dict(zeros, status=2)
    m = comp.shape[0]
    Dm = torch.zeros(m, n, dtype=F64, device=dev)
    rows = torch.arange(m, device=dev)
    Dm[rows, comp[:, 0].long()] += 1.0
    Dm[rows, comp[:, 1].long()] -= 1.0
    DL = Dm @ L
    if f_init is None:
        wins = Dm.sum(0)
        f_init = (wins - wins.mean()) / wins.std(unbiased=False).clamp_min(1e-6) * os_.sqrt()
    a = torch.linalg.solve_triangular(L, f_init.reshape(n, 1), upper=False).reshape(n)

    def evaluate(a):
        z, lp, h, c = _probit_terms(DL @ a / _SQRT2)
        g = a - DL.mT @ h / _SQRT2
        return g, c, lp.sum(), h

    def newton_chol(c):
        return torch.linalg.cholesky(eye + DL.mT @ (c.unsqueeze(-1) * DL))

    g, c, sumlog, h = evaluate(a)
    it, status = 0, 3
    while it < maxfev:
        it += 1
        dl = torch.cholesky_solve(g.reshape(n, 1), newton_chol(c)).reshape(n)
        dmax, amax = float(dl.abs().max()), float(a.abs().max())
        if not math.isfinite(dmax):
            return dict(zeros, status=1, iters=it)
        small = dmax <= tol * max(1.0, amax)
        t, g2, stalled = 1.0, float(g @ g), False
        for hv in range(9):
            an = a - t * dl
            gn, cn, sln, hn = evaluate(an)
            if small or float(gn @ gn) < g2:
                break
            if hv == 8:
                stalled = True
                break
            t *= 0.5
        a, g, c, sumlog, h = an, gn, cn, sln, hn
        if not math.isfinite(float(g @ g)):
            return dict(zeros, status=1, iters=it)
        if small or (stalled and dmax <= 1e-9 * max(1.0, amax)):
            status = 0
            break
    Lm = newton_chol(c)
    psi = sumlog - 0.5 * (a @ a) - Lm.diagonal().log().sum()
    alpha = torch.linalg.solve_triangular(L.mT, a.reshape(n, 1), upper=True).reshape(n)
    Cm = Dm.mT @ (c.unsqueeze(-1) * Dm)
    R = torch.linalg.solve_triangular(L.mT, torch.cholesky_solve(L.mT @ Cm, Lm), upper=True)
    R = 0.5 * (R + R.mT)
    out = dict(f=L @ a, alpha=alpha, psi=psi, R=R, iters=it, status=status, grad=None)
    if want_grad:
        zr = DL @ a / _SQRT2
        iota = (zr.abs() <= ZLIM).to(F64)
        z = zr.clamp(-ZLIM, ZLIM)
        Q = torch.linalg.solve_triangular(Lm, DL.mT, upper=False)     # L_m^{-1} L^T d_k
        s = (Q * Q).sum(0)
        hp = -h * (h + z)
        cp = 0.5 * (hp * (2.0 * h + z) + h)
        u = Dm.mT @ (-(1.0 - iota) * h / _SQRT2 - 0.5 * iota * cp * s / _SQRT2)
        Lmi = newton_chol(iota * c) if bool((iota == 0).any()) else Lm
        v = torch.linalg.solve_triangular(
            L.mT, torch.cholesky_solve((L.mT @ u).reshape(n, 1), Lmi), upper=True).reshape(n)
        W = 0.5 * (torch.outer(alpha, alpha) - R + torch.outer(alpha, v) + torch.outer(v, alpha))
        diff2 = (X.unsqueeze(1) - X.unsqueeze(0)) ** 2
        g_ls = -2.0 * os_ * torch.einsum("ik,ikj->j", W * dkb, diff2) / ls ** 3
        out["grad"] = torch.cat([(W * (kb + jitter * eye)).sum().reshape(1), g_ls])
    bad = not all(bool(torch.isfinite(t).all()) for t in (out["f"], alpha, psi, R)
                  + ((out["grad"],) if want_grad else ()))
    return dict(zeros, status=1, iters=it) if bad else out


def pairwise_laplace_torch(X: Tensor, comp: Tensor, hyper: Tensor, kind: int,
                           f_init: Optional[Tensor] = None, jitter: float = 0.0,
                           tol: float = 1e-13, maxfev: int = 50, want_grad: bool = True):
    """kernels.pairwise_laplace's contract in torch fp64 on X's device: Newton on the
    whitened system, the closed-form gradient and the same statuses, a row at a time."""
    C = hyper.shape[0]
    with torch.no_grad():
        rows = [_laplace_row(X.to(F64), comp, hyper[c].to(F64), kind,
                             None if f_init is None else f_init[c], jitter, tol, maxfev, want_grad)
                for c in range(C)]
    out = {k: torch.stack([r[k] for r in rows]) for k in ("f", "alpha", "psi", "R")}
    out["grad"] = torch.stack([r["grad"] for r in rows]) if want_grad else None
    for k in ("iters", "status"):
        out[k] = torch.tensor([r[k] for r in rows], dtype=torch.int32, device=X.device)
    return out


# ---- likelihood -----------------------------------------------------------------------------------
class PairwiseProbitLikelihood:
    """models/likelihoods/pairwise.py:102-169 in torch (``D``: the m x n comparison matrix)."""

    _zlim = ZLIM

    def _z(self, utility, D):
        return (D.to(utility) @ (utility / _SQRT2).unsqueeze(-1)).squeeze(-1).clamp(-ZLIM, ZLIM)

    def p(self, utility, D):
        return torch.special.ndtr(self._z(utility, D))

    def log_p(self, utility, D):
        return torch.special.log_ndtr(self._z(utility, D))

    def negative_log_gradient_sum(self, utility, D):
        h = _probit_terms(self._z(utility, D))[2]
        return ((h / _SQRT2).unsqueeze(-2) @ (-D.to(utility))).squeeze(-2)

    def negative_log_hessian_sum(self, utility, D):
        c = _probit_terms(self._z(utility, D))[3]
        D = D.to(utility)
        return D.mT @ (c.unsqueeze(-1) * D)


class PairwiseLogitLikelihood:
    def __init__(self, *a, **k):
        raise UnsupportedError("PairwiseLogitLikelihood is not on the accelerated path "
                               "(PairwiseProbitLikelihood is)")


# ---- the model --------------------------------------------------------------------------------------
class PairwiseGP(Model):
    """models/pairwise_gp.py:117-1152 for one set of datapoints (n x d) and comparisons
    (m x 2, "first preferred to second"): probit likelihood, zero prior mean, a
    ScaleKernel over an RBF or Matern-5/2 ARD kernel.  ``model._route`` forces the
    "fused" or the "torch" route; None takes the fused one for device data where it was
    measured to win (``fused``, ``fused_posterior``)."""

    _is_pairwise = True
    _route = None

    def __init__(self, datapoints, comparisons, likelihood=None, covar_module=None,
                 input_transform=None, *, jitter: float = 1e-6, xtol: Optional[float] = None,
                 consolidate_rtol: float = 0.0, consolidate_atol: float = 1e-4,
                 maxfev: Optional[int] = None):
        super().__init__()
        if input_transform is not None:
            raise UnsupportedError("PairwiseGP: `input_transform` is not on the accelerated path")
        if likelihood is not None and not isinstance(likelihood, PairwiseProbitLikelihood):
            raise UnsupportedError("PairwiseGP: only PairwiseProbitLikelihood is supported "
                                   "(PairwiseLogitLikelihood is not)")
        if datapoints is not None and datapoints.dim() != 2:
            raise UnsupportedError("PairwiseGP: batched datapoints are not on the accelerated path")
        self.likelihood = likelihood if likelihood is not None else PairwiseProbitLikelihood()
        self._jitter, self._xtol, self._maxfev = jitter, xtol, maxfev
        self._consolidate_rtol, self._consolidate_atol = consolidate_rtol, consolidate_atol
        self.dim = None if datapoints is None else datapoints.shape[-1]
        if covar_module is None:
            if self.dim is None:
                raise ValueError("PairwiseGP: a covar_module is required without datapoints")
            prior = GammaPrior(2.4, 2.7)
            covar_module = ScaleKernel(
                RBFKernel(ard_num_dims=self.dim, lengthscale_prior=prior, lengthscale_lower=1e-4,
                          initial=prior.mode),
                outputscale=1.0, outputscale_prior=SmoothedBoxPrior(1e-2, 1e2))
            covar_module.outputscale_bounds = (0.005, 200.0)
        if not (isinstance(covar_module, ScaleKernel)
                and isinstance(covar_module.base_kernel, (RBFKernel, MaternKernel))):
            raise UnsupportedError("PairwiseGP: covar_module must be a ScaleKernel over an "
                                   "RBFKernel or a MaternKernel")
        self.covar_module = covar_module
        self._x0 = None
        self.set_train_data(datapoints, comparisons)

    # -- data
    def _has_no_data(self) -> bool:
        return self.datapoints is None or self.comparisons is None

    def set_train_data(self, datapoints=None, comparisons=None, strict=False, update_model=True):
        if datapoints is None or comparisons is None:
            self.unconsolidated_datapoints = self.unconsolidated_comparisons = None
            self.datapoints = self.comparisons = self._incidence = None
            self.train_inputs, self.train_targets = None, None
            self._cache = None
            return
        if datapoints.dim() != 2:
            raise UnsupportedError("PairwiseGP: batched datapoints are not on the accelerated path")
        self.unconsolidated_datapoints, self.unconsolidated_comparisons = datapoints, comparisons
        X, comp = self._consolidate_duplicates(datapoints.to(F64), comparisons.long())
        self.datapoints, self.comparisons = X.contiguous(), comp
        self.n, self.m, self.dim = X.shape[0], comp.shape[0], X.shape[1]
        self._incidence = kernels.pairwise_incidence(comp, self.n)  # (also validates comp)
        self.train_inputs, self.train_targets = (self.datapoints,), comp
        self._x0 = self._cache = None
        self.covar_module.to(X.device)

    def _consolidate_duplicates(self, X: Tensor, comp: Tensor):
        """pairwise_gp.py:704-745 on the host: datapoints within rtol / atol of an earlier
        one are merged into it and the comparisons renumbered."""
        Xh = X.detach().cpu()
        n = Xh.shape[0]
        close = torch.isclose(Xh.unsqueeze(1), Xh.unsqueeze(0), rtol=self._consolidate_rtol,
                              atol=self._consolidate_atol).all(-1)
        first = close.to(torch.int64).argmax(dim=1)           # the earliest close point
        if bool((first == torch.arange(n)).all()):
            return X, comp
        keep = torch.unique(first)
        new_index = torch.full((n,), -1, dtype=torch.int64)
        new_index[keep] = torch.arange(keep.numel())
        return X[keep.to(X.device)], new_index[first][comp.cpu()].to(comp.device)

    @property
    def utility(self) -> Optional[Tensor]:
        return None if self._has_no_data() else self._laplace()["f"]

    @property
    def num_outputs(self) -> int:
        return 1

    @property
    def batch_shape(self):
        return torch.Size()

    # -- the Laplace approximation
    def fused(self) -> bool:
        """Whether the Laplace approximation takes the fused launch: device data inside
        the kernel's limits with n in the measured range where it wins."""
        if self._route is not None:
            return self._route == "fused"
        if not self.datapoints.is_cuda or self.n > FUSED_LAPLACE_MAX_N:
            return False
        try:
            kernels.pairwise_laplace_check(self.n, self.m, self.dim, 1)
        except ValueError:
            return False
        return True

    def fused_posterior(self, needs_grad: bool) -> bool:
        """Whether ``posterior`` takes the fused moments (posteriors._PairwiseMoments)."""
        if self._route is not None:
            return self._route == "fused"
        return self.datapoints.is_cuda and (needs_grad or self.n <= FUSED_POSTERIOR_FORWARD_MAX_N)

    def hyper_vector(self) -> Tensor:
        return torch.cat([self.covar_module.outputscale.detach().reshape(1),
                          self.covar_module.lengthscale.detach().reshape(-1)]).to(F64)

    def laplace(self, hyper: Tensor, want_grad: bool, warm: bool = True):
        """The Laplace launch at hyper (1 x (d + 1), on the data's device) with the jitter
        ladder of _ensure_psd_with_jitter: no jitter first, then jitter 10^i, i = 0, 1, 2;
        NotPSDError after the last.  Status 3 warns; status 1 is returned as it is."""
        X, kind = self.datapoints, self.covar_module.kind
        tol = 1e-13 if self._xtol is None else self._xtol
        maxfev = 50 if self._maxfev is None else self._maxfev
        f0 = self._x0 if warm else None
        for jit in [0.0] + [self._jitter * 10 ** i for i in range(3)]:
            if self.fused():
                from . import ops  # noqa: F401
                if getattr(self, "_work", None) is None or self._work.device != X.device:
                    self._work = torch.empty(
                        kernels.pairwise_laplace_work(self.n, self.m, self.dim, 1), dtype=F64,
                        device=X.device)
                out = kernels.pairwise_laplace(X, self._incidence, hyper, kind, f0, jit, tol,
                                               maxfev, want_grad, self._work)
            else:
                out = pairwise_laplace_torch(X, self.comparisons, hyper, kind, f0, jit, tol,
                                             maxfev, want_grad)
            # the launch's one device-to-host transfer: [status, psi, gradient]
            parts = [out["status"].to(F64).reshape(-1), out["psi"].reshape(-1)]
            host = torch.cat(parts + ([out["grad"].reshape(-1)] if want_grad else [])).cpu()
            status = int(host[0])
            if status != 2:
                break
        if status == 2:
            raise NotPSDError("PairwiseGP: the covariance is not positive definite after "
                              f"jitter up to {self._jitter * 100:.1e}")
        if status == 3:
            warnings.warn("PairwiseGP: the Newton iteration reached its cap (maxfev)",
                          NumericalWarning)
        if status in (0, 3):
            self._x0 = out["f"].clone()
        out["status_host"], out["host"] = status, host[1:].numpy()
        return out

    def _laplace(self):
        """The cached approximation at the module's hyperparameters, rebuilt lazily after
        a change of data or hyperparameters."""
        ps = (self.covar_module.raw_outputscale, self.covar_module.base_kernel.raw_lengthscale)
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if self._cache is None or self._cache[0] != key:
            hyper = self.hyper_vector().reshape(1, -1).to(self.datapoints.device)
            out = self.laplace(hyper, want_grad=False)
            if out["status_host"] == 1:
                raise NotPSDError("PairwiseGP: non-finite values in the Laplace approximation")
            self._cache = (key, dict(f=out["f"][0], alpha=out["alpha"][0].contiguous(),
                                     R=out["R"][0].contiguous(), psi=out["psi"][0]))
        return self._cache[1]

    # -- posterior
    def posterior(self, X, output_indices=None, observation_noise=False, posterior_transform=None):
        from .posteriors import GPyTorchPosterior, MultivariateNormal, pairwise_moments
        if output_indices is not None:
            raise RuntimeError("output_indices is not None. PairwiseGP should not be a "
                               "multi-output model.")
        mean, cov = pairwise_moments(self, X.to(F64))
        post = GPyTorchPosterior(MultivariateNormal(mean, cov), model=self, X=X)
        return post if posterior_transform is None else posterior_transform(post)

    def condition_on_observations(self, X, Y, **kwargs):
        """pairwise_gp.py:1100-1152: X new datapoints, Y integer comparison pairs among
        them; the model is rebuilt on the joined data."""
        if Y.is_floating_point():
            raise ValueError("PairwiseGP.condition_on_observations: Y must hold integer pairs")
        if self._has_no_data():
            dp, comp = X, Y
        else:
            dp = torch.cat([self.unconsolidated_datapoints, X.to(self.datapoints)], dim=0)
            comp = torch.cat([self.unconsolidated_comparisons,
                              Y.to(self.unconsolidated_comparisons)
                              + self.unconsolidated_datapoints.shape[0]], dim=0)
        import copy
        new = PairwiseGP(dp, comp, likelihood=self.likelihood,
                         covar_module=copy.deepcopy(self.covar_module), jitter=self._jitter,
                         xtol=self._xtol, consolidate_rtol=self._consolidate_rtol,
                         consolidate_atol=self._consolidate_atol, maxfev=self._maxfev)
        new._route = self._route
        return new


class PairwiseLaplaceMarginalLogLikelihood:
    """models/pairwise_gp.py:1155-1217; fit_gpytorch_mll fits it through fit._PairwiseLayout."""

    def __init__(self, likelihood, model: PairwiseGP):
        self.likelihood, self.model = likelihood, model

    def train(self):
        self.model.train()
        return self

    def eval(self):
        self.model.eval()
        return self

    training = property(lambda self: self.model.training)


# ---- acquisition ------------------------------------------------------------------------------------
class AnalyticExpectedUtilityOfBestOption:
    """acquisition/preference.py:38-128: EUBO of a pair (q = 2), or of one point against
    ``previous_winner`` (q = 1), in closed form on the preference model's posterior."""

    def __init__(self, pref_model, outcome_model=None, previous_winner: Optional[Tensor] = None):
        if not getattr(pref_model, "_is_pairwise", False):
            raise UnsupportedError("AnalyticExpectedUtilityOfBestOption needs a PairwiseGP as its "
                                   f"preference model, not a {type(pref_model).__name__}")
        self.model, self.outcome_model, self.previous_winner = pref_model, outcome_model, previous_winner

    def forward(self, X: Tensor) -> Tensor:
        if not ((X.shape[-2] == 2) or (X.shape[-2] == 1 and self.previous_winner is not None)):
            raise UnsupportedError(f"{X.shape[-2]} points were given, but EUBO takes q = 2, or q = 1 "
                                   "with a previous winner")
        Y = X if self.outcome_model is None else self.outcome_model.posterior(X).mean
        if self.previous_winner is not None:
            Y = torch.cat([Y, self.previous_winner.expand(*Y.shape[:-2], -1, -1).to(Y)], dim=-2)
        post = self.model.posterior(Y)
        mean, cov = post.mean.squeeze(-1), post.distribution.covariance_matrix
        delta = mean[..., 0] - mean[..., 1]
        sigma = torch.sqrt((cov[..., 0, 0] + cov[..., 1, 1] - cov[..., 0, 1] - cov[..., 1, 0])
                           .clamp_min(SIGMA_JITTER))
        u = delta / sigma
        pdf = torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
        return mean[..., 1] + sigma * pdf + delta * torch.special.ndtr(u)

    __call__ = forward


class qExpectedUtilityOfBestOption:
    """acquisition/preference.py:131-206: E[max_i f(x_i)] on the preference model's
    posterior, which is qSimpleRegret's reduction: the points (with the pending ones)
    go through the outcome model, if there is one, and then to a qSimpleRegret."""

    def __init__(self, pref_model, outcome_model=None, sampler=None, objective=None,
                 posterior_transform=None, X_pending: Optional[Tensor] = None):
        from .acquisition import qSimpleRegret
        self.model, self.outcome_model, self.X_pending = pref_model, outcome_model, X_pending
        self._reduction = qSimpleRegret(pref_model, sampler=sampler, objective=objective,
                                        posterior_transform=posterior_transform)

    def forward(self, X: Tensor) -> Tensor:
        if self.X_pending is not None:
            X = torch.cat([X, self.X_pending.expand(*X.shape[:-2], -1, -1).to(X)], dim=-2)
        return self._reduction(X if self.outcome_model is None else self.outcome_model.posterior(X).mean)

    __call__ = forward
