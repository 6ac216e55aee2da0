"""Exact GP models with BoTorch's posterior API, backed by the gfx950 kernels.

Mirrors botorch/models/gp_regression.py:68-254 (SingleTaskGP), the default
modules of botorch/models/utils/gpytorch_modules.py:74-127, the Standardize
outcome transform (botorch/models/transforms/outcome.py:217-447) and
ModelListGP (botorch/models/model_list_gp_regression.py:24).  Hyperparameters
are plain fp64 ``nn.Parameter``s holding the constrained values directly (the
reference's constraints use ``transform=None``: raw value == value); their
lower bounds are enforced by L-BFGS-B in ``fit.py`` exactly as
botorch/optim/utils/model_utils.py:69-109 does.

Eval-mode prediction caches (Cholesky factor, L^{-T}, alpha, beta) live on the
device and are rebuilt when any hyperparameter or training tensor changes
version, or on ``train()`` (mirrors [G] ExactGP dropping prediction_strategy).
"""
from __future__ import annotations

import math
import warnings
from typing import List, Optional, Sequence, Union

import torch
from torch import nn

from . import _lib
from .exceptions import InputDataWarning, UnsupportedError

MIN_INFERRED_NOISE_LEVEL = 1e-4  # gpytorch_modules.py:29
LENGTHSCALE_LOWER = 2.5e-2       # gpytorch_modules.py:123
SQRT2, SQRT3 = math.sqrt(2), math.sqrt(3)


# Generation of the model trees' structure: bumped whenever a parameter or a
# submodule is (re)assigned inside one (an in-place change of a parameter's
# values bumps its tensor _version instead).  SingleTaskGP._key() reuses its
# list of parameters until this changes -- walking the module tree on every
# acquisition call was its largest host cost.
_STRUCTURE = [0]


class _TrackedModule(nn.Module):
    """nn.Module whose parameter / submodule (re)assignments bump _STRUCTURE."""

    def __setattr__(self, name, value):
        super().__setattr__(name, value)
        if isinstance(value, (nn.Parameter, nn.Module)):
            _STRUCTURE[0] += 1

    def __delattr__(self, name):
        super().__delattr__(name)
        _STRUCTURE[0] += 1

    def register_parameter(self, name, param):
        super().register_parameter(name, param)
        _STRUCTURE[0] += 1

    def add_module(self, name, module):
        super().add_module(name, module)
        _STRUCTURE[0] += 1


class LogNormalPrior:
    """[G] LogNormalPrior(loc, scale) (torch LogNormal)."""

    def __init__(self, loc: float, scale: float):
        self.loc, self.scale = float(loc), float(scale)

    @property
    def mode(self) -> float:
        return math.exp(self.loc - self.scale ** 2)

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        lx = torch.log(x)
        return (-((lx - self.loc) ** 2) / (2 * self.scale ** 2) - math.log(self.scale)
                - 0.5 * math.log(2 * math.pi) - lx)


class GammaPrior:
    """[G] GammaPrior(concentration, rate) (torch Gamma)."""

    def __init__(self, concentration: float, rate: float):
        self.concentration, self.rate = float(concentration), float(rate)

    @property
    def mode(self) -> float:
        return max(self.concentration - 1.0, 0.0) / self.rate

    def log_prob(self, x: torch.Tensor) -> torch.Tensor:
        a, b = self.concentration, self.rate
        return a * math.log(b) + (a - 1.0) * torch.log(x) - b * x - math.lgamma(a)


class _Kernel(_TrackedModule):
    kind = _lib.RBF

    def __init__(self, ard_num_dims: int, lengthscale_prior: Optional[LogNormalPrior] = None,
                 lengthscale_lower: float = LENGTHSCALE_LOWER, initial: Optional[float] = None):
        super().__init__()
        self.ard_num_dims = ard_num_dims
        self.lengthscale_prior = lengthscale_prior
        self.lengthscale_lower = lengthscale_lower
        init = initial if initial is not None else (
            lengthscale_prior.mode if lengthscale_prior is not None else 1.0)
        self.raw_lengthscale = nn.Parameter(torch.full((1, ard_num_dims), init, dtype=torch.float64))

    @property
    def lengthscale(self) -> torch.Tensor:
        return self.raw_lengthscale

    @lengthscale.setter
    def lengthscale(self, value):
        with torch.no_grad():
            self.raw_lengthscale.copy_(torch.as_tensor(value, dtype=torch.float64).expand_as(self.raw_lengthscale))

    outputscale = 1.0


class RBFKernel(_Kernel):
    """exp(-||(x - x')/ell||^2 / 2)  ([G] RBFKernel)."""
    kind = _lib.RBF


class MaternKernel(_Kernel):
    """Matern-5/2 ([G] MaternKernel(nu=2.5))."""
    kind = _lib.MATERN52

    def __init__(self, nu: float = 2.5, **kw):
        if nu != 2.5:
            raise UnsupportedError("only nu = 2.5 is on the accelerated path")
        super().__init__(**kw)


class ScaleKernel(_TrackedModule):
    """outputscale * base_kernel ([G] ScaleKernel)."""

    def __init__(self, base_kernel: _Kernel, outputscale: float = 1.0, outputscale_prior=None):
        super().__init__()
        self.base_kernel = base_kernel
        self.outputscale_prior = outputscale_prior
        self.raw_outputscale = nn.Parameter(torch.tensor(float(outputscale), dtype=torch.float64))

    kind = property(lambda self: self.base_kernel.kind)
    ard_num_dims = property(lambda self: self.base_kernel.ard_num_dims)

    @property
    def lengthscale(self):
        return self.base_kernel.lengthscale

    @property
    def outputscale(self):
        return self.raw_outputscale

    @outputscale.setter
    def outputscale(self, v):
        with torch.no_grad():
            self.raw_outputscale.fill_(float(v))


class GaussianLikelihood(_TrackedModule):
    """Homoskedastic Gaussian noise ([G] GaussianLikelihood) with BoTorch's
    LogNormal(-4, 1) prior and noise >= 1e-4 (gpytorch_modules.py:74-97)."""

    def __init__(self, noise_prior: Optional[LogNormalPrior] = None,
                 noise_lower: float = MIN_INFERRED_NOISE_LEVEL, initial: Optional[float] = None):
        super().__init__()
        self.noise_prior = noise_prior
        self.noise_lower = noise_lower
        init = initial if initial is not None else (noise_prior.mode if noise_prior else 1e-4)
        self.raw_noise = nn.Parameter(torch.tensor([init], dtype=torch.float64))

    @property
    def noise(self):
        return self.raw_noise

    @noise.setter
    def noise(self, v):
        with torch.no_grad():
            self.raw_noise.copy_(torch.as_tensor(v, dtype=torch.float64).reshape(1))


class FixedNoiseGaussianLikelihood(_TrackedModule):
    """Observed per-point noise variances ([G] FixedNoiseGaussianLikelihood with
    learn_additional_noise=False), the likelihood SingleTaskGP builds from
    train_Yvar (botorch/models/gp_regression.py:187-194).  Nothing is learned:
    ``noise`` is a buffer, there is no prior, and the MLL's K + s2 I becomes
    K + diag(noise)."""

    noise_prior = None
    noise_lower = 0.0

    def __init__(self, noise: torch.Tensor):
        super().__init__()
        self.register_buffer("noise", torch.as_tensor(noise, dtype=torch.float64).reshape(-1).clone())


class ConstantMean(_TrackedModule):
    def __init__(self):
        super().__init__()
        self.raw_constant = nn.Parameter(torch.tensor(0.0, dtype=torch.float64))

    @property
    def constant(self):
        return self.raw_constant

    @constant.setter
    def constant(self, v):
        with torch.no_grad():
            self.raw_constant.fill_(float(v))


def get_covar_module_with_dim_scaled_prior(ard_num_dims: int, use_rbf_kernel: bool = True):
    """gpytorch_modules.py:100-127: LogNormal(sqrt2 + ln(d)/2, sqrt3) lengthscale
    prior, initialised at its mode, lengthscale >= 0.025."""
    prior = LogNormalPrior(SQRT2 + 0.5 * math.log(ard_num_dims), SQRT3)
    cls = RBFKernel if use_rbf_kernel else MaternKernel
    return cls(ard_num_dims=ard_num_dims, lengthscale_prior=prior)


def get_gaussian_likelihood_with_lognormal_prior():
    """gpytorch_modules.py:74-97."""
    return GaussianLikelihood(noise_prior=LogNormalPrior(-4.0, 1.0))


def get_matern_kernel_with_gamma_prior(ard_num_dims: int):
    """gpytorch_modules.py:34-50: ScaleKernel(Matern-5/2) with a Gamma(3, 6) prior on
    the lengthscales and a Gamma(2, 0.15) prior on the outputscale, both starting
    at the reference's initial value softplus(0) = ln 2.  The lengthscales keep
    this package's lower bound (the parameters are the natural values, so
    L-BFGS-B needs one above zero)."""
    base = MaternKernel(ard_num_dims=ard_num_dims, lengthscale_prior=GammaPrior(3.0, 6.0),
                        initial=math.log(2.0))
    return ScaleKernel(base, outputscale=math.log(2.0), outputscale_prior=GammaPrior(2.0, 0.15))


def get_gaussian_likelihood_with_gamma_prior():
    """gpytorch_modules.py:53-71: Gamma(1.1, 0.05) noise prior, noise >=
    MIN_INFERRED_NOISE_LEVEL, initialised at the prior's mode."""
    prior = GammaPrior(1.1, 0.05)
    return GaussianLikelihood(noise_prior=prior, noise_lower=MIN_INFERRED_NOISE_LEVEL,
                              initial=prior.mode)


ICM_VAR_LOWER = 1e-6  # floor of IndexKernel.var in the fit: B[t][t] > 0 for the task view


class IndexKernel(_TrackedModule):
    """[G] IndexKernel(num_tasks, rank): the task covariance B = F F^T + diag(v) of
    the intrinsic coregionalisation model, ``covar_factor`` F (T x rank) and
    ``var`` v (T, the natural values).  Initialised from the global torch
    generator as the reference's is: F ~ randn(T, rank), then v = softplus of
    randn(T) (its Positive constraint at a standard-normal raw value)."""

    def __init__(self, num_tasks: int, rank: int = 1, prior=None):
        super().__init__()
        if prior is not None:
            raise UnsupportedError("IndexKernel: a prior on the task covariance (LKJ) is not "
                                   "on the accelerated path")
        if rank > num_tasks:
            raise RuntimeError("Cannot create a task covariance matrix larger than the number "
                               "of tasks")
        self.num_tasks, self.rank = int(num_tasks), int(rank)
        F = torch.randn(num_tasks, rank).to(torch.float64)
        v = torch.nn.functional.softplus(torch.randn(num_tasks).to(torch.float64))
        self.covar_factor = nn.Parameter(F)
        self.raw_var = nn.Parameter(v.clamp_min(ICM_VAR_LOWER))

    @property
    def var(self) -> torch.Tensor:
        return self.raw_var

    @var.setter
    def var(self, value):
        with torch.no_grad():
            self.raw_var.copy_(torch.as_tensor(value, dtype=torch.float64).reshape(-1))

    @property
    def covar_matrix(self) -> torch.Tensor:
        return self.covar_factor @ self.covar_factor.mT + torch.diag(self.raw_var)


class Standardize(_TrackedModule):
    """Outcome standardisation (botorch/models/transforms/outcome.py:217-447)."""

    def __init__(self, m: int, min_stdv: float = 1e-8):
        super().__init__()
        self._m = m
        self._min_stdv = min_stdv
        self.register_buffer("means", torch.zeros(1, m, dtype=torch.float64))
        self.register_buffer("stdvs", torch.ones(1, m, dtype=torch.float64))
        self._is_trained = False

    def forward(self, Y: torch.Tensor, Yvar: Optional[torch.Tensor] = None):
        if self.training:
            if Y.shape[-2] < 1:
                raise ValueError("Can't standardize with no observations.")
            if Y.shape[-2] == 1:
                stdvs = torch.ones(1, Y.shape[-1], dtype=Y.dtype, device=Y.device)
            else:
                stdvs = Y.std(dim=-2, keepdim=True)
            stdvs = stdvs.where(stdvs >= self._min_stdv, torch.full_like(stdvs, 1.0))
            self.means = Y.mean(dim=-2, keepdim=True)
            self.stdvs = stdvs
            self._is_trained = True
            self._generation = getattr(self, "_generation", 0) + 1
        Y_tf = (Y - self.means) / self.stdvs
        Yvar_tf = Yvar / self.stdvs.pow(2) if Yvar is not None else None
        return Y_tf, Yvar_tf

    def untransform(self, Y, Yvar=None):
        return self.means + self.stdvs * Y, (self.stdvs.pow(2) * Yvar if Yvar is not None else None)


class _StackedView:
    """Read-only view of one module of a multi-output SingleTaskGP's members,
    stacking an attribute over the outputs in the reference's batched shapes
    (likelihood.noise m x 1, covar_module.lengthscale m x 1 x d,
    mean_module.constant m)."""

    def __init__(self, members, name: str):
        object.__setattr__(self, "_mods", [getattr(mm, name) for mm in members])

    def __getattr__(self, attr):
        vals = [getattr(mod, attr) for mod in self._mods]
        if all(torch.is_tensor(v) for v in vals):
            return torch.stack([v.detach() for v in vals])
        if all(isinstance(v, (int, float)) for v in vals):
            return torch.tensor(vals, dtype=torch.float64)
        return vals

    def __setattr__(self, attr, value):
        raise AttributeError("set the hyperparameters of a multi-output SingleTaskGP through "
                             "model.models[t]")


class Model(_TrackedModule):
    """Abstract model with BoTorch's ``posterior`` contract (models/model.py:82-117)."""

    _num_outputs = 1

    @property
    def num_outputs(self) -> int:
        return self._num_outputs

    def posterior(self, X, output_indices=None, observation_noise=False, posterior_transform=None):
        raise NotImplementedError

    def condition_on_observations(self, X, Y, **kwargs):
        """models/model.py:149."""
        raise NotImplementedError(
            f"`condition_on_observations` not implemented for {type(self).__name__}")

    def fantasize(self, X, sampler, observation_noise=None, **kwargs):
        """models/model.py:328-407.  Only a single-output SingleTaskGP builds
        fantasy models here (SingleTaskGP.fantasize)."""
        raise UnsupportedError(
            f"fantasize: {type(self).__name__} is not on the accelerated path (fantasy models "
            "are built from a single-output SingleTaskGP only)")

    def outcome_stats(self):
        """(mean, std) of the Standardize transform as host floats, read back once
        per change of the buffers (not per acquisition call: each read is a
        device-to-host sync)."""
        ot = self._modules.get("outcome_transform")
        if ot is None:
            return 0.0, 1.0
        bufs = ot._buffers  # (direct: nn.Module attribute lookups cost per call)
        m, s = bufs["means"], bufs["stdvs"]
        key = (ot.__dict__.get("_generation", 0), m.data_ptr(), m._version, s.data_ptr(),
               s._version)
        if getattr(self, "_ostats_key", None) != key:
            self._ostats = (float(m.reshape(-1)[0]), float(s.reshape(-1)[0]))
            self._ostats_key = key
        return self._ostats


class SingleTaskGP(Model):
    """Single-output exact GP (botorch/models/gp_regression.py:130-254).

    Defaults: RBF-ARD kernel without outputscale, LogNormal priors,
    ConstantMean, GaussianLikelihood, Standardize(m=1) outcome transform.
    """

    def __init__(self, train_X: torch.Tensor, train_Y: torch.Tensor,
                 train_Yvar: Optional[torch.Tensor] = None, likelihood=None, covar_module=None,
                 mean_module=None, outcome_transform="DEFAULT", input_transform=None):
        super().__init__()
        if input_transform is not None:
            raise UnsupportedError("input transforms are not on the accelerated path")
        if train_X.dim() != 2 or train_Y.dim() != 2 or train_X.shape[0] != train_Y.shape[0]:
            raise UnsupportedError("SingleTaskGP here takes train_X n x d and train_Y n x m")
        if train_Yvar is not None and train_Yvar.shape != train_Y.shape:
            raise ValueError(f"train_Yvar of shape {tuple(train_Yvar.shape)} does not match "
                             f"train_Y of shape {tuple(train_Y.shape)}")
        train_X = train_X.to(torch.float64)
        train_Y = train_Y.to(torch.float64)
        from .exceptions import InputDataError
        if torch.isnan(train_X).any() or torch.isnan(train_Y).any():
            raise InputDataError("Input data contains NaN values.")
        if train_Yvar is not None:
            train_Yvar = train_Yvar.to(torch.float64)
            if torch.isnan(train_Yvar).any():
                raise InputDataError("Input data contains NaN values.")
            if (train_Yvar < 0).any():  # models/utils/assorted.py validate_input_scaling
                raise InputDataError("Input data contains negative variances.")
        if train_Y.shape[-1] > 1:
            self._init_multi_output(train_X, train_Y, train_Yvar, likelihood, covar_module,
                                    mean_module, outcome_transform)
            return
        if outcome_transform == "DEFAULT":
            outcome_transform = Standardize(m=1)
        if outcome_transform is not None:
            outcome_transform.train()
            train_Y_tf, train_Yvar_tf = outcome_transform(train_Y, train_Yvar)
            self.outcome_transform = outcome_transform
        else:
            train_Y_tf, train_Yvar_tf = train_Y, train_Yvar
        self._check_scaling(train_X, train_Y_tf)
        self.train_inputs = (train_X,)
        self.train_targets = train_Y_tf.squeeze(-1)
        self._raw_train_Y = train_Y
        d = train_X.shape[-1]
        if likelihood is None and train_Yvar_tf is not None:
            likelihood = FixedNoiseGaussianLikelihood(train_Yvar_tf.squeeze(-1))
        self.likelihood = likelihood if likelihood is not None else get_gaussian_likelihood_with_lognormal_prior()
        self.mean_module = mean_module if mean_module is not None else ConstantMean()
        self.covar_module = covar_module if covar_module is not None else get_covar_module_with_dim_scaled_prior(d)
        self._cache = None
        self._cache_key = None
        self.to(train_X.device)

    def _init_multi_output(self, train_X, train_Y, train_Yvar, likelihood, covar_module,
                           mean_module, outcome_transform):
        """m > 1 outputs: the reference's batched multi-output model
        (models/gpytorch.py:327-355 BatchedMultiOutputGPyTorchModel, batch shape
        [m] of independent GPs with their own hyperparameters) as m single-output
        members sharing train_X.  Standardize(m) standardises each column on its
        own, so each member's Standardize(1) holds exactly its column's
        statistics; the posterior is the members' block-diagonal joint (the
        from_batch_mvn MTMVN), which the ModelListGP routes (qEHVI / qNEHVI /
        scalarised qEI) consume through ``models``; fit_gpytorch_mll minimises
        the summed loss jointly over all members' parameters."""
        m = train_Y.shape[-1]
        if likelihood is not None or covar_module is not None or mean_module is not None:
            raise UnsupportedError("custom modules of a multi-output SingleTaskGP (batched "
                                   "modules) are not on the accelerated path")
        if outcome_transform == "DEFAULT":
            outcome_transform = Standardize(m=m)
        if outcome_transform is not None and not (isinstance(outcome_transform, Standardize)
                                                  and outcome_transform._m == m):
            raise UnsupportedError("a multi-output SingleTaskGP takes Standardize(m) or no "
                                   "outcome transform here")
        if outcome_transform is not None:
            # statistics of the full n x m Y (the reference's reduction), each
            # member then holds its column of them
            outcome_transform.train()
            Y_tf, Yvar_tf = outcome_transform(train_Y, train_Yvar)
            outcome_transform.eval()
            self.outcome_transform = outcome_transform
        else:
            Y_tf, Yvar_tf = train_Y, train_Yvar
        members = []
        for t in range(m):
            mm = SingleTaskGP(train_X, Y_tf[:, t:t + 1],
                              None if Yvar_tf is None else Yvar_tf[:, t:t + 1],
                              outcome_transform=None)
            if outcome_transform is not None:
                col = Standardize(m=1, min_stdv=outcome_transform._min_stdv)
                col.means = outcome_transform.means[..., t:t + 1].clone()
                col.stdvs = outcome_transform.stdvs[..., t:t + 1].clone()
                col._is_trained = True
                col.eval()
                mm.outcome_transform = col
                mm._raw_train_Y = train_Y[:, t:t + 1]
            members.append(mm)
        self.models = nn.ModuleList(members)
        self._num_outputs = m
        for name in ("likelihood", "covar_module", "mean_module"):
            setattr(self, name, _StackedView(members, name))
        self.train_inputs = (train_X,)
        self.train_targets = torch.stack([mm.train_targets for mm in members])  # m x n
        self._cache = None
        self._cache_key = None

    @property
    def _is_multi_output(self) -> bool:
        return self._num_outputs > 1

    @staticmethod
    def _check_scaling(X, Y):
        """botorch/models/utils/assorted.py:219-261 (warnings only)."""
        if X.numel() and (X.min() < -1e-8 or X.max() > 1 + 1e-8):
            warnings.warn("Input data is not contained to the unit cube. Please consider "
                          "min-max scaling the input data.", InputDataWarning)

    # -- hyperparameter accessors ------------------------------------------------
    @property
    def kind(self) -> int:
        return self.covar_module.kind

    def hyper(self):
        if self._is_multi_output:
            raise UnsupportedError("hyper() of a multi-output SingleTaskGP: use model.models[t]")
        ls = self.covar_module.lengthscale.detach().reshape(-1)
        os_ = float(self.covar_module.outputscale.detach()) if isinstance(self.covar_module, ScaleKernel) else 1.0
        return ls, os_, float(self.likelihood.noise.detach().mean()), float(self.mean_module.constant.detach())

    def train(self, mode: bool = True):
        if mode:
            self._cache = None
            self._cache_key = None
            self._cache_jit = None
        return super().train(mode)

    @property
    def batch_shape(self) -> torch.Size:
        return torch.Size([])

    def _key(self):
        if self._is_multi_output:
            return tuple(mm._key() for mm in self.models)
        d = self.__dict__
        if d.get("_plist_gen") != _STRUCTURE[0]:
            d["_plist"] = list(self.parameters())
            d["_plist_gen"] = _STRUCTURE[0]
        ps = [self.train_inputs[0], self.train_targets] + d["_plist"]
        return tuple((p.data_ptr(), p._version) for p in ps)

    def prediction_cache(self, key=None):
        """Device caches of [G] exact prediction; rebuilt on any change.
        ``key``: this model's _key(), when the caller has just computed it."""
        from . import kernels
        if self._is_multi_output:
            raise UnsupportedError("a multi-output SingleTaskGP keeps one cache per output "
                                   "(model.models[t].prediction_cache())")
        from .settings import propagate_grads
        if propagate_grads.on() and (self.train_inputs[0].requires_grad or self.train_targets.requires_grad):
            from .exceptions import UnsupportedError
            raise UnsupportedError(
                "settings.propagate_grads: posterior gradients to the training data are not "
                "supported (the prediction caches are built without a backward to them)")
        if key is None:
            key = self._key()
        if self._cache is None or self._cache_key != key:
            from . import ops  # noqa: F401  (torch.ops.bo registration)
            ls, os_, noise, c = self.hyper()
            Xt = self.train_inputs[0].contiguous()
            nv = self.likelihood.noise if isinstance(self.likelihood, FixedNoiseGaussianLikelihood) else None
            L, Linv, U, beta, alpha, Xs, jit = torch.ops.bo.gp_cache(
                Xt, self.train_targets.contiguous(), ls.contiguous(), float(os_), float(noise),
                float(c), int(self.kind), nv)
            n, d = Xt.shape
            self._cache = kernels.GPCache(self.kind, n, d, U.shape[0], Xt, Xs, ls.contiguous(),
                                          float(os_), float(noise), float(c), L, Linv, U, beta,
                                          alpha, 0.0)
            self._cache_key = key
            self._cache_jit = jit  # device scalar, not read back here
        return self._cache

    def posterior(self, X: torch.Tensor, output_indices=None, observation_noise=False,
                  posterior_transform=None):
        """botorch/models/gpytorch.py:405-466 (m > 1: :327-355).  The model
        computes in fp64: X of another floating dtype is promoted (the
        gradient flows back through the cast)."""
        from .posteriors import GPyTorchPosterior, PosteriorList
        if X.dtype != torch.float64:
            X = X.to(torch.float64)
        if self._is_multi_output:
            idx = output_indices if output_indices is not None else range(self._num_outputs)
            prime_prediction_caches([self.models[i] for i in idx])
            post = PosteriorList(*[self.models[i].posterior(X, observation_noise=observation_noise)
                                   for i in idx])
            return post if posterior_transform is None else posterior_transform(post)
        if output_indices not in (None, [0]):
            raise UnsupportedError("single-output model")
        self.eval()
        post = GPyTorchPosterior.from_model(self, X, observation_noise=observation_noise)
        if posterior_transform is not None:
            return posterior_transform(post)
        return post

    # -- fantasy models -----------------------------------------------------------
    def fantasize(self, X: torch.Tensor, sampler, observation_noise=None, **kwargs):
        """botorch/models/model.py:328-407: the batch of N_f fantasy models that
        condition this model on (X, Y_f), Y_f = mu(X) + L z_f drawn from the
        posterior at X under observation noise (L L^T = Sigma(X, X) + diag(s'^2),
        z_f row f of ``sampler.base_samples_2d(q_a, device)``: the sampler fixes
        the fantasies across calls, as in qKnowledgeGradient).

        X: q_a x d or b x q_a x d (promoted to fp64).  ``sampler``: an MCSampler
        with a one-dimensional ``sample_shape`` [N_f].  ``observation_noise``:
        None -- the likelihood's noise (a fixed-noise likelihood: the mean
        training noise) -- or a 1 x 1 / q_a x 1 tensor in the transformed
        (standardised) space; a bool raises DeprecationError as in the reference.

        Returns a :class:`FantasizedGP` with ``batch_shape`` (N_f, *X.shape[:-2]).
        It keeps a reference to this model (not a copy) and X with its graph:
        every ``posterior`` call recomputes the joint moments at [X; X'], so the
        result is differentiable in X' and in X whenever either requires a
        gradient, a later change of this model's hyperparameters is seen, and
        nothing stale is kept between calls.  ``propagate_grads`` is accepted
        and has no further effect: the derivative with respect to X is the one
        qKnowledgeGradient returns for its candidates."""
        from .exceptions import DeprecationError
        if observation_noise is not None and not torch.is_tensor(observation_noise):
            raise DeprecationError(
                "`fantasize` no longer accepts a boolean for `observation_noise`.")
        if self._is_multi_output:
            raise UnsupportedError("fantasize: a multi-output SingleTaskGP is not on the "
                                   "accelerated path (single-output SingleTaskGP only)")
        kwargs.pop("propagate_grads", None)
        if kwargs:
            raise UnsupportedError(f"fantasize: unsupported arguments {sorted(kwargs)}")
        shape = getattr(sampler, "sample_shape", None)
        if shape is None or len(shape) != 1 or shape[0] < 1:
            raise ValueError("fantasize: the sampler's sample_shape must be one-dimensional "
                             f"([N_f]), got {tuple(shape) if shape is not None else None}")
        d = self.train_inputs[0].shape[-1]
        if X.dim() < 2 or X.shape[-1] != d:
            raise ValueError(f"fantasize: X must be (b x) q_a x {d}, got {tuple(X.shape)}")
        if X.shape[-2] == 0:
            raise UnsupportedError("fantasize: q_a = 0 (a fantasy model without fantasised "
                                   "points) is not on the accelerated path")
        if observation_noise is not None:
            q_a = X.shape[-2]
            if tuple(observation_noise.shape) not in ((1, 1), (q_a, 1)):
                raise ValueError(f"fantasize: observation_noise must be 1 x 1 or {q_a} x 1, got "
                                 f"{tuple(observation_noise.shape)}")
        return FantasizedGP(self, X.to(torch.float64), sampler, observation_noise)

    # -- conditioning on new observations ------------------------------------------
    def _blank_copy(self, train_X):
        """A SingleTaskGP shell with the new inputs and no modules yet (the
        constructor's checks and statistics do not apply to a conditioned model)."""
        new = SingleTaskGP.__new__(SingleTaskGP)
        Model.__init__(new)
        new.train_inputs = (train_X,)
        new._cache = None
        new._cache_key = None
        new._cache_jit = None
        return new

    def condition_on_observations(self, X: torch.Tensor, Y: torch.Tensor,
                                  noise: Optional[torch.Tensor] = None, **kwargs):
        """botorch/models/gpytorch.py:468-531 (model.py:149): a new eval-mode
        SingleTaskGP on cat(train_X, X) with the same hyperparameters; the source
        model and its caches are untouched.  X: k x d, Y: k x m in the original
        outcome space (it goes through the outcome transform with its fitted
        statistics, which are not refitted); ``noise`` (k x m, a fixed-noise
        likelihood's observed variances) is taken as already transformed.

        When this model holds a valid prediction cache and k is at most
        kernels.EXTEND_MAX_K, the new model's cache is the bordered update of
        it (kernels.extend_gp_cache, O(n^2 k)); otherwise the new model builds
        its cache on its first posterior as any model does.  Both give the same
        model.  The new model carries no gradient to X or Y."""
        from . import kernels
        from .exceptions import InputDataError
        from .settings import propagate_grads
        if kwargs:
            raise UnsupportedError("condition_on_observations: unsupported arguments "
                                   f"{sorted(kwargs)}")
        if X.dim() > 2 or Y.dim() > 2 or (noise is not None and noise.dim() > 2):
            raise UnsupportedError("condition_on_observations takes X k x d and Y k x m here: "
                                   "batched fantasy models are not on the accelerated path")
        train_X = self.train_inputs[0]
        if X.dim() != 2 or Y.dim() != 2:
            raise ValueError("condition_on_observations: expected X k x d and Y k x m")
        if X.shape[-1] != train_X.shape[-1]:
            raise ValueError(f"condition_on_observations: X has {X.shape[-1]} features, the model "
                             f"{train_X.shape[-1]}")
        if Y.shape[-1] != self._num_outputs:
            raise ValueError(f"condition_on_observations: Y has {Y.shape[-1]} outputs, the model "
                             f"{self._num_outputs}")
        if X.shape[0] != Y.shape[0]:
            raise ValueError(f"condition_on_observations: {X.shape[0]} points but {Y.shape[0]} "
                             "observations")
        if noise is not None and noise.shape != Y.shape:
            raise ValueError(f"condition_on_observations: noise of shape {tuple(noise.shape)} does "
                             f"not match Y of shape {tuple(Y.shape)}")
        if propagate_grads.on() and (X.requires_grad or Y.requires_grad):
            raise UnsupportedError(
                "settings.propagate_grads: posterior gradients to the training data are not "
                "supported (the prediction caches are built without a backward to them)")
        X = X.detach().to(train_X)
        Y = Y.detach().to(train_X)
        if noise is not None:
            noise = noise.detach().to(train_X)
        if torch.isnan(X).any() or torch.isnan(Y).any() or (
                noise is not None and torch.isnan(noise).any()):
            raise InputDataError("Input data contains NaN values.")
        if self._is_multi_output:
            return self._condition_multi_output(X, Y, noise)
        import copy
        fixed = isinstance(self.likelihood, FixedNoiseGaussianLikelihood)
        if fixed and noise is None:
            raise RuntimeError("FixedNoiseGaussianLikelihood.fantasize requires a `noise` kwarg")
        if not fixed and noise is not None:
            raise UnsupportedError("condition_on_observations: `noise` needs a fixed-noise "
                                   "likelihood (a SingleTaskGP built with train_Yvar)")
        ot = self._modules.get("outcome_transform")
        if ot is not None:
            was_training = ot.training
            ot.eval()  # the fitted statistics, never refitted here
            try:
                Y_tf, _ = ot(Y)
            finally:
                ot.train(was_training)
        else:
            Y_tf = Y
        y_new = Y_tf.squeeze(-1)
        k = X.shape[0]
        new = self._blank_copy(torch.cat([train_X, X]))
        new.train_targets = torch.cat([self.train_targets.detach(), y_new])
        new._raw_train_Y = torch.cat([self._raw_train_Y.detach().to(Y), Y])
        if ot is not None:
            new.outcome_transform = copy.deepcopy(ot)
        if fixed:
            new.likelihood = FixedNoiseGaussianLikelihood(
                torch.cat([self.likelihood.noise, noise.reshape(-1)]))
        else:
            new.likelihood = copy.deepcopy(self.likelihood)
        new.mean_module = copy.deepcopy(self.mean_module)
        new.covar_module = copy.deepcopy(self.covar_module)
        new.eval()
        cache = self._cache
        if (not self.training and cache is not None and self._cache_key == self._key()
                and k <= kernels.EXTEND_MAX_K):
            if k > 0:
                cache = kernels.extend_gp_cache(
                    cache, X, y_new, noise_new=noise.reshape(-1) if fixed else None,
                    y_old=self.train_targets, noise_old=self.likelihood.noise if fixed else None,
                    jitter_dev=self.__dict__.get("_cache_jit"))
                cache.Xt = new.train_inputs[0]
            else:
                new._cache_jit = self.__dict__.get("_cache_jit")
            new._cache = cache
            new._cache_key = new._key()
        return new

    def _condition_multi_output(self, X, Y, noise):
        """m > 1: each output's member is conditioned on its column; the parent's
        m x (n + k) targets and stacked views are rebuilt."""
        import copy
        members = [mm.condition_on_observations(
            X, Y[:, t:t + 1], None if noise is None else noise[:, t:t + 1])
            for t, mm in enumerate(self.models)]
        shared = members[0].train_inputs[0]
        for mm in members[1:]:  # the members share train_X, as the constructor's do
            mm.train_inputs = (shared,)
            if mm._cache is not None:
                mm._cache.Xt = shared
                mm._cache_key = mm._key()
        new = self._blank_copy(shared)
        ot = self._modules.get("outcome_transform")
        if ot is not None:
            new.outcome_transform = copy.deepcopy(ot)
        new.models = nn.ModuleList(members)
        new._num_outputs = self._num_outputs
        for name in ("likelihood", "covar_module", "mean_module"):
            setattr(new, name, _StackedView(members, name))
        new.train_targets = torch.stack([mm.train_targets for mm in members])  # m x (n + k)
        new.eval()
        return new


class FantasizedGP(Model):
    """The batch of fantasy models of ``SingleTaskGP.fantasize`` (the reference's
    batched model after models/model.py:328-407): N_f x b exact GPs on the n +
    q_a points [train_X; X_b] with targets [y; Y_f], never built -- with all
    moments of the source model's joint posterior at [X; X'] in outcome space,

        A     = Sigma(X, X) + diag(s'^2)         L = psd_safe_cholesky(A)
        V_f   = Sigma(X'_f, X) L^{-T}
        mu'_f = mu(X'_f) + V_f z_f               (Y_f - mu(X) = L z_f)
        S'_f  = Sigma(X'_f, X'_f) - V_f V_f^T

    so conditioning is a rank-q_a correction that needs no new n x n work and
    all fantasies of a t-batch share L.  For q_a + q <= FUSED_ROWS, d <=
    kernels.DP and X on the device the points are packed into tiles of at most
    16 rows (kernels.fantasy_tile_plan), the fused posterior runs once over all
    tiles and bo::fantasy_posterior conditions them; otherwise the generic
    posterior kernels give the joint moments and the formula runs in torch.

    There is no ``prediction_cache``: acquisition functions on a fantasy model
    take their generic routes through :meth:`posterior`."""

    FUSED_ROWS = 16  # largest q_a + q on the fused route (one 16-row tile holds X and one group)

    def __init__(self, source: "SingleTaskGP", X: torch.Tensor, sampler, observation_noise=None):
        super().__init__()
        # references, not submodules: the source model is neither copied nor trained through this
        self.__dict__["source"] = source
        self.__dict__["_sampler"] = sampler
        self._X = X
        self._obs_noise = observation_noise
        self.num_fantasies = int(sampler.sample_shape[0])
        self._tile_index = {}

    @property
    def batch_shape(self) -> torch.Size:
        return torch.Size([self.num_fantasies]) + self._X.shape[:-2]

    def outcome_stats(self):
        return self.source.outcome_stats()

    # -- the pieces every call recomputes -------------------------------------------
    def _base_samples(self) -> torch.Tensor:
        return self._sampler.base_samples_2d(self._X.shape[-2], self._X.device)

    def _noise(self) -> torch.Tensor:
        """s'^2 of the fantasy observations in outcome space (q_a)."""
        q_a = self._X.shape[-2]
        ystd = self.source.outcome_stats()[1]
        if self._obs_noise is None:  # qKnowledgeGradient._noise
            s2 = self.source.prediction_cache().noise * ystd * ystd
            return torch.full((q_a,), s2, dtype=torch.float64, device=self._X.device)
        s2 = self._obs_noise.detach().to(self._X).reshape(-1) * (ystd * ystd)
        return s2.expand(q_a).contiguous()

    def _fantasy_targets(self) -> torch.Tensor:
        """Y_f = mu(X) + L z_f in outcome space, N_f x b x q_a (detached)."""
        from . import kernels
        from .posteriors import posterior_moments
        with torch.no_grad():
            mean, cov = posterior_moments(self.source, self._X.detach())
            L = kernels.chol_jitter(cov + torch.diag_embed(self._noise()))
            Z = self._base_samples()
            return mean + torch.einsum("...ij,fj->f...i", L, Z)

    @property
    def train_inputs(self):
        """(N_f x b x (n + q_a) x d,), as the reference's batched model holds them."""
        Xt = self.source.train_inputs[0].detach()
        X = self._X.detach()
        both = torch.cat([Xt.expand(*X.shape[:-2], *Xt.shape), X], dim=-2)
        return (both.expand(self.num_fantasies, *both.shape),)

    @property
    def train_targets(self) -> torch.Tensor:
        """N_f x b x (n + q_a), in the source model's transformed space."""
        ymean, ystd = self.source.outcome_stats()
        Yf = (self._fantasy_targets() - ymean) / ystd
        y = self.source.train_targets.detach()
        return torch.cat([y.expand(*Yf.shape[:-1], y.shape[-1]), Yf], dim=-1)

    def fantasize(self, X, sampler, observation_noise=None, **kwargs):
        raise UnsupportedError("fantasize: nested fantasies (a fantasy model of a FantasizedGP) "
                               "are not on the accelerated path")

    def condition_on_observations(self, X, Y, **kwargs):
        raise UnsupportedError("condition_on_observations of a FantasizedGP (nested "
                               "conditioning) is not on the accelerated path")

    # -- posterior -----------------------------------------------------------------
    def _broadcast(self, Xp: torch.Tensor):
        """(X B x q_a x d, X' B x F x q x d, shared, batch): X' broadcast against
        (N_f, b); F = 1 when one set of points serves every fantasy."""
        N_f, X = self.num_fantasies, self._X
        d, bshape = X.shape[-1], X.shape[:-2]
        if Xp.dim() < 2 or Xp.shape[-1] != d:
            raise ValueError(f"FantasizedGP.posterior: X must be ... x q x {d}, got "
                             f"{tuple(Xp.shape)}")
        pb = Xp.shape[:-2]
        lead = 1
        if len(pb) > len(bshape) + 1:
            raise ValueError(f"FantasizedGP.posterior: X of batch shape {tuple(pb)} does not "
                             f"broadcast against {tuple(self.batch_shape)}")
        if len(pb) == len(bshape) + 1:
            lead, pb = pb[0], pb[1:]
        try:
            if lead not in (1, N_f):
                raise RuntimeError
            batch = torch.broadcast_shapes(bshape, pb)
        except RuntimeError:
            raise ValueError(f"FantasizedGP.posterior: X of batch shape {tuple(Xp.shape[:-2])} "
                             f"does not broadcast against {tuple(self.batch_shape)}") from None
        q = Xp.shape[-2]
        shared = lead == 1
        F = 1 if shared else N_f
        Xp = Xp.reshape(F, *([1] * (len(batch) - len(pb))), *pb, q, d)
        Xp = Xp.expand(F, *batch, q, d).reshape(F, -1, q, d)
        Xa = X.expand(*batch, *X.shape[-2:]).reshape(-1, X.shape[-2], d)
        return Xa, Xp.transpose(0, 1), shared, batch

    def _fused(self, Xa, Xp, Z, noise, shared):
        from . import kernels, ops  # noqa: F401  (torch.ops.bo registration)
        from .posteriors import _fused_moments
        B, q_a, d = Xa.shape
        F, q = Xp.shape[1], Xp.shape[2]
        T, slots = kernels.fantasy_tile_plan(q_a, q, F)
        key = (F, T, slots, Xa.device)
        idx = self._tile_index.get(key)
        if idx is None:  # group of each slot; the spare slots repeat the last one
            idx = torch.arange(T * slots, device=Xa.device).clamp_max(F - 1)
            self._tile_index[key] = idx
        groups = Xp[:, idx].reshape(B, T, slots * q, d)
        tiles = torch.cat([Xa.unsqueeze(1).expand(B, T, q_a, d), groups], dim=2)
        mean, cov = _fused_moments(tiles.reshape(B * T, q_a + slots * q, d), self.source)
        mean_f, cov_f, _, _, jit, info = torch.ops.bo.fantasy_posterior(
            mean, cov, Z, noise, q_a, q, slots, shared)
        kernels.raise_not_psd_deferred(info, jit, type(self).__name__)
        return mean_f, cov_f

    def _generic(self, Xa, Xp, Z, noise):
        """posterior_moments on cat([X, X']) and the same formula in torch
        (qKnowledgeGradient._generic's shape of it); also the in-library
        cross-check of the fused route."""
        from .posteriors import _CholJitter, posterior_moments
        B, q_a, d = Xa.shape
        F = Xp.shape[1]
        mean, cov = posterior_moments(
            self.source, torch.cat([Xa.unsqueeze(1).expand(B, F, q_a, d), Xp], dim=-2))
        L = _CholJitter.apply(cov[:, 0, :q_a, :q_a] + torch.diag_embed(noise))      # B x q_a x q_a
        C = cov[:, :, q_a:, :q_a]                                                     # B x F x q x q_a
        V = torch.linalg.solve_triangular(L.unsqueeze(1), C.mT, upper=False).mT      # C L^{-T}
        # F = 1: the one group (g) serves every fantasy
        mean_f = mean[:, :, q_a:] + torch.einsum("bgrj,fj->bfr" if F == 1 else "bfrj,fj->bfr", V, Z)
        return mean_f, cov[:, :, q_a:, q_a:] - V @ V.mT

    def posterior(self, X: torch.Tensor, output_indices=None, observation_noise=False,
                  posterior_transform=None):
        """The fantasy models' posterior at X: q x d or b x q x d (shared by all
        fantasies), N_f x b x q x d (one set per fantasy), a 1 in place of b or
        N_f broadcasting -> GPyTorchPosterior with mean N_f x b x q x 1 and
        covariance N_f x b x q x q (for a shared X an expanded view: it does not
        depend on the fantasy).  ``observation_noise=True`` adds the fantasy
        noise s'^2 (its mean, if per row) to the diagonal."""
        from . import kernels
        from .posteriors import GPyTorchPosterior, MultivariateNormal
        if output_indices not in (None, [0]):
            raise UnsupportedError("single-output model")
        if not isinstance(observation_noise, bool):
            raise UnsupportedError("FantasizedGP.posterior: observation_noise is True or False "
                                   "here (the fantasy noise), not a tensor")
        if X.dtype != torch.float64:
            X = X.to(torch.float64)
        self.source.eval()
        Xa, Xp, shared, batch = self._broadcast(X)
        N_f, q_a, q, d = self.num_fantasies, Xa.shape[-2], Xp.shape[-2], Xa.shape[-1]
        Z, noise = self._base_samples(), self._noise()
        if q_a + q <= self.FUSED_ROWS and d <= kernels.DP and Xa.is_cuda:
            mean, cov = self._fused(Xa, Xp, Z, noise, shared)
        else:
            mean, cov = self._generic(Xa, Xp, Z, noise)
        mean = mean.transpose(0, 1).reshape(N_f, *batch, q)
        cov = cov.transpose(0, 1).reshape(-1, *batch, q, q).expand(N_f, *batch, q, q)
        if observation_noise:
            cov = cov + noise.mean() * torch.eye(q, dtype=cov.dtype, device=cov.device)
        post = GPyTorchPosterior(MultivariateNormal(mean, cov), model=self, X=X)
        return post if posterior_transform is None else posterior_transform(post)


def prime_prediction_caches(models):
    """Build the missing prediction caches of several single-output exact GPs
    (a ModelListGP's members, the outputs of a multi-output SingleTaskGP, the
    SAAS ensemble's members) with ONE batched factorisation
    (kernels.build_gp_caches: the members' K + s2 I in one persistent DAG
    launch, one status read-back); each model.prediction_cache() then returns
    its cache without a launch.  When every model already holds a cache this
    returns at once (a stale cache, after new hyperparameters, is rebuilt by
    its own prediction_cache()).  The caches are bit-identical to the
    per-model builds; fixed-noise members and unequal orders keep the
    per-model path.  Returns each model's version key (None where not
    computed), for prediction_cache(key=...): one key computation per model
    and forward."""
    from . import kernels
    from .settings import propagate_grads
    if all(getattr(mm, "_cache", None) is not None for mm in models):
        # every model has a cache: a stale one (new hyperparameters) is rebuilt
        # by its own prediction_cache(); this keeps the per-forward host cost
        # of the common case (all fresh) at one attribute read per model
        return [None] * len(models)
    stale, keys = [], []
    pg = propagate_grads.on()
    for mm in models:
        keys.append(None)
        if not isinstance(mm, SingleTaskGP) or mm._is_multi_output:
            continue
        if isinstance(mm.likelihood, FixedNoiseGaussianLikelihood):
            continue
        if pg and (mm.train_inputs[0].requires_grad or mm.train_targets.requires_grad):
            continue  # prediction_cache raises the reference's error
        key = keys[-1] = mm._key()
        if mm._cache is not None and mm._cache_key == key:
            continue
        stale.append((mm, key))
    if len(stale) < 2:
        return keys
    specs = []
    for mm, _ in stale:
        ls, os_, noise, c = mm.hyper()
        specs.append(dict(Xt=mm.train_inputs[0].contiguous(), y=mm.train_targets.contiguous(),
                          lengthscale=ls.contiguous(), noise=float(noise), constant=float(c),
                          kind=int(mm.kind), outputscale=float(os_)))
    for (mm, key), cache in zip(stale, kernels.build_gp_caches(specs)):
        mm._cache = cache
        mm._cache_key = key
        mm._cache_jit = None  # cache.jitter is exact here
    return keys


class ModelListGP(Model):
    """Independent single-output GPs (botorch/models/model_list_gp_regression.py:24);
    its posterior is block-diagonal across outputs (models/gpytorch.py:629-726)."""

    def __init__(self, *models: SingleTaskGP):
        super().__init__()
        self.models = nn.ModuleList(models)
        self._num_outputs = len(models)

    def posterior(self, X, output_indices=None, observation_noise=False, posterior_transform=None):
        from .posteriors import PosteriorList
        idx = output_indices if output_indices is not None else range(len(self.models))
        prime_prediction_caches([self.models[i] for i in idx])
        post = PosteriorList(*[self.models[i].posterior(X, observation_noise=observation_noise) for i in idx])
        if posterior_transform is not None:
            return posterior_transform(post)
        return post

    def condition_on_observations(self, X: List[torch.Tensor], Y: torch.Tensor,
                                  noise: Optional[torch.Tensor] = None, **kwargs):
        """botorch/models/model_list_gp_regression.py:58-129: X is a list with one
        k x d tensor per output, Y k x m; each member is conditioned on its own
        inputs and its slice of Y.  ``noise`` (k x m, original outcome space)
        goes through each member's outcome transform with Y, as there."""
        from .exceptions import BotorchTensorDimensionError
        if Y.shape[-1] != self.num_outputs:
            raise BotorchTensorDimensionError(
                "Incorrect number of outputs for observations. Received "
                f"{Y.shape[-1]} observation outputs, but model has {self.num_outputs} outputs.")
        if len(X) != self.num_outputs:
            raise BotorchTensorDimensionError(
                "Incorrect number of inputs for observations. Received "
                f"{len(X)} observation inputs, but model has {self.num_outputs} outputs.")
        if noise is not None and noise.shape != Y.shape[-noise.dim():]:
            raise BotorchTensorDimensionError(
                "The shape of observation noise does not agree with the outcomes. "
                f"Received {tuple(noise.shape)} noise with {tuple(Y.shape)} outcomes.")
        if Y.dim() > 2 or any(x.dim() > 2 for x in X):
            raise UnsupportedError("condition_on_observations takes X k x d and Y k x m here: "
                                   "batched fantasy models are not on the accelerated path")
        members, i = [], 0
        for model in self.models:
            j = i + model.num_outputs
            noise_i = None
            if noise is not None:
                noise_i = noise[..., i:j]
                ot = model._modules.get("outcome_transform")
                if ot is not None:
                    noise_i = noise_i.to(ot.stdvs) / ot.stdvs.pow(2)
            # (a multi-output member takes the inputs of its first output)
            members.append(model.condition_on_observations(X[i], Y[..., i:j], noise=noise_i,
                                                           **kwargs))
            i = j
        return ModelListGP(*members)

    def train(self, mode: bool = True):
        for m in self.models:
            m.train(mode)
        return super().train(mode)


MCMC_DIM = -3  # models/fully_bayesian.py: posterior batch dim of the MCMC samples


class GenericDeterministicModel(Model):
    """A deterministic model defined by a callable (models/deterministic.py):
    ``f`` maps ``batch_shape x q x d`` to ``batch_shape x q x m``.  Its posterior
    is the point mass at f(X) (posteriors.DeterministicPosterior); a posterior
    transform with ``evaluate`` (ScalarizedPosteriorTransform) is applied to
    the values."""

    _is_ensemble = False

    def __init__(self, f, num_outputs: int = 1):
        super().__init__()
        self._f = f
        self._num_outputs = num_outputs

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return self._f(X)

    def posterior(self, X, output_indices=None, observation_noise=False, posterior_transform=None):
        from .posteriors import DeterministicPosterior
        if observation_noise is not False:
            raise UnsupportedError("a deterministic model has no observation noise")
        values = self.forward(X)
        if output_indices is not None:
            values = values[..., list(output_indices)]
        if posterior_transform is not None:
            if not hasattr(posterior_transform, "evaluate"):
                raise UnsupportedError("a deterministic model takes posterior transforms with "
                                       "`evaluate` (ScalarizedPosteriorTransform)")
            values = posterior_transform.evaluate(values).unsqueeze(-1)
        return DeterministicPosterior(values)


def sample_saas_prior(d: int, num_samples: int, seed: int = 0, dtype=torch.float64):
    """Hyperparameter sets from the SAAS prior (models/fully_bayesian.py:168-247):
    outputscale ~ Gamma(2, 0.15), mean ~ N(0, 1), noise = 1e-4 + Gamma(0.9, 10),
    tau^2 ~ HalfCauchy(0.1), inv_len^2 ~ HalfCauchy(1)^d, lengthscale =
    (tau^2 inv_len^2)^{-1/2}.  (Posterior draws: fit.fit_fully_bayesian_model_nuts.)"""
    g = torch.Generator().manual_seed(seed)
    M = num_samples

    def gamma(conc, rate, shape):
        # Marsaglia-Tsang through torch's generator-aware _standard_gamma
        return torch._standard_gamma(torch.full(shape, conc, dtype=dtype), generator=g) / rate

    def half_cauchy(scale, shape):
        u = torch.rand(shape, generator=g, dtype=dtype)
        return scale * torch.tan(0.5 * math.pi * u)

    tausq = half_cauchy(0.1, (M, 1))
    inv_len_sq = half_cauchy(1.0, (M, d))
    return {
        "outputscale": gamma(2.0, 0.15, (M,)),
        "mean": torch.randn(M, generator=g, dtype=dtype),
        "noise": MIN_INFERRED_NOISE_LEVEL + gamma(0.9, 10.0, (M,)),
        "lengthscale": (tausq * inv_len_sq).rsqrt(),
    }


class SaasFullyBayesianSingleTaskGP(Model):
    """Fully Bayesian SAAS GP (models/fully_bayesian.py:315-546): M hyperparameter
    sets (MCMC samples) of a ScaleKernel(Matern-5/2) GP with constant mean and
    Gaussian noise, evaluated as an ensemble.  The posterior at X (b x q x d) has
    batch shape b x M (X is broadcast over MCMC_DIM = -3); acquisition values are
    averaged over M (utils/transforms.py:289-293).

    Each member is an exact GP with its own device caches (Matern-5/2 kernel
    matrix, blocked MFMA Cholesky, L^{-T}); the q-batch posterior runs through
    the generic kernels (d = 50 exceeds the fused kernel's register-resident
    inputs)."""

    _is_fully_bayesian = True
    _is_ensemble = True

    def __init__(self, train_X, train_Y, train_Yvar=None, outcome_transform=None,
                 input_transform=None, pyro_model=None):
        super().__init__()
        if not (train_X.ndim == train_Y.ndim == 2 and len(train_X) == len(train_Y)
                and train_Y.shape[-1] == 1):
            raise ValueError("Expected train_X to have shape n x d and train_Y to have shape n x 1")
        if train_Yvar is not None or input_transform is not None:
            raise UnsupportedError("fixed noise / input transforms are not on the accelerated path")
        train_X = train_X.to(torch.float64)
        train_Y = train_Y.to(torch.float64)
        if outcome_transform is not None:
            outcome_transform.train()
            train_Y, _ = outcome_transform(train_Y)
            self.outcome_transform = outcome_transform
        self.train_inputs = (train_X,)
        self.train_targets = train_Y.squeeze(-1)
        self.pyro_model = pyro_model  # (fit_fully_bayesian_model_nuts refuses any but None)
        self._members = None
        self._ens = None
        self._ens_key = None

    def ensemble_cache(self):
        """The members' prediction caches stacked for the batched ensemble path:
        U (M x n x n, each L_m^{-T}), alpha (M x n), lengthscale (M x d),
        outputscale (M), constant (M); rebuilt whenever a member's cache is."""
        keys = prime_prediction_caches(self._members)
        caches = [m.prediction_cache(key=k) for m, k in zip(self._members, keys)]
        key = tuple(id(c) for c in caches)
        if self._ens is None or self._ens_key != key:
            n = caches[0].n
            dev = caches[0].U.device
            f64 = dict(dtype=torch.float64, device=dev)
            self._ens = dict(
                n=n, kind=caches[0].kind, Xt=caches[0].Xt.contiguous(),
                U=torch.stack([c.U[:n, :n] for c in caches]).contiguous(),
                alpha=torch.stack([c.alpha.reshape(-1)[:n] for c in caches]).contiguous(),
                ls=torch.stack([c.lengthscale.reshape(-1) for c in caches]).contiguous(),
                os=torch.tensor([c.outputscale for c in caches], **f64),
                os_host=[float(c.outputscale) for c in caches],
                const=torch.tensor([c.constant for c in caches], **f64))
            self._ens_key = key
        return self._ens

    def load_mcmc_samples(self, mcmc_samples) -> None:
        """models/fully_bayesian.py:249-312 (batched modules from the samples)."""
        X = self.train_inputs[0]
        d = X.shape[-1]
        M = len(mcmc_samples["mean"])
        members = []
        for i in range(M):
            base = MaternKernel(ard_num_dims=d, lengthscale_lower=0.0, initial=1.0)
            base.lengthscale = mcmc_samples["lengthscale"][i].reshape(1, d)
            k = ScaleKernel(base, outputscale=float(mcmc_samples["outputscale"][i]))
            lik = GaussianLikelihood(noise_lower=MIN_INFERRED_NOISE_LEVEL, initial=max(
                float(mcmc_samples["noise"][i]), MIN_INFERRED_NOISE_LEVEL))
            mean = ConstantMean()
            mean.constant = float(mcmc_samples["mean"][i])
            mdl = SingleTaskGP(X, self.train_targets.unsqueeze(-1), likelihood=lik, covar_module=k,
                               mean_module=mean, outcome_transform=None)
            members.append(mdl.eval())
        self._members = nn.ModuleList(members)
        self._ens = None

    def condition_on_observations(self, X, Y, **kwargs):
        raise UnsupportedError("condition_on_observations of a fully Bayesian model (a batch "
                               "of fantasy models over the MCMC samples) is not on the "
                               "accelerated path")

    @property
    def num_mcmc_samples(self) -> int:
        if self._members is None:
            raise RuntimeError("Model has not been fitted. You need to call "
                               "`fit_fully_bayesian_model_nuts` to fit the model.")
        return len(self._members)

    @property
    def batch_shape(self) -> torch.Size:
        return torch.Size([self.num_mcmc_samples])

    def train(self, mode: bool = True):
        super().train(mode)
        if mode:
            self._members = None
        return self

    def posterior(self, X, output_indices=None, observation_noise=False, posterior_transform=None):
        """models/fully_bayesian.py:509-546 -> GaussianMixturePosterior (batch b x M)."""
        from .posteriors import GaussianMixturePosterior, MultivariateNormal, posterior_moments
        M = self.num_mcmc_samples
        batch, q, d = X.shape[:-2], X.shape[-2], X.shape[-1]
        X3 = X.reshape(-1, q, d)
        means, covs = [], []
        for mdl in self._members:
            mu, cov = posterior_moments(mdl, X3)  # differentiable (generic kernels at d > 8)
            if observation_noise is True:
                # noise joins in the model's (standardised) space, before the
                # outcome untransform (models/gpytorch.py:446-466)
                cov = cov + mdl.likelihood.noise.reshape(()) * torch.eye(q, dtype=cov.dtype, device=cov.device)
            if hasattr(self, "outcome_transform"):
                tf = self.outcome_transform
                s = float(tf.stdvs.reshape(-1)[0])
                mu = float(tf.means.reshape(-1)[0]) + s * mu
                cov = cov * (s * s)
            means.append(mu)
            covs.append(cov)
        mean = torch.stack(means, dim=1).reshape(*batch, M, q)
        cov = torch.stack(covs, dim=1).reshape(*batch, M, q, q)
        post = GaussianMixturePosterior(MultivariateNormal(mean, cov), model=self, X=X)
        return post if posterior_transform is None else posterior_transform(post)


class _TaskView:
    """One output task of a MultiTaskGP as the posterior kernels see a
    single-output exact GP: ``prediction_cache`` (the task view of the base
    caches) and ``outcome_stats``."""

    def __init__(self, model: "MultiTaskGP", t: int):
        self.model, self.t = model, t

    def prediction_cache(self, key=None):
        return self.model._task_view(self.t)

    def outcome_stats(self):
        return self.model.outcome_stats()


class MultiTaskGP(Model):
    """Long-format multi-task exact GP with the intrinsic coregionalisation
    kernel k((x, a), (x', b)) = k_x(x, x') B[a, b], B = F F^T + diag(v)
    (botorch/models/multitask.py:123-333, models/gpytorch.py:732-918).

    train_X: n x (d + 1) with the task values in column ``task_feature``;
    train_Y: n x 1; ``train_Yvar`` (n x 1) gives a fixed-noise likelihood.
    ``all_tasks`` defaults to the task values in the data (a superset may be
    given: tasks without data); raw task values are remapped to 0..T-1 in sorted
    order.  Defaults as the reference's: ScaleKernel(Matern-5/2) with Gamma
    priors, Gamma(1.1, 0.05) noise prior, full-rank IndexKernel, no outcome
    transform (``Standardize(m=1)`` is accepted), one noise level shared by the
    tasks.  ``task_covar_prior`` and ``input_transform`` raise UnsupportedError.

    ``posterior(X)``: X with d columns gives the one output task (``output_tasks``
    or ``output_indices`` of length 1); X with d + 1 columns gives each point's
    own task and is single-output.  One task throughout takes that task's view
    of the caches (kernels.icm_task_view) through the single-task posterior
    kernels; mixed tasks inside a q-batch take posteriors._ICMGeneralMoments.
    Several output tasks with X lacking the task column (the multi-output
    posterior with cross-task covariance) raise UnsupportedError.

    With one output task ``prediction_cache()`` returns that task's view, which
    is what admits the model to the fused acquisition routes; the view's ``L``
    is None."""

    _is_multitask = True

    def __init__(self, train_X: torch.Tensor, train_Y: torch.Tensor, task_feature: int,
                 train_Yvar: Optional[torch.Tensor] = None, mean_module=None, covar_module=None,
                 likelihood=None, task_covar_prior=None, output_tasks: Optional[List[int]] = None,
                 rank: Optional[int] = None, all_tasks: Optional[List[int]] = None,
                 input_transform=None, outcome_transform=None):
        super().__init__()
        from .exceptions import InputDataError
        if input_transform is not None:
            raise UnsupportedError("MultiTaskGP: input transforms are not on the accelerated path")
        if task_covar_prior is not None:
            raise UnsupportedError("MultiTaskGP: a `task_covar_prior` (LKJ) is not on the "
                                   "accelerated path")
        if train_X.ndim != 2:
            raise ValueError(f"Unsupported shape {train_X.shape} for train_X.")
        if train_Y.dim() != 2 or train_Y.shape != (train_X.shape[0], 1):
            raise UnsupportedError("MultiTaskGP takes train_X n x (d + 1) and train_Y n x 1")
        if train_Yvar is not None and train_Yvar.shape != train_Y.shape:
            raise ValueError(f"train_Yvar of shape {tuple(train_Yvar.shape)} does not match "
                             f"train_Y of shape {tuple(train_Y.shape)}")
        d = train_X.shape[-1] - 1
        if not (-d <= task_feature <= d):
            raise ValueError(f"Must have that -{d} <= task_feature <= {d}")
        task_feature = task_feature % (d + 1)
        train_X = train_X.to(torch.float64)
        train_Y = train_Y.to(torch.float64)
        if torch.isnan(train_X).any() or torch.isnan(train_Y).any():
            raise InputDataError("Input data contains NaN values.")
        if train_Yvar is not None:
            train_Yvar = train_Yvar.to(torch.float64)
            if torch.isnan(train_Yvar).any():
                raise InputDataError("Input data contains NaN values.")
            if (train_Yvar < 0).any():
                raise InputDataError("Input data contains negative variances.")
        all_tasks_inferred = train_X[:, task_feature].unique(sorted=True).to(torch.long).tolist()
        if all_tasks is not None and not set(all_tasks_inferred).issubset(all_tasks):
            raise UnsupportedError(
                f"The provided {all_tasks=} does not contain all the task features "
                f"inferred from the training data {all_tasks_inferred=}. "
                "This is not allowed as it will lead to errors during model training.")
        all_tasks = sorted(all_tasks) if all_tasks else all_tasks_inferred
        self.num_tasks = len(all_tasks)
        self.num_non_task_features = d
        if outcome_transform is not None:
            if not (isinstance(outcome_transform, Standardize) and outcome_transform._m == 1):
                raise UnsupportedError("MultiTaskGP takes Standardize(m=1) or no outcome "
                                       "transform here")
            outcome_transform.train()
            train_Y_tf, train_Yvar_tf = outcome_transform(train_Y, train_Yvar)
            self.outcome_transform = outcome_transform
        else:
            train_Y_tf, train_Yvar_tf = train_Y, train_Yvar
        if output_tasks is None:
            output_tasks = list(all_tasks)
        elif set(output_tasks) - set(all_tasks):
            raise RuntimeError("All output tasks must be present in input data.")
        self._output_tasks = list(output_tasks)
        self._num_outputs = len(output_tasks)
        self._task_feature = task_feature
        self._d = d
        self._all_tasks = list(all_tasks)
        self._expected_task_values = set(all_tasks)
        self._task_index = {int(v): i for i, v in enumerate(all_tasks)}
        # raw task value -> index (NaN where the value is no task), None when the values
        # are already 0..T-1 (get_task_value_remapping)
        if list(all_tasks) == list(range(len(all_tasks))):
            self._task_mapper = None
        else:
            if min(all_tasks) < 0:
                raise ValueError(f"task values must be non-negative integers, got {all_tasks}")
            mapper = torch.full((max(all_tasks) + 1,), float("nan"), dtype=torch.float64)
            mapper[torch.tensor(all_tasks, dtype=torch.long)] = torch.arange(
                len(all_tasks), dtype=torch.float64)
            self.register_buffer("_task_mapper", mapper)
        self._base_idxr = [j for j in range(d + 1) if j != task_feature]
        Xd = train_X[:, self._base_idxr].contiguous()
        self._check_scaling(Xd, train_Y_tf)
        self.train_inputs = (train_X,)
        self.train_targets = train_Y_tf.squeeze(-1)
        self._raw_train_Y = train_Y
        self._Xd = Xd
        if likelihood is None:
            likelihood = (get_gaussian_likelihood_with_gamma_prior() if train_Yvar_tf is None
                          else FixedNoiseGaussianLikelihood(train_Yvar_tf.squeeze(-1)))
        self.likelihood = likelihood
        self.mean_module = mean_module if mean_module is not None else ConstantMean()
        self.covar_module = (covar_module if covar_module is not None
                             else get_matern_kernel_with_gamma_prior(ard_num_dims=d))
        self._rank = rank if rank is not None else self.num_tasks
        self.task_covar_module = IndexKernel(num_tasks=self.num_tasks, rank=self._rank)
        self.to(train_X.device)
        self._is_multitask = True  # (an instance attribute: read from __dict__ on hot paths)
        self._task_long = self._map_tasks(train_X[:, task_feature].to(torch.long)).contiguous()
        self._task_i32 = self._task_long.to(torch.int32).contiguous()
        self._cache = None
        self._cache_key = None
        self._views = {}
        self._view_models = {}
        self._noise_by_task = None

    _check_scaling = staticmethod(SingleTaskGP._check_scaling)

    # -- tasks ------------------------------------------------------------------------
    def _map_tasks(self, task_values: torch.Tensor) -> torch.Tensor:
        """models/gpytorch.py:739-770: raw task values (long) -> task indices."""
        mapper = self._buffers.get("_task_mapper")
        if mapper is None:
            if not (torch.all(0 <= task_values) and torch.all(task_values < self.num_tasks)):
                raise ValueError("Expected all task features in `X` to be between 0 and "
                                 f"self.num_tasks - 1. Got {task_values}.")
            return task_values.long()
        task_values = task_values.long()
        unexpected = set(task_values.unique().tolist()).difference(self._expected_task_values)
        if len(unexpected) > 0:
            raise ValueError("Received invalid raw task values. Expected raw value to be in"
                             f" {self._expected_task_values}, but got unexpected task values:"
                             f" {unexpected}.")
        return mapper[task_values].long()

    def _split_inputs(self, X: torch.Tensor):
        """The d non-task columns and the task indices (long) of X (... x (d + 1))."""
        return X[..., self._base_idxr], self._map_tasks(X[..., self._task_feature].long())

    # -- hyperparameters and caches -----------------------------------------------------
    @property
    def kind(self) -> int:
        return self.covar_module.kind

    @property
    def batch_shape(self) -> torch.Size:
        return torch.Size([])

    def hyper(self):
        ls = self.covar_module.lengthscale.detach().reshape(-1)
        os_ = float(self.covar_module.outputscale.detach()) if isinstance(self.covar_module, ScaleKernel) else 1.0
        return ls, os_, float(self.likelihood.noise.detach().mean()), float(self.mean_module.constant.detach())

    def train(self, mode: bool = True):
        if mode:
            self._drop_caches()
        return super().train(mode)

    def _drop_caches(self):
        self._cache = None
        self._cache_key = None
        self._views = {}

    def _key(self):
        d = self.__dict__
        if d.get("_plist_gen") != _STRUCTURE[0]:
            d["_plist"] = list(self.parameters())
            d["_plist_gen"] = _STRUCTURE[0]
        ps = [self.train_inputs[0], self.train_targets] + d["_plist"]
        return tuple((p.data_ptr(), p._version) for p in ps)

    def _base_cache(self):
        """The caches of the ICM training covariance (its L, L^{-1}, U, beta,
        alpha) over the non-task columns; rebuilt, and every task view dropped,
        on any change of a parameter or training tensor (SingleTaskGP._key)."""
        from . import kernels
        from .settings import propagate_grads
        if propagate_grads.on() and (self.train_inputs[0].requires_grad or self.train_targets.requires_grad):
            raise UnsupportedError(
                "settings.propagate_grads: posterior gradients to the training data are not "
                "supported (the prediction caches are built without a backward to them)")
        key = self._key()
        if self._cache is None or self._cache_key != key:
            ls, os_, noise, c = self.hyper()
            fixed = isinstance(self.likelihood, FixedNoiseGaussianLikelihood)
            Bm = self.task_covar_module.covar_matrix.detach().contiguous()
            if kernels.icm_fused_ok(self.num_tasks, self._d):
                cache, _ = kernels.build_icm_cache(
                    self._Xd, self._task_i32, self.train_targets, ls, Bm,
                    self.likelihood.noise if fixed else noise, c, kind=int(self.kind),
                    outputscale=os_)
            else:
                cache = self._base_cache_generic(ls, os_, noise, c, Bm, fixed)
            self._drop_caches()
            self._cache, self._cache_key = cache, key
            self._B_dev, self._B_host = Bm, Bm.cpu()
        return self._cache

    def _base_cache_generic(self, ls, os_, noise, c, Bm, fixed):
        """T > 16 or d > 64: the covariance as a torch composition on the device
        (covar_matrix, a gather of B), factorised by kernels.cholesky_with_inverse."""
        from . import kernels
        Xd, n = self._Xd, self._Xd.shape[0]
        K = kernels.covar_matrix(Xd, Xd, ls.contiguous(), int(self.kind), os_)
        A = K * Bm[self._task_long][:, self._task_long]
        A = A + torch.diag(self.likelihood.noise if fixed else torch.full_like(self.train_targets, noise))
        L, Linv, jit = kernels.cholesky_with_inverse(A)
        np_ = kernels.padded_order(n)

        def pad(M):  # the caches' layout: np x np with the identity pad
            P = torch.eye(np_, dtype=torch.float64, device=Xd.device)
            P[:n, :n] = M
            return P

        Lp, Lip = pad(L), pad(Linv)
        U = Lip.mT.contiguous()
        beta = Linv @ (self.train_targets - c)
        alpha = Linv.mT @ beta
        Xs = torch.zeros(n, kernels.DP, dtype=torch.float64, device=Xd.device)
        if self._d <= kernels.DP:
            Xs[:, :self._d] = Xd / ls
        return kernels.GPCache(int(self.kind), n, self._d, np_, Xd, Xs, ls.contiguous(), os_,
                               noise, c, Lp, Lip, U, beta.contiguous(), alpha.contiguous(), jit)

    def _task_view(self, t: int):
        """The GPCache view of output task index t (cached until the base caches change)."""
        from . import kernels
        base = self._base_cache()
        view = self._views.get(t)
        if view is None:
            Btt = float(self._B_host[t, t])
            if kernels.icm_fused_ok(self.num_tasks, self._d):
                view = kernels.icm_task_view(base, self._task_i32, self._B_dev, t, Btt)
            else:
                D = torch.ones(base.np, dtype=torch.float64, device=base.U.device)
                D[:base.n] = self._B_dev[t][self._task_long] / Btt
                U = (D.unsqueeze(-1) * base.U).contiguous()
                view = kernels.GPCache(base.kind, base.n, base.d, base.np, base.Xt, base.Xt_scaled,
                                       base.lengthscale, base.outputscale * Btt, base.noise,
                                       base.constant, None, U.mT.contiguous(), U, base.beta,
                                       (D[:base.n] * base.alpha).contiguous(), base.jitter)
            self._views[t] = view
        return view

    def _view_model(self, t: int) -> _TaskView:
        vm = self._view_models.get(t)
        if vm is None:
            vm = self._view_models[t] = _TaskView(self, t)
        return vm

    def prediction_cache(self, key=None):
        """The task view of the one output task (what the fused acquisition routes
        read); a model with several output tasks has no single cache."""
        if self._num_outputs != 1:
            raise UnsupportedError(
                "MultiTaskGP.prediction_cache: the model has several output tasks; the fused "
                "routes take a model with exactly one (output_tasks=[t])")
        return self._task_view(self._task_index[int(self._output_tasks[0])])

    # -- posterior -----------------------------------------------------------------------
    def _observation_noise(self, tq: torch.Tensor) -> torch.Tensor:
        """The noise variance of each test point's task in the model's (transformed)
        space: the inferred noise, or with fixed noise the mean observed noise of
        the task's training points (models/gpytorch.py:772-832)."""
        if not isinstance(self.likelihood, FixedNoiseGaussianLikelihood):
            return self.likelihood.noise.detach().reshape(()).expand(tq.shape)
        nz = self.likelihood.noise
        key = (nz.data_ptr(), nz._version)
        if self._noise_by_task is None or self._noise_by_task[0] != key:
            nbt = torch.zeros(self.num_tasks, dtype=torch.float64, device=tq.device)
            for t in self._task_long.unique().tolist():
                nbt[t] = nz[self._task_long == t].mean()
            self._noise_by_task = (key, nbt)
        return self._noise_by_task[1][tq]

    def posterior(self, X: torch.Tensor, output_indices=None, observation_noise=False,
                  posterior_transform=None):
        """models/gpytorch.py:834-918, computing in fp64."""
        from .posteriors import (GPyTorchPosterior, MultivariateNormal, _ICMGeneralMoments,
                                 posterior_moments)
        if torch.is_tensor(observation_noise):
            raise NotImplementedError(
                "Passing a tensor of observations is not supported by MultiTaskGP.")
        if X.dtype != torch.float64:
            X = X.to(torch.float64)
        d = self._d
        if X.shape[-1] == d + 1:
            if output_indices is not None:
                raise ValueError("`output_indices` must be None when `X` includes task features.")
            Xd, tq = self._split_inputs(X)
            tasks = tq.unique().tolist()
        elif X.shape[-1] == d:
            raw = self._output_tasks if output_indices is None else list(output_indices)
            bad = set(raw).difference(self._expected_task_values)
            if bad:
                raise ValueError("Received invalid raw task values. Expected raw value to be in"
                                 f" {self._expected_task_values}, but got unexpected task values:"
                                 f" {bad}.")
            if len(raw) != 1:
                raise UnsupportedError(
                    "MultiTaskGP.posterior: several output tasks for X without the task column "
                    "(the multi-output posterior with cross-task covariance) are not on the "
                    "accelerated path.  Supported: X with d columns and exactly one output task "
                    "(output_tasks=[t] or output_indices=[t]), or X with the task column "
                    "(d + 1 columns), which is single-output.")
            Xd, tq = X, None
            tasks = [self._task_index[int(raw[0])]]
        else:
            raise ValueError(f"MultiTaskGP.posterior: X has {X.shape[-1]} columns, expected {d} "
                             f"or {d + 1}")
        self.eval()
        batch, q = Xd.shape[:-2], Xd.shape[-2]
        if len(tasks) == 1:
            mean, cov = posterior_moments(self._view_model(int(tasks[0])), Xd)
            if observation_noise is True and tq is None:
                tq = torch.full(Xd.shape[:-1], int(tasks[0]), dtype=torch.long, device=Xd.device)
        else:
            X3 = Xd.reshape(-1, q, d).contiguous()
            mean, cov = _ICMGeneralMoments.apply(X3, tq.reshape(-1, q), self)
            mean, cov = mean.reshape(*batch, q), cov.reshape(*batch, q, q)
        if observation_noise is True:
            _, ystd = self.outcome_stats()
            cov = cov + torch.diag_embed(self._observation_noise(tq) * (ystd * ystd))
        post = GPyTorchPosterior(MultivariateNormal(mean, cov), model=self, X=X)
        return post if posterior_transform is None else posterior_transform(post)

    # -- what stays off the accelerated path -----------------------------------------------
    def condition_on_observations(self, X, Y, **kwargs):
        raise UnsupportedError("condition_on_observations: MultiTaskGP is not on the accelerated "
                               "path (conditioning of multi-task models)")

    def fantasize(self, X, sampler, observation_noise=None, **kwargs):
        raise UnsupportedError("fantasize: MultiTaskGP is not on the accelerated path (fantasy "
                               "models of multi-task models)")

    def subset_output(self, idcs):
        raise UnsupportedError("Subsetting outputs is not supported by `MultiTaskGPyTorchModel`.")


def __getattr__(name):
    # fit_fully_bayesian_model_nuts lives in fit.py, where the reference has it
    # (fit.py imports this module, so the re-export resolves on first use)
    if name == "fit_fully_bayesian_model_nuts":
        from .fit import fit_fully_bayesian_model_nuts
        return fit_fully_bayesian_model_nuts
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
