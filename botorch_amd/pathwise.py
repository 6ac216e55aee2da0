"""Pathwise posterior sampling (Matheron paths) of exact GPs
(botorch/sampling/pathwise): function draws

    (f | y)(.) = f(.) + K(., X) (K + noise)^{-1} (y - f(X) - eps)

whose prior part f is a linear model on random Fourier features and whose
update part is the kernel row against the weights V.  Drawing is a handful of
small device calls (Sobol normals, the prior at the training inputs, two GEMMs
against the prediction cache's L^{-1}); evaluating S paths at R points is one
fused launch (``torch.ops.bo.paths_eval``, csrc/paths.hip) that keeps the
R x M features and the R x n kernel rows in registers.

A single-output member with kernel kind, lengthscale l, outputscale o, mean
constant c, training inputs Xt, outcome statistics (ymean, ystd), frequencies
Omega (H x d, H = M / 2), prior weights W (S x M), update weights V (S x n):

    theta_j(x) = sum_t Omega[j, t] x_t / l_t
    g_s(x) = c + sqrt(2 o / M) sum_{j<H} (W[s, j] sin theta_j(x) + W[s, H + j] cos theta_j(x))
               + sum_i V[s, i] o k(x, Xt_i)
    f_s(x) = ymean + ystd g_s(x)

Broadcasting (the reference's): X of shape ``... x P x d`` whose dimensions
before ``P`` end in ``sample_shape`` is evaluated path by path (path s on its
own points, the kernel's *mapped* mode) and returns ``X.shape[:-1]``; any other
X is evaluated on every path (*all* mode) and returns ``sample_shape x ... x P``.
"""
from __future__ import annotations

import math
from typing import Callable, List, Optional

import torch
from torch import Size, Tensor, nn

from .exceptions import UnsupportedError

F64 = torch.float64
MATERN_NU = 2.5


# ---- model checks (all on the host, before any native call) -----------------------------------
def _members(model) -> Optional[list]:
    """The single-output members of a ModelListGP or a multi-output SingleTaskGP
    (None: the model is itself one)."""
    from .models import ModelListGP, SingleTaskGP
    if isinstance(model, ModelListGP):
        return list(model.models)
    if isinstance(model, SingleTaskGP) and model._is_multi_output:
        return list(model.models)
    return None


def _check_model(model) -> None:
    from .models import ModelListGP, SaasFullyBayesianSingleTaskGP, SingleTaskGP
    if isinstance(model, SaasFullyBayesianSingleTaskGP):
        raise NotImplementedError(
            f"Pathwise sampling is not implemented for {type(model).__name__} (fully Bayesian "
            "models are not supported).")
    if getattr(model, "_is_multitask", False):
        raise UnsupportedError("Pathwise sampling: MultiTaskGP is not on the accelerated path "
                               "(the paths' prior features take a single-task kernel).")
    if not isinstance(model, (SingleTaskGP, ModelListGP)):
        raise NotImplementedError(f"Pathwise sampling is not implemented for {type(model).__name__}.")
    if model.training:
        raise UnsupportedError("Pathwise sampling needs a model in eval mode (model.eval()): the "
                               "paths are drawn from the trained model's prediction caches.")


def _check_features(num_features: int, d: int) -> None:
    from . import kernels
    if num_features % 2:
        raise UnsupportedError(
            f"Expected an even number of output features, but received num_outputs={num_features}.")
    if num_features < 2:
        raise UnsupportedError(f"Expected at least two features, but received {num_features}.")
    if d > kernels.PATHS_DMAX:
        raise UnsupportedError(f"Pathwise sampling supports d <= {kernels.PATHS_DMAX} (got {d}).")


def _sample_shape(sample_shape) -> Size:
    return Size([sample_shape]) if isinstance(sample_shape, int) else Size(sample_shape)


# ---- evaluation ------------------------------------------------------------------------------
class _Member:
    """The hyperparameters of one single-output member, read once per draw."""

    def __init__(self, model):
        from .models import FixedNoiseGaussianLikelihood
        ls, o, noise, c = model.hyper()
        self.kind = int(model.kind)
        self.lengthscale = ls.to(F64).contiguous()
        self.outputscale = float(o)
        self.constant = float(c)
        self.Xt = model.train_inputs[0]
        self.Xt_scaled = (self.Xt / self.lengthscale).contiguous()
        self.fixed = isinstance(model.likelihood, FixedNoiseGaussianLikelihood)
        self.noise = model.likelihood.noise.detach().reshape(-1).to(F64) if self.fixed \
            else float(noise)


def _evaluate(X: Tensor, sample_shape: Size, mem: _Member, Omega: Tensor, W: Tensor,
              V: Optional[Tensor], constant: float, ymean: float, ystd: float) -> Tensor:
    """The broadcasting of the module docstring over one ``bo::paths_eval`` call."""
    from . import ops  # noqa: F401  (torch.ops.bo registration)
    if X.dim() < 2 or X.shape[-1] != Omega.shape[-1]:
        raise ValueError(f"Expected X of shape `... x P x {Omega.shape[-1]}`, got {tuple(X.shape)}.")
    if X.dtype != F64:
        X = X.to(F64)
    d = X.shape[-1]
    lead, k = X.shape[:-2], len(sample_shape)
    mapped = k > 0 and len(lead) >= k and tuple(lead[-k:]) == tuple(sample_shape)
    inner = X.shape[-2] if mapped else 0
    out = torch.ops.bo.paths_eval(X.reshape(-1, d), mem.lengthscale, Omega, W,
                                  mem.Xt_scaled if V is not None else None, V, mem.kind,
                                  mem.outputscale, constant, ymean, ystd, inner)
    return out.view(X.shape[:-1]) if mapped else out.view(*sample_shape, *X.shape[:-1])


class FourierFeatureMap(nn.Module):
    """The random Fourier features of a stationary kernel: ``weight`` holds the
    frequencies Omega (H x d); phi(x) = sqrt(2 o / M) [sin, cos](Omega (x / l))
    (features/generators.py:66-193)."""

    def __init__(self, weight: Tensor):
        super().__init__()
        self.register_buffer("weight", weight)


class KernelEvaluationMap(nn.Module):
    """The canonical features k(., points) of the update (features/maps.py)."""

    def __init__(self, points: Tensor):
        super().__init__()
        self.register_buffer("points", points)


class KernelFeaturePaths(nn.Module):
    """Prior paths: the mean constant plus ``weight`` (S x M) on the Fourier
    features (prior_samplers.py:52-106).  Evaluates in the model's transformed
    outcome space, as the reference's prior paths do."""

    def __init__(self, mem: _Member, sample_shape: Size, Omega: Tensor, weight: Tensor):
        super().__init__()
        self._mem = mem
        self.sample_shape = sample_shape
        self.feature_map = FourierFeatureMap(Omega)
        self.register_buffer("weight", weight)

    def forward(self, X: Tensor) -> Tensor:
        return _evaluate(X, self.sample_shape, self._mem, self.feature_map.weight, self.weight,
                         None, self._mem.constant, 0.0, 1.0)


class KernelUpdatePaths(nn.Module):
    """Update paths: ``weight`` (S x n) on the kernel row against the training
    inputs (update_strategies.py:94-104)."""

    def __init__(self, mem: _Member, sample_shape: Size, weight: Tensor):
        super().__init__()
        self._mem = mem
        self.sample_shape = sample_shape
        self.feature_map = KernelEvaluationMap(mem.Xt)
        self.register_buffer("weight", weight)

    def forward(self, X: Tensor) -> Tensor:
        S, d = self.weight.shape[0], self._mem.Xt.shape[1]
        zero = self.weight.new_zeros
        return _evaluate(X, self.sample_shape, self._mem, zero(1, d), zero(S, 2), self.weight,
                         0.0, 0.0, 1.0)


class MatheronPath(nn.Module):
    """Posterior function draws by Matheron's rule (posterior_samplers.py:50-88):
    the sum of ``paths["prior_paths"]`` and ``paths["update_paths"]``, passed
    through the outcome untransform -- evaluated in one fused launch and
    differentiable in X."""

    def __init__(self, prior_paths: KernelFeaturePaths, update_paths: KernelUpdatePaths,
                 ymean: float = 0.0, ystd: float = 1.0):
        super().__init__()
        self.paths = nn.ModuleDict({"prior_paths": prior_paths, "update_paths": update_paths})
        self.ymean, self.ystd = float(ymean), float(ystd)

    @property
    def sample_shape(self) -> Size:
        return self.paths["prior_paths"].sample_shape

    def forward(self, X: Tensor) -> Tensor:
        prior, update = self.paths["prior_paths"], self.paths["update_paths"]
        return _evaluate(X, prior.sample_shape, prior._mem, prior.feature_map.weight, prior.weight,
                         update.weight, prior._mem.constant, self.ymean, self.ystd)


class PathList(nn.Module):
    """One path set per output (paths.py PathList).  Returns the list of the
    members' values, or ``join`` of it."""

    def __init__(self, paths: List[nn.Module], join: Optional[Callable] = None):
        super().__init__()
        self.paths = nn.ModuleList(paths)
        self.join = join

    @property
    def sample_shape(self) -> Size:
        return self.paths[0].sample_shape

    def forward(self, X: Tensor):
        outs = [p(X) for p in self.paths]
        return outs if self.join is None else self.join(outs)


def _stack_last(outs):
    return torch.stack(outs, dim=-1)


def _per_member(model, fn):
    """fn over the members of a list / multi-output model (their values stack on
    the last dim for a multi-output SingleTaskGP), or fn(model)."""
    from .models import ModelListGP
    members = _members(model)
    if members is None:
        return fn(model)
    if any(_members(m) is not None for m in members):
        raise UnsupportedError("A model-list of multi-output models is not supported.")
    return PathList([fn(m) for m in members],
                    join=None if isinstance(model, ModelListGP) else _stack_last)


# ---- drawing ---------------------------------------------------------------------------------
def draw_kernel_feature_paths(model, sample_shape, num_features: int = 1024):
    """Prior paths of ``model`` on ``num_features`` random Fourier features
    (prior_samplers.py:52-106).  Frequencies: an H x d Sobol-normal draw, each
    row scaled by Gamma(nu, nu)^{-1/2} for Matern-5/2 (generators.py:112-168);
    weights: an S x M Sobol-normal draw -- both from the device Sobol generator
    (kernels.sobol_normal), unseeded as the reference's."""
    from . import kernels
    _check_model(model)
    sample_shape = _sample_shape(sample_shape)
    members = _members(model)
    if members is not None:
        return _per_member(model, lambda m: draw_kernel_feature_paths(m, sample_shape, num_features))
    d = model.train_inputs[0].shape[-1]
    _check_features(num_features, d)
    with torch.no_grad():
        mem = _Member(model)
        dev = mem.Xt.device
        S, H = max(sample_shape.numel(), 1), num_features // 2
        Omega = kernels.sobol_normal(d, H, None, dev)
        if mem.kind == kernels._lib.MATERN52:
            nu = torch.tensor(MATERN_NU, dtype=F64, device=dev)
            Omega = torch.distributions.Gamma(nu, nu).rsample((H, 1)).rsqrt() * Omega
        W = kernels.sobol_normal(num_features, S, None, dev)
    return KernelFeaturePaths(mem, sample_shape, Omega.contiguous(), W.contiguous())


def gaussian_update(model, sample_values: Tensor, target_values: Optional[Tensor] = None, *,
                    noise_values: Optional[Tensor] = None) -> KernelUpdatePaths:
    """The update paths of an exact GP (update_strategies.py:72-135):
    V = A^{-1} (target - sample_values - eps), A = K + noise (+ the cache's
    jitter), eps ~ N(0, noise) per training point.  ``sample_values``:
    ``sample_shape x n`` prior values at the training inputs in the model's
    transformed outcome space; ``target_values`` defaults to the transformed
    training targets.  A comes factored from the prediction cache: V =
    Linv^T (Linv E) is two GEMMs on n x S, nothing is factorised again.
    ``noise_values`` (an extension): eps itself, ``sample_shape x n``, instead
    of a draw."""
    from . import kernels
    _check_model(model)
    if _members(model) is not None:
        raise UnsupportedError("gaussian_update takes a single-output model (use "
                               "draw_matheron_paths for lists and multi-output models).")
    with torch.no_grad():
        mem = _Member(model)
        cache = model.prediction_cache()
        n = cache.n
        if sample_values.shape[-1] != n:
            raise ValueError(f"sample_values must end in n = {n}, got {tuple(sample_values.shape)}")
        sample_shape = sample_values.shape[:-1]
        F = sample_values.reshape(-1, n).to(F64)
        S = F.shape[0]
        y = (model.train_targets if target_values is None else target_values).to(F64).reshape(-1)
        if noise_values is None:
            sd = mem.noise.sqrt() if mem.fixed else math.sqrt(mem.noise)
            eps = torch.randn(S, n, dtype=F64, device=F.device) * sd
        else:
            eps = noise_values.reshape(S, n).to(F64)
        E = (y.unsqueeze(0) - F - eps).t().contiguous()  # n x S
        ld = cache.Linv.shape[1]
        T = torch.empty(n, S, dtype=F64, device=F.device)
        Vt = torch.empty(n, S, dtype=F64, device=F.device)
        # the leading n x n block of the (padded) L^{-1}, read in place
        kernels.gemm_strided(n, S, n, cache.Linv, ld, 0, E, S, 0, T, S, 0, 1)
        kernels.gemm_strided(n, S, n, cache.Linv, ld, 0, T, S, 0, Vt, S, 0, 1, transA=True)
        V = Vt.t().contiguous()
    return KernelUpdatePaths(mem, Size(sample_shape), V)


def draw_matheron_paths(model, sample_shape, prior_sampler: Callable = draw_kernel_feature_paths,
                        update_strategy: Callable = gaussian_update):
    """Function draws from the posterior of ``model`` (posterior_samplers.py:
    147-224): a :class:`MatheronPath`, or a :class:`PathList` of them for a
    ModelListGP (a list of values) and a multi-output SingleTaskGP (values
    stacked on the last dim).  The prior values at the training inputs are the
    fused kernel itself run on them with the update switched off; the outcome
    transform is left out of the draw and applied to the evaluated sum."""
    _check_model(model)
    sample_shape = _sample_shape(sample_shape)
    if _members(model) is not None:
        return _per_member(model, lambda m: draw_matheron_paths(m, sample_shape, prior_sampler,
                                                                update_strategy))
    prior_paths = prior_sampler(model=model, sample_shape=sample_shape)
    with torch.no_grad():
        sample_values = prior_paths(model.train_inputs[0])  # sample_shape x n
    update_paths = update_strategy(model=model, sample_values=sample_values,
                                   target_values=model.train_targets)
    ymean, ystd = model.outcome_stats()
    return MatheronPath(prior_paths, update_paths, ymean, ystd)


def get_matheron_path_model(model, sample_shape: Optional[Size] = None):
    """A deterministic model that evaluates one Matheron path draw of ``model``
    with the output dimension last (posterior_samplers.py:91-144): X of shape
    ``batch_shape x q x d`` -> ``batch_shape x q x m``.  With ``sample_shape``
    the inputs carry it in front of ``q`` (``... x sample_shape x q x d``)."""
    from .models import GenericDeterministicModel, ModelListGP
    sample_shape = Size() if sample_shape is None else _sample_shape(sample_shape)
    path = draw_matheron_paths(model, sample_shape=sample_shape)
    num_outputs = model.num_outputs
    listed = isinstance(model, ModelListGP)

    def f(X: Tensor) -> Tensor:
        if num_outputs == 1 and not isinstance(path, PathList):
            return path(X).unsqueeze(-1)
        return torch.stack(path(X), dim=-1) if listed else path(X)

    path_model = GenericDeterministicModel(f=f, num_outputs=num_outputs)
    path_model._is_ensemble = len(sample_shape) > 0
    return path_model


# ---- optimising the draws ----------------------------------------------------------------------
def optimize_posterior_samples(paths, bounds: Tensor, candidates: Optional[Tensor] = None,
                               raw_samples: Optional[int] = 1024, num_restarts: int = 20,
                               maximize: bool = True, **kwargs):
    """Maximise (or minimise) each of the S sample paths over the box
    (utils/sampling.py:988-1053): every path is evaluated on ``raw_samples``
    scrambled-Sobol points (plus ``candidates``, n_c x d, when given) in one
    *all*-mode call, the ``num_restarts`` best points of each path are refined on
    the *mapped* path function, and the best of the starts and the refined points
    is returned: ``X_opt`` (S x d) and ``f_opt`` (S x 1), with f_opt = paths(X_opt).

    Deviation: the reference refines with ``gen_candidates_torch`` (Adam); this
    project has no such generator and uses its ``gen_candidates_scipy``
    (L-BFGS-B on the box, all S x num_restarts points in one problem).  ``kwargs``
    go to it (e.g. ``options``)."""
    from .optim import gen_candidates_scipy
    from torch.quasirandom import SobolEngine
    if isinstance(paths, PathList):
        raise UnsupportedError("optimize_posterior_samples takes the paths of a single-output model.")
    sample_shape = paths.sample_shape
    if len(sample_shape) > 1:
        raise UnsupportedError("optimize_posterior_samples takes paths with one sample dimension.")
    sign = 1.0 if maximize else -1.0
    dev, d = paths.paths["prior_paths"].weight.device, bounds.shape[-1]
    bounds = bounds.to(device=dev, dtype=F64)
    unit = SobolEngine(dimension=d, scramble=True).draw(raw_samples, dtype=F64).to(dev)
    cand = bounds[0] + (bounds[1] - bounds[0]) * unit
    if candidates is not None:
        cand = torch.cat([cand, candidates.to(cand).reshape(-1, d)], dim=0)
    with torch.no_grad():
        queries = sign * paths(cand).reshape(-1, cand.shape[0])  # S x N, all mode
    k = min(num_restarts, cand.shape[0])
    X0 = cand[torch.topk(queries, k, dim=-1).indices]  # S x k x d

    def path_func(X):  # S x k x d -> S x k, mapped mode
        return sign * paths(X.reshape(*sample_shape, k, d)).reshape(-1, k)

    X1, _ = gen_candidates_scipy(X0, path_func, lower_bounds=bounds[0], upper_bounds=bounds[1],
                                 **kwargs)
    X_all = torch.cat([X0, X1.to(X0)], dim=1)  # the starts stay eligible
    with torch.no_grad():
        f_all = sign * paths(X_all.reshape(*sample_shape, 2 * k, d)).reshape(-1, 2 * k)
    f_opt, arg = f_all.max(dim=-1, keepdim=True)
    X_opt = X_all.gather(1, arg.unsqueeze(-1).expand(-1, 1, d)).squeeze(1)
    return X_opt, sign * f_opt


def get_optimal_samples(model, bounds: Tensor, num_optima: int, raw_samples: int = 1024,
                        num_restarts: int = 20, maximize: bool = True):
    """``num_optima`` posterior draws and their optimisers (acquisition/utils.py:
    487-520): (X_opt num_optima x d, f_opt num_optima x 1)."""
    paths = draw_matheron_paths(model, sample_shape=Size([num_optima]))
    return optimize_posterior_samples(paths, bounds=bounds, raw_samples=raw_samples,
                                      num_restarts=num_restarts, maximize=maximize)
