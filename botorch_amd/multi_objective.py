"""Pareto front and non-dominated box decomposition (setup side of qEHVI).

Restates botorch/utils/multi_objective/pareto.py:16-64 (is_non_dominated) and
box_decompositions/{non_dominated.py:353-457, box_decomposition.py, utils.py}
(FastNondominatedPartitioning: Alg. 1 of Lacour et al. 2017 applied twice, as
in Yang et al. 2019; the direct sweep for m = 2).  Runs once per acquisition
function on the host, like the reference; the hot path consumes only the
resulting hypercell bounds.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def is_non_dominated(Y: torch.Tensor, maximize: bool = True, deduplicate: bool = True) -> torch.Tensor:
    """pareto.py:16-64: device fp64 inputs run bo_pareto_mask (any batch
    shape, m <= 8, one launch); host inputs the pairwise torch form (the loop
    form beyond n = 2000, as the reference)."""
    n = Y.shape[-2]
    if n == 0:
        return torch.zeros(Y.shape[:-1], dtype=torch.bool, device=Y.device)
    if Y.is_cuda and Y.dtype == torch.float64 and Y.shape[-1] <= 8:
        from . import kernels
        return kernels.pareto_mask(Y, maximize, deduplicate)
    if n > 2000:
        return _is_non_dominated_loop(Y, maximize, deduplicate)
    Y1 = Y.unsqueeze(-3)
    Y2 = Y.unsqueeze(-2)
    if maximize:
        dominates = (Y1 >= Y2).all(dim=-1) & (Y1 > Y2).any(dim=-1)
    else:
        dominates = (Y1 <= Y2).all(dim=-1) & (Y1 < Y2).any(dim=-1)
    nd_mask = ~(dominates.any(dim=-1))
    if deduplicate:
        indices = (Y1 == Y2).all(dim=-1).long().argmax(dim=-1)
        keep = torch.zeros_like(nd_mask)
        keep.scatter_(dim=-1, index=indices, value=1.0)
        return nd_mask & keep
    return nd_mask


def _is_non_dominated_loop(Y, maximize=True, deduplicate=True):
    is_efficient = torch.ones(Y.shape[:-1], dtype=torch.bool, device=Y.device)
    for i in range(Y.shape[-2]):
        vals = Y[..., i:i + 1, :]
        if maximize:
            update = (Y > vals).any(dim=-1)
        else:
            update = (Y < vals).any(dim=-1)
        if not deduplicate:
            update = update | (Y == vals).all(dim=-1)
        update[..., i] = True
        is_efficient = is_efficient & (update | ~is_efficient[..., i:i + 1])
    return is_efficient


class FastNondominatedPartitioning:
    """box_decompositions/non_dominated.py:353-457 (maximisation)."""

    def __init__(self, ref_point: torch.Tensor, Y: Optional[torch.Tensor] = None):
        self.ref_point = ref_point.to(torch.float64)
        self.num_outcomes = ref_point.shape[-1]
        self.Y = None
        if Y is not None:
            self.update(Y)

    def update(self, Y: torch.Tensor) -> None:
        Y = Y.to(torch.float64).to(self.ref_point.device)
        self.Y = Y if self.Y is None else torch.cat([self.Y, Y], dim=-2)
        mask = is_non_dominated(self.Y) & (self.Y > self.ref_point).all(dim=-1)
        pareto = self.Y[mask]
        if self.num_outcomes == 2:
            pareto = pareto[torch.argsort(pareto[:, 0])]
        self.pareto_Y = pareto
        self._partition()

    def _partition(self) -> None:
        """Lacour17 (utils.py:103-288) in native host code: bo_nd_partition_host."""
        from . import kernels
        lo, hi = kernels.nd_partition_host(self.Y, self.ref_point.cpu())
        dev = self.ref_point.device
        self.hypercell_bounds = torch.stack([lo, hi]).to(dev)

    def get_hypercell_bounds(self) -> torch.Tensor:
        return self.hypercell_bounds

    def compute_hypervolume(self) -> torch.Tensor:
        """non_dominated.py:442-457."""
        if self.pareto_Y.shape[0] == 0:
            return torch.tensor(0.0, dtype=torch.float64)
        ideal = self.pareto_Y.max(dim=-2, keepdim=True).values
        total = (ideal.squeeze(-2) - self.ref_point).clamp_min(0.0).prod(dim=-1)
        finite = torch.min(self.hypercell_bounds, ideal)
        non_dom = (finite[1] - finite[0]).clamp_min(0.0).prod(dim=-1).sum(dim=-1)
        return total - non_dom


NondominatedPartitioning = FastNondominatedPartitioning


class ChebyshevScalarization:
    """The augmented Chebyshev scalarization of :func:`get_chebyshev_scalarization` as
    an object: ``obj(Y, X=None) = -(max_i p_i + alpha sum_i p_i)`` with the per-outcome
    affine form ``p_i = a_i y_i + b_i`` (``a``, ``b``: what bo_qmc_cheb takes), where
    p_i = w_i y~_i and y~ is -y normalised by ``Y_bounds`` (shifted by -1 for a negative
    weight), or -y itself when no baseline outcomes were given.  ``outcomes`` (set by
    :meth:`over_outcomes`): the columns of the samples it reads, None for all."""

    def __init__(self, weights: torch.Tensor, Y_bounds: Optional[torch.Tensor], alpha: float,
                 outcomes=None):
        self.weights, self.Y_bounds, self.alpha = weights, Y_bounds, float(alpha)
        self.outcomes = None if outcomes is None else [int(i) for i in outcomes]
        if Y_bounds is None:
            self.a, self.b = -weights, torch.zeros_like(weights)
        else:
            span = Y_bounds[1] - Y_bounds[0]
            self.a = -weights / span
            self.b = weights * (-Y_bounds[0] / span - (weights < 0).to(weights))

    def over_outcomes(self, outcomes) -> "ChebyshevScalarization":
        """The same scalarization reading the ``outcomes`` columns of wider samples."""
        return ChebyshevScalarization(self.weights, self.Y_bounds, self.alpha, outcomes)

    def __call__(self, Y: torch.Tensor, X: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.outcomes is not None:
            Y = Y[..., self.outcomes]
        p = self.a.to(Y) * Y + self.b.to(Y)
        return -(p.max(dim=-1).values + self.alpha * p.sum(dim=-1))


def get_chebyshev_scalarization(weights: torch.Tensor, Y: torch.Tensor,
                                alpha: float = 0.05) -> ChebyshevScalarization:
    """utils/multi_objective/scalarization.py [Knowles2005]: the augmented Chebyshev
    scalarization g(y) = max_i w_i y_i + alpha sum_i w_i y_i, to be minimised over
    outcomes that are to be minimised.  Outcomes here are maximised, so the returned
    objective negates its input, normalises it with the bounds of the negated baseline
    ``Y`` (n x m) to [0, 1] -- to [-1, 0] for a negative weight, which stands for an
    outcome to minimise -- and returns -g.  ``Y`` with n = 0 leaves the outcomes
    unnormalised (negative weights are then unsupported)."""
    from .exceptions import BotorchTensorDimensionError, UnsupportedError
    if weights.shape != Y.shape[-1:]:
        raise BotorchTensorDimensionError(f"one weight per outcome is required: weights has shape "
                                          f"{tuple(weights.shape)}, Y {tuple(Y.shape)}")
    if Y.ndim > 2:
        raise NotImplementedError(f"Y must be n x m, got {Y.ndim} dimensions")
    if Y.shape[-2] == 0:
        if (weights < 0).any():
            raise UnsupportedError("a negative weight (an outcome to minimise) needs baseline "
                                   "outcomes Y to normalise with; Y has no rows")
        return ChebyshevScalarization(weights, None, alpha)
    Yn = -Y
    return ChebyshevScalarization(weights, torch.stack([Yn.min(dim=-2).values,
                                                        Yn.max(dim=-2).values]), alpha)
