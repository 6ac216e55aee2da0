"""Risk measures as MC objectives (botorch/acquisition/risk_measures.py): posterior
samples at the ``q n_w`` perturbed copies of ``q`` inputs (an ``InputPerturbation``
transform) become ``q`` samples of a risk measure over each input's ``n_w`` copies.

These are ordinary torch objectives, on any device and any MC acquisition class.  On
qSimpleRegret, qExpectedImprovement and qLogExpectedImprovement over a perturbed
SingleTaskGP, the four measures with the identity preprocessing function run fused
(``kernels.qmc_risk``, csrc/risk.hip): ``risk_kind_k`` is what that kernel takes.

The measures read the lower tail: larger is better, as everywhere in this library.
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import torch
from torch import Tensor

from .objective import IdentityMCObjective, MCAcquisitionObjective


class RiskMeasureMCObjective(MCAcquisitionObjective):
    """The base: ``preprocessing_function`` (default: the identity on one output) maps
    ``... x (q n_w) x m`` samples to ``... x (q n_w)``, ``_prepare_samples`` splits the
    last dimension into ``q x n_w``."""

    def __init__(self, n_w: int, preprocessing_function: Optional[Callable[[Tensor], Tensor]] = None):
        super().__init__()
        self.n_w = int(n_w)
        self.preprocessing_function = (preprocessing_function if preprocessing_function is not None
                                       else IdentityMCObjective())

    def _prepare_samples(self, samples: Tensor) -> Tensor:
        if samples.shape[-1] > 1 and isinstance(self.preprocessing_function, IdentityMCObjective):
            raise RuntimeError("Multi-output samples should be scalarized using a "
                               "`preprocessing_function`.")
        samples = self.preprocessing_function(samples)
        return samples.reshape(*samples.shape[:-1], -1, self.n_w)

    def risk_kind_k(self):
        """(kind, k) of ``kernels.qmc_risk``, or None when the kernel has no such measure."""
        return None

    def forward(self, samples: Tensor, X: Optional[Tensor] = None) -> Tensor:
        raise NotImplementedError


class CVaR(RiskMeasureMCObjective):
    """Conditional value-at-risk at level ``alpha`` in (0, 1]: the mean of the
    ``n_w - (ceil(n_w alpha) - 1)`` smallest of each input's ``n_w`` samples."""

    def __init__(self, alpha: float, n_w: int,
                 preprocessing_function: Optional[Callable[[Tensor], Tensor]] = None):
        super().__init__(n_w=n_w, preprocessing_function=preprocessing_function)
        if not 0 < alpha <= 1:
            raise ValueError("alpha must be in (0.0, 1.0]")
        self.alpha = alpha
        self.alpha_idx = math.ceil(n_w * alpha) - 1

    def risk_kind_k(self):
        return 0, self.n_w - self.alpha_idx

    def forward(self, samples: Tensor, X: Optional[Tensor] = None) -> Tensor:
        prepared = self._prepare_samples(samples)
        return torch.topk(prepared, k=self.n_w - self.alpha_idx, largest=False,
                          dim=-1).values.mean(dim=-1)


class VaR(CVaR):
    """Value-at-risk at level ``alpha``: the largest of the samples CVaR averages, i.e. the
    ``n_w - (ceil(n_w alpha) - 1)``-th smallest."""

    def risk_kind_k(self):
        return 1, self.n_w - self.alpha_idx

    def forward(self, samples: Tensor, X: Optional[Tensor] = None) -> Tensor:
        prepared = self._prepare_samples(samples)
        return torch.kthvalue(prepared, k=self.n_w - self.alpha_idx, dim=-1).values


class WorstCase(RiskMeasureMCObjective):
    """The smallest of each input's ``n_w`` samples."""

    def risk_kind_k(self):
        return 0, 1

    def forward(self, samples: Tensor, X: Optional[Tensor] = None) -> Tensor:
        return self._prepare_samples(samples).min(dim=-1).values


class Expectation(RiskMeasureMCObjective):
    """The mean of each input's ``n_w`` samples."""

    def risk_kind_k(self):
        return 0, self.n_w

    def forward(self, samples: Tensor, X: Optional[Tensor] = None) -> Tensor:
        return self._prepare_samples(samples).mean(dim=-1)


__all__ = ["RiskMeasureMCObjective", "CVaR", "VaR", "WorstCase", "Expectation"]
