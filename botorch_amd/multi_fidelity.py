"""Synthetic multi-fidelity problems (botorch/test_functions/multi_fidelity.py)."""
from __future__ import annotations

import torch

from .test_functions import _H6_A, _H6_P, _H_ALPHA, Hartmann


class AugmentedHartmann:
    """Augmented Hartmann (botorch/test_functions/multi_fidelity.py:57-115): Hartmann-6
    over x_1..x_6 with ALPHA_1 replaced by ALPHA_1 - 0.1 (1 - x_7); the seventh column
    is the fidelity.  Minimiser (0.20169, 0.150011, 0.476874, 0.275332, 0.311652,
    0.6573, 1.0), H_min = -3.32237."""

    dim = 7
    _optimal_value = -3.32237
    _optimizers = [(0.20169, 0.150011, 0.476874, 0.275332, 0.311652, 0.6573, 1.0)]

    def __init__(self, noise_std=None, negate: bool = False):
        self.noise_std = noise_std
        self.negate = negate
        self.bounds = torch.tensor([[0.0] * 7, [1.0] * 7])

    def evaluate_true(self, X: torch.Tensor) -> torch.Tensor:
        A = torch.tensor(_H6_A).to(X)
        P = torch.tensor(_H6_P).to(X)
        alpha = torch.tensor(_H_ALPHA).to(X)
        inner = torch.sum(A * (X[..., :6].unsqueeze(-2) - 0.0001 * P).pow(2), dim=-1)
        alpha1 = alpha[0] - 0.1 * (1 - X[..., 6])
        return -(alpha1 * torch.exp(-inner[..., 0])
                 + torch.sum(alpha[1:] * torch.exp(-inner[..., 1:]), dim=-1))

    __call__ = Hartmann.__call__
