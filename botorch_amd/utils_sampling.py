"""Quasi-random design helpers (botorch/utils/sampling.py:40-137)."""
from __future__ import annotations

from contextlib import contextmanager
from typing import Optional

import torch
from torch.quasirandom import SobolEngine


@contextmanager
def manual_seed(seed: Optional[int] = None):
    """botorch/utils/sampling.py:40-63."""
    old = torch.random.get_rng_state()
    try:
        if seed is not None:
            torch.random.manual_seed(seed)
        yield
    finally:
        if seed is not None:
            torch.random.set_rng_state(old)


def draw_sobol_samples(bounds: torch.Tensor, n: int, q: int, batch_shape=None,
                       seed: Optional[int] = None) -> torch.Tensor:
    """n x (batch_shape) x q x d scrambled-Sobol points in the box
    (botorch/utils/sampling.py:66-105).  Drawn on the host (as the reference
    does) -- these are the raw-sample designs, not the hot path."""
    batch_shape = torch.Size(batch_shape or [])
    batch_size = int(torch.prod(torch.tensor(batch_shape))) if len(batch_shape) else 1
    d = bounds.shape[-1]
    lower = bounds[0]
    rng = bounds[1] - bounds[0]
    eng = SobolEngine(q * d, scramble=True, seed=seed)
    raw = eng.draw(batch_size * n, dtype=lower.dtype)
    raw = raw.view(*batch_shape, n, q, d).to(device=lower.device)
    if len(batch_shape):
        raw = raw.permute(-3, *range(len(batch_shape)), -2, -1)
    return lower + rng * raw


def sample_simplex(d: int, n: int = 1, qmc: bool = False, seed: Optional[int] = None,
                   device=None, dtype=None) -> torch.Tensor:
    """utils/sampling.py:178-216: n uniform draws from the d-simplex (n x d, rows
    non-negative with sum 1), as the gaps of d - 1 sorted uniforms in [0, 1]; ``qmc``
    takes the uniforms from a scrambled Sobol sequence."""
    if d == 1:
        return torch.ones(n, 1, device=device, dtype=dtype)
    if qmc:
        u = SobolEngine(d - 1, scramble=True, seed=seed).draw(n, dtype=dtype)
    else:
        with manual_seed(seed=seed):
            u = torch.rand(n, d - 1, dtype=dtype)
    edges = torch.cat([torch.zeros(n, 1, dtype=dtype), u.sort(dim=-1).values,
                       torch.ones(n, 1, dtype=dtype)], dim=-1)
    gaps = edges[..., 1:] - edges[..., :-1]
    return gaps.to(device) if device is not None else gaps
