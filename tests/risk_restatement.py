"""bo_qmc_risk restated in torch fp64 on the CPU: f = mean + Z tril(L)^T, a sort per
n_w-block, the mode's formula, gradients by autograd.  ``form`` 1 is the same mathematics
in another order of operations (f accumulated column by column, the samples reduced in
descending order): the two forms' disagreement sizes the tests' tolerance."""
import torch

from botorch_amd import _lib
from botorch_amd.safe_math import (TAU_MAX, TAU_RELU, fatmax, log_improvement, logmeanexp,
                                   smooth_amax)

# (q, n_w): smallest block; Q inside one tile; blocks straddling a tile edge; n_w straddling
# tiles; Q, n_w and q at their limits
SHAPES = [(1, 2), (3, 5), (3, 7), (2, 33), (4, 32), (1, 128), (16, 8)]
MODES = [_lib.QMC_QSR, _lib.QMC_QEI, _lib.QMC_QLOGEI]
CASES = []  # (q, n_w, k, S, B, kind, mode, fat)
for _i, (_q, _nw) in enumerate(SHAPES):
    for _kind in (0, 1):
        for _m, _mode in enumerate(MODES):
            CASES.append((_q, _nw, (1, (_nw + 1) // 2, _nw)[(_i + _kind + _m) % 3],
                          (24, 64, 100)[(_i + _m) % 3], (1, 3)[(_i + _kind) % 2], _kind, _mode,
                          _i % 2 == 0))


def make_inputs(q, n_w, S, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    Q = q * n_w
    mean = torch.randn(B, Q, dtype=torch.float64, generator=g)
    A = torch.randn(B, Q, Q, dtype=torch.float64, generator=g) / Q ** 0.5
    L = A.tril(-1) + torch.diag_embed(0.5 + torch.rand(B, Q, dtype=torch.float64, generator=g))
    Z = torch.randn(S, Q, dtype=torch.float64, generator=g)
    return mean, L, Z


def risk_samples(mean, L, Z, q, n_w, k, kind, form=0):
    """r (S x B x q) and the sorted blocks (S x B x q x n_w)."""
    Lt = L.tril()
    if form == 0:
        f = mean + (Z @ Lt.mT).transpose(0, 1)                 # S x B x Q
    else:
        f = mean.expand(Z.shape[0], *mean.shape)
        for i in range(Z.shape[1]):
            f = f + Z[:, None, i:i + 1] * Lt[None, :, :, i]
    srt = f.reshape(*f.shape[:-1], q, n_w).sort(dim=-1).values
    r = srt[..., :k].mean(dim=-1) if kind == 0 else srt[..., k - 1]
    return r, srt


def restate(mean, L, Z, q, n_w, k, kind, mode, best_f, fat, form=0):
    """acq (B), as bo_qmc_risk's contract states it."""
    r, _ = risk_samples(mean, L, Z, q, n_w, k, kind, form)
    if form == 1:
        r = r.flip(0)
    if mode == _lib.QMC_QSR:
        return r.amax(dim=-1).mean(dim=0)
    if mode == _lib.QMC_QEI:
        return (r - best_f).clamp_min(0).amax(dim=-1).mean(dim=0)
    li = log_improvement(r, torch.tensor(best_f, dtype=torch.float64), tau=TAU_RELU, fat=fat)
    return logmeanexp((fatmax if fat else smooth_amax)(li, dim=-1, tau=TAU_MAX), dim=0)


def well_separated(mean, L, Z, q, n_w, k, kind, mode):
    """(best_f, margin): best_f between the two middle values of r, and the smallest of the
    gaps a rounding error could flip a selection across -- the k-th to the (k + 1)-th
    smallest of a block, the two largest r over a, and |r - best_f|."""
    r, srt = risk_samples(mean, L, Z, q, n_w, k, kind)
    flat = r.flatten().sort().values
    best_f = float(0.5 * (flat[flat.numel() // 2 - 1] + flat[flat.numel() // 2]))
    gaps = []
    if k < n_w:
        gaps.append((srt[..., k] - srt[..., k - 1]).min())
    if q > 1:
        top = r.topk(2, dim=-1).values
        gaps.append((top[..., 0] - top[..., 1]).min())
    if mode != _lib.QMC_QSR:
        gaps.append((r - best_f).abs().min())
    return best_f, float(torch.stack(gaps).min()) if gaps else float("inf")


def value_and_grads(mean, L, Z, q, n_w, k, kind, mode, best_f, fat, dacq, form=0):
    mean, L = mean.clone().requires_grad_(True), L.clone().requires_grad_(True)
    acq = restate(mean, L, Z, q, n_w, k, kind, mode, best_f, fat, form)
    (acq * dacq).sum().backward()
    return acq.detach(), mean.grad, L.grad
