"""bo_analytic_v / bo_analytic_backward_v alone (kernels.analytic,
kernels.analytic_backward) against the torch restatement of the six modes and
the feasibility terms (tests/analytic_restatement.py), CPU autograd through it,
and the 80-digit truth of tests/golden/golden_analytic.npz.

Every tensor argument is a window of a larger buffer filled with NaN: a read
outside an array reaches the outputs, and these must be finite.  Every call is
repeated once and compared bitwise (no atomics).  Bound against the restatement
(the project's kernel-against-torch bound): max|got - ref| <= 1e-9 max|ref| + 1e-10.

Shapes.  R in {1, 255, 256, 257, 1025} (one thread per row, 256-thread blocks:
one block, its edge, past four blocks); Mt in {1, 2, 4, 16}; the constraint sets
none, one lower, one upper, one two-sided, three mixed and fifteen, wherever
Mt holds them; all six modes, both signs of w, best_f a scalar and per row.  The
rows of a case are the first R of one reference of 1025 rows per (Mt,
constraints, mode, w, best_f) -- rows are independent -- computed once.

Against the truth.  Values: |got - truth| / max(1, |truth|) <= 64 x the
reference's worst recorded value error over the grid (a few ulp of difference
between the device's and the host's erfcx / erfc / log / exp).  Gradients:
relative error <= max(64 x the reference's worst recorded gradient error on
u in (-1, 10], 2 x the reference's own recorded error at that point).  The
two-sided pairs run through one constraint on a member with mean 0 and variance
1 beside an objective term that is exactly 0 (log Phi(40)); its dmean =
-(d/da + d/db) and dvar = -(a d/da + b d/db) / 2 are measured relative to
|d/da| + |d/db| and (|a d/da| + |b d/db|) / 2 of the truth -- the size of the
terms, since the sums themselves may vanish (a = -b) -- and the reference's own
error is taken in the same measure from its recorded d/da and d/db."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import analytic_restatement as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
RS = [1, 255, 256, 257, 1025]
RMAX = 1025
CONSETS = ["none", "lower", "upper", "both", "mixed3", "all15"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_analytic.npz")


def _bound(got, ref, what):
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs().max().item()
    lim = 1e-9 * ref.abs().max().item() + 1e-10
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"
    return err


def _window(t):
    """t on the device as a window of a NaN buffer (64 doubles before and after)."""
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=F64, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1).to(DEV)
    return buf[64:64 + t.numel()].view(t.shape)


def _layout(Mt, conset):
    """(obj, constraints) of a case, or None where Mt does not hold the set."""
    obj = Mt // 2
    others = [j for j in range(Mt) if j != obj][::-1]  # (not in member order)
    kinds = {"none": [], "lower": [ar.LOWER], "upper": [ar.UPPER], "both": [ar.BOTH],
             "mixed3": [ar.BOTH, ar.LOWER, ar.UPPER],
             "all15": [(ar.LOWER, ar.UPPER, ar.BOTH)[c % 3] for c in range(15)]}[conset]
    if len(kinds) > len(others):
        return None
    cons = [(others[c], -2.0 + 0.1 * c, 2.0 - 0.07 * c, kind) for c, kind in enumerate(kinds)]
    return obj, cons


LAYOUTS = [(Mt, cs) for Mt in (1, 2, 4, 16) for cs in CONSETS if _layout(Mt, cs) is not None]


@functools.lru_cache(maxsize=None)
def _inputs(Mt):
    g = torch.Generator().manual_seed(100 + Mt)
    mean = torch.randn(Mt, RMAX, generator=g, dtype=F64)
    var = 0.05 + torch.rand(Mt, RMAX, generator=g, dtype=F64)
    bf_row = 0.5 * torch.randn(RMAX, generator=g, dtype=F64)
    dacq = torch.randn(RMAX, generator=g, dtype=F64)
    return mean, var, bf_row, dacq


@functools.lru_cache(maxsize=None)
def _reference(Mt, conset, mode, w, per_row):
    """(acq, dmean, dvar) of the 1025 rows on the CPU, once per case."""
    obj, cons = _layout(Mt, conset)
    mean, var, bf_row, dacq = _inputs(Mt)
    best_f = bf_row if per_row else torch.tensor(0.3, dtype=F64)
    return ar.analytic_with_grad(mean, var, best_f, mode, dacq, obj=obj, w=w, beta=0.7,
                                 constraints=cons)


def _run(mean, var, best_f, mode, dacq, **kw):
    """Forward and backward through windows, each twice and compared bitwise."""
    from botorch_amd import kernels
    args = (_window(mean), _window(var), None if best_f is None else _window(best_f), mode)
    acq = kernels.analytic(*args, **kw)
    assert torch.equal(acq, kernels.analytic(*args, **kw))
    dw = _window(dacq)
    dmean, dvar = kernels.analytic_backward(dw, *args, **kw)
    dmean2, dvar2 = kernels.analytic_backward(dw, *args, **kw)
    assert torch.equal(dmean, dmean2) and torch.equal(dvar, dvar2)
    return acq.cpu(), dmean.cpu(), dvar.cpu()


@pytest.mark.parametrize("Mt,conset", LAYOUTS)
def test_random_rows(Mt, conset):
    obj, cons = _layout(Mt, conset)
    mean, var, bf_row, dacq = _inputs(Mt)
    read = {obj} | {c[0] for c in cons}
    unread = [j for j in range(Mt) if j not in read]
    worst = 0.0
    for mode in range(6):
        for w in (1.0, -1.0):
            for per_row in (False, True):
                if mode >= ar.UCB and per_row:
                    continue  # (no best_f in these modes)
                acq_r, dmean_r, dvar_r = _reference(Mt, conset, mode, w, per_row)
                for R in RS:
                    best_f = None if mode >= ar.UCB else (
                        bf_row[:R] if per_row else torch.tensor([0.3], dtype=F64))
                    acq, dmean, dvar = _run(mean[:, :R].contiguous(), var[:, :R].contiguous(),
                                            best_f, mode, dacq[:R], obj=obj, w=w, beta=0.7,
                                            constraints=cons)
                    what = f"Mt={Mt} {conset} mode={mode} w={w} per_row={per_row} R={R}"
                    assert acq.shape == (R,) and dmean.shape == dvar.shape == (Mt, R)
                    worst = max(worst, _bound(acq, acq_r[:R], what + " acq"),
                                _bound(dmean, dmean_r[:, :R], what + " dmean"),
                                _bound(dvar, dvar_r[:, :R], what + " dvar"))
                    for j in unread:  # members that no term reads: exactly zero
                        assert not dmean[j].any() and not dvar[j].any(), what
                    if mode != ar.STD:
                        assert dmean[obj].abs().max() > 0, what
                    assert dvar[obj].abs().max() > 0, what
    print(f"Mt={Mt} {conset}: worst error {worst:.3e}")


def _golden():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


def _grid(mode, x):
    """(acq, d acq / d mean) of the points x with mean = x, var = 1, best_f = 0."""
    zero = torch.zeros(1, dtype=F64)
    acq, dmean, _ = _run(x[None].contiguous(), torch.ones(1, x.numel(), dtype=F64), zero, mode,
                         torch.ones(x.numel(), dtype=F64))
    return acq, dmean[0]


def test_log_ei_grid_against_truth():
    G = _golden()
    u, tv, tg = G["lei_u"], G["lei_true"], G["lei_true_grad"]
    acq, grad = _grid(ar.LOG_EI, u)
    assert torch.isfinite(acq).all() and torch.isfinite(grad).all()
    verr = ((acq - tv).abs() / tv.abs().clamp_min(1.0)).max().item()
    vlim = 64 * G["lei_ref_err"].max().item()
    print(f"log_ei value error against the truth: {verr:.3e} (limit {vlim:.3e})")
    assert verr <= vlim
    gerr = (grad - tg).abs() / tg.abs()
    up = (u > -1) & (u <= 10)
    floor = 64 * G["lei_ref_grad_err"][up].max().item()
    glim = torch.maximum(torch.full_like(gerr, floor), 2 * G["lei_ref_grad_err"])
    for lo in range(0, 7):
        sel = (-u >= 10.0 ** lo) & (-u < 10.0 ** (lo + 1))
        print(f"|u| in [1e{lo}, 1e{lo + 1}): gradient error {gerr[sel].max().item():.3e} "
              f"(the reference: {G['lei_ref_grad_err'][sel].max().item():.3e})")
    print(f"u in (-1, 10]: gradient error {gerr[up].max().item():.3e}; "
          f"|u| >= 1e7: {gerr[u <= -1e7].max().item():.3e}; floor {floor:.3e}")
    bad = (gerr > glim).nonzero().reshape(-1).tolist()
    assert not bad, [(u[i].item(), gerr[i].item(), glim[i].item()) for i in bad]
    assert (grad > 0).all()


def test_log_ndtr_grid_against_truth():
    G = _golden()
    x, tv, tg = G["lnd_x"], G["lnd_true"], G["lnd_true_grad"]
    acq, grad = _grid(ar.LOG_PI, x)
    assert torch.isfinite(acq).all() and torch.isfinite(grad).all()
    verr = ((acq - tv).abs() / tv.abs().clamp_min(1.0)).max().item()
    vlim = 64 * G["lei_ref_err"].max().item()
    gerr = (grad - tg).abs() / tg.abs()
    up = (G["lei_u"] > -1) & (G["lei_u"] <= 10)
    floor = 64 * G["lei_ref_grad_err"][up].max().item()
    glim = torch.maximum(torch.full_like(gerr, floor), 2 * G["lnd_ref_grad_err"])
    print(f"log_ndtr: value error {verr:.3e} (limit {vlim:.3e}), gradient error "
          f"{gerr.max().item():.3e} (floor {floor:.3e})")
    assert verr <= vlim
    assert (gerr <= glim).all(), (gerr, glim)


def test_two_sided_pairs_against_truth():
    G = _golden()
    up = (G["lei_u"] > -1) & (G["lei_u"] <= 10)
    floor = 64 * G["lei_ref_grad_err"][up].max().item()
    vlim = 64 * G["lei_ref_err"].max().item()
    mean = torch.tensor([[40.0], [0.0]], dtype=F64)  # log Phi(40) = 0 exactly
    one = torch.ones(2, 1, dtype=F64)
    for i, (a, b) in enumerate(G["lpn_ab"].tolist()):
        acq, dmean, dvar = _run(mean, one, torch.zeros(1, dtype=F64), ar.LOG_PI,
                                torch.ones(1, dtype=F64), constraints=[(1, a, b, ar.BOTH)])
        tv, ta, tb = (G[k][i].item() for k in ("lpn_true", "lpn_true_da", "lpn_true_db"))
        ra, rb = G["lpn_ref_da"][i].item(), G["lpn_ref_db"][i].item()
        smu, svar = abs(ta) + abs(tb), 0.5 * (abs(a * ta) + abs(b * tb))
        verr = abs(acq.item() - tv) / max(1.0, abs(tv))
        emu = abs(dmean[1].item() + (ta + tb)) / smu
        evar = abs(dvar[1].item() + 0.5 * (a * ta + b * tb)) / svar
        ref_mu = abs((ra + rb) - (ta + tb)) / smu
        ref_var = 0.5 * abs((a * ra + b * rb) - (a * ta + b * tb)) / svar
        print(f"pair ({a}, {b}): value {verr:.2e}, dmean {emu:.2e} (reference {ref_mu:.2e}), "
              f"dvar {evar:.2e} (reference {ref_var:.2e})")
        assert np.isfinite([acq.item(), dmean[1].item(), dvar[1].item()]).all()
        assert verr <= vlim, (a, b)
        assert emu <= max(floor, 2 * ref_mu), (a, b)
        assert evar <= max(floor, 2 * ref_var), (a, b)
        assert dmean[0].item() == 0.0 or abs(dmean[0].item()) < 1e-300  # phi(40) / Phi(40)


def test_variance_floor():
    """var in {0, 1e-13, 1e-12, 2e-12} against min_var = 1e-12, on the objective
    and on a constrained member: values against the restatement; dvar is exactly 0
    at and below the floor and not above it."""
    var = torch.tensor([0.0, 1e-13, 1e-12, 2e-12], dtype=F64)
    mean = torch.tensor([[1e-6, -2e-6, 3e-6, 5e-7], [2e-6, 1e-6, -1e-6, 3e-6]], dtype=F64)
    var2 = torch.stack([var, var.flip(0)])
    cons = [(1, -3e-6, 4e-6, ar.BOTH)]
    for mode in range(6):
        best_f = None if mode >= ar.UCB else torch.zeros(1, dtype=F64)
        acq, dmean, dvar = _run(mean, var2, best_f, mode, torch.ones(4, dtype=F64), beta=2.0,
                                constraints=cons)
        ref = ar.analytic(mean, var2, best_f, mode, beta=2.0, constraints=cons)
        _bound(acq, ref, f"floor mode={mode}")
        assert torch.isfinite(dmean).all() and torch.isfinite(dvar).all()
        assert dvar[0, :3].tolist() == [0.0, 0.0, 0.0] and dvar[0, 3] != 0
        assert dvar[1, 1:].tolist() == [0.0, 0.0, 0.0] and dvar[1, 0] != 0


def test_bad_arguments_raise_before_any_launch():
    from botorch_amd import kernels
    z = lambda *s: torch.zeros(*s, dtype=F64, device=DEV)  # noqa: E731
    bf = z(1)
    ok = dict(constraints=[(1, 0.0, 1.0, ar.BOTH)])
    with pytest.raises(ValueError, match="Mt"):
        kernels.analytic(z(17, 3), z(17, 3), bf, ar.LOG_EI)
    with pytest.raises(ValueError, match="at most 15"):
        kernels.analytic(z(16, 3), z(16, 3), bf, ar.LOG_EI,
                         constraints=[(1, 0.0, 0.0, ar.LOWER)] * 16)
    with pytest.raises(ValueError, match="objective"):
        kernels.analytic(z(2, 3), z(2, 3), bf, ar.LOG_EI, obj=1, **ok)
    with pytest.raises(ValueError, match="upper > lower"):
        kernels.analytic(z(2, 3), z(2, 3), bf, ar.LOG_EI, constraints=[(1, 1.0, 1.0, ar.BOTH)])
    with pytest.raises(ValueError, match="min_var"):
        kernels.analytic(z(2, 3), z(2, 3), bf, ar.LOG_EI, min_var=0.0, **ok)
    with pytest.raises(ValueError, match="mode"):
        kernels.analytic(z(2, 3), z(2, 3), bf, 6, **ok)
    with pytest.raises(ValueError, match="mode"):
        kernels.analytic_backward(z(3), z(2, 3), z(2, 3), bf, 6, **ok)
    out = kernels.analytic(z(2, 0), z(2, 0), bf, ar.LOG_EI, **ok)
    assert out.shape == (0,) and out.dtype == F64
    dmean, dvar = kernels.analytic_backward(z(0), z(2, 0), z(2, 0), bf, ar.LOG_EI, **ok)
    assert dmean.shape == dvar.shape == (2, 0)


def test_op_matches_the_wrappers_and_differentiates():
    """torch.ops.bo.analytic is the same launch and its registered backward the
    same gradient as kernels.analytic_backward."""
    from botorch_amd import kernels, ops  # noqa: F401
    obj, cons = _layout(4, "mixed3")
    mean, var, bf_row, dacq = _inputs(4)
    R = 300
    m = mean[:, :R].to(DEV).requires_grad_(True)
    v = var[:, :R].to(DEV).requires_grad_(True)
    bf, d = bf_row[:R].to(DEV), dacq[:R].to(DEV)
    lists = ([c[0] for c in cons], [c[1] for c in cons], [c[2] for c in cons],
             [c[3] for c in cons])
    for mode in (ar.LOG_EI, ar.EI):
        acq = torch.ops.bo.analytic(m, v, bf, mode, obj, -1.0, 0.0, 1e-12, *lists)
        want = kernels.analytic(m.detach(), v.detach(), bf, mode, obj=obj, w=-1.0,
                                constraints=cons)
        assert torch.equal(acq, want)
        gm, gv = torch.autograd.grad(acq, (m, v), d)
        wm, wv = kernels.analytic_backward(d, m.detach(), v.detach(), bf, mode, obj=obj, w=-1.0,
                                           constraints=cons)
        assert torch.equal(gm, wm) and torch.equal(gv, wv)
