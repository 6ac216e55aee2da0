"""The five max-value entropy search entry points alone (bo_mes_v,
bo_mes_backward_v, bo_gibbon_v, bo_gibbon_backward_v, bo_mv_quantiles_v) against
the torch restatement of the definitions (tests/mes_restatement.py) and CPU
autograd through it.

Every input is a window of a larger buffer filled with NaN: a read outside an
array reaches the outputs, and these must be finite.  Every call is repeated
once and compared bitwise (no atomics).  Bound for values and gradients (the
project's kernel-against-torch bound): max|got - ref| <= 1e-9 max|ref| + 1e-10.

Shapes.  MES: R in {1, 15, 63, 64, 65, 257} (one wave per row: one block up to
past 256 blocks), (S_M, S_m) in {(1, 2), (3, 7), (10, 128), (33, 130)} (fewer
pairs than lanes, pairs that wrap a lane over several j, the defaults, and S_m
past two lane strides with S_M past the 16- and 32-lane marks), both signs of w,
tau2 in {1e-6, 0.3}.  GIBBON: the same R (16 rows per block), S_M in {1, 10,
33} (below, within and past one 16-lane stride), m in {0, 1, 4, 15}.  The
rows of a case are the first R of one reference per (S_M, S_m, w, tau2) --
rows are independent -- computed once and shared.

The gradient cases drop the generated rows on which a quantity of the
restatement lies within 1 % of a clamp boundary, and assert that at most a
tenth are dropped (tests/test_mes_cpu.py checks this for every reference, on
the CPU alone).  The clamp cases are values only, except
GIBBON's clamped repulsion row, whose gradient (through qf) is checked too."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import mes_restatement as mr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
RS = [1, 15, 63, 64, 65, 257]
PAIRS = [(1, 2), (3, 7), (10, 128), (33, 130)]
RMAX, RGEN = 257, 280  # rows kept / generated per reference (a tenth may be dropped)


def _bound(got, ref, what):
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs().max().item()
    lim = 1e-9 * ref.abs().max().item() + 1e-10
    print(f"{what}: max err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def _window(t):
    """t on the device as a window of a NaN buffer (64 doubles before and after)."""
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=F64, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1).to(DEV)
    return buf[64:64 + t.numel()].view(t.shape)


def _rows(g, w, S_M):
    mu = torch.randn(RGEN, generator=g, dtype=F64)
    var = 0.05 + torch.rand(RGEN, generator=g, dtype=F64)
    fstar = (w * mu).max() + 0.2 + 1.5 * torch.rand(S_M, generator=g, dtype=F64)
    dout = torch.randn(RGEN, generator=g, dtype=F64)
    return mu, var, fstar, dout


def _keep(clamped):
    """The first RMAX generated rows off every clamp boundary; at most a tenth dropped."""
    near = mr.near_clamp(clamped)
    dropped = int(near.sum())
    assert dropped <= RGEN // 10, f"{dropped} of {RGEN} rows within 1 % of a clamp"
    idx = (~near).nonzero().reshape(-1)[:RMAX]
    assert idx.numel() == RMAX
    return idx, dropped


@functools.lru_cache(maxsize=None)
def mes_reference(S_M, S_m, w, tau2):
    """(mu, var, fstar, z, dout, ig, dmu, dvar) on the CPU, RMAX rows."""
    g = torch.Generator().manual_seed(1000 * S_M + S_m + (7 if w < 0 else 0))
    mu, var, fstar, dout = _rows(g, w, S_M)
    z = torch.randn(S_m, generator=g, dtype=F64)
    idx, _ = _keep(mr.mes(mu, var, fstar, z, tau2, w).clamped)
    mu, var, dout = mu[idx], var[idx], dout[idx]
    mur, varr = mu.clone().requires_grad_(True), var.clone().requires_grad_(True)
    ig = mr.mes(mur, varr, fstar, z, tau2, w).ig
    dmu, dvar = torch.autograd.grad((ig * dout).sum(), (mur, varr))
    assert dmu.abs().max() > 0 and dvar.abs().max() > 0
    return mu, var, fstar, z, dout, ig.detach(), dmu, dvar


@functools.lru_cache(maxsize=None)
def gibbon_reference(S_M, m, w, tau2=0.3):
    """(mu, var, fstar, A, Binv, dout, acq, dmu, dvar, dA) on the CPU, RMAX rows."""
    g = torch.Generator().manual_seed(500 * S_M + m + (7 if w < 0 else 0))
    mu, var, fstar, dout = _rows(g, w, S_M)
    A = Binv = None
    if m:
        G = torch.randn(m, m, generator=g, dtype=F64)
        Binv = torch.linalg.inv(G @ G.T + torch.eye(m, dtype=F64))
        A = torch.randn(RGEN, m, generator=g, dtype=F64)
        # qf between 5 % and 60 % of vm
        want = (0.05 + 0.55 * torch.rand(RGEN, generator=g, dtype=F64)) * (var + tau2)
        A = A * (want / ((A @ Binv) * A).sum(-1)).sqrt()[:, None]
    idx, _ = _keep(mr.gibbon(mu, var, fstar, tau2, w, A, Binv).clamped)
    mu, var, dout = mu[idx], var[idx], dout[idx]
    A = A[idx] if m else None
    leaves = [t.clone().requires_grad_(True) for t in ((mu, var, A) if m else (mu, var))]
    acq = mr.gibbon(leaves[0], leaves[1], fstar, tau2, w, leaves[2] if m else None, Binv).acq
    grads = torch.autograd.grad((acq * dout).sum(), leaves)
    return mu, var, fstar, A, Binv, dout, acq.detach(), grads[0], grads[1], grads[2] if m else None


def reference_rows_meet_the_cap():
    """The seeds: every reference drops at most a tenth of its generated rows
    (asserted inside), on the restatement alone; tests/test_mes_cpu.py runs it."""
    for S_M, S_m in PAIRS:
        for w in (1.0, -1.0):
            for tau2 in (1e-6, 0.3):
                mes_reference(S_M, S_m, w, tau2)
    for S_M in (1, 10, 33):
        for m in (0, 1, 4, 15):
            for w in (1.0, -1.0):
                gibbon_reference(S_M, m, w)


@pytest.mark.parametrize("tau2", [1e-6, 0.3])
@pytest.mark.parametrize("w", [1.0, -1.0])
@pytest.mark.parametrize("S_M, S_m", PAIRS)
@pytest.mark.parametrize("R", RS)
def test_mes_forward_and_backward(R, S_M, S_m, w, tau2):
    from botorch_amd import kernels, ops  # noqa: F401
    mu, var, fstar, z, dout, ig, dmu, dvar = (t[:R] if i in (0, 1, 4, 5, 6, 7) else t for i, t in
                                              enumerate(mes_reference(S_M, S_m, w, tau2)))
    consts = mr.host_constants(z)
    a_mu, a_var = _window(mu).requires_grad_(True), _window(var).requires_grad_(True)
    a_f, a_z, a_d = _window(fstar), _window(z), _window(dout)
    out = torch.ops.bo.mes(a_mu, a_var, a_f, a_z, *consts, tau2, w)
    assert tuple(out.shape) == (R,)
    g_mu, g_var = torch.autograd.grad((out * a_d).sum(), (a_mu, a_var))
    tag = f"R={R} S_M={S_M} S_m={S_m} w={w} tau2={tau2}"
    _bound(out.detach().cpu(), ig, f"ig   {tag}")
    _bound(g_mu.cpu(), dmu, f"dmu  {tag}")
    _bound(g_var.cpu(), dvar, f"dvar {tag}")
    for _ in range(2):  # repeated calls are bit-identical
        assert torch.equal(kernels.mes(a_mu.detach(), a_var.detach(), a_f, a_z, consts, tau2, w),
                           out.detach())
        b_mu, b_var = kernels.mes_backward(a_d, a_mu.detach(), a_var.detach(), a_f, a_z, consts,
                                           tau2, w)
        assert torch.equal(b_mu, g_mu) and torch.equal(b_var, g_var)


@pytest.mark.parametrize("m", [0, 1, 4, 15])
@pytest.mark.parametrize("S_M", [1, 10, 33])
@pytest.mark.parametrize("R", RS)
def test_gibbon_forward_and_backward(R, S_M, m):
    from botorch_amd import kernels, ops  # noqa: F401
    w, tau2 = (1.0 if (R + S_M + m) % 2 else -1.0), 0.3
    mu, var, fstar, A, Binv, dout, acq, dmu, dvar, dA = gibbon_reference(S_M, m, w)
    mu, var, dout, acq, dmu, dvar = (t[:R] for t in (mu, var, dout, acq, dmu, dvar))
    a_mu, a_var = _window(mu).requires_grad_(True), _window(var).requires_grad_(True)
    a_f, a_d = _window(fstar), _window(dout)
    a_A = _window(A[:R]).requires_grad_(True) if m else None
    a_B = _window(Binv) if m else None
    out = torch.ops.bo.gibbon(a_mu, a_var, a_A, a_B, a_f, tau2, w)
    assert tuple(out.shape) == (R,)
    grads = torch.autograd.grad((out * a_d).sum(), (a_mu, a_var) + ((a_A,) if m else ()))
    tag = f"R={R} S_M={S_M} m={m} w={w}"
    _bound(out.detach().cpu(), acq, f"acq  {tag}")
    _bound(grads[0].cpu(), dmu, f"dmu  {tag}")
    _bound(grads[1].cpu(), dvar, f"dvar {tag}")
    if m:
        assert dA[:R].abs().max() > 0
        _bound(grads[2].cpu(), dA[:R], f"dA   {tag}")
    det = lambda t: None if t is None else t.detach()  # noqa: E731
    for _ in range(2):
        assert torch.equal(kernels.gibbon(det(a_mu), det(a_var), det(a_A), a_B, a_f, tau2, w),
                           out.detach())
        again = kernels.gibbon_backward(a_d, det(a_mu), det(a_var), det(a_A), a_B, a_f, tau2, w)
        assert all(torch.equal(x, y) for x, y in zip(again, grads))
        assert (again[2] is None) == (m == 0)


@pytest.mark.parametrize("w", [1.0, -1.0])
def test_mes_values_on_the_clamps(w):
    """Values only.  Rows 0-3 have sigma^2 = 1e-9 (vM and s2n both clamp); max
    value 0 lies ten sigma below every mean (both Phi floors apply)."""
    from botorch_amd import kernels
    g = torch.Generator().manual_seed(3)
    R, S_M, S_m, tau2 = 20, 3, 7, 0.3
    mu = torch.randn(R, generator=g, dtype=F64)
    var = 0.05 + torch.rand(R, generator=g, dtype=F64)
    var[:4] = 1e-9
    z = torch.randn(S_m, generator=g, dtype=F64)
    fstar = (w * mu).max() + 0.2 + torch.rand(S_M, generator=g, dtype=F64)
    fstar[0] = (w * mu).min() - 10.0 * (var.max() + tau2).sqrt()
    ref = mr.mes(mu, var, fstar, z, tau2, w)
    cl = ref.clamped
    assert (cl["vM"][0][:4] < 1e-8).all() and (cl["s2n"][0][:4] < 1e-8).all()
    assert (cl["Phin"][0][4:, 0] < 1e-8).all() and (cl["Phi0"][0][4:, 0] < 1e-8).all()
    assert (cl["Phin"][0][4:, 1:] > 1e-8).any()
    a = [_window(t) for t in (mu, var, fstar, z)]
    consts = mr.host_constants(z)
    out = kernels.mes(*a, consts, tau2, w)
    _bound(out.cpu(), ref.ig, f"ig on the clamps w={w}")
    assert torch.equal(kernels.mes(*a, consts, tau2, w), out)


def test_gibbon_clamped_repulsion_value_and_gradient():
    """Rows 0 and 5 have qf = 1.5 vm: the repulsion term clamps and its
    gradient runs through qf (dA non-zero, dvar only through -log vm)."""
    from botorch_amd import kernels, ops  # noqa: F401
    g = torch.Generator().manual_seed(9)
    R, S_M, m, tau2, w = 20, 10, 4, 0.3, 1.0
    mu = torch.randn(R, generator=g, dtype=F64)
    var = 0.05 + torch.rand(R, generator=g, dtype=F64)
    fstar = mu.max() + 0.2 + torch.rand(S_M, generator=g, dtype=F64)
    dout = torch.randn(R, generator=g, dtype=F64)
    G = torch.randn(m, m, generator=g, dtype=F64)
    Binv = torch.linalg.inv(G @ G.T + torch.eye(m, dtype=F64))
    A = torch.randn(R, m, generator=g, dtype=F64)
    frac = torch.full((R,), 0.3, dtype=F64)
    frac[0] = frac[5] = 1.5
    A = A * (frac * (var + tau2) / ((A @ Binv) * A).sum(-1)).sqrt()[:, None]
    leaves = [t.clone().requires_grad_(True) for t in (mu, var, A)]
    ref = mr.gibbon(leaves[0], leaves[1], fstar, tau2, w, leaves[2], Binv)
    vm, lim = ref.clamped["vdet"]
    clamped = (vm < lim).detach()
    assert clamped.tolist() == [i in (0, 5) for i in range(R)]
    dmu, dvar, dA = torch.autograd.grad((ref.acq * dout).sum(), leaves)
    assert dA[0].abs().max() > 0
    a_mu, a_var, a_A = (_window(t).requires_grad_(True) for t in (mu, var, A))
    a_B, a_f, a_d = _window(Binv), _window(fstar), _window(dout)
    out = torch.ops.bo.gibbon(a_mu, a_var, a_A, a_B, a_f, tau2, w)
    grads = torch.autograd.grad((out * a_d).sum(), (a_mu, a_var, a_A))
    _bound(out.detach().cpu(), ref.acq.detach(), "acq, clamped repulsion")
    _bound(grads[0].cpu(), dmu, "dmu, clamped repulsion")
    _bound(grads[1].cpu(), dvar, "dvar, clamped repulsion")
    _bound(grads[2].cpu(), dA, "dA, clamped repulsion")
    _bound(grads[2][clamped].cpu(), dA[clamped], "dA of the clamped rows")
    assert torch.equal(kernels.gibbon(a_mu.detach(), a_var.detach(), a_A.detach(), a_B, a_f, tau2,
                                      w), out.detach())


def _brentq_quantiles(mu, sigma):
    from scipy.optimize import brentq
    from scipy.stats import norm
    lo, hi = (mu - 3 * sigma).min().item(), (mu + 5 * sigma).max().item()
    dist = norm(mu.numpy(), sigma.numpy())
    return [brentq(lambda t: np.exp(np.sum(dist.logcdf(t))) - p, lo, hi) for p in mr.QUANTILE_P]


def _check_quantiles(mu, sigma, tag):
    from botorch_amd import kernels
    a_mu, a_s = _window(mu), _window(sigma)
    y = kernels.mv_quantiles(a_mu, a_s)
    assert tuple(y.shape) == (3,) and torch.isfinite(y).all()
    for p, got, want in zip(mr.QUANTILE_P, y.tolist(), _brentq_quantiles(mu, sigma)):
        print(f"{tag} p={p}: {got!r} against brentq {want!r}, diff {abs(got - want):.2e}")
        assert abs(got - want) <= 1e-11 + 1e-14 * abs(want)
    assert y[0] < y[1] < y[2]
    assert torch.equal(kernels.mv_quantiles(a_mu, a_s), y)
    return y


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1500])
def test_mv_quantiles_against_brentq(N):
    """Agreement with brentq on the reference's own objective to 1e-11 + 1e-14 |y|
    (brentq's default xtol 2e-12 and rtol 4 eps, with a factor of five)."""
    g = torch.Generator().manual_seed(N)
    mu = 2.0 * torch.randn(N, generator=g, dtype=F64)
    sigma = 10.0 ** (-4.0 + 5.0 * torch.rand(N, generator=g, dtype=F64))
    if N >= 2:
        sigma[0], sigma[1] = 1e-4, 10.0
    _check_quantiles(mu, sigma, f"N={N}")


def test_mv_quantiles_with_an_infinite_partial_sum():
    """Candidate 1 lies 60 of its sigma above the bracket's low end: log Phi
    underflows to -inf there, which counts as below p."""
    mu = torch.tensor([0.0, -2.4, 0.5, -1.0], dtype=F64)
    sigma = torch.tensor([1.0, 0.01, 0.3, 0.2], dtype=F64)
    lo = (mu - 3 * sigma).min().item()
    assert lo == -3.0 and abs((lo - mu[1].item()) / sigma[1].item() + 60.0) < 1e-9
    assert mr.quantile_objective(lo, mu, sigma) == -math.inf
    _check_quantiles(mu, sigma, "-inf partial sum")


def test_mv_quantiles_status_through_the_host_check():
    """Hand-set end points above every root: the status words are non-zero and
    the host raises brentq's ValueError."""
    from botorch_amd import kernels, ops  # noqa: F401
    mu = torch.tensor([0.0, 1.0, -1.0], dtype=F64, device=DEV)
    sigma = torch.tensor([1.0, 0.5, 2.0], dtype=F64, device=DEV)
    with pytest.raises(ValueError, match=r"f\(a\) and f\(b\) must have different signs"):
        kernels.mv_quantiles(mu, sigma, bounds=(20.0, 30.0))
    y, status = torch.ops.bo.mv_quantiles(mu, sigma, True, 20.0, 30.0)
    assert status.tolist() == [1, 1, 1] and y.tolist() == [25.0, 25.0, 25.0]
    y, status = torch.ops.bo.mv_quantiles(mu, sigma, True, -20.0, 30.0)
    assert status.tolist() == [0, 0, 0]
    torch.testing.assert_close(y, kernels.mv_quantiles(mu, sigma), rtol=0, atol=1e-12)


def test_wrappers_refuse_bad_arguments():
    from botorch_amd import kernels
    z = lambda *s: torch.zeros(*s, dtype=F64, device=DEV)  # noqa: E731
    consts = (0.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="2 <= S_m"):
        kernels.mes(z(4), z(4), z(3), z(1), consts, 0.1)
    with pytest.raises(ValueError, match="1 <= S_M"):
        kernels.mes(z(4), z(4), z(0), z(5), consts, 0.1)
    with pytest.raises(ValueError, match="R entries"):
        kernels.mes(z(4), z(3), z(2), z(5), consts, 0.1)
    with pytest.raises(ValueError, match="dout must be"):
        kernels.mes_backward(z(3), z(4), z(4), z(2), z(5), consts, 0.1)
    with pytest.raises(ValueError, match="m <= 15"):
        kernels.gibbon(z(4), z(4), z(4, 16), z(16, 16), z(3), 0.1)
    with pytest.raises(ValueError, match="A must be"):
        kernels.gibbon(z(4), z(4), z(3, 2), z(2, 2), z(3), 0.1)
    with pytest.raises(ValueError, match=r"\+1 or -1"):
        kernels.gibbon(z(4), z(4), None, None, z(3), 0.1, w=0.0)
