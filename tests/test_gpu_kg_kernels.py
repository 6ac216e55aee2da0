"""kernels.kg / kernels.kg_backward (bo_kg_v, bo_kg_backward_v) alone, against
CPU autograd through the torch restatement of the packed definition
(tests/kg_restatement.kg_values_packed).

Every entry of ``mean`` and ``cov`` that the definition does not read -- the
mean at the actual rows, the fantasy x fantasy block, the X x X blocks of the
tiles t > 0, the upper cross block, the spare slots -- is NaN: the outputs must
be finite and the cotangents there exactly zero.  ``dacq`` is random with
mixed signs.  Bound (the project's kernel-against-torch bound):
max|got - ref| <= 1e-9 max|ref| + 1e-10.

Cases (q_a, N_f, B): the smallest shape; one full tile; a ragged second tile;
each q_a bucket of the kernel (<= 4, <= 8, <= 15); one slot per tile; more
fantasies than a wavefront, than a workgroup's threads (the forward's loop)
and than a backward chunk; a ``slots`` smaller than the plan's."""
import math

import pytest
import torch

from tests.kg_restatement import kg_values_packed, read_entries, tile_plan

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
NOISE = 1e-2
#        q_a, N_f, B, slots (None: the plan's), dvalues
CASES = [(1, 1, 1, None, False), (1, 15, 2, None, False), (1, 16, 2, None, True),
         (2, 5, 3, None, False), (4, 12, 1, None, False), (4, 13, 2, None, True),
         (8, 64, 2, None, False), (15, 3, 2, None, False), (3, 70, 1, None, False),
         (2, 300, 1, None, True), (2, 5, 3, 2, False)]


def _bound(got, ref, what):
    err = (got - ref).abs().max().item()
    lim = 1e-9 * ref.abs().max().item() + 1e-10
    print(f"{what}: max err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def _inputs(q_a, N_f, B, slots, seed, xx=None):
    """Packed moments with NaN wherever the definition does not read."""
    g = torch.Generator().manual_seed(seed)
    T = math.ceil(N_f / slots)
    qp = q_a + slots
    mean = torch.full((B * T, qp), float("nan"), dtype=F64)
    cov = torch.full((B * T, qp, qp), float("nan"), dtype=F64)
    read_m = torch.zeros_like(mean, dtype=torch.bool)
    read_c = torch.zeros_like(cov, dtype=torch.bool)
    if xx is None:
        G = torch.randn(B, q_a, q_a, generator=g, dtype=F64)
        xx = G @ G.mT / q_a + 0.1 * torch.eye(q_a, dtype=F64)
    cov[::T, :q_a, :q_a] = xx
    read_c[::T, :q_a, :q_a] = True
    tile, row = read_entries(B, q_a, N_f, slots)
    mean[tile, row] = 1.0 + torch.randn(B, N_f, generator=g, dtype=F64)
    cov[tile, row, :q_a] = torch.randn(B, N_f, q_a, generator=g, dtype=F64)
    read_m[tile, row] = True
    read_c[tile, row, :q_a] = True
    Z = torch.randn(N_f, q_a, generator=g, dtype=F64)
    dacq = torch.randn(B, generator=g, dtype=F64)
    dvalues = torch.randn(B, N_f, generator=g, dtype=F64)
    if B > 1:
        dacq[0], dacq[1] = -abs(dacq[0]), abs(dacq[1])  # mixed signs
    return mean, cov, Z, dacq, dvalues, read_m, read_c


def _check(q_a, N_f, B, slots, with_dv, noise, xx=None, seed=0):
    from botorch_amd import kernels
    mean, cov, Z, dacq, dvalues, read_m, read_c = _inputs(q_a, N_f, B, slots, seed, xx)
    m_ref = mean.clone().requires_grad_(True)
    c_ref = cov.clone().requires_grad_(True)
    values, jitter = kg_values_packed(m_ref, c_ref, Z, noise, q_a, slots)
    acq = values.mean(dim=-1)
    loss = (dacq * acq).sum() + ((dvalues * values).sum() if with_dv else 0.0)
    dm_ref, dc_ref = torch.autograd.grad(loss, (m_ref, c_ref))
    assert dm_ref[~read_m].eq(0).all() and dc_ref[~read_c].eq(0).all()
    assert dm_ref[read_m].ne(0).all() and dc_ref[read_c].abs().max() > 0

    out = kernels.kg(mean.to(DEV), cov.to(DEV), Z.to(DEV), noise, q_a, slots)
    assert out["acq"].shape == (B,) and out["values"].shape == (B, N_f)
    assert out["L"].shape == (B, q_a, q_a) and out["W"].shape == (B, N_f, q_a)
    for k in ("acq", "values", "L", "W"):
        assert torch.isfinite(out[k]).all(), k
    assert out["info"].cpu().eq(0).all()
    assert torch.equal(out["jitter"].cpu(), jitter.detach())
    _bound(out["values"].cpu(), values.detach(), "values")
    _bound(out["acq"].cpu(), acq.detach(), "acq")
    again = kernels.kg(mean.to(DEV), cov.to(DEV), Z.to(DEV), noise, q_a, slots)
    assert torch.equal(again["acq"], out["acq"])  # fixed summation order

    dmean, dcov = kernels.kg_backward(cov.to(DEV), out["L"], out["W"], dacq.to(DEV), slots,
                                      dvalues.to(DEV) if with_dv else None)
    dmean, dcov = dmean.cpu(), dcov.cpu()
    assert dmean.shape == mean.shape and dcov.shape == cov.shape
    assert torch.isfinite(dmean).all() and torch.isfinite(dcov).all()
    assert dmean[~read_m].eq(0).all() and dcov[~read_c].eq(0).all()  # exactly zero
    _bound(dmean, dm_ref, "dmean")
    _bound(dcov, dc_ref, "dcov")
    return out, jitter


@pytest.mark.parametrize("q_a, N_f, B, slots, with_dv", CASES)
def test_kg_kernels_against_cpu_autograd(q_a, N_f, B, slots, with_dv):
    plan = tile_plan(q_a, N_f)
    if slots is None:
        slots = plan[1]
    else:
        assert slots < plan[1]  # the kernel honours the argument, not the plan
    _check(q_a, N_f, B, slots, with_dv, NOISE, seed=q_a * 1000 + N_f)


def test_kg_kernel_jitter_ladder():
    """Restart 0: Sigma(X, X) = Q diag(1, 0.5, -2e-5) Q^T, noise 0 -- the plain
    factorisation and the jitters 1e-8 ... 1e-5 fail, 1e-4 succeeds (smallest
    eigenvalue then 8e-5, condition number about 1.3e4).  Restart 1 is well
    conditioned and gets no jitter.  The reported jitter is the oracle's
    psd_safe_cholesky's and the same bound holds."""
    from oracle.gp import psd_safe_cholesky
    g = torch.Generator().manual_seed(3)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    bad = Q @ torch.diag(torch.tensor([1.0, 0.5, -2e-5], dtype=F64)) @ Q.T
    bad = 0.5 * (bad + bad.T)
    G = torch.randn(3, 3, generator=g, dtype=F64)
    xx = torch.stack([bad, G @ G.T / 3 + 0.1 * torch.eye(3, dtype=F64)])
    assert torch.linalg.cholesky_ex(bad).info.item() > 0  # the plain factorisation fails
    assert torch.linalg.cholesky_ex(bad + 1e-5 * torch.eye(3, dtype=F64)).info.item() > 0
    _, added = psd_safe_cholesky(xx)
    assert added[0].item() == pytest.approx(1e-4, rel=1e-12) and added[1].item() == 0.0
    q_a, N_f, B = 3, 7, 2
    out, jitter = _check(q_a, N_f, B, tile_plan(q_a, N_f)[1], False, 0.0, xx=xx, seed=9)
    assert torch.equal(jitter, added)
    assert torch.equal(out["jitter"].cpu(), added)


def test_opcheck_kg_ops():
    """torch.library.opcheck of bo::kg and bo::kg_backward (schema, fake
    implementation, autograd registration), and the op's autograd against the
    direct kernel calls."""
    from botorch_amd import kernels, ops  # noqa: F401  (registers torch.ops.bo)
    q_a, N_f, B = 3, 7, 2
    slots = tile_plan(q_a, N_f)[1]
    mean, cov, Z, dacq, _, read_m, read_c = _inputs(q_a, N_f, B, slots, 21)
    mean = torch.where(read_m, mean, torch.zeros_like(mean)).to(DEV).requires_grad_(True)
    cov = torch.where(read_c, cov, torch.zeros_like(cov)).to(DEV).requires_grad_(True)
    Z, dacq = Z.to(DEV), dacq.to(DEV)
    torch.library.opcheck(torch.ops.bo.kg.default, (mean, cov, Z, NOISE, q_a, slots),
                          test_utils=["test_schema", "test_faketensor",
                                      "test_autograd_registration"])
    acq, values, L, W, jit, info = torch.ops.bo.kg(mean, cov, Z, NOISE, q_a, slots)
    torch.library.opcheck(torch.ops.bo.kg_backward.default,
                          (dacq, None, cov.detach(), L, W, slots),
                          test_utils=["test_schema", "test_faketensor"])
    gm, gc = torch.autograd.grad((acq * dacq).sum(), (mean, cov))
    dmean, dcov = kernels.kg_backward(cov.detach(), L, W, dacq, slots)
    assert torch.equal(gm, dmean) and torch.equal(gc, dcov)
    assert not (L.requires_grad or W.requires_grad or jit.requires_grad)


def test_kg_kernel_failed_ladder_reports_info():
    """A matrix the whole ladder cannot repair: info > 0 and NaN outputs for
    that restart only."""
    from botorch_amd import kernels
    q_a, N_f, B = 2, 3, 2
    slots = tile_plan(q_a, N_f)[1]
    xx = torch.stack([torch.diag(torch.tensor([1.0, -1.0], dtype=F64)), torch.eye(2, dtype=F64)])
    mean, cov, Z, *_ = _inputs(q_a, N_f, B, slots, 1, xx)
    out = kernels.kg(mean.to(DEV), cov.to(DEV), Z.to(DEV), 0.0, q_a, slots)
    assert out["info"].cpu().tolist()[0] > 0 and out["info"].cpu().tolist()[1] == 0
    assert torch.isnan(out["acq"][0]) and torch.isfinite(out["acq"][1])
    assert torch.isnan(out["values"][0]).all() and torch.isfinite(out["values"][1]).all()
