"""kernels.fantasy_posterior / fantasy_posterior_backward (bo_fantasy_posterior,
bo_fantasy_posterior_backward) alone, against CPU autograd through the torch
restatement of the packed definition (tests/fantasy_restatement.
fantasy_moments_packed).

Every entry of ``mean`` and ``cov`` that the definition does not read -- the
mean at the fantasised rows, the X x X blocks of the tiles t > 0, the upper
cross block, the blocks between different groups, the spare groups -- is NaN:
the outputs must be finite and the cotangents there exactly zero.  The
cotangents of the outputs are random.  Bound (the project's
kernel-against-torch bound): max|got - ref| <= 1e-9 max|ref| + 1e-10.

Cases (q_a, q, N_f, shared, B): the smallest shape; a ragged plan; the bucket
edge q_a = 8 with two groups per tile; bucket 16 with one group per tile and
more fantasies than a wavefront; more fantasies than a workgroup's threads
(several chunks); one group shared by all fantasies; q_a + q = 16 exactly."""
import math

import pytest
import torch

from tests.fantasy_restatement import fantasy_moments_packed, read_masks, tile_plan

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
#        q_a, q, N_f, shared, B
CASES = [(1, 1, 5, False, 2), (3, 2, 5, False, 2), (8, 4, 3, False, 2), (15, 1, 70, False, 1),
         (4, 1, 260, False, 1), (2, 3, 7, True, 2), (5, 11, 2, False, 1)]


def _bound(got, ref, what):
    err = (got - ref).abs().max().item()
    lim = 1e-9 * ref.abs().max().item() + 1e-10
    print(f"{what}: max err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def _inputs(q_a, q, N_f, shared, B, seed, xx=None, noise=None):
    """Packed moments with NaN wherever the definition does not read."""
    g = torch.Generator().manual_seed(seed)
    F = 1 if shared else N_f
    T, slots = tile_plan(q_a, q, F)
    qp = q_a + slots * q
    read_m, read_c = read_masks(B, q_a, q, F, slots)
    if xx is None:
        G = torch.randn(B, q_a, q_a, generator=g, dtype=F64)
        xx = G @ G.mT / q_a + 0.1 * torch.eye(q_a, dtype=F64)
    mean = torch.where(read_m, 1.0 + torch.randn(B * T, qp, generator=g, dtype=F64), float("nan"))
    body = torch.randn(B * T, qp, qp, generator=g, dtype=F64)
    body = body + 2.0 * torch.eye(qp, dtype=F64)  # the diagonal blocks need not be symmetric
    cov = torch.where(read_c, body, float("nan"))
    cov[::T, :q_a, :q_a] = xx
    Z = torch.randn(N_f, q_a, generator=g, dtype=F64)
    if noise is None:
        noise = 1e-2 * (1.0 + torch.rand(q_a, generator=g, dtype=F64))
    dmo = torch.randn(B, N_f, q, generator=g, dtype=F64)
    dco = torch.randn(B, F, q, q, generator=g, dtype=F64)
    return mean, cov, Z, noise, dmo, dco, read_m, read_c, slots


def _check(q_a, q, N_f, shared, B, seed, xx=None, noise=None, **kw):
    from botorch_amd import kernels
    mean, cov, Z, noise, dmo, dco, read_m, read_c, slots = _inputs(q_a, q, N_f, shared, B, seed,
                                                                   xx, noise)
    F = 1 if shared else N_f
    assert (math.ceil(F / slots), slots) == kernels.fantasy_tile_plan(q_a, q, F)
    m_ref = mean.clone().requires_grad_(True)
    c_ref = cov.clone().requires_grad_(True)
    z_ref = Z.clone().requires_grad_(True)
    mo, co, L, jitter = fantasy_moments_packed(m_ref, c_ref, z_ref, noise, q_a, q, slots, shared)
    loss = (dmo * mo).sum() + (dco * co).sum()
    dm_ref, dc_ref, dz_ref = torch.autograd.grad(loss, (m_ref, c_ref, z_ref))
    assert dm_ref[~read_m].eq(0).all() and dc_ref[~read_c].eq(0).all()
    assert dm_ref[read_m].ne(0).all() and dc_ref[read_c].ne(0).all()

    args = (mean.to(DEV), cov.to(DEV), Z.to(DEV), noise.to(DEV), q_a, q, slots, shared)
    out = kernels.fantasy_posterior(*args, **kw)
    assert out["mean_out"].shape == (B, N_f, q) and out["cov_out"].shape == (B, F, q, q)
    assert out["L"].shape == (B, q_a, q_a) and out["V"].shape == (B, F, q, q_a)
    for k in ("mean_out", "cov_out", "L", "V"):
        assert torch.isfinite(out[k]).all(), k
    assert out["info"].cpu().eq(0).all()
    assert torch.equal(out["jitter"].cpu(), jitter.detach())
    _bound(out["mean_out"].cpu(), mo.detach(), "mean_out")
    _bound(out["cov_out"].cpu(), co.detach(), "cov_out")
    _bound(out["L"].cpu(), L.detach(), "L")
    again = kernels.fantasy_posterior(*args, **kw)
    for k in ("mean_out", "cov_out", "L", "V"):
        assert torch.equal(again[k], out[k]), k  # bitwise reproducible

    bargs = (Z.to(DEV), out["L"], out["V"], dmo.to(DEV), dco.to(DEV), slots, shared)
    dmean, dcov, dZ = kernels.fantasy_posterior_backward(*bargs, need_dZ=True)
    dmean2, dcov2, dZ2 = kernels.fantasy_posterior_backward(*bargs, need_dZ=True)
    assert torch.equal(dmean, dmean2) and torch.equal(dcov, dcov2) and torch.equal(dZ, dZ2)
    assert kernels.fantasy_posterior_backward(*bargs)[2] is None
    dmean, dcov, dZ = dmean.cpu(), dcov.cpu(), dZ.cpu()
    assert dmean.shape == mean.shape and dcov.shape == cov.shape and dZ.shape == Z.shape
    assert torch.isfinite(dmean).all() and torch.isfinite(dcov).all()
    assert dmean[~read_m].eq(0).all() and dcov[~read_c].eq(0).all()  # exactly zero
    _bound(dmean, dm_ref, "dmean")
    _bound(dcov, dc_ref, "dcov")
    _bound(dZ, dz_ref, "dZ")
    return out, jitter


@pytest.mark.parametrize("q_a, q, N_f, shared, B", CASES)
def test_fantasy_kernels_against_cpu_autograd(q_a, q, N_f, shared, B):
    _check(q_a, q, N_f, shared, B, seed=q_a * 1000 + q * 100 + N_f)


def test_fantasy_kernel_per_batch_noise():
    """A noise vector per t-batch (noise_stride = q_a) against the restatement."""
    from botorch_amd import kernels
    q_a, q, N_f, B = 3, 2, 8, 2
    mean, cov, Z, _, _, _, _, _, slots = _inputs(q_a, q, N_f, False, B, 5)
    T = math.ceil(N_f / slots)
    assert T == 2
    noise = torch.tensor([[1e-2, 2e-2, 3e-2], [0.5, 0.1, 0.3]], dtype=F64)
    ref = [fantasy_moments_packed(mean[b * T:(b + 1) * T], cov[b * T:(b + 1) * T], Z, noise[b], q_a,
                                  q, slots, False) for b in range(B)]
    out = kernels.fantasy_posterior(mean.to(DEV), cov.to(DEV), Z.to(DEV), noise.to(DEV), q_a, q,
                                    slots, False)
    _bound(out["mean_out"].cpu(), torch.cat([r[0] for r in ref]), "mean_out")
    _bound(out["cov_out"].cpu(), torch.cat([r[1] for r in ref]), "cov_out")


def test_fantasy_kernel_jitter_ladder():
    """T-batch 0: Sigma(X, X) = Q diag(1, 0.5, -2e-5) Q^T, noise 0 -- the plain
    factorisation and the jitters 1e-8 ... 1e-5 fail, 1e-4 succeeds.  T-batch 1
    is well conditioned and gets no jitter.  The reported jitter is the
    oracle's psd_safe_cholesky's and the same bound holds against the
    restatement with the jittered root."""
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
    out, jitter = _check(3, 2, 7, False, 2, seed=9, xx=xx, noise=torch.zeros(3, dtype=F64))
    assert torch.equal(jitter, added)
    assert torch.equal(out["jitter"].cpu(), added)


def test_opcheck_fantasy_ops():
    """torch.library.opcheck of bo::fantasy_posterior and its backward (schema,
    fake implementation, autograd registration), and the op's autograd against
    the direct kernel calls."""
    from botorch_amd import kernels, ops  # noqa: F401  (registers torch.ops.bo)
    q_a, q, N_f, B = 3, 2, 7, 2
    mean, cov, Z, noise, dmo, dco, read_m, read_c, slots = _inputs(q_a, q, N_f, False, B, 21)
    mean = torch.where(read_m, mean, torch.zeros_like(mean)).to(DEV).requires_grad_(True)
    cov = torch.where(read_c, cov, torch.zeros_like(cov)).to(DEV).requires_grad_(True)
    Z, noise, dmo, dco = Z.to(DEV), noise.to(DEV), dmo.to(DEV), dco.to(DEV)
    torch.library.opcheck(torch.ops.bo.fantasy_posterior.default,
                          (mean, cov, Z, noise, q_a, q, slots, False),
                          test_utils=["test_schema", "test_faketensor",
                                      "test_autograd_registration"])
    mo, co, L, V, jit, info = torch.ops.bo.fantasy_posterior(mean, cov, Z, noise, q_a, q, slots,
                                                             False)
    torch.library.opcheck(torch.ops.bo.fantasy_posterior_backward.default,
                          (dmo, dco, Z, L, V, slots, False),
                          test_utils=["test_schema", "test_faketensor"])
    (gm_only,) = torch.autograd.grad(mo.sum(), (mean,), retain_graph=True)  # cov_out unused
    assert torch.isfinite(gm_only).all()
    gm, gc = torch.autograd.grad((mo * dmo).sum() + (co * dco).sum(), (mean, cov))
    dmean, dcov, _ = kernels.fantasy_posterior_backward(Z, L, V, dmo, dco, slots, False)
    assert torch.equal(gm, dmean) and torch.equal(gc, dcov)
    assert not (L.requires_grad or V.requires_grad or jit.requires_grad)


def test_fantasy_kernel_failed_ladder_reports_info():
    """A matrix the whole ladder cannot repair (eigenvalue -1, three tries):
    info > 0 and NaN outputs for that t-batch only, reported by the kernel
    itself."""
    from botorch_amd import kernels
    q_a, q, N_f, B = 2, 2, 3, 2
    xx = torch.stack([torch.diag(torch.tensor([1.0, -1.0], dtype=F64)), torch.eye(2, dtype=F64)])
    mean, cov, Z, _, _, _, _, _, slots = _inputs(q_a, q, N_f, False, B, 1, xx)
    out = kernels.fantasy_posterior(mean.to(DEV), cov.to(DEV), Z.to(DEV),
                                    torch.zeros(q_a, dtype=F64, device=DEV), q_a, q, slots, False,
                                    max_tries=3)
    info = out["info"].cpu().tolist()
    assert info[0] > 0 and info[1] == 0
    for k in ("mean_out", "cov_out", "L", "V"):
        assert torch.isnan(out[k][0]).all() and torch.isfinite(out[k][1]).all(), k
