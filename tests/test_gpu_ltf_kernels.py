"""The four kernels of ltf.hip against tests/ltf_restatement.py (torch fp64 on the host).
Both tolerances are 10 x the largest disagreement of the restatement's two forms over
these same cases, measured once on the CPU.  Values, relative to the entry's bound
o (1 + |c|): pow against exp(p log1p(t)), 2.63e-16, so VAL_TOL = 2.7e-15.  The MLL sums
and dX, relative to sum |summand|: ll_closed against ll_autograd, 2.25e-15, so SUM_TOL =
2.3e-14.  n = 257 is one past a full column tile (256) of the covariance kernel."""
import pytest
import torch

from tests import ltf_restatement as R

pytestmark = pytest.mark.gpu

VAL_TOL = 2.7e-15
SUM_TOL = 2.3e-14
NFS, DXS, NS = (1, 2), (1, 8, 9, 16), (1, 17, 130, 257)
DEV = "cuda"


def _spec(p):
    from botorch_amd import kernels
    return kernels.LTFSpec(tuple(p["xc"]), tuple(p["fc"]), torch.cat([p["l0"], p["l1"]]).to(DEV),
                           float(p["pw"]), float(p["o"]))


@pytest.mark.parametrize("fixed", (False, True))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dx", DXS)
@pytest.mark.parametrize("nf", NFS)
def test_covar_and_mll_terms(nf, dx, n, fixed):
    from botorch_amd import kernels
    Z, y, p, noise, c = R.make_case(nf, dx, n, fixed_noise=fixed)
    spec, Zd = _spec(p), Z.to(DEV)
    nz = (0.0, noise.to(DEV)) if fixed else (float(noise), None)
    A = kernels.ltf_covar(Zd, spec, *nz)
    assert torch.equal(A, kernels.ltf_covar(Zd, spec, *nz))
    A = A.cpu()
    Afull = R.kernel(Z, Z, p) + R._noise_matrix(noise, n)
    err = (A[:n, :n] - torch.tril(Afull)).abs() / (R.bound(Z, Z, p) + R._noise_matrix(noise, n))
    print("covar", float(err.max()))
    assert err.max() <= VAL_TOL
    pad = torch.eye(A.shape[0], dtype=torch.float64)
    assert torch.equal(A[n:], pad[n:]) and torch.equal(A[:, n:], pad[:, n:])
    # the sums, with W formed from the restatement's own alpha and A^{-1}
    _, _, S, W = R.ll_closed(Z, y, p, noise, c)
    Ainv, L = torch.linalg.inv(Afull), torch.linalg.cholesky(Afull)
    alpha = Ainv @ (y - c)
    beta = torch.linalg.solve_triangular(L, (y - c).unsqueeze(-1), upper=False).squeeze(-1)
    args = [t.contiguous().to(DEV) for t in (L, Ainv, alpha, beta)]
    part = kernels.ltf_mll_partials(Zd, spec, *args)
    assert torch.equal(part, kernels.ltf_mll_partials(Zd, spec, *args))
    part = part.cpu()
    scale = {"l0": 0.5 / p["l0"] ** 3, "l1": 0.5 / p["l1"] ** 3, "pw": 0.5, "o": 0.5}
    cols = {"l0": slice(0, dx), "l1": slice(16, 16 + dx), "pw": slice(32, 33), "o": slice(33, 34)}
    low = torch.tril(torch.ones(n, n, dtype=torch.float64), -1).unsqueeze(-1)
    for name in R.NAMES:
        s = S[name].reshape(n, n, -1)
        ref = (2.0 * low * s).sum(1) + torch.diagonal(s, dim1=0, dim2=1).mT   # row sums, k <= i
        mass = (2.0 * low * s.abs()).sum(1) + torch.diagonal(s.abs(), dim1=0, dim2=1).mT
        err = (part[:, cols[name]] * scale[name] - ref).abs()
        print(name, float((err / mass.clamp_min(1e-300)).max()))
        assert (err <= SUM_TOL * mass).all(), name
    padc = torch.ones(40, dtype=torch.bool)
    for sl in cols.values():
        padc[sl] = False
    padc[34:38] = False
    assert (part[:, padc] == 0.0).all()
    ref4 = torch.stack([torch.diagonal(W), torch.log(torch.diagonal(L)), beta * beta, alpha], dim=1)
    torch.testing.assert_close(part[:, 34:38], ref4, rtol=1e-13, atol=1e-13)


CROSS = [(nf, dx, n, Bq, None) for nf in NFS for dx in DXS for n in NS for Bq in ((1, 1), (5, 3), (2, 17))]
CROSS += [(nf, 9, 17, (5, 3), 1e-4) for nf in NFS]   # the power at its lower bound in the fit


@pytest.mark.parametrize("nf,dx,n,Bq,pw", CROSS)
def test_cross_and_cross_grad(nf, dx, n, Bq, pw):
    from botorch_amd import kernels
    Z, y, p, noise, c = R.make_case(nf, dx, n, pw=pw)
    X = R.make_queries(Z, p, *Bq)
    B, q = Bq
    spec, Zd, Xd = _spec(p), Z.to(DEV), X.to(DEV)
    Kx, Kxx = kernels.ltf_cross(Xd, Zd, spec)
    ex = (Kx.cpu().view(B, q, n) - R.kernel(X, Z, p)).abs() / R.bound(X, Z, p)
    exx = (Kxx.cpu() - R.kernel(X, X, p)).abs() / R.bound(X, X, p)
    print("cross", float(ex.max()), float(exx.max()))
    assert ex.max() <= VAL_TOL and exx.max() <= VAL_TOL
    assert all(torch.equal(a, b) for a, b in zip((Kx, Kxx), kernels.ltf_cross(Xd, Zd, spec)))
    # the target-fidelity rows (the last t-batch at least) down the general path: the same bits
    assert (X[-1][:, p["fc"]] >= 1).all()
    assert all(torch.equal(a, b) for a, b in zip((Kx, Kxx),
                                                 kernels.ltf_cross(Xd, Zd, spec, skip_target=False)))
    g = torch.Generator().manual_seed(5)
    dK = torch.randn(B, q, n, dtype=torch.float64, generator=g)
    G = torch.randn(B, q, q, dtype=torch.float64, generator=g)
    G = G + G.mT
    gargs = (dK.view(B * q, n).to(DEV), G.to(DEV))
    dX = kernels.ltf_cross_grad(Xd, Zd, spec, *gargs)
    assert torch.equal(dX, kernels.ltf_cross_grad(Xd, Zd, spec, *gargs))
    assert torch.equal(dX, kernels.ltf_cross_grad(Xd, Zd, spec, *gargs, skip_target=False))
    dX = dX.cpu()
    ref, mass = R.cross_grad(X, Z, p, dK, G)
    err = (dX - ref).abs()
    print("grad", float((err / mass.clamp_min(1e-300)).max()))
    assert torch.isfinite(dX).all() and (err <= SUM_TOL * mass).all()
    shut = (X[..., p["fc"]] < 0) | (X[..., p["fc"]] > 1)   # the clamp is active: exactly 0
    assert (dX[..., p["fc"]][shut] == 0.0).all()


def test_limits_are_refused():
    from botorch_amd import kernels
    Z, y, p, noise, c = R.make_case(1, 3, 17)
    spec = _spec(p)
    spec.xcols = (spec.xcols[0], spec.xcols[0], spec.xcols[2])  # a column named twice: the library refuses
    with pytest.raises(ValueError, match="partition"):
        kernels.ltf_covar(Z.to(DEV), spec)
    assert kernels.ltf_fused_ok(16, 2) and kernels.ltf_fused_ok(1, 1)
    assert not kernels.ltf_fused_ok(17, 1) and not kernels.ltf_fused_ok(0, 1) and not kernels.ltf_fused_ok(3, 3)
    wide = kernels.LTFSpec(tuple(range(17)), (17,), torch.ones(34, dtype=torch.float64, device=DEV), 1.0, 1.0)
    with pytest.raises(ValueError, match="d_x = 17"):
        kernels.ltf_covar(torch.zeros(4, 18, dtype=torch.float64, device=DEV), wide)
