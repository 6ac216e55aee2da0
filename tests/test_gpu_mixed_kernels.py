"""The four kernels of mixed.hip against tests/mixed_restatement.py (torch fp64 on the
host).  Values hold to 2e-13 absolute (entries below 3, under 100 flops each); the
MLL sums and dX are held relative to sum |summand| of the restatement at SUM_TOL =
10 x the largest disagreement of the restatement's two forms (ll_closed against
ll_autograd) over these same cases, measured once on the CPU: 9.6e-16."""
import pytest
import torch

from tests import mixed_restatement as R

pytestmark = pytest.mark.gpu

VAL_TOL = 2e-13
SUM_TOL = 1e-14  # 10 x 9.6e-16 (measured, see above)
KINDS, DIMS, NS = (0, 1), ((1, 1), (3, 2), (8, 8)), (1, 17, 70, 130)
DEV = "cuda"


def _spec(p):
    from botorch_amd import kernels
    hyper = torch.cat([p["l1"], p["lam1"], p["l2"], p["lam2"]]).to(DEV)
    return kernels.MixedSpec(p["kind"], tuple(p["cont"]), tuple(p["cat"]), hyper, float(p["os"]),
                             float(p["oc"]), float(p["op"]))


@pytest.mark.parametrize("fixed", (False, True))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_covar_and_mll_terms(kind, dims, n, fixed):
    from botorch_amd import kernels
    Z, y, p, noise, c = R.make_case(kind, *dims, n, fixed_noise=fixed)
    spec, Zd = _spec(p), Z.to(DEV)
    A = kernels.mixed_covar(Zd, spec, 0.0 if fixed else float(noise), noise.to(DEV) if fixed else None)
    Aref = torch.eye(A.shape[0], dtype=torch.float64)
    Aref[:n, :n] = torch.tril(R.kernel(Z, Z, p) + R._noise_matrix(noise, n))
    assert (A.cpu() - Aref).abs().max() <= VAL_TOL
    assert torch.equal(A, kernels.mixed_covar(Zd, spec, 0.0 if fixed else float(noise),
                                              noise.to(DEV) if fixed else None))
    # the sums, with W formed from the restatement's own alpha and A^{-1}
    _, _, S, W = R.ll_closed(Z, y, p, noise, c)
    Afull = R.kernel(Z, Z, p) + R._noise_matrix(noise, n)
    Ainv, L = torch.linalg.inv(Afull), torch.linalg.cholesky(Afull)
    alpha = Ainv @ (y - c)
    beta = torch.linalg.solve_triangular(L, (y - c).unsqueeze(-1), upper=False).squeeze(-1)
    args = [t.contiguous().to(DEV) for t in (L, Ainv, alpha, beta)]
    part = kernels.mixed_mll_partials(Zd, spec, *args)
    assert torch.equal(part, kernels.mixed_mll_partials(Zd, spec, *args))
    part = part.cpu()
    dc, dk = dims
    scale = {"l1": 0.5 / p["l1"] ** 3, "lam1": 0.5 / (dk * p["lam1"] ** 2), "l2": 0.5 / p["l2"] ** 3,
             "lam2": 0.5 / (dk * p["lam2"] ** 2), "os": 0.5, "oc": 0.5, "op": 0.5}
    cols = {"l1": slice(0, dc), "lam1": slice(8, 8 + dk), "l2": slice(16, 16 + dc),
            "lam2": slice(24, 24 + dk), "os": slice(32, 33), "oc": slice(33, 34), "op": slice(34, 35)}
    for name in R.NAMES:
        s = S[name].reshape(n, n, -1)
        low = torch.tril(torch.ones(n, n, dtype=torch.float64), -1).unsqueeze(-1)
        ref = (2.0 * low * s).sum(1) + torch.diagonal(s, dim1=0, dim2=1).mT   # row sums, k <= i
        bound = SUM_TOL * (2.0 * low * s.abs()).sum(1) + SUM_TOL * torch.diagonal(s.abs(), dim1=0, dim2=1).mT
        got = part[:, cols[name]] * scale[name]
        print(name, float(((got - ref).abs() / bound.clamp_min(1e-300)).max()) * SUM_TOL)
        assert ((got - ref).abs() <= bound).all(), name
    pad = torch.ones(40, dtype=torch.bool)
    for sl in cols.values():
        pad[sl] = False
    pad[35:39] = False
    assert (part[:, pad] == 0.0).all()
    ref4 = torch.stack([torch.diagonal(W), torch.log(torch.diagonal(L)), beta * beta, alpha], dim=1)
    torch.testing.assert_close(part[:, 35:39], ref4, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("Bq", ((1, 1), (5, 3), (2, 17)))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dims", DIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_cross_and_cross_grad(kind, dims, n, Bq):
    from botorch_amd import kernels
    Z, y, p, noise, c = R.make_case(kind, *dims, n)
    X = R.make_queries(Z, p, *Bq)
    B, q = Bq
    spec, Zd, Xd = _spec(p), Z.to(DEV), X.to(DEV)
    Kx, Kxx = kernels.mixed_cross(Xd, Zd, spec)
    assert (Kx.cpu() - R.kernel(X, Z, p).reshape(B * q, n)).abs().max() <= VAL_TOL
    assert (Kxx.cpu() - R.kernel(X, X, p)).abs().max() <= VAL_TOL
    assert all(torch.equal(a, b) for a, b in zip((Kx, Kxx), kernels.mixed_cross(Xd, Zd, spec)))
    Kx2, Kxx2 = kernels.mixed_cross(Xd, Zd, spec, kappa_direct=True)
    assert (Kx2 - Kx).abs().max() <= VAL_TOL and (Kxx2 - Kxx).abs().max() <= VAL_TOL
    g = torch.Generator().manual_seed(5)
    dK = torch.randn(B * q, n, dtype=torch.float64, generator=g)
    G = torch.randn(B, q, q, dtype=torch.float64, generator=g)
    G = G + G.mT
    dX = kernels.mixed_cross_grad(Xd, Zd, spec, dK.to(DEV), G.to(DEV))
    assert torch.equal(dX, kernels.mixed_cross_grad(Xd, Zd, spec, dK.to(DEV), G.to(DEV)))
    dX = dX.cpu()
    assert (dX[..., p["cat"]] == 0.0).all() and torch.isfinite(dX).all()
    # reference and sum |summand| per (row, column): the first argument's gradient of each pair
    diff_t = X[..., p["cont"]].unsqueeze(-2) - Z[:, p["cont"]]                      # B q n dc
    diff_q = X[..., p["cont"]].unsqueeze(-2) - X[..., p["cont"]].unsqueeze(-3)      # B q q dc

    def pair_grad(diff, Xa, Xb, w):
        _, ne = R._parts(Xa, Xb, p)
        _, g1 = R._kbar_g(diff, p["l1"], kind)
        _, g2 = R._kbar_g(diff, p["l2"], kind)
        kp2 = torch.exp(-(ne / p["lam2"]).mean(-1))
        f = -(p["os"] * g1.unsqueeze(-1) / p["l1"] ** 2 + p["op"] * (kp2 * g2).unsqueeze(-1) / p["l2"] ** 2)
        return w.unsqueeze(-1) * f * diff

    terms = torch.cat([pair_grad(diff_t, X, Z, dK.view(B, q, n)), pair_grad(diff_q, X, X, G)], dim=-2)
    ref, mass = terms.sum(-2), terms.abs().sum(-2)
    err = (dX[..., p["cont"]] - ref).abs()
    print(float((err / mass.clamp_min(1e-300)).max()))
    assert (err <= SUM_TOL * mass).all()


def test_limits_are_refused():
    from botorch_amd import kernels
    Z, y, p, noise, c = R.make_case(0, 3, 2, 17)
    spec = _spec(p)
    spec.cont = (spec.cont[0], spec.cont[0], spec.cont[2])  # a column named twice: the library refuses
    with pytest.raises(ValueError, match="partition"):
        kernels.mixed_covar(Z.to(DEV), spec)
    assert kernels.mixed_fused_ok(8, 8) and not kernels.mixed_fused_ok(9, 2) and not kernels.mixed_fused_ok(0, 3)
