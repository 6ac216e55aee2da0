"""bo_input_warp, bo_input_warp_bwd and bo_mll_dx against the restatement."""
import numpy as np
import pytest
import torch

from tests import warp_restatement as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CONCS = (1e-4, 0.3, 1.0, 2.5, 8.0)
# the host evaluation of the log-space form against 50 digits on this grid (4.3e-16 absolute
# on z, 1.7e-14 relative on dz/du), times 8 for the device's exp / log against libm's
Z_ATOL, DZ_RTOL = 8 * 4.3e-16, 8 * 1.7e-14


@pytest.fixture(scope="module")
def grid():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.tensor([0.0, 1.0, 0.5, 1e-3, 1 - 1e-3], dtype=torch.float64),
                   torch.rand(40, dtype=torch.float64, generator=g)])
    mp = {(a, b): np.array([ref.kumaraswamy_mp(float(v), a, b) for v in x])
          for a in CONCS for b in CONCS}
    return x, mp


def _spec(d, a, b):
    """Column 1 normalised only, column 2 untouched, every other column warped."""
    from botorch_amd import kernels
    flag = torch.ones(d, dtype=torch.bool)
    offset, rscale = torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)
    if d > 2:
        flag[1] = flag[2] = False
        offset[1], rscale[1] = -0.75, 1.0 / 3.0
    mask = sum(1 << c for c in range(d) if flag[c])
    spec = kernels.WarpSpec(offset.to(DEV), rscale.to(DEV),
                            torch.full((d,), a, dtype=torch.float64, device=DEV),
                            torch.full((d,), b, dtype=torch.float64, device=DEV), mask, ref.EPS)
    return spec, flag, offset, rscale


@pytest.mark.parametrize("d", [1, 6, 9, 64])
def test_forward_and_dx_against_mpmath(grid, d):
    from botorch_amd import kernels
    x, mp = grid
    X = x.unsqueeze(-1).expand(-1, d).contiguous()
    raw = x * (1.0 - 2.0 * ref.EPS) + ref.EPS
    passes = ((raw >= ref.EPS) & (raw <= 1.0 - ref.EPS)).double().numpy() * (1.0 - 2.0 * ref.EPS)
    worst_z = worst_dz = 0.0
    for (a, b), want in mp.items():
        spec, flag, offset, rscale = _spec(d, a, b)
        Z = kernels.input_warp(X.to(DEV), spec).cpu().numpy()
        dX, _, _ = kernels.input_warp_bwd(torch.ones(X.shape, dtype=torch.float64, device=DEV),
                                          X.to(DEV), spec)
        dX = dX.cpu().numpy()
        for c in range(d):
            if flag[c]:
                worst_z = max(worst_z, np.abs(Z[:, c] - want[:, 0]).max())
                wdx = want[:, 1] * passes
                worst_dz = max(worst_dz, (np.abs(dX[:, c] - wdx) / np.abs(want[:, 1])).max())
            else:
                np.testing.assert_array_equal(Z[:, c], ((x - offset[c]) * rscale[c]).numpy())
                np.testing.assert_array_equal(dX[:, c], np.full(len(x), float(rscale[c])))
    print(f"d={d}: max |z - z50| = {worst_z:.3e}, max rel dz/du error = {worst_dz:.3e}")
    assert worst_z <= Z_ATOL and worst_dz <= DZ_RTOL


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1025])
@pytest.mark.parametrize("d", [6, 9])
def test_column_sums_match_autograd_and_repeat_bitwise(R, d):
    """dZ > 0, so every column sum has terms of one sign: 2 x 8 x 1.7e-14 for the two
    evaluations of dz/da, dz/db plus R 2^-53 for the order of the sum."""
    from botorch_amd import kernels
    g = torch.Generator().manual_seed(R * 100 + d)
    X = torch.rand(R, d, dtype=torch.float64, generator=g) * 3.0 - 0.75
    dZ = torch.rand(R, d, dtype=torch.float64, generator=g) + 0.1
    spec, flag, offset, rscale = _spec(d, 0.3, 2.5)
    spec.conc1 = (0.3 + 0.2 * torch.arange(d, dtype=torch.float64)).to(DEV)
    spec.conc0 = (2.5 - 0.2 * torch.arange(d, dtype=torch.float64)).to(DEV)
    offset = offset.clone()
    rscale = rscale.clone()
    offset[flag], rscale[flag] = -0.75, 1.0 / 3.0
    spec.offset, spec.rscale = offset.to(DEV), rscale.to(DEV)
    Xr = X.clone().requires_grad_(True)
    a = spec.conc1.cpu().requires_grad_(True)
    b = spec.conc0.cpu().requires_grad_(True)
    (ref.warp_logspace(Xr, offset, rscale, a, b, flag) * dZ).sum().backward()
    out = [kernels.input_warp_bwd(dZ.to(DEV), X.to(DEV), spec) for _ in range(2)]
    for u, v in zip(*out):
        assert torch.equal(u, v)
    _, da, db = (t.cpu() for t in out[0])
    tol = dict(rtol=2 * DZ_RTOL + R * 2.0 ** -53, atol=0.0)
    torch.testing.assert_close(da, torch.where(flag, a.grad, torch.zeros(d, dtype=torch.float64)), **tol)
    torch.testing.assert_close(db, torch.where(flag, b.grad, torch.zeros(d, dtype=torch.float64)), **tol)


def _dx_case(kind, has_os, fixed, d, n, coincident=False):
    from botorch_amd import kernels
    g = torch.Generator().manual_seed(1000 * d + n)
    X = torch.rand(n, d, dtype=torch.float64, generator=g)
    if coincident:
        X[n - 1] = X[3]
    y = torch.randn(n, dtype=torch.float64, generator=g)
    ls = 0.3 + torch.rand(d, dtype=torch.float64, generator=g)
    os_ = 1.7 if has_os else 1.0
    noise = 0.05 + 0.1 * torch.rand(n, dtype=torch.float64, generator=g) if fixed else 0.08
    Xr = X.clone().requires_grad_(True)
    ref.mll(Xr, y, ls, noise, 0.2, os_, kind).backward()
    cache = kernels.build_gp_cache(X.to(DEV), y.to(DEV), ls.to(DEV),
                                   noise.to(DEV) if fixed else noise, 0.2, kind=kind,
                                   outputscale=os_)
    Ainv = kernels.ainv(cache)
    forms = (0, 1) if d < 32 else (0,)
    got = [[kernels.mll_dx(kind, X.to(DEV), ls.to(DEV), os_, Ainv, cache.alpha, form=f)
            for _ in range(2)] for f in forms]
    return Xr.grad, got


# the kernel's row block and column tile are both 64
@pytest.mark.parametrize("d", [1, 6, 8, 9, 64])
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("has_os", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_mll_dx_against_autograd(kind, has_os, fixed, d):
    for n in (1, 2, 63, 64, 65, 130):  # 130: three row blocks -- diagonal, direct and mirrored tiles
        want, got = _dx_case(kind, has_os, fixed, d, n)
        for a, b in got:
            assert torch.equal(a, b)
            torch.testing.assert_close(a.cpu(), want, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("kind", [0, 1])
def test_mll_dx_coincident_rows_stay_finite(kind):
    want, got = _dx_case(kind, True, False, 6, 67, coincident=True)
    for a, _ in got:
        assert torch.isfinite(a).all()
        torch.testing.assert_close(a.cpu(), want, rtol=1e-6, atol=1e-9)
