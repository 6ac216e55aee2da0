"""The fused SAAS potential (bo_saas_potential_v, torch.ops.bo.saas_potential)
against the restatement (tests/saas_nuts_restatement.py): the regular and the
ill-conditioned cases of tests/test_nuts_cpu.py with the same bounds, shapes on
both sides of an MFMA block, of a 128 panel and of 256, d past the MLL
kernel's 64 and at the limit, one, a few and many rows; every input a window of
a NaN-filled buffer; repeated calls and rows of a larger call bit-identical;
the status rows; the limits."""
import functools
import math

import pytest
import torch

from tests import saas_nuts_restatement as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64

# (n, d, C): the kernel's edges
EDGES = [(15, 1, 1), (16, 65, 3), (17, 3, 17), (129, 65, 3), (257, 4, 1), (33, 256, 1)]


def _window(t):
    """t on the device as a window of a NaN buffer (64 doubles before and after)."""
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=F64, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1).to(DEV)
    return buf[64:64 + t.numel()].view(t.shape)


@functools.lru_cache(maxsize=None)
def _case(n, d, C):
    """(X, y, z, U, grad) of a regular case, the oracle computed once."""
    X, y = sr.data(n, d)
    z = sr.regular_z(d, C=C)
    U, G, _ = sr.potential(z, X, y)
    return X, y, z, U, G


def _fused(z, X, y):
    from botorch_amd import kernels, ops  # noqa: F401
    n, d = X.shape
    work = torch.full((max(1, kernels.saas_potential_work(n, d, z.shape[0])),), float("nan"),
                      dtype=F64, device=DEV)
    U, g, status = torch.ops.bo.saas_potential(_window(z), _window(X), _window(y), work)
    return U.cpu(), g.cpu(), status.cpu()


def _check(what, got, ref, limit):
    err = float((got - ref).abs().max())
    print(f"{what}: max |got - ref| {err:.3e} (limit {limit:.3e}, max |ref| "
          f"{float(ref.abs().max()):.3e})")
    assert torch.isfinite(got).all() and err <= limit


@pytest.mark.parametrize("n,d,C", [(n, d, 3) for n, d in sr.REGULAR] + EDGES)
def test_fused_potential_matches_restatement(n, d, C):
    X, y, z, U, G = _case(n, d, C)
    u, g, status = _fused(z, X, y)
    assert status.dtype == torch.int32 and status.tolist() == [0] * C
    _check(f"({n}, {d}, C = {C}) U", u, U, sr.project_bound(U))
    _check(f"({n}, {d}, C = {C}) grad", g, G, sr.project_bound(G))
    u2, g2, s2 = _fused(z, X, y)
    assert torch.equal(u, u2) and torch.equal(g, g2) and torch.equal(status, s2)


@pytest.mark.parametrize("n,d", sr.ILL)
def test_fused_potential_ill_conditioned(n, d):
    X, y = sr.data(n, d)
    z = sr.ill_z(d)
    lim_u, lim_g, U, G = sr.ill_limits(X, y, z)
    u, g, status = _fused(z, X, y)
    assert status.tolist() == [0]
    _check(f"ill ({n}, {d}) U", u, U, lim_u)
    _check(f"ill ({n}, {d}) grad", g, G, lim_g)


def test_rows_do_not_depend_on_the_batch():
    """Row c of the 17-row call equals the one-row call on that row, bit for
    bit, through the operator and through the ctypes binding."""
    from botorch_amd import kernels
    X, y, z, _, _ = _case(17, 3, 17)
    u, g, _ = _fused(z, X, y)
    for c in (0, 5, 16):
        u1, g1, s1 = _fused(z[c:c + 1], X, y)
        assert torch.equal(u1[0], u[c]) and torch.equal(g1[0], g[c]) and s1.tolist() == [0]
    uk, gk, sk = kernels.saas_potential(z.to(DEV), X.to(DEV), y.to(DEV))
    assert torch.equal(uk.cpu(), u) and torch.equal(gk.cpu(), g) and sk.tolist() == [0] * 17


def test_status_rows():
    """A NaN row and a row with z0 = 800: status 1, U = +inf, a zero gradient,
    their neighbours on the oracle.  Duplicated points under a huge outputscale
    and no noise: status 2."""
    X, y, z, U, G = _case(17, 3, 17)
    z = z[:5].clone()
    z[1, 2] = math.nan
    z[3, 0] = 800.0
    u, g, status = _fused(z, X, y)
    assert status.tolist() == [0, 1, 0, 1, 0]
    for bad in (1, 3):
        assert u[bad] == math.inf and g[bad].abs().max() == 0.0
    good = [0, 2, 4]
    _check("neighbours U", u[good], U[good], sr.project_bound(U[good]))
    _check("neighbours grad", g[good], G[good], sr.project_bound(G[good]))
    zd = torch.cat([torch.tensor([[60.0, 0.0, -40.0, 0.0, 0.0, 0.0, 0.0]], dtype=F64), z[:1]])
    u, g, status = _fused(zd, torch.cat([X, X]), torch.cat([y, y]))
    assert status.tolist() == [2, 0] and u[0] == math.inf and g[0].abs().max() == 0.0
    assert torch.isfinite(u[1]) and torch.isfinite(g[1]).all()


def test_limits_raise_on_the_host():
    from botorch_amd import kernels, ops  # noqa: F401
    e = lambda *s: torch.zeros(*s, dtype=F64, device=DEV)  # noqa: E731
    for n, d in ((1025, 3), (4, 257), (4, 0)):
        with pytest.raises(ValueError, match="saas_potential"):
            kernels.saas_potential(e(1, d + 4), e(n, d), e(n))
        with pytest.raises(ValueError, match="saas_potential"):
            torch.ops.bo.saas_potential(e(1, d + 4), e(n, d), e(n), None)
    with pytest.raises(ValueError, match="work"):
        kernels.saas_potential(e(1, 7), e(17, 3), e(17), work=e(8))
