"""kxt_build_kernel (csrc/post.hip) through its three C entry points --
bo_post_kxt, bo_post_kxt_rows, bo_post_kxt_rows_members -- on random scaled
training rows (no model, no Cholesky): K*x^T = outputscale k(X / ls, Xt),
np x nrows_pad, k-major, and the padded rows Xq = X / ls, nrows_pad x 8.

The restatement is torch fp64 on the CPU: the same X / ls, the squared
distance summed in the order t = 0..d-1, outputscale * exp(-d2 / 2) or the
Matern-5/2 form.  Inputs lie in the unit cube with lengthscale 0.5, so d2 <= 32
and the rounding of d2 (at most (2 d + 1) 2^-53 * 16 = 3e-14 absolute in the
exponent) plus a 2-ulp exp stay inside rtol 1e-13 at atol 0.

Rows a >= q inside a t-batch's Qp rows are zero rows of Xq, and like every
row below B * Qp they are evaluated: their K*x^T entries are the kernel at the
origin -- bit for bit the values a real candidate at x = 0 gets -- and not
0.0.  The posterior kernels never read them into a result.  Exact zeros are
the rows k >= n and the rows from B * Qp up to nrows_pad.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
RBF, MATERN = 0, 1
LS = 0.5


@functools.lru_cache(maxsize=None)
def _inputs(B, q, d, n, seed=0):
    """X (B x q x d) and the scaled training rows (n x 8), on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + 97 * B + 13 * q + 7 * d + n)
    X = torch.rand(B, q, d, dtype=torch.float64, generator=g)
    Xt = torch.zeros(n, 8, dtype=torch.float64)
    Xt[:, :d] = torch.rand(n, d, dtype=torch.float64, generator=g) / LS
    return X, Xt


def _geometry(B, q, n):
    from botorch_amd import kernels
    Qp, nrows_pad, nC = kernels.geometry(B, q, n)
    return Qp, nrows_pad, nC * 128


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _kxt_rows(kind, X, ls, Xt, n, os_):
    """bo_post_kxt_rows into NaN-filled outputs -> (Xq, Kt)."""
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    B, q, d = X.shape
    _, nrows_pad, np_ = _geometry(B, q, n)
    Xq, Kt = _nan(nrows_pad, 8), _nan(np_, nrows_pad)
    check(lib().bo_post_kxt_rows(kind, kernels._p(X), B, q, d, kernels._p(ls), kernels._p(Xt), n, os_,
                                 kernels._p(Xq), kernels._p(Kt), kernels._stream(X.device)),
          "post_kxt_rows")
    return Xq, Kt


def _kxt(kind, Xq, B, q, d, Xt, n, os_):
    """bo_post_kxt on prepared rows into a NaN-filled output -> Kt."""
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    _, nrows_pad, np_ = _geometry(B, q, n)
    Kt = _nan(np_, nrows_pad)
    check(lib().bo_post_kxt(kind, kernels._p(Xq), B, q, d, kernels._p(Xt), n, os_, kernels._p(Kt),
                            kernels._stream(Xq.device)), "post_kxt")
    return Kt


def _kxt_members(kind, X, lss, Xts, n, oss):
    """bo_post_kxt_rows_members into NaN-filled outputs -> ([Xq], [Kt])."""
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    B, q, d = X.shape
    nm = len(lss)
    _, nrows_pad, np_ = _geometry(B, q, n)
    Xqs = [_nan(nrows_pad, 8) for _ in range(nm)]
    Kts = [_nan(np_, nrows_pad) for _ in range(nm)]
    P = ctypes.c_void_p * nm
    check(lib().bo_post_kxt_rows_members(
        nm, kind, kernels._p(X), B, q, d, P(*[t.data_ptr() for t in lss]),
        P(*[t.data_ptr() for t in Xts]), (ctypes.c_double * nm)(*oss), n,
        P(*[t.data_ptr() for t in Xqs]), P(*[t.data_ptr() for t in Kts]),
        kernels._stream(X.device)), "post_kxt_rows_members")
    return Xqs, Kts


def _restate(kind, X, ls, Xt, n, os_, Qp, nrows_pad, np_):
    """(Xq, Kt) on the CPU: rows below B * Qp evaluated, everything else 0."""
    B, q, d = X.shape
    Xq = torch.zeros(nrows_pad, 8, dtype=torch.float64)
    Xq[:B * Qp].view(B, Qp, 8)[:, :q, :d] = X / ls
    d2 = torch.zeros(n, B * Qp, dtype=torch.float64)
    for t in range(d):
        df = Xq[:B * Qp, t][None, :] - Xt[:n, t][:, None]
        d2 = df * df + d2
    if kind == RBF:
        k = torch.exp(-0.5 * d2)
    else:
        s5r = 2.23606797749978969641 * torch.sqrt(d2.clamp_min(1e-30))
        k = (1.0 + s5r + (5.0 / 3.0) * d2) * torch.exp(-s5r)
    Kt = torch.zeros(np_, nrows_pad, dtype=torch.float64)
    Kt[:n, :B * Qp] = os_ * k
    return Xq, Kt


@pytest.mark.parametrize("n", [100, 130])
@pytest.mark.parametrize("B,q", [(3, 5), (1, 16)])
@pytest.mark.parametrize("d", [1, 3, 6, 8])
@pytest.mark.parametrize("kind", [RBF, MATERN])
def test_values_and_structure_against_host_restatement(kind, d, B, q, n):
    """Every entry written (NaN-filled outputs, nrows_pad = 128), values to
    rtol 1e-13 at atol 0, exact zeros for k >= n and rows >= B * Qp, Xq equal
    to the padded X / ls, and the a >= q rows equal to a candidate at x = 0."""
    X, Xt = _inputs(B, q, d, n)
    os_ = 1.7
    ls = torch.full((d,), LS, dtype=torch.float64)
    Qp, nrows_pad, np_ = _geometry(B, q, n)
    assert nrows_pad == 128
    Xq, Kt = _kxt_rows(kind, X.to(DEV), ls.to(DEV), Xt.to(DEV), n, os_)
    Xq, Kt = Xq.cpu(), Kt.cpu()
    assert not torch.isnan(Kt).any() and not torch.isnan(Xq).any()
    Xq_ref, Kt_ref = _restate(kind, X, ls, Xt, n, os_, Qp, nrows_pad, np_)
    assert torch.equal(Xq, Xq_ref)
    assert (Kt[n:] == 0).all() and (Kt[:, B * Qp:] == 0).all()
    assert (Kt[:n, :B * Qp] > 0).all()
    torch.testing.assert_close(Kt, Kt_ref, rtol=1e-13, atol=0)
    if Qp > q:
        X0 = torch.zeros(1, 1, d, dtype=torch.float64, device=DEV)
        _, K0 = _kxt_rows(kind, X0, ls.to(DEV), Xt.to(DEV), n, os_)
        pad = Kt[:, :B * Qp].reshape(np_, B, Qp)[:, :, q:]
        assert torch.equal(pad, K0.cpu()[:, :1, None].expand_as(pad))


@pytest.mark.parametrize("B,q,n", [(3, 5, 130),        # nrows_pad 128, small grid
                                   (20, 16, 130),      # nrows_pad 384, small grid
                                   (3, 5, 16300),      # nrows_pad 128, half a block of the large grid
                                   (20, 16, 8100),     # nrows_pad 384, large grid, ragged last k-chunk
                                   (3, 5, 65500),      # 2048 workgroups of two rows per thread:
                                   (20, 16, 65500)])   # a quarter and three quarters of their 512 rows
def test_every_entry_written(B, q, n):
    """NaN-filled Kt and Xq come back without a NaN over np x nrows_pad, on
    grids whose last workgroup covers rows beyond nrows_pad, with the zero
    structure in place; all three entry points."""
    d = 6
    X, Xt = _inputs(B, q, d, n)
    X, Xt = X.to(DEV), Xt.to(DEV)
    Qp, nrows_pad, np_ = _geometry(B, q, n)
    assert nrows_pad == (128 if B == 3 else 384)
    lss = [torch.full((d,), LS + 0.1 * m, dtype=torch.float64, device=DEV) for m in range(3)]
    oss = [1.0, 0.6, 2.5]
    Xq, Kt = _kxt_rows(RBF, X, lss[0], Xt, n, oss[0])
    Kt2 = _kxt(RBF, Xq, B, q, d, Xt, n, oss[0])
    Xqs, Kts = _kxt_members(RBF, X, lss, [Xt] * 3, n, oss)
    for xq, kt in [(Xq, Kt), (Xq, Kt2)] + list(zip(Xqs, Kts)):
        assert not torch.isnan(kt).any() and not torch.isnan(xq).any()
        assert (kt[n:] == 0).all() and (kt[:, B * Qp:] == 0).all()
        assert (kt[:n, :B * Qp] > 0).all()
        assert (xq[B * Qp:] == 0).all() and (xq[:, d:] == 0).all()


def test_unaligned_kt_equals_aligned():
    """A Kt 8 bytes off a 16-byte boundary (one row per thread, 8-byte stores)
    gets the bits of an aligned one (two rows per thread at this shape)."""
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    B, q, d, n = 3, 5, 6, 65500
    X, Xt = _inputs(B, q, d, n)
    X, Xt = X.to(DEV), Xt.to(DEV)
    ls = torch.full((d,), LS, dtype=torch.float64, device=DEV)
    _, nrows_pad, np_ = _geometry(B, q, n)
    Xq, Kt = _kxt_rows(RBF, X, ls, Xt, n, 1.3)
    buf = _nan(np_ * nrows_pad + 1)
    Kt_off = buf[1:].view(np_, nrows_pad)
    assert Kt.data_ptr() % 16 == 0 and Kt_off.data_ptr() % 16 == 8
    Xq_off = _nan(nrows_pad, 8)
    check(lib().bo_post_kxt_rows(RBF, kernels._p(X), B, q, d, kernels._p(ls), kernels._p(Xt), n, 1.3,
                                 kernels._p(Xq_off), kernels._p(Kt_off), kernels._stream(X.device)),
          "post_kxt_rows")
    assert torch.equal(Kt_off, Kt) and torch.equal(Xq_off, Xq)


@pytest.mark.parametrize("kind,B,q,n", [(RBF, 3, 5, 130), (MATERN, 3, 5, 130),   # small grid
                                        # 1024 workgroups of 256 x 16: the large grid, one row per thread
                                        (RBF, 64, 16, 4096), (MATERN, 64, 16, 4096),
                                        # C3, 2048 workgroups of 512 x 32: two rows per thread
                                        (RBF, 512, 16, 4096)])
def test_routes_agree_bit_for_bit(kind, B, q, n):
    """bo_post_kxt on the rows bo_post_kxt_rows wrote, bo_post_kxt_rows, and
    each member of bo_post_kxt_rows_members write the same bits; and the
    columns of t-batch b equal a B = 1 call on that t-batch (another grid)."""
    d = 6
    X, Xt0 = _inputs(B, q, d, n)
    X = X.to(DEV)
    Xts = [_inputs(B, q, d, n, seed=m)[1].to(DEV) for m in range(3)]
    assert torch.equal(Xts[0].cpu(), Xt0)
    lss = [torch.full((d,), LS + 0.1 * m, dtype=torch.float64, device=DEV) for m in range(3)]
    oss = [1.0, 0.6, 2.5]
    Qp, nrows_pad, np_ = _geometry(B, q, n)
    Xqs, Kts = _kxt_members(kind, X, lss, Xts, n, oss)
    for m in range(3):
        Xq, Kt = _kxt_rows(kind, X, lss[m], Xts[m], n, oss[m])
        assert torch.equal(Xqs[m], Xq)
        assert torch.equal(Kts[m], Kt)
        assert torch.equal(_kxt(kind, Xq, B, q, d, Xts[m], n, oss[m]), Kt)
    for b in (0, B - 1):
        Xq1, Kt1 = _kxt_rows(kind, X[b:b + 1].contiguous(), lss[0], Xts[0], n, oss[0])
        assert torch.equal(Kt1[:, :Qp], Kts[0][:, b * Qp:(b + 1) * Qp])
        assert torch.equal(Xq1[:Qp], Xqs[0][b * Qp:(b + 1) * Qp])
