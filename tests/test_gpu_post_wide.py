"""The 8-wave ("wide") one-pass paired forward kernel against the 256-thread
kernel it stands in for: bo_post_set_wide(1) against (-1) in one process.

The wide kernel keeps every output element's k-walk, zero-block skip and
epilogue summation order, so Spart, mpart and R^T (both layouts) have to be
torch.equal, not close.  Shapes: the smallest that reach each branch of the
wide schedule (one super-tile is 8 column tiles x 4 double row tiles):

  (n, B, q)          what it reaches
  (2048, 64, 16)     one column pair, one row group
  (2000, 64, 16)     ragged last k-step and ragged diagonal block
  (2048, 192, 16)    three row groups: surplus blocks take the early return
  (4096, 64, 16)     two column pairs
  (2048, 128, 5)     Qp = 8

The 256-thread route itself is held to the host by test_gpu_post_pipeline.py.
"""
import ctypes
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
SHAPES = [(2048, 64, 16), (2000, 64, 16), (2048, 192, 16), (4096, 64, 16), (2048, 128, 5)]
IDS = [f"n{n}-b{B}-q{q}" for n, B, q in SHAPES]


@functools.lru_cache(maxsize=None)
def _cache(n, ls=0.35):
    from botorch_amd import kernels
    from botorch_amd.test_functions import Hartmann
    from oracle.gp import ExactGPOracle, GPHyper
    from oracle.sampling import draw_sobol_samples
    lo = torch.zeros(6, dtype=F64)
    X = draw_sobol_samples(lo, lo + 1, n, 1, 0).squeeze(1)
    Y = Hartmann(dim=6, negate=True)(X).unsqueeze(-1)
    h = GPHyper(torch.full((6,), ls, dtype=F64), 1e-3, 0.1)
    orc = ExactGPOracle(X, Y, h)
    return kernels.build_gp_cache(X.to(DEV), orc.train_y.to(DEV), h.lengthscale.to(DEV), h.noise,
                                  h.constant)


def _X(n, B, q):
    g = torch.Generator().manual_seed(n + B)
    return torch.rand(B, q, 6, generator=g, dtype=F64).to(DEV)


def _applies(B, q, n, kc_len=0, cross=False, kt=True):
    from botorch_amd._lib import check, lib
    out = ctypes.c_int(-1)
    check(lib().bo_post_wide_applies(B, q, n, kc_len, int(cross), int(kt), ctypes.byref(out)),
          "post_wide_applies")
    return out.value


class _wide:
    """bo_post_set_wide(mode) for the block, the library's choice afterwards."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from botorch_amd._lib import check, lib
        check(lib().bo_post_set_wide(self.mode), "post_set_wide")

    def __exit__(self, *exc):
        from botorch_amd._lib import lib
        lib().bo_post_set_wide(0)


def _partials(cache, X, mode, rt_layout):
    """One-pass partials over K*x^T on the route `mode` forces (asserted)."""
    from botorch_amd import kernels
    with _wide(mode):
        assert _applies(X.shape[0], X.shape[1], cache.n) == (1 if mode == 1 else 0)
        pp = kernels.post_partials(cache, X, store_R=True, split=0, kxt=True, rt_layout=rt_layout,
                                   small=False)
        torch.cuda.synchronize()
    return pp


def _assert_same(a, b, what):
    for name in ("Spart", "mpart", "Rt"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape, f"{what} {name}: shape"
        assert torch.isfinite(x).all(), f"{what} {name}: non-finite"
        assert x.abs().max() > 0, f"{what} {name}: trivial"
        assert torch.equal(x, y), (f"{what} {name}: {(x != y).sum().item()} elements differ, "
                                   f"max |d| = {(x - y).abs().max().item():.3e}")


@pytest.mark.parametrize("layout", ["rowmajor", "blocked"])
@pytest.mark.parametrize("n,B,q", SHAPES, ids=IDS)
def test_wide_equals_narrow(n, B, q, layout):
    from botorch_amd import _lib
    rt = _lib.RT_ROWMAJOR if layout == "rowmajor" else _lib.RT_BLOCKED
    cache, X = _cache(n), _X(n, B, q)
    _assert_same(_partials(cache, X, 1, rt), _partials(cache, X, -1, rt), layout)


def test_wide_never_multiplies_zero_blocks():
    """NaN in every 16 x 16 block on the zero side of U leaves every output of
    the wide kernel torch.equal to the clean run's."""
    from botorch_amd import _lib
    n, B, q = SHAPES[1]  # ragged diagonal block
    cache, X = _cache(n), _X(n, B, q)
    nb = cache.U.shape[0] // 16
    kb = torch.arange(nb, device=DEV).view(-1, 1)
    cb = torch.arange(nb, device=DEV).view(1, -1)
    mask = (kb > cb).repeat_interleave(16, 0).repeat_interleave(16, 1)
    U = cache.U.clone()
    U[mask] = float("nan")
    bad = dataclasses.replace(cache, U=U)
    for rt in (_lib.RT_ROWMAJOR, _lib.RT_BLOCKED):
        _assert_same(_partials(bad, X, 1, rt), _partials(cache, X, 1, rt), f"poisoned layout {rt}")


def test_wide_applies_only_where_eligible():
    from botorch_amd import kernels
    n, B, q = SHAPES[0]
    with _wide(1):
        assert _applies(B, q, n) == 1
        assert _applies(B + 8, q, n) == 0               # nI = 9: not a multiple of 8
        assert _applies(B, q, n, cross=True) == 0       # cross term
        assert _applies(B, q, n, kc_len=-1) == 0        # stream-K plan
        assert _applies(B, q, n, kc_len=16) == 0        # uniform split plan
        assert _applies(B, q, n, kt=False) == 0         # no K*x^T
        assert _applies(B, q, 1024) == 0                # nC = 8: no column pairs
        # the library's own plan at this shape is a split plan: not the wide kernel
        kc, _ = kernels.split_plan(B, q, n)
        assert _applies(B, q, n, kc_len=kc) == (1 if kc == 0 else 0)
    with _wide(-1):
        assert _applies(B, q, n) == 0
    from botorch_amd._lib import lib
    assert lib().bo_post_set_wide(2) != 0 and lib().bo_post_set_wide(-2) != 0


@pytest.mark.parametrize("split", [0, None], ids=["one_pass", "library_plan"])
def test_qei_forward_equal_between_modes(split):
    """qEI forward at n = 2048, b = 64: the same bits on both routes."""
    from botorch_amd import _lib, kernels
    from oracle.sampling import draw_sobol_normal_samples
    n, B, q = SHAPES[0]
    cache, X = _cache(n), _X(n, B, q)
    Z = draw_sobol_normal_samples(q, 64, 3).to(DEV)
    out = {}
    for mode in (1, -1):
        with _wide(mode):
            pp = kernels.post_partials(cache, X, split=split, kxt=True, small=False)
            out[mode] = kernels.qmc_finalize(cache, pp, _lib.QMC_QEI, 0.0, 1.0, Z=Z, best_f=-0.5)
            torch.cuda.synchronize()
    assert (out[1]["acq"] > 0).any(), "degenerate check (zero improvement everywhere)"
    for k in ("acq", "mean", "cov"):
        assert torch.equal(out[1][k], out[-1][k]), k
