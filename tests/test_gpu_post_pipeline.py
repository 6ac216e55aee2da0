"""post_partials_kernel's k-loop on every schedule, against CPU fp64.

The kernel skips the MFMAs of the 16 x 16 blocks of its triangular U operand
that lie on the zero side of the diagonal (U = L^-T: blocks with k-block >
column block; the mirrored kernels' U = L^-1: k-block < column block).  Two
properties are checked on the smallest shape that reaches each schedule:

  values     R^T = U^T K*x^T, the column-tile partials Spart / mpart (and the
             cross term Cx, W^T = L^-T R^T, A^-1 = L^-T L^-1, the fused dX) from
             the device's own operands copied to the host and multiplied there
             in fp64;
  the skip   with NaN written into every 16 x 16 block of U on the zero side
             the outputs are torch.equal to the clean run: those blocks are
             never multiplied.  (bo_ainv passes one buffer as both operands, so
             it has no poisoned run.)

Tolerance: summation order only.  TOL holds, per (n, output), the largest
|got - ref| of the build BEFORE the skip on these same inputs against this
same reference, measured on MI355X (the skipped products are exact zeros, so
the build with the skip reproduced every figure bit for bit):

  n      Rt         Spart      mpart      other
  16     0          0          5.551e-17
  37     0          1.388e-17  2.776e-16
  130    0          2.776e-17  8.882e-16  Wt 4.441e-16   Ainv 0
  256    5.357e-15  2.498e-15  1.574e-14
  300    3.331e-15  1.860e-15  7.105e-15
  1024   2.223e-15  3.331e-16  4.940e-15  Cx 3.375e-14
  2048   1.455e-14  4.302e-15  5.196e-14  Wt 6.661e-15   Ainv 8.527e-13  dX 3.650e-13

The bound is 4 x that figure.  Where the figure is below the host reference's
own last-place rounding, 2^-53 max|ref| (it is exactly 0 at the smallest
shapes, where another BLAS's summation order on the host alone could move the
reference by that much), that rounding takes its place.  Every comparison also
has to stay inside the project's existing bounds
(CAP: test_post_partials_split_k's rtol 1e-11, atol 2.5e-13 max(1, n / 1024)
for the posterior outputs; the bounds of the existing W / A^-1 / dX tests for
those).

bo_post_w and bo_post_w_dx run one-pass grids of 8 x 8 super-tiles only, which
n = 130 (two column tiles) cannot form: there the mirrored kernel is reached
through its stream-K entry (bo_post_w_split) and bo_ainv.
"""
import ctypes
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
NAN = float("nan")

# (n, output) -> the largest absolute error of the build before the skip (the table above)
TOL = {
    (16, "Rt"): 0.0, (16, "Spart"): 0.0, (16, "mpart"): 5.551e-17,
    (37, "Rt"): 0.0, (37, "Spart"): 1.388e-17, (37, "mpart"): 2.776e-16,
    (130, "Rt"): 0.0, (130, "Spart"): 2.776e-17, (130, "mpart"): 8.882e-16,
    (130, "Wt"): 4.441e-16, (130, "Ainv"): 0.0,
    (256, "Rt"): 5.357e-15, (256, "Spart"): 2.498e-15, (256, "mpart"): 1.574e-14,
    (300, "Rt"): 3.331e-15, (300, "Spart"): 1.860e-15, (300, "mpart"): 7.105e-15,
    (1024, "Rt"): 2.223e-15, (1024, "Spart"): 3.331e-16, (1024, "mpart"): 4.940e-15,
    (1024, "Cx"): 3.375e-14,
    (2048, "Rt"): 1.455e-14, (2048, "Spart"): 4.302e-15, (2048, "mpart"): 5.196e-14,
    (2048, "Wt"): 6.661e-15, (2048, "Ainv"): 8.527e-13, (2048, "dX"): 3.650e-13,
}
CAP_RTOL, CAP_ATOL = 1e-11, 2.5e-13


def _hartmann_cache(n, ls=0.35):
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


def _poison(M, lower):
    """A copy of the np x np operand with NaN in every 16 x 16 block strictly
    below (lower) or above the block diagonal."""
    nb = M.shape[0] // 16
    kb = torch.arange(nb, device=M.device).view(-1, 1)
    cb = torch.arange(nb, device=M.device).view(1, -1)
    mask = (kb > cb) if lower else (kb < cb)
    mask = mask.repeat_interleave(16, 0).repeat_interleave(16, 1)
    P = M.clone()
    P[mask] = NAN
    return P


def _kxt(cache, X):
    """The device's own K*x^T (np x nrows_pad) of X, as post_partials builds it."""
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    B, q, d = X.shape
    _, nrows_pad, _ = kernels.geometry(B, q, cache.n)
    st = kernels._stream(X.device)
    Xq = torch.empty(nrows_pad, 8, dtype=F64, device=X.device)
    check(lib().bo_prepare_rows(kernels._p(X.contiguous()), B, q, d, kernels._p(cache.lengthscale),
                                kernels._p(Xq), st), "prepare_rows")
    Kt = torch.empty(cache.np, nrows_pad, dtype=F64, device=X.device)
    check(lib().bo_post_kxt(cache.kind, kernels._p(Xq), B, q, d, kernels._p(cache.Xt_scaled), cache.n,
                            cache.outputscale, kernels._p(Kt), st), "post_kxt")
    return Kt


def _reference(cache, Kt):
    """R^T = U^T K*x^T and its column-tile partials on the host, fp64."""
    U, Kt = cache.U.cpu(), Kt.cpu()
    nC, nrows = cache.np // 128, Kt.shape[1]
    Rt = U.T @ Kt
    T = Rt.view(nC, 128, nrows // 16, 16)
    S = torch.einsum("xcra,xcrb->xrab", T, T)
    beta = torch.zeros(cache.np, dtype=F64)
    beta[: cache.n] = cache.beta.cpu()
    m = torch.einsum("xcr,xc->xr", Rt.view(nC, 128, nrows), beta.view(nC, 128))
    return {"Rt": Rt, "Spart": S, "mpart": m, "Kt": Kt}


@functools.lru_cache(maxsize=None)
def _problem(n, B, q):
    """One cache, one X, one host reference per shape, shared by every test."""
    cache = _hartmann_cache(n)
    g = torch.Generator().manual_seed(n + B)
    X = torch.rand(B, q, 6, generator=g, dtype=F64).to(DEV)
    ref = _reference(cache, _kxt(cache, X))
    bad = dataclasses.replace(cache, U=_poison(cache.U, lower=True),
                              Linv=_poison(cache.Linv, lower=False))
    return cache, bad, X, ref


def _check(n, name, got, ref, case, cap=None):
    got = got.detach().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{case} {name}: non-finite output"
    assert ref.abs().max() > 0, f"{case} {name}: trivial reference"
    err = (got - ref).abs()
    rtol, atol = cap if cap is not None else (CAP_RTOL, CAP_ATOL * max(1.0, n / 1024))
    over = (err / (atol + rtol * ref.abs())).max().item()
    print(f"[post_pipeline] n={n} {name} {case}: max|got-ref| = {err.max().item():.3e}  "
          f"max|ref| = {ref.abs().max().item():.3e}  of the cap = {over:.3f}")
    tol = 4.0 * max(TOL[(n, name)], 2.0 ** -53 * ref.abs().max().item())
    assert err.max().item() <= tol, f"{case} {name}: {err.max().item():.3e} > {tol:.3e}"
    assert over <= 1.0, f"{case} {name}: {over:.3f} x the project's bound"


def _row_major(pp):
    """R^T of a PostPartials as np x nrows_pad, whichever layout it was stored in."""
    if pp.Rt.dim() == 2:
        return pp.Rt
    blk = pp.Rt.view(-1, pp.nrows_pad // 16, 4, 4, 16)  # [kb][ib][k % 16 / 4][k % 4][i % 16]
    return blk.permute(0, 2, 3, 1, 4).reshape(-1, pp.nrows_pad)


# id, n, B, q, options: the smallest shape that reaches each schedule
CASES = [
    ("one_step", 16, 1, 1, {}),                  # one k-step
    ("ragged3", 37, 5, 3, {}),                   # three ragged steps
    ("two_tiles", 130, 9, 5, {}),                # second column tile, ragged diagonal block
    ("grouped", 1024, 64, 16, {"split": 0}),     # 8 x 8 super-tiles
    ("paired", 2048, 64, 16, {"split": 0}),      # reversed walk from inside the diagonal block
    ("split16", 300, 33, 16, {"split": 16}),     # one-step segments
    ("streamk", 300, 33, 16, {"split": -1}),
    ("cross", 1024, 64, 16, {"split": 0, "cross": 3}),
]


def _run(cache, X, opts, kxt, rt_layout=0):
    from botorch_amd import kernels
    o = dict(opts)
    cross = None
    if "cross" in o:
        g = torch.Generator().manual_seed(5)
        cross = torch.randn(o.pop("cross"), cache.n, generator=g, dtype=F64).to(DEV)
    if "split" not in o:  # the library's plan, held to the 128-tile kernel: one pass here
        assert kernels.split_plan(X.shape[0], X.shape[1], cache.n)[0] == 0
        o["small"] = False
    pp = kernels.post_partials(cache, X, store_R=True, kxt=kxt, rt_layout=rt_layout, cross=cross, **o)
    return pp, cross


def _layouts(opts):
    from botorch_amd import _lib
    one_pass = opts.get("split", 0) == 0 and "cross" not in opts
    return (_lib.RT_ROWMAJOR, _lib.RT_BLOCKED) if one_pass else (_lib.RT_ROWMAJOR,)


@pytest.mark.parametrize("kxt", [True, False], ids=["kxt", "eval"])
@pytest.mark.parametrize("case,n,B,q,opts", CASES, ids=[c[0] for c in CASES])
def test_post_partials_matches_host(case, n, B, q, opts, kxt):
    cache, _, X, ref = _problem(n, B, q)
    for layout in _layouts(opts):
        pp, cross = _run(cache, X, opts, kxt, layout)
        tag = f"{case} kxt={kxt} layout={layout}"
        _check(n, "Rt", _row_major(pp), ref["Rt"], tag)
        _check(n, "Spart", pp.Spart, ref["Spart"], tag)
        _check(n, "mpart", pp.mpart, ref["mpart"], tag)
        if cross is not None:
            assert pp.Cx is not None
            _check(n, "Cx", pp.Cx, cross.cpu() @ ref["Kt"][:n], tag)


@pytest.mark.parametrize("kxt", [True, False], ids=["kxt", "eval"])
@pytest.mark.parametrize("case,n,B,q,opts", CASES, ids=[c[0] for c in CASES])
def test_zero_blocks_of_u_are_never_multiplied(case, n, B, q, opts, kxt):
    cache, bad, X, _ = _problem(n, B, q)
    for layout in _layouts(opts):
        clean, _ = _run(cache, X, opts, kxt, layout)
        nan, _ = _run(bad, X, opts, kxt, layout)
        for name in ("Rt", "Spart", "mpart", "Cx"):
            a, b = getattr(clean, name), getattr(nan, name)
            if a is not None:
                assert torch.equal(a, b), f"{case} layout={layout}: {name} changed under the poisoned U"


@functools.lru_cache(maxsize=None)
def _members(n=256, B=176, q=16):
    caches = [_hartmann_cache(n, ls) for ls in (0.30, 0.35, 0.40)]
    X = torch.rand(B, q, 6, generator=torch.Generator().manual_seed(n + B), dtype=F64).to(DEV)
    refs = [_reference(c, _kxt(c, X)) for c in caches]
    bad = [dataclasses.replace(c, U=_poison(c.U, lower=True)) for c in caches]
    return caches, bad, X, refs


def _members_run(caches, X):
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    B, q, _ = X.shape
    we = ctypes.c_int64()
    check(lib().bo_post_members_work(len(caches), B, q, caches[0].n, ctypes.byref(we)), "members_work")
    assert we.value >= 0, "the member-batched stream-K plan should apply at this shape"
    return kernels._post_members_streamk(caches, X, True, we.value)


def test_members_match_host_and_skip():
    caches, bad, X, refs = _members()
    pps = _members_run(caches, X)
    for m, (pp, ref) in enumerate(zip(pps, refs)):
        for name in ("Rt", "Spart", "mpart"):
            _check(caches[0].n, name, getattr(pp, name), ref[name], f"member {m}")
    for pp, pn in zip(pps, _members_run(bad, X)):
        for name in ("Rt", "Spart", "mpart"):
            assert torch.equal(getattr(pp, name), getattr(pn, name)), f"{name} changed under the poisoned U"


# ---- the mirrored (lower k-range) kernels: U operand = L^-1 ------------------------
def _w_split(cache, pp):
    """W^T = L^-T R^T through the stream-K entry, whatever the library's plan."""
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    dev = pp.Rt.device
    Wt = torch.empty(cache.np, pp.nrows_pad, dtype=F64, device=dev)
    # one 128 x 128 partial tile per segment at the most: tiles + resident slots
    work = torch.empty((pp.nC * (pp.nrows_pad // 128) + 512) * 128 * 128, dtype=F64, device=dev)
    check(lib().bo_post_w_split(kernels._p(cache.Linv), cache.np, kernels._p(pp.Rt), pp.B, pp.q, cache.n,
                                kernels._p(Wt), kernels._p(work), kernels._stream(dev)), "post_w_split")
    return Wt


@pytest.mark.parametrize("n,B,q", [(130, 9, 5), (2048, 64, 16)])
def test_w_matches_host_and_skip(n, B, q):
    from botorch_amd import kernels
    cache, bad, X, _ = _problem(n, B, q)
    pp, _ = _run(cache, X, {"split": 0}, True)
    if n == 130:
        Wt, Wn = _w_split(cache, pp), _w_split(bad, pp)
    else:
        W, Wb = kernels.w_matrix(cache, pp, post_w=True), kernels.w_matrix(bad, pp, post_w=True)
        assert W.kmajor and Wb.kmajor  # bo_post_w, not the GEMM
        Wt, Wn = W.t, Wb.t
    ref = cache.Linv.cpu().T @ pp.Rt.cpu()
    # the bound of test_post_w_stream_k_matches_gemm
    _check(n, "Wt", Wt[:n], ref[:n], "post_w", cap=(1e-10, 1e-11 * max(1.0, n / 1024)))
    assert torch.equal(Wt, Wn), "W^T changed under the poisoned L^-1"


@pytest.mark.parametrize("n", [130, 2048])
def test_ainv_matches_host(n):
    from botorch_amd import kernels
    cache, _, _, _ = _problem(*{130: (130, 9, 5), 2048: (2048, 64, 16)}[n])
    Ai = kernels.ainv(cache).cpu()[:n, :n]
    Li = cache.Linv.cpu()
    ref = (Li.T @ Li)[:n, :n]
    tiles = torch.arange(n) // 128
    low = tiles.view(-1, 1) >= tiles.view(1, -1)  # the lower 128 x 128 tiles are written
    # the bound of test_ainv_lower_tiles
    _check(n, "Ainv", Ai[low], ref[low], "ainv", cap=(1e-10, 1e-10 * float(ref.abs().max())))


def test_post_w_dx_matches_autograd_and_skip():
    """bo_post_w_dx on its smallest one-pass grid at n = 2048 (16 x 64 paired
    tiles): dX of one t-batch per row tile against autograd through
    phi(X) = sum(D * Kx(X)) + ystd^2 sum(dcov * Kxx(X)), D = ystd dmean alpha^T
    - ystd^2 (dcov + dcov^T) W_b with W = R L^-1 from the device's R^T and L^-1
    multiplied on the host."""
    from botorch_amd import _lib, kernels
    n, B, q, ystd = 2048, 512, 16, 0.7
    cache = _problem(n, 64, 16)[0]
    bad = _problem(n, 64, 16)[1]
    g = torch.Generator().manual_seed(11)
    X = torch.rand(B, q, 6, generator=g, dtype=F64)
    dmean = torch.randn(B, q, generator=g, dtype=F64)
    dcov = torch.randn(B, q, q, generator=g, dtype=F64)
    pp = kernels.post_partials(cache, X.to(DEV), store_R=True, rt_layout=_lib.RT_BLOCKED)
    dX = kernels.post_w_dx(cache, pp, dmean.to(DEV), dcov.to(DEV), ystd)
    assert dX is not None, "the fused one-pass grid should apply here"
    dXn = kernels.post_w_dx(bad, pp, dmean.to(DEV), dcov.to(DEV), ystd)
    assert torch.equal(dX, dXn), "dX changed under the poisoned L^-1"

    sel = torch.tensor([8 * j + j % 8 for j in range(B // 8)])  # one t-batch per 128-row tile
    rows = (sel.view(-1, 1) * q + torch.arange(q).view(1, -1)).reshape(-1)  # Qp = q = 16
    R = _row_major(pp)[:, rows.to(DEV)].cpu().T                    # rows x np
    W = (R @ cache.Linv.cpu())[:, :n].view(len(sel), q, n)
    ls, alpha = cache.lengthscale.cpu(), cache.alpha.cpu()
    Xs = X[sel].clone().requires_grad_(True)
    pts = cache.Xt.cpu() / ls

    def k(a, b):
        diff = a.unsqueeze(-2) - b.unsqueeze(-3)
        return cache.outputscale * torch.exp(-0.5 * (diff * diff).sum(-1))

    D = ystd * dmean[sel].unsqueeze(-1) * alpha.view(1, 1, n) - ystd ** 2 * (dcov[sel] + dcov[sel].mT) @ W
    phi = (D * k(Xs / ls, pts)).sum() + ystd ** 2 * (dcov[sel] * k(Xs / ls, Xs / ls)).sum()
    (ref,) = torch.autograd.grad(phi, Xs)
    # the bound of test_gpu_backward_kernels: 1e-9 max|ref| + 1e-10
    _check(n, "dX", dX[sel.to(DEV)], ref, "post_w_dx", cap=(0.0, 1e-9 * float(ref.abs().max()) + 1e-10))
