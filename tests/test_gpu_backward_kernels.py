"""Each hand-written backward kernel, called directly through its
``botorch_amd.kernels`` wrapper, against CPU fp64 torch autograd through a
plain restatement of the operation it differentiates:

  bo_chol_backward                 torch.linalg.cholesky
  bo_qmc_backward                  mean + chol(Sigma) z (+ F) -> oracle qEI / qLogEI reductions
  bo_post_backward(_jobs)          sum(D * Kx(X)) + ystd^2 sum(dcov * Kxx(X)), the covariances
                                   written here from explicit scaled differences
  bo_kernel_grad                   sum(dK * K(X, Y)), the same covariance in the original scale
  bo_qehvi / bo_qehvi_backward     mean + L z (+ F) -> oracle qehvi_from_samples

The reference is never another route of the library.  Every output array is
compared whole under  max|got - ref| <= 1e-9 max|ref| + 1e-10  (the project's
bound for a kernel against torch), every case asserts that its reference is
non-trivial, and every comparison prints its measured deviation.

Cotangents are random and never all ones.  With three or more entries they
hold both signs and one exact 0.0; a pair holds both signs; a single entry
(B = 1) is one non-zero number -- a zero there would make the reference
trivial, and two entries cannot hold a zero and both signs at once.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
RTOL, ATOL = 1e-9, 1e-10
RBF, MATERN = 0, 1


# ---- CPU references and helpers ---------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k) + 1
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F64)


def _cotangent(g, *shape):
    """Random cotangent: mixed sign and one exact 0.0 (see the module docstring)."""
    c = _randn(g, *shape)
    v = c.view(-1)
    n = v.numel()
    if n == 1:
        v[0] = v[0].abs() + 0.25
        if torch.rand(1, generator=g).item() < 0.5:
            v[0] = -v[0]
    else:
        v[0] = v[0].abs() + 0.1
        v[n - 1] = -(v[n - 1].abs() + 0.1)
        if n >= 3:
            v[n // 2] = 0.0
    return c


def _pow2(q):
    Qp = 1
    while Qp < q:
        Qp *= 2
    return Qp


def _check(tag, name, got, ref, half_nonzero=False):
    """The comparison rule of this file; prints the measured deviation."""
    got = got.detach().cpu()
    ref = ref.detach()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    scale = ref.abs().max().item()
    dev = (got - ref).abs().max().item()
    nz = (ref != 0).double().mean().item()
    print(f"[{tag}] {name}: max|got-ref| = {dev:.3e}  max|ref| = {scale:.3e}  "
          f"rel = {dev / scale if scale > 0 else float('nan'):.3e}  nonzero = {nz:.2f}")
    assert scale > 0, f"{name}: trivial reference"
    if half_nonzero:
        assert nz >= 0.5, f"{name}: only {nz:.2f} of the reference is non-zero"
    assert dev <= RTOL * scale + ATOL, f"{name}: {dev:.3e} > {RTOL} * {scale:.3e} + {ATOL}"


def _sym(A):
    return 0.5 * (A + A.mT)


def _spd(g, B, q):
    M = _randn(g, B, q, q)
    return M @ M.mT / q + torch.eye(q, dtype=F64)


def _kernel_value(d2, kind):
    """RBF exp(-d2 / 2); Matern-5/2 (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r) with
    r = sqrt(max(d2, 1e-30)) as oracle/gp.py:55-67 (zero derivative at r = 0)."""
    if kind == RBF:
        return torch.exp(-0.5 * d2)
    r = d2.clamp_min(1e-30).sqrt()
    return (1 + math.sqrt(5) * r + 5.0 / 3.0 * r * r) * torch.exp(-math.sqrt(5) * r)


def _covar_direct(x1, x2, ls, kind, outputscale=1.0):
    """k(x1_a, x2_k) from explicit scaled differences (no quadratic expansion):
    d2 = sum(((x1_a - x2_k) / ell)^2)."""
    diff = (x1.unsqueeze(-2) - x2.unsqueeze(-3)) / ls
    return outputscale * _kernel_value((diff * diff).sum(-1), kind)


@pytest.mark.parametrize("kind", [RBF, MATERN])
def test_direct_covariance_matches_oracle_covar(kind):
    """The covariance the post_backward / kernel_grad references differentiate
    is the oracle's (quadratic-expansion) covariance to 1e-12."""
    from oracle.gp import covar
    g = _gen(7, kind)
    x1, x2 = _rand(g, 9, 5), _rand(g, 40, 5)
    ls = 0.3 + _rand(g, 5)
    got = _covar_direct(x1, x2, ls, kind, 1.7)
    ref = covar(x1, x2, ls, kind, 1.7)
    dev = (got - ref).abs().max().item()
    print(f"[reference] covar kind={kind}: max|direct - oracle| = {dev:.3e}")
    assert dev <= 1e-12


# ---- 1. bo_chol_backward ------------------------------------------------------------
def _chol_case(q, B):
    g = _gen(1, q, B)
    A = _spd(g, B, q).requires_grad_(True)
    L = torch.linalg.cholesky(A)
    dL = _cotangent(g, B, q, q).tril()
    (gA,) = torch.autograd.grad(L, A, dL)
    return L.detach(), dL, _sym(gA)


@pytest.mark.parametrize("B", [1, 300])
@pytest.mark.parametrize("q", [1, 2, 7, 15, 16, 17, 64])
def test_chol_backward_matches_autograd(q, B):
    """q <= 16: the small kernel (chol_backward_lds, shared with both
    qmc_backward kernels); 17 and 64: the edges of the 64 x 64 one."""
    from botorch_amd import kernels
    L, dL, ref = _chol_case(q, B)
    got = kernels.chol_backward(L.to(DEV), dL.to(DEV)).cpu()
    _check("bo_chol_backward", f"q={q} B={B} dA (symmetrised)", _sym(got), ref)


# ---- 2. bo_qmc_backward -------------------------------------------------------------
QEI, QNEI, QLOGEI, QLOGNEI = 1, 2, 4, 5


def _qmc_reference(mode, mean, Sigma, Z, dacq, best_f, best_f_s, F, fat):
    """autograd of the oracle's reduction of mean + chol(Sigma) z (+ F) w.r.t.
    mean, Sigma (and F): -> acq, dmean, dSigma (symmetrised), dF."""
    from oracle.acquisition import TAU_MAX, TAU_RELU, qei_from_samples, qlogei_from_samples
    mean = mean.clone().requires_grad_(True)
    Sigma = Sigma.clone().requires_grad_(True)
    leaves = [mean, Sigma]
    f = mean.unsqueeze(0) + torch.einsum("bij,sj->sbi", torch.linalg.cholesky(Sigma), Z)
    if F is not None:
        F = F.clone().requires_grad_(True)
        leaves.append(F)
        f = f + F
    if mode in (QEI, QNEI):
        bf = best_f if mode == QEI else best_f_s.view(-1, 1, 1)
        acq = qei_from_samples(f, bf)
    else:
        bf = best_f if mode == QLOGEI else best_f_s
        acq = qlogei_from_samples(f, bf, fat=bool(fat), tau_relu=TAU_RELU, tau_max=TAU_MAX)
    grads = torch.autograd.grad(acq, leaves, dacq)
    return acq.detach(), grads[0], _sym(grads[1]), (grads[2] if F is not None else None)


def _qmc_case(mode, q, S, B, fat=1):
    g = _gen(2, mode, q, S, B, fat)
    Qp = _pow2(q)
    mean = 0.3 * _randn(g, B, q)
    Sigma = _spd(g, B, q)
    Z = _randn(g, S, q)
    dacq = _cotangent(g, B)
    # below the typical maximum of the q samples, so most samples improve
    best_f = -0.75 if q == 1 else -0.25
    best_f_s, Fk, F = None, None, None
    if mode in (QNEI, QLOGNEI):
        best_f_s = best_f + 0.3 * _randn(g, S)
        ldF = B * Qp + 5                      # ldF > B * Qp; padding holds values never to be read
        Fk = 0.3 * _randn(g, S, ldF)
        F = Fk[:, : B * Qp].reshape(S, B, Qp)[:, :, :q].clone()
    acq, dmean, dcov, dF = _qmc_reference(mode, mean, Sigma, Z, dacq, best_f, best_f_s, F, fat)
    dFk = None
    if dF is not None:
        dFk = torch.zeros(S, ldF, dtype=F64)
        dFk[:, : B * Qp].view(S, B, Qp)[:, :, :q] = dF
    return dict(mean=mean, L=torch.linalg.cholesky(Sigma).contiguous(), Z=Z, dacq=dacq, best_f=best_f,
                best_f_s=best_f_s, Fk=Fk, acq=acq, dmean=dmean, dcov=dcov, dFk=dFk, Qp=Qp)


def _run_qmc_backward(mode, c, fat=1):
    from botorch_amd import kernels
    from oracle.acquisition import TAU_MAX, TAU_RELU
    dv = lambda t: t.to(DEV) if t is not None else None  # noqa: E731
    log = mode in (QLOGEI, QLOGNEI)
    out = kernels.qmc_backward(mode, dv(c["mean"]), dv(c["L"]), dv(c["Z"]), dv(c["dacq"]),
                               best_f=c["best_f"], best_f_s=dv(c["best_f_s"]), F=dv(c["Fk"]),
                               acq_fwd=dv(c["acq"]) if log else None,
                               log_params=(fat, TAU_RELU, TAU_MAX) if log else None)
    return [o.cpu() for o in out]


def _check_qmc(tag, c, out, half_nonzero, half_nonzero_dcov=None):
    B, q = c["mean"].shape
    if half_nonzero_dcov is None:
        half_nonzero_dcov = half_nonzero
    _check("bo_qmc_backward", f"{tag} dmean", out[0], c["dmean"], half_nonzero)
    _check("bo_qmc_backward", f"{tag} dcov (symmetrised)", _sym(out[1]), c["dcov"], half_nonzero_dcov)
    # the header calls dcov symmetric
    _check("bo_qmc_backward", f"{tag} dcov^T vs dcov", out[1].mT, out[1])
    if c["dFk"] is not None:
        _check("bo_qmc_backward", f"{tag} dF", out[2], c["dFk"])
        pad = torch.ones_like(out[2], dtype=torch.bool)
        pad[:, : B * c["Qp"]].view(-1, B, c["Qp"])[:, :, :q] = False
        assert (out[2][pad] == 0).all(), "dF: padding columns written"


# (q, S, B): S in {1, 5, 256, 257, 600} crosses the SMAX = 256 sample chunk
@pytest.mark.parametrize("q,S,B", [(1, 1, 1), (3, 5, 70), (5, 256, 1), (16, 257, 70), (16, 600, 1),
                                   (5, 600, 70)])
def test_qmc_backward_qei(q, S, B):
    c = _qmc_case(QEI, q, S, B)
    _check_qmc(f"QEI q={q} S={S} B={B}", c, _run_qmc_backward(QEI, c), True)


@pytest.mark.parametrize("q,S,B", [(1, 5, 70), (3, 257, 70), (5, 600, 1), (16, 256, 70), (1, 1, 1),
                                   (5, 5, 70)])
def test_qmc_backward_qnei(q, S, B):
    """Per-sample best_f_s, F with ldF > B Qp; dF compared whole, its padding
    columns (q = 3: Qp = 4, q = 5: Qp = 8) exactly 0."""
    c = _qmc_case(QNEI, q, S, B)
    _check_qmc(f"QNEI q={q} S={S} B={B}", c, _run_qmc_backward(QNEI, c), True)


@pytest.mark.parametrize("q,S,B,fat", [(1, 1, 1, 0), (3, 5, 70, 1), (5, 257, 1, 0), (16, 600, 70, 1),
                                       (5, 256, 70, 0), (16, 5, 1, 1)])
def test_qmc_backward_qlogei(q, S, B, fat):
    """acq_fwd is the CPU reference's forward value, so the backward is isolated."""
    c = _qmc_case(QLOGEI, q, S, B, fat)
    _check_qmc(f"QLOGEI fat={fat} q={q} S={S} B={B}", c, _run_qmc_backward(QLOGEI, c, fat), False)


@pytest.mark.parametrize("q,S,B,fat", [(1, 5, 1, 1), (3, 256, 70, 0), (5, 600, 1, 1), (16, 257, 70, 0),
                                       (3, 1, 70, 1), (5, 5, 70, 0)])
def test_qmc_backward_qlognei(q, S, B, fat):
    c = _qmc_case(QLOGNEI, q, S, B, fat)
    _check_qmc(f"QLOGNEI fat={fat} q={q} S={S} B={B}", c, _run_qmc_backward(QLOGNEI, c, fat), False)


def test_qmc_backward_takes_column_major_factor():
    """torch.linalg.cholesky returns each factor column-major; the wrapper hands
    the kernel row-major operands whatever the strides of its arguments."""
    c = _qmc_case(QEI, 5, 256, 1)
    Lc = c["L"].mT.contiguous().mT
    assert not Lc.is_contiguous() and torch.equal(Lc, c["L"])
    c["L"] = Lc
    _check_qmc("QEI q=5 S=256 B=1 column-major L", c, _run_qmc_backward(QEI, c), True)


def test_qmc_backward_ties_and_exact_zeros():
    """torch semantics on one deterministic input (q = 3, S = 4, B = 1,
    best_f = 0): amax splits its gradient evenly over ALL maximal entries after
    the clamp, clamp_min(0) passes it where the value is >= 0.  Samples
    f = mean + L z:
      z = (1, 0, 0)      -> (1, 1, -1):      two-way tie at 1        -> (1/2, 1/2, 0)
      z = (0, 0, 0)      -> (0, 0, -1):      clamped (0, 0, 0), three maximal entries,
                                              two of them pass        -> (1/3, 1/3, 0)
      z = (-1, 0, 0)     -> (-1, -1, -1):    none passes             -> (0, 0, 0)
      z = (.5, .25, 0)   -> (.5, .75, -1):   no tie                  -> (0, 1, 0)
    so dmean = dacq / 4 * (5/6, 11/6, 0)."""
    mean = torch.tensor([[0.0, 0.0, -1.0]], dtype=F64)
    L = torch.tensor([[[1.0, 0, 0], [1.0, 1.0, 0], [0, 0, 1.0]]], dtype=F64)
    Z = torch.tensor([[1.0, 0, 0], [0, 0, 0], [-1.0, 0, 0], [0.5, 0.25, 0]], dtype=F64)
    dacq = torch.tensor([-0.75], dtype=F64)
    Sigma = L @ L.mT
    assert torch.equal(torch.linalg.cholesky(Sigma), L)  # the reference sees the same ties
    acq, dmean, dcov, _ = _qmc_reference(QEI, mean, Sigma, Z, dacq, 0.0, None, None, 1)
    c = dict(mean=mean, L=L, Z=Z, dacq=dacq, best_f=0.0, best_f_s=None, Fk=None, acq=acq,
             dmean=dmean, dcov=dcov, dFk=None, Qp=4)
    out = _run_qmc_backward(QEI, c)
    # dmean has 2 of 3 entries non-zero; the third point never wins, so row and
    # column 2 of dcov are zero (4 of 9 entries non-zero)
    _check_qmc("QEI ties", c, out, True, False)
    hand = dacq.item() / 4 * torch.tensor([[5.0 / 6.0, 11.0 / 6.0, 0.0]], dtype=F64)
    _check("bo_qmc_backward", "QEI ties reference dmean vs hand values", dmean, hand)
    _check("bo_qmc_backward", "QEI ties dmean vs hand values", out[0], hand)
    assert out[0][0, 2].item() == 0.0


# ---- 3. bo_post_backward --------------------------------------------------------------
YSTD = 0.7
OUTPUTSCALE = 1.3


def _gp(kind, d, n, seed=0):
    """(device cache, CPU lengthscale, CPU training inputs) of an n-point GP."""
    from botorch_amd import kernels
    g = _gen(3, kind, d, n, seed)
    Xt = _rand(g, n, d)
    y = _randn(g, n)
    ls = 0.3 + 0.4 * _rand(g, d)
    cache = kernels.build_gp_cache(Xt.to(DEV), y.to(DEV), ls.to(DEV), 1e-2, 0.1, kind=kind,
                                   outputscale=OUTPUTSCALE)
    return cache, ls, Xt


def _post_reference(kind, X, ls, pts_scaled, alpha, W, dmean, dcov, E, Qp):
    """dX of phi(X) = sum(D * Kx(X)) + ystd^2 sum(dcov * Kxx(X)) with the
    cotangents held constant, D = ystd dmean alpha^T - ystd^2 (dcov + dcov^T) W_b
    + E (include/botorch_amd.h, bo_post_backward).  pts_scaled: the training (or
    other) points divided by the lengthscale, n x d.  W, E: nrows_pad x n, rows
    b * Qp + a."""
    B, q, d = X.shape
    n = pts_scaled.shape[0]
    rows = lambda M: M[: B * Qp].view(B, Qp, n)[:, :q]  # noqa: E731
    X = X.clone().requires_grad_(True)
    one = torch.ones(d, dtype=F64)
    Kx = _covar_direct(X / ls, pts_scaled, one, kind, OUTPUTSCALE)      # B x q x n
    D = torch.zeros(B, q, n, dtype=F64)
    if dmean is not None:
        D = D + YSTD * dmean.unsqueeze(-1) * alpha.view(1, 1, n)
    if dcov is not None and W is not None:
        D = D - YSTD ** 2 * (dcov + dcov.mT) @ rows(W)
    if E is not None:
        D = D + rows(E)
    phi = (D * Kx).sum()
    if dcov is not None:
        Kxx = _covar_direct(X / ls, X / ls, one, kind, OUTPUTSCALE)   # B x q x q
        phi = phi + YSTD ** 2 * (dcov * Kxx).sum()
    (gX,) = torch.autograd.grad(phi, X)
    return gX


# kind, d, q, n, B, terms, accumulate, W k-major
#   (7, 3): fewer than 16 points; (128, 2): one chunk, no split; (129, 2): two
#   splits, the second of one point; (1000, 3): 8 splits, the last ragged;
#   (300, 300): B >= 256, one pass.  d = 6 alone takes the ND = 6 instantiation.
POST_CASES = [
    (RBF, 1, 1, 7, 3, "all", False, False),
    (MATERN, 3, 5, 128, 2, "dmean", False, False),
    (RBF, 6, 16, 129, 2, "dcov", False, True),
    (MATERN, 8, 5, 1000, 3, "all", True, True),
    (RBF, 3, 5, 300, 300, "all", True, False),
    (MATERN, 6, 16, 129, 2, "E", False, False),
    (RBF, 8, 16, 1000, 3, "all", False, False),
    (MATERN, 1, 1, 128, 2, "all", False, True),
    (MATERN, 6, 16, 300, 300, "dcov", False, True),
]


@pytest.mark.parametrize("kind,d,q,n,B,terms,accumulate,kmajor", POST_CASES)
def test_post_backward_matches_formula(kind, d, q, n, B, terms, accumulate, kmajor):
    """Random W, E, dmean and a non-symmetric dcov; each term alone and all
    together; `accumulate` on a pre-filled dX in a split and an unsplit case."""
    from botorch_amd import kernels
    cache, ls, Xt = _gp(kind, d, n)
    g = _gen(4, kind, d, q, n, B)
    X = _rand(g, B, q, d)
    pp = kernels.post_partials(cache, X.to(DEV), store_R=True)
    Qp, nrows = pp.Qp, pp.nrows_pad
    assert Qp == _pow2(q)
    W = _randn(g, nrows, n) if terms in ("all", "dcov") else None
    dcov = _cotangent(g, B, q, q) if terms in ("all", "dcov") else None
    dmean = _cotangent(g, B, q) if terms in ("all", "dmean") else None
    E = _randn(g, nrows, n) if terms in ("all", "E") else None
    alpha = cache.alpha.cpu()
    ref = _post_reference(kind, X, ls, Xt / ls, alpha, W, dmean, dcov, E, Qp)
    dv = lambda t: t.to(DEV) if t is not None else None  # noqa: E731
    Wm = None
    if W is not None:
        Wm = kernels.WMat(W.T.contiguous().to(DEV), True) if kmajor else kernels.WMat(W.to(DEV), False)
    dX0 = _randn(g, B, q, d) if accumulate else None
    got = kernels.post_backward(cache, pp, Wm, dv(dmean), dv(dcov), YSTD, E=dv(E),
                                dX=dX0.clone().to(DEV) if accumulate else None)
    if accumulate:
        _check("bo_post_backward", f"kind={kind} d={d} q={q} n={n} B={B} {terms} accumulated - prefill",
               got.cpu() - dX0, ref)
        ref = ref + dX0
    _check("bo_post_backward", f"kind={kind} d={d} q={q} n={n} B={B} {terms} acc={accumulate} dX",
           got, ref)


def _other_points(g, d, r=40):
    from botorch_amd import kernels
    Xo = torch.zeros(r, kernels.DP, dtype=F64)
    Xo[:, :d] = 3.0 * _rand(g, r, d)   # scaled coordinates (the unit box over ell ~ 1/3)
    return Xo


@pytest.mark.parametrize("kind,d,q,B", [(RBF, 6, 5, 3), (MATERN, 3, 16, 2)])
def test_post_backward_other_points(kind, d, q, B):
    """Xt_scaled = 40 other (scaled) points, only E, no alpha: the gradient
    through K(points, X) (the qNEI baseline pass)."""
    from botorch_amd import kernels
    cache, ls, _ = _gp(kind, d, 64)
    g = _gen(5, kind, d, q, B)
    X = _rand(g, B, q, d)
    pp = kernels.post_partials(cache, X.to(DEV), store_R=True)
    Xo = _other_points(g, d)
    r = Xo.shape[0]
    E = _cotangent(g, pp.nrows_pad, r)
    ref = _post_reference(kind, X, ls, Xo[:, :d], None, None, None, None, E, pp.Qp)
    got = kernels.post_backward(cache, pp, None, None, None, YSTD, E=E.to(DEV),
                                Xt_scaled=Xo.to(DEV), n=r)
    _check("bo_post_backward", f"other points kind={kind} d={d} q={q} B={B} dX", got, ref)


@pytest.mark.parametrize("kind", [RBF, MATERN])
def test_post_backward_jobs_matches_formula(kind):
    """Two jobs (a training pass with every term, a baseline pass over other
    points) in one launch against the sum of the two references."""
    from botorch_amd import kernels
    n, B, q, d = 300, 5, 4, 6
    cache, ls, Xt = _gp(kind, d, n)
    g = _gen(6, kind)
    X = _rand(g, B, q, d)
    pp = kernels.post_partials(cache, X.to(DEV), store_R=True)
    W, E = _randn(g, pp.nrows_pad, n), _randn(g, pp.nrows_pad, n)
    dmean, dcov = _cotangent(g, B, q), _cotangent(g, B, q, q)
    Xo = _other_points(g, d)
    r = Xo.shape[0]
    Eo = _cotangent(g, pp.nrows_pad, r)
    ref = (_post_reference(kind, X, ls, Xt / ls, cache.alpha.cpu(), W, dmean, dcov, E, pp.Qp)
           + _post_reference(kind, X, ls, Xo[:, :d], None, None, None, None, Eo, pp.Qp))
    jobs = [dict(cache=cache, pp=pp, W=kernels.WMat(W.to(DEV), False), dmean=dmean.to(DEV),
                 dcov=dcov.to(DEV), ystd=YSTD, E=E.to(DEV)),
            dict(cache=cache, pp=pp, ystd=YSTD, E=Eo.to(DEV), Xt_scaled=Xo.to(DEV), n=r)]
    got = kernels.post_backward_jobs(jobs)
    _check("bo_post_backward_jobs", f"kind={kind} n={n} B={B} q={q} dX", got, ref)


# ---- 4. bo_kernel_grad ------------------------------------------------------------------
def _kernel_grad_reference(kind, X, Y, ls, outputscale, dK):
    """dX of phi = sum(dK * K(X, Y)), inputs in the original scale."""
    X = X.clone().requires_grad_(True)
    (gX,) = torch.autograd.grad((dK * _covar_direct(X, Y, ls, kind, outputscale)).sum(), X)
    return gX


def _kernel_grad_inputs(g, rows, n, d):
    X, Y = _rand(g, rows, d), _rand(g, n, d)
    # d2 = sum(((x - y) / ell)^2) ~ d / (6 ell^2): ell ~ sqrt(d) keeps k away from 0
    ls = math.sqrt(d) * (0.3 + 0.3 * _rand(g, d))
    return X, Y, ls


# n in {1023, 1025, 2500} crosses the CH = 1024 point chunk
@pytest.mark.parametrize("kind,d,n,accumulate", [
    (RBF, 1, 1, False), (MATERN, 50, 1023, False), (RBF, 128, 1025, False),
    (MATERN, 128, 2500, True), (RBF, 50, 2500, True), (MATERN, 1, 1025, False),
    (MATERN, 50, 1, True), (RBF, 128, 1023, False)])
def test_kernel_grad_matches_autograd(kind, d, n, accumulate):
    from botorch_amd import kernels
    rows = 5
    g = _gen(8, kind, d, n)
    X, Y, ls = _kernel_grad_inputs(g, rows, n, d)
    dK = _cotangent(g, rows, n)
    ref = _kernel_grad_reference(kind, X, Y, ls, 1.7, dK)
    dX0 = _randn(g, rows, d) if accumulate else None
    got = kernels.kernel_grad(X.to(DEV), Y.to(DEV), dK.to(DEV), ls.to(DEV), kind, outputscale=1.7,
                              dX=dX0.clone().to(DEV) if accumulate else None)
    if accumulate:
        _check("bo_kernel_grad", f"kind={kind} d={d} n={n} accumulated - prefill", got.cpu() - dX0, ref)
        ref = ref + dX0
    _check("bo_kernel_grad", f"kind={kind} d={d} n={n} acc={accumulate} dX", got, ref)


@pytest.mark.parametrize("kind,d,accumulate", [(RBF, 50, True), (MATERN, 128, False), (MATERN, 1, True)])
def test_kernel_grad_group(kind, d, accumulate):
    """group = 3, rows = 12: row i pairs with the 3 rows of its own block of Y
    (dK has 3 columns) and its self pair (column i % 3) contributes nothing --
    Y differs from X here, so a self pair that did contribute would show."""
    from botorch_amd import kernels
    rows, group = 12, 3
    g = _gen(9, kind, d)
    X, Y, ls = _kernel_grad_inputs(g, rows, rows, d)
    dK = _cotangent(g, rows, group)
    Xr = X.clone().requires_grad_(True)
    Kb = _covar_direct(Xr.view(rows // group, group, d), Y.view(rows // group, group, d), ls, kind, 0.8)
    mask = 1.0 - torch.eye(group, dtype=F64)
    (ref,) = torch.autograd.grad((dK.view(rows // group, group, group) * mask * Kb).sum(), Xr)
    dX0 = _randn(g, rows, d) if accumulate else None
    got = kernels.kernel_grad(X.to(DEV), Y.to(DEV), dK.to(DEV), ls.to(DEV), kind, outputscale=0.8,
                              group=group, dX=dX0.clone().to(DEV) if accumulate else None)
    if accumulate:
        ref = ref + dX0
    _check("bo_kernel_grad", f"group=3 kind={kind} d={d} acc={accumulate} dX", got, ref)


def test_kernel_grad_matern_coincident_pair():
    """X[0] == Y[4] exactly under Matern-5/2: the derivative at zero distance
    is 0, so the result is finite and equals the reference with that pair's dK
    set to 0."""
    from botorch_amd import kernels
    rows, n, d = 5, 9, 50
    g = _gen(10)
    X, Y, ls = _kernel_grad_inputs(g, rows, n, d)
    Y[4] = X[0]
    dK = _cotangent(g, rows, n)
    dK[0, 4] = 2.5
    dK0 = dK.clone()
    dK0[0, 4] = 0.0
    ref = _kernel_grad_reference(MATERN, X, Y, ls, 1.7, dK0)
    got = kernels.kernel_grad(X.to(DEV), Y.to(DEV), dK.to(DEV), ls.to(DEV), MATERN, outputscale=1.7)
    _check("bo_kernel_grad", "Matern coincident pair dX", got, ref)


# ---- 5. bo_qehvi / bo_qehvi_backward --------------------------------------------------
def _qehvi_case(m, q, S, B, K, per_sample=False, with_F=False):
    """Inputs (mean, L, Z, cells[, F]) and the reference value and gradients:
    f = mean + L z (+ F) -> oracle.acquisition.qehvi_from_samples, autograd
    w.r.t. mean, L (and F) with a random dacq."""
    from oracle.acquisition import qehvi_from_samples
    g = _gen(11, m, q, S, B, K, per_sample, with_F)
    mean = (0.5 * _randn(g, m, B, q)).requires_grad_(True)
    L = (0.3 * _randn(g, m, B, q, q).tril() + torch.eye(q, dtype=F64)).requires_grad_(True)
    Z = _randn(g, S, q * m)
    cshape = (S, K, m) if per_sample else (K, m)
    lo = -2.0 * _rand(g, *cshape)
    hi = lo + 2.0 * _rand(g, *cshape)
    dacq = _cotangent(g, B)
    leaves = [mean, L]
    f = mean.permute(1, 2, 0).unsqueeze(0) + torch.einsum("tbpj,sjt->sbpt", L, Z.view(S, q, m))
    Fk, Qp = None, 0
    if with_F:
        Qp = _pow2(q)
        ldF = B * Qp + 3                      # ldF > B Qp
        Fk = (0.3 * _randn(g, m, S, ldF)).requires_grad_(True)
        leaves.append(Fk)
        f = f + Fk[:, :, : B * Qp].view(m, S, B, Qp)[..., :q].permute(1, 2, 3, 0)
    if per_sample:
        acq = torch.stack([qehvi_from_samples(f[s:s + 1], lo[s], hi[s]) for s in range(S)]).mean(0)
    else:
        acq = qehvi_from_samples(f, lo, hi)
    grads = torch.autograd.grad(acq, leaves, dacq)
    return dict(mean=mean.detach(), L=L.detach(), Z=Z, lo=lo, hi=hi, dacq=dacq,
                Fk=Fk.detach() if with_F else None, Qp=Qp, acq=acq.detach(), dmean=grads[0],
                dL=grads[1], dF=grads[2] if with_F else None)


# m, q, S, B, K, per-sample cells, F
QEHVI_CASES = [
    (4, 12, 16, 2, 16, False, False),    # m = 4 with the q <= 12 bucket, sample split
    (4, 5, 24, 3, 20, False, False),     # m = 4, q <= 8 bucket
    (4, 2, 16, 2, 300, False, False),    # m = 4, cells not in LDS (K m > 1024)
    (2, 12, 32, 3, 40, False, False),    # q <= 12 bucket, m = 2
    (3, 9, 16, 2, 30, False, False),     # q <= 12 bucket, m = 3
    (2, 3, 16, 2, 600, False, False),    # shared cells from global memory
    (3, 2, 3, 1, 8, False, False),       # S smaller than the split (H = min(8, S))
    (2, 2, 8, 300, 4, False, False),     # no split in the backward (B >= 256)
    (2, 2, 8, 1100, 4, False, False),    # no split in the forward either (1024 / B = 0)
    (3, 4, 16, 2, 10, True, False),      # cell_stride > 0
    (3, 4, 16, 2, 10, True, True),       # cell_stride > 0 with F (Qp = 4, ldF > B Qp)
]


@pytest.mark.parametrize("m,q,S,B,K,per_sample,with_F", QEHVI_CASES)
def test_qehvi_value_and_backward(m, q, S, B, K, per_sample, with_F):
    from botorch_amd import kernels
    c = _qehvi_case(m, q, S, B, K, per_sample, with_F)
    dv = lambda t: t.to(DEV) if t is not None else None  # noqa: E731
    args = [dv(c[k]) for k in ("mean", "L", "Z", "lo", "hi")]
    tag = f"m={m} q={q} S={S} B={B} K={K}" + (" per-sample" if per_sample else "") + (" F" if with_F else "")
    acq = kernels.qehvi(*args, F=dv(c["Fk"]), Qp=c["Qp"])
    _check("bo_qehvi", f"{tag} acq", acq, c["acq"], True)
    out = kernels.qehvi_backward(*args, dv(c["dacq"]), F=dv(c["Fk"]), Qp=c["Qp"])
    low = torch.ones(q, q, dtype=torch.bool).tril()
    _check("bo_qehvi_backward", f"{tag} dmean", out[0], c["dmean"], True)
    dL = out[1].cpu()
    _check("bo_qehvi_backward", f"{tag} dL (lower)", dL[..., low], c["dL"][..., low], True)
    assert (dL[..., ~low] == 0).all(), "dL: strict upper triangle not zero"
    if with_F:
        _check("bo_qehvi_backward", f"{tag} dF", out[2], c["dF"])
