"""The device Cholesky family against the extended-precision reference of
chol_restatement.py: bo_cholesky_inverse (the persistent task DAG of
csrc/chol_dag.hip), chol_small_kernel (bo_chol_small, q <= 64) and
bo_cholesky_jitter (the ladder around the DAG).

The bound.  For each metric m (omega, eta, fwd of L; both inverse residuals and
fwd of L^{-1}) the test measures m_dev of the device result and m_ref of
LAPACK on the CPU (torch.linalg.cholesky, solve_triangular of its factor) on
the same matrix, both against the longdouble reference, and asserts

    m_dev <= R max(m_ref, u),   u = 2^-53,   R = 16

(R lives in chol_restatement.py; DESIGN.md section 4 has the measured ratios it
was set from).  Independently of R, omega <= 2 (n + 1) u: Higham's Theorem 10.3
holds for any summation order, the factor 2 allows for the few-ulp square root
piv * rsq(piv).  Every figure is printed before it is asserted (pytest -s).

The cases come from chol_restatement.py; test_chol_restatement_cpu.py shows on
the host that each is well posed, so none is skipped here on numerical
grounds.  The two orders 64 T - 1 with T = 6 and T = 4 (383, 255) are the
smallest at which the DAG's queue holds a batched column update / inverse
step; both are below 1024 and take every metric."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests import chol_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FACTOR_KEYS = ("omega", "eta", "fwd")


def _reference_of(A, inverse=True):
    """(Lx, Xx, LAPACK's metrics) of one f64 matrix."""
    Lx, info = R.ext_cholesky(A)
    assert info == 0
    Lt = torch.linalg.cholesky(R.tensor(A))
    ref = R.factor_metrics(A, Lt, Lx)
    Xx = None
    if inverse:
        Xx = R.ext_tri_inverse(Lx)
        Xt = torch.linalg.solve_triangular(Lt, torch.eye(A.shape[0], dtype=torch.float64),
                                           upper=False)
        ref.update(R.inverse_metrics(Lt, Xt, Xx))
    return Lx, Xx, ref


@functools.lru_cache(maxsize=None)
def _reference(family, n):
    return _reference_of(R.matrix(family, n))


def _shape_ok(M):
    """Strictly upper part exactly zero, diagonal positive."""
    M = M.cpu()
    assert torch.equal(M.triu(1), torch.zeros_like(M))
    assert (M.diagonal() > 0).all()
    return M


def _hold(label, dev, ref, n=None):
    """m_dev <= R max(m_ref, u) for every metric of dev; all figures printed
    first, all misses reported together."""
    missed = []
    for key, m_dev in dev.items():
        m_ref = max(ref[key], R.U)
        print(f"RATIO {label} {key} dev={m_dev:.3e} ref={ref[key]:.3e} ratio={m_dev / m_ref:.2f}")
        if not m_dev <= R.R * m_ref:
            missed.append((key, m_dev, ref[key]))
    if n is not None and not dev["omega"] <= 2 * (n + 1) * R.U:
        missed.append(("omega ceiling", dev["omega"], 2 * (n + 1) * R.U))
    assert not missed, (label, missed)


def _check_factor(label, A, L, Lx, ref, Linv=None, Xx=None):
    L = _shape_ok(L)
    dev = R.factor_metrics(A, L, Lx)
    if Linv is not None:
        dev.update(R.inverse_metrics(L, _shape_ok(Linv), Xx))
    _hold(label, dev, ref, A.shape[0])


# ---- (a) the DAG ----------------------------------------------------------------

@pytest.mark.parametrize("c", R.DAG_CASES, ids=R.case_id)
def test_dag_factor_and_inverse(c):
    """The clustered cases are the ones that found the tile solves' missing
    refinement step: with L_ik = A_ik D_k^T alone, omega
    at n = 129, 193, 385 was 44, 65, 52 times LAPACK's, where the twins' small
    pivots share a diagonal tile."""
    from botorch_amd import kernels
    A = R.matrix(c.family, c.n)
    L, Linv, info = kernels.cholesky_inverse(R.tensor(A).to(DEV))
    assert info == 0
    Lx, Xx, ref = _reference(c.family, c.n)
    _check_factor(R.case_id(c), A, L, Lx, ref, Linv, Xx)


# ---- (b) padding and complete writes ----------------------------------------------

@pytest.mark.parametrize("n", R.PAD_ORDERS)
def test_padding_and_complete_writes(n):
    """bo_cholesky_inverse writes all of Linv (NaN before the call) and leaves
    both buffers lower triangular with the identity in rows and columns >= n,
    bit for bit: post_partials reads U = Linv^T over all np columns."""
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    A = R.tensor(R.matrix("gp_rbf", n))
    np_ = kernels.padded_order(n)
    W = torch.eye(np_, dtype=torch.float64)
    W[:n, :n] = torch.tril(A)
    W = W.to(DEV)
    Linv = torch.full((np_, np_), float("nan"), dtype=torch.float64, device=DEV)
    work = torch.empty_like(W)
    info = torch.zeros(1, dtype=torch.int32, device=DEV)
    P = kernels._p
    check(lib().bo_cholesky_inverse(P(W), P(Linv), P(work), np_, P(info),
                                    kernels._stream(torch.device(DEV))), "chol")
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    W, Linv = W.cpu(), Linv.cpu()
    eye = torch.eye(np_, dtype=torch.float64)
    for M in (W, Linv):
        assert not torch.isnan(M).any()
        assert torch.equal(M.triu(1), torch.zeros_like(M))
        assert torch.equal(M[n:, :], eye[n:, :]) and torch.equal(M[:, n:], eye[:, n:])


def test_cache_U_is_Linv_transposed():
    from botorch_amd import kernels
    X, y, ls, noise = R.cache_inputs()
    c = kernels.build_gp_cache(X.to(DEV), y.to(DEV), torch.full((6,), ls, dtype=torch.float64,
                                                               device=DEV), noise, 0.0)
    assert c.jitter == 0.0
    assert c.U.shape == (c.np, c.np) and torch.equal(c.U, c.Linv.T)


# ---- (c) failure reporting ------------------------------------------------------------

def _next_call_is_right():
    """The counters are re-zeroed: a good matrix factors after a failed call."""
    from botorch_amd import kernels
    A = R.tensor(R.matrix("gp_rbf", 193))
    L, _, info = kernels.cholesky_inverse(A.to(DEV))
    assert info == 0
    Lr = torch.linalg.cholesky(A)
    assert (L.cpu() - Lr).abs().max() < 1e-12 * Lr.abs().max()


@pytest.mark.parametrize("n,p", R.FAIL_CASES)
def test_info_of_a_failing_minor(n, p):
    from botorch_amd import kernels
    B = R.tensor(R.fail_at(n, p))
    _, _, info = kernels.cholesky_inverse(B.to(DEV))
    assert info == p + 1
    assert info == int(torch.linalg.cholesky_ex(B)[1])
    _next_call_is_right()


@pytest.mark.parametrize("p", R.NAN_DIAG)
def test_nan_pivot_fails_at_its_own_column(p):
    from botorch_amd import kernels
    A = R.tensor(R.matrix("gp_rbf", 193))
    A[p, p] = float("nan")
    _, _, info = kernels.cholesky_inverse(A.to(DEV))
    assert info == p + 1
    _next_call_is_right()


def test_nan_off_the_diagonal_fails_at_its_row():
    """A[i, j] = nan, i > j, reaches no pivot before the i-th, in any order of
    the updates."""
    from botorch_amd import kernels
    i, j = R.NAN_OFF
    A = R.tensor(R.matrix("gp_rbf", 193))
    A[i, j] = A[j, i] = float("nan")
    _, _, info = kernels.cholesky_inverse(A.to(DEV))
    assert info == i + 1
    _next_call_is_right()


# ---- (d) scale invariance ---------------------------------------------------------------

@pytest.mark.parametrize("e", [100, -100])
def test_scale_invariance(e):
    """4^e A is exact in f64 and its factor is 2^e L: the scaled-back device
    factor holds the unscaled bounds (no absolute threshold, no denormal
    shortcut on the pivot path)."""
    from botorch_amd import kernels
    A = R.matrix(*R.SCALE_CASE)
    L, Linv, info = kernels.cholesky_inverse((R.tensor(A) * 4.0 ** e).to(DEV))
    assert info == 0
    Lx, Xx, ref = _reference(*R.SCALE_CASE)
    _check_factor(f"scale4^{e}", A, L / 2.0 ** e, Lx, ref, Linv * 2.0 ** e, Xx)


# ---- (e) the small kernel and the ladder ---------------------------------------------------

@pytest.mark.parametrize("q", R.SMALL_ORDERS)
def test_small_batch(q):
    """chol_jitter on a batch of five (q <= 64: chol_small_kernel, one launch;
    beyond: bo_cholesky_jitter per member, where cholesky_with_inverse gives
    the same factor with its inverse)."""
    from botorch_amd import kernels
    batch = torch.stack([R.tensor(R.matrix(f, q)) for f in R.SMALL_BATCH])
    Ls = kernels.chol_jitter(batch.to(DEV))
    assert Ls.shape == batch.shape
    for b, f in enumerate(R.SMALL_BATCH):
        A = R.matrix(f, q)
        Lx, Xx, ref = _reference(f, q)
        if q <= 64:
            _check_factor(f"small-{f}-{q}", A, Ls[b], Lx, {k: ref[k] for k in FACTOR_KEYS})
        else:
            L, Linv, jit = kernels.cholesky_with_inverse(batch[b].to(DEV))
            assert jit == 0.0 and torch.equal(L, Ls[b])
            _check_factor(f"jitter-{f}-{q}", A, L, Lx, ref, Linv, Xx)


def _plus_jitter(A, j):
    Aj = np.array(A)
    Aj[np.diag_indices_from(Aj)] += j      # in f64, as the kernels add it
    return Aj


def _chol_small(batch):
    from botorch_amd import kernels
    from botorch_amd._lib import check, lib
    A3 = batch.to(DEV).contiguous()
    B, q = A3.shape[0], A3.shape[-1]
    L = torch.full_like(A3, float("nan"))
    info = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    jit = torch.full((B,), float("nan"), dtype=torch.float64, device=DEV)
    P = kernels._p
    check(lib().bo_chol_small(P(A3), B, q, R.LADDER_TRIES, R.LADDER_JITTER0, P(L), P(info), P(jit),
                              kernels._stream(torch.device(DEV))), "chol_small")
    torch.cuda.synchronize()
    return L.cpu(), info.cpu().tolist(), jit.cpu().tolist()


@pytest.mark.parametrize("q", [q for q in R.LADDER_ORDERS if q <= 64])
def test_ladder_small(q):
    """Four members needing the rungs 0, 1e-8, 1e-6, 1e-4 in one batch take them
    independently; a fifth that no rung repairs fails alone (NaN factor, info
    set), leaves the others' results bit-identical and makes chol_jitter raise
    what the oracle's psd_safe_cholesky raises."""
    from botorch_amd import kernels
    from botorch_amd.exceptions import NotPSDError
    As, lams = R.ladder_batch(q)
    L, info, jit = _chol_small(torch.from_numpy(As))
    assert info == [0, 0, 0, 0]
    np.testing.assert_allclose(jit, R.LADDER_RUNGS, rtol=1e-12)
    for b in range(4):
        Aj = _plus_jitter(As[b], jit[b])
        Lx, _, ref = _reference_of(Aj, inverse=False)
        _check_factor(f"ladder-{q}-lam{lams[b]:g}", Aj, L[b], Lx, ref)
    bad, lams_bad = R.ladder_batch(q, with_bad=True)
    k = lams_bad.index(1.0)
    Lb, info_b, jit_b = _chol_small(torch.from_numpy(bad))
    assert info_b[k] > 0 and torch.isnan(Lb[k]).all()
    rest = [b for b in range(5) if b != k]
    assert [info_b[b] for b in rest] == [0, 0, 0, 0]
    assert [jit_b[b] for b in rest] == jit
    assert torch.equal(Lb[rest], L)
    with pytest.raises(NotPSDError) as exc:
        kernels.chol_jitter(torch.from_numpy(bad).to(DEV), R.LADDER_TRIES, R.LADDER_JITTER0)
    assert type(exc.value).__name__ == "NotPSDError"


def test_ladder_beyond_64():
    """q = 65: bo_cholesky_jitter, one matrix per call; the member no rung
    repairs raises, and the calls after it are right."""
    from botorch_amd import kernels
    from botorch_amd.exceptions import NotPSDError, NumericalWarning
    q = 65
    bad, lams = R.ladder_batch(q, with_bad=True)
    rungs = dict(zip(R.LADDER_LAMBDAS, R.LADDER_RUNGS))
    for A, lam in zip(bad, lams):
        Ad = torch.from_numpy(A).to(DEV)
        if lam == 1.0:
            with pytest.raises(NotPSDError):
                kernels.cholesky_with_inverse(Ad, R.LADDER_TRIES, R.LADDER_JITTER0)
            continue
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            L, Linv, jit = kernels.cholesky_with_inverse(Ad, R.LADDER_TRIES, R.LADDER_JITTER0)
        assert any(issubclass(w.category, NumericalWarning) for w in caught) == (lam > 0)
        assert jit == pytest.approx(rungs[lam], rel=1e-12)
        Aj = _plus_jitter(A, jit)
        Lx, Xx, ref = _reference_of(Aj)
        _check_factor(f"ladder-{q}-lam{lam:g}", Aj, L, Lx, ref, Linv, Xx)


# ---- (f) one cache-level check ---------------------------------------------------------------

def test_cache_alpha_against_a_longdouble_solve():
    """build_gp_cache on clustered points (n = 193, noise 1e-6): alpha =
    A^{-1} y against a longdouble solve with the kernel matrix the device
    itself forms (bo_covar_matrix, so the comparison is of the factorisation
    and the two triangular products, not of exp); the yardstick is torch's
    cholesky_solve on the same matrix."""
    from botorch_amd import kernels
    X, y, ls, noise = R.cache_inputs()
    lsd = torch.full((6,), ls, dtype=torch.float64, device=DEV)
    Xd, yd = X.to(DEV), y.to(DEV)
    c = kernels.build_gp_cache(Xd, yd, lsd, noise, 0.0)
    assert c.jitter == 0.0
    K = kernels.covar_matrix(Xd, Xd, lsd, diag_add=noise).cpu()
    K = (K.tril() + K.tril(-1).T).numpy()         # the factorisation reads the lower part
    ax = R.ext_solve(K, y.numpy())
    at = torch.cholesky_solve(y.reshape(-1, 1), torch.linalg.cholesky(torch.from_numpy(K)))

    def err(a):
        return float(R._fro(R.ld(a.reshape(-1)) - ax) / R._fro(ax))

    _hold("cache-alpha", {"alpha": err(c.alpha.cpu())}, {"alpha": err(at)})
