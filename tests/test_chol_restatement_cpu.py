"""chol_restatement.py pinned and calibrated on the host: the longdouble
Cholesky and triangular inverse against mpmath at 50 digits, and every case
test_gpu_chol_accuracy.py runs on the device shown well posed here -- LAPACK
factors it (cholesky_ex info 0), its condition number lies in the band the
case is there to cover, the failing-minor cases fail where they say, and the
ladder cases take the rung they say in oracle.gp.psd_safe_cholesky.  With that
no device case needs a skip on numerical grounds."""
import math

import numpy as np
import pytest
import torch

from tests import chol_restatement as R

mpmath = pytest.importorskip("mpmath")


def _mp_cholesky(A):
    n = A.shape[0]
    M = mpmath.matrix(n, n)
    for i in range(n):
        for j in range(n):
            M[i, j] = mpmath.mpf(float(A[i, j]))
    L = mpmath.matrix(n, n)
    for j in range(n):
        for i in range(j, n):
            s = M[i, j] - mpmath.fsum(L[i, k] * L[j, k] for k in range(j))
            L[i, j] = mpmath.sqrt(s) if i == j else s / L[j, j]
    return L


def _mp_tri_inverse(L, n):
    X = mpmath.matrix(n, n)
    for j in range(n):
        X[j, j] = 1 / L[j, j]
        for i in range(j + 1, n):
            X[i, j] = -mpmath.fsum(L[i, k] * X[k, j] for k in range(j, i)) / L[i, i]
    return X


def _rel(M_ld, M_mp, n):
    """||M_ld - M_mp||_F / ||M_mp||_F, the difference taken at 50 digits."""
    num = den = mpmath.mpf(0)
    for i in range(n):
        for j in range(i + 1):
            hi = np.float64(M_ld[i, j])     # a longdouble as the exact sum of two doubles
            lo = np.float64(M_ld[i, j] - R.LD(hi))
            d = mpmath.mpf(float(hi)) + mpmath.mpf(float(lo)) - M_mp[i, j]
            num += d * d
            den += M_mp[i, j] * M_mp[i, j]
    return float(mpmath.sqrt(num / den))


# One matrix of each family at which a forward comparison to 1e-17 is well
# posed: the factor of A moves by cond(A) times a relative change of A, and
# longdouble itself rounds at 1.1e-19, so the condition number has to stay
# below a few tens (graded: of the matrix it scales, the scaling being exact).
MILD = {
    "gp_rbf": lambda n: R.matrix("gp_rbf", n),
    "gp_matern": lambda n: R.matrix("gp_matern", n),
    "gp_clustered": lambda n: R.gp_clustered(R.RBF, n, 0.3, 0.1),
    "spectrum": lambda n: R.spectrum(n, 10.0),
    "graded": lambda n: R.matrix("graded", n),
}


@pytest.mark.parametrize("n", [1, 2, 17, 40])
@pytest.mark.parametrize("family", sorted(MILD))
def test_reference_against_mpmath(family, n):
    A = MILD[family](n)
    with mpmath.workdps(50):
        Lm = _mp_cholesky(A)
        L, info = R.ext_cholesky(A)
        assert info == 0
        X = R.ext_tri_inverse(L)
        assert not np.triu(L, 1).any() and not np.triu(X, 1).any()
        eL = _rel(L, Lm, n)
        eX = _rel(X, _mp_tri_inverse(Lm, n), n)
    assert eL < 1e-17, eL
    assert eX < 1e-17, eX


@pytest.mark.parametrize("n", [2, 17, 40])
@pytest.mark.parametrize("family", ["clustered", "spectrum1e6", "spectrum1e12", "gp_hard"])
def test_reference_on_the_hard_families(family, n):
    """At condition 1e6 .. 1e12 no factor computed at eps = 1.1e-19 agrees with
    the exact one to 1e-17 (clustered, n = 17 measures 1.3e-17), so the
    reference is pinned there by what does not grow with the conditioning:
    its componentwise backward error, and its inverse against the 50-digit
    inverse of the same factor, both to 1e-17."""
    A = R.matrix(family, n)
    with mpmath.workdps(50):
        L, info = R.ext_cholesky(A)
        assert info == 0
        Lp = _to_mp(L, n)
        worst = mpmath.mpf(0)
        for i in range(n):
            for j in range(i + 1):
                r = abs(mpmath.mpf(float(A[i, j])) - mpmath.fsum(Lp[i, k] * Lp[j, k] for k in range(j + 1)))
                s = mpmath.fsum(abs(Lp[i, k] * Lp[j, k]) for k in range(j + 1))
                worst = max(worst, r / s)
        eX = _rel(R.ext_tri_inverse(L), _mp_tri_inverse(Lp, n), n)
    assert float(worst) < 1e-17, float(worst)
    assert eX < 1e-17, eX


def _to_mp(M, n):
    out = mpmath.matrix(n, n)
    for i in range(n):
        for j in range(i + 1):
            hi = np.float64(M[i, j])     # a longdouble as the exact sum of two doubles
            lo = np.float64(M[i, j] - R.LD(hi))
            out[i, j] = mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))
    return out


def test_metrics_on_a_known_perturbation():
    """The metrics see what they are meant to see: a factor with one entry moved
    by 2^-40 relative shows omega, eta and fwd of that size, the exact-in-f64
    factor of a small integer matrix shows zero."""
    L0 = np.tril(np.arange(1.0, 26.0).reshape(5, 5) % 7 + 1.0)
    A = L0 @ L0.T
    Lx, info = R.ext_cholesky(A)
    assert info == 0 and R.fwd(L0, Lx) == 0.0
    assert R.omega(A, L0) == 0.0 and R.eta(A, L0) == 0.0
    X = R.ext_tri_inverse(Lx)
    assert max(R.inv_res(L0, np.asarray(X, dtype=np.float64))) < 4 * R.U
    L1 = L0.copy()
    L1[3, 1] *= 1.0 + 2.0 ** -40
    for m in (R.omega(A, L1), R.eta(A, L1), R.fwd(L1, Lx)):
        assert 2.0 ** -48 < m < 2.0 ** -38, m
    fm = R.factor_metrics(A, L1, Lx)
    assert fm == {"omega": R.omega(A, L1), "eta": R.eta(A, L1), "fwd": R.fwd(L1, Lx)}


def _well_posed(c):
    A = R.matrix(c.family, c.n)
    assert A.shape == (c.n, c.n) and np.array_equal(A, A.T)
    _, info = torch.linalg.cholesky_ex(R.tensor(A))
    assert int(info) == 0
    cond = float(np.linalg.cond(A))
    assert c.lo <= cond < c.hi, (cond, c.lo, c.hi)


@pytest.mark.parametrize("c", R.DAG_CASES, ids=R.case_id)
def test_dag_case_is_well_posed(c):
    _well_posed(c)


@pytest.mark.parametrize("c", R.SMALL_CASES, ids=R.case_id)
def test_small_case_is_well_posed(c):
    _well_posed(c)


def test_dag_cases_cover_every_order():
    """Every order has the benign gp and a case of condition >= 1e6 (n = 1 has
    neither: a 1 x 1 matrix has condition 1)."""
    orders = R.DAG_ORDERS + [640, 64 * R.T_FIRST_BATCHED_COLUPD - 1, 64 * R.T_FIRST_BATCHED_XSTEP - 1]
    for n in orders:
        mine = [c for c in R.DAG_CASES if c.n == n]
        assert any(c.family == "gp_rbf" for c in mine)
        assert n == 1 or any(c.lo >= 0.99e6 for c in mine), n
    assert len([c for c in R.DAG_CASES if c.n == 640]) <= 2
    assert all(c.n <= 385 or c.n == 640 for c in R.DAG_CASES)
    assert any(c.family == "gp_hard" and c.n == 385 for c in R.DAG_CASES)


def test_batched_task_orders():
    """The two orders 64 T - 1 of the case list are the smallest at which the
    DAG's queue holds a batched (nk > 1) column update / inverse step."""
    assert R.first_batched(R.T_COLUPD) == R.T_FIRST_BATCHED_COLUPD
    assert R.first_batched(R.T_XSTEP) == R.T_FIRST_BATCHED_XSTEP


@pytest.mark.parametrize("n,p", R.FAIL_CASES)
def test_fail_at_fails_where_it_says(n, p):
    B = R.fail_at(n, p)
    assert np.array_equal(B, B.T)
    _, info = torch.linalg.cholesky_ex(R.tensor(B))
    assert int(info) == p + 1
    _, info_x = R.ext_cholesky(B)
    assert info_x == p + 1


def test_nan_cases_fail_where_they_say():
    base = R.matrix("gp_rbf", 193)
    for p in R.NAN_DIAG:
        A = np.array(base)
        A[p, p] = np.nan
        assert R.ext_cholesky(A)[1] == p + 1
    i, j = R.NAN_OFF
    A = np.array(base)
    A[i, j] = A[j, i] = np.nan
    assert R.ext_cholesky(A)[1] == i + 1


@pytest.mark.parametrize("q", R.LADDER_ORDERS)
def test_ladder_cases_take_their_rungs(q):
    from oracle.gp import NotPSDError, psd_safe_cholesky
    As, lams = R.ladder_batch(q)
    for A, lam in zip(As, lams):
        w = np.linalg.eigvalsh(A)
        assert abs(w[0] - (-lam if lam > 0 else w[0])) < 1e-13 and 0.5 <= w[1] and w[-1] <= 2.0
        assert lam > 0 or w[0] >= 0.5
    L, added = psd_safe_cholesky(torch.from_numpy(As), jitter=R.LADDER_JITTER0,
                                 max_tries=R.LADDER_TRIES)
    np.testing.assert_allclose(added.numpy(), R.LADDER_RUNGS, rtol=1e-12)
    # each rung a factor of three or more from the eigenvalue it has to clear
    for lam, rung in zip(lams[1:], R.LADDER_RUNGS[1:]):
        assert rung / 10 * 3 <= lam * (1 + 1e-12) and lam * 3 <= rung * (1 + 1e-12)
    bad, lams_bad = R.ladder_batch(q, with_bad=True)
    assert lams_bad.count(1.0) == 1
    with pytest.raises(NotPSDError):
        psd_safe_cholesky(torch.from_numpy(bad), jitter=R.LADDER_JITTER0, max_tries=R.LADDER_TRIES)


def test_scale_and_cache_cases():
    """4^(+-100) A is exact in f64 (no entry leaves the normal range), and the
    cache case's matrix is one LAPACK factors."""
    A = R.matrix(*R.SCALE_CASE)
    for e in (100, -100):
        S = A * 4.0 ** e
        assert np.array_equal(S / 4.0 ** e, A) and np.isfinite(S).all()
        assert np.abs(S[S != 0]).min() > 1e-250
    n, ls, noise = R.CACHE_CASE
    K = R.gp_clustered(R.RBF, n, ls, noise)
    assert int(torch.linalg.cholesky_ex(torch.from_numpy(K))[1]) == 0
    X, y, _, _ = R.cache_inputs()
    assert X.shape == (n, 6) and y.shape == (n,) and math.isfinite(float(y.sum()))
