"""The Cholesky factorisation and the triangular inverse restated in numpy at
np.longdouble (the x87 format, 64-bit mantissa, eps = 2^-63): the reference of
the device Cholesky family (csrc/chol_dag.hip behind bo_cholesky_inverse,
chol_small_kernel behind bo_chol_small, bo_cholesky_jitter), with the error
metrics the tests hold them to and the matrix families they run on.

  ext_cholesky     column Cholesky: c = A[j:, j] - L[j:, :j] L[j, :j],
                   L[j:, j] = c / sqrt(c[0]); info as torch.linalg.cholesky_ex
                   (0, or the 1-based order of the first non-positive pivot;
                   a NaN pivot is not positive)
  ext_tri_inverse  forward substitution, row by row
  omega            max_ij |A - L L^T|_ij / (|L| |L^T|)_ij   (componentwise
                   backward error; Higham, Accuracy and Stability of Numerical
                   Algorithms, Theorem 10.3: <= (n + 1) u for any summation order)
  eta              ||A - L L^T||_F / ||A||_F
  fwd              ||L - Lx||_F / ||Lx||_F
  inv_res          max |X L - I| / (|X| |L|) and max |L X - I| / (|L| |X|)

Every residual is accumulated in longdouble from the f64 inputs.  The
denominators |L| |L^T| and |X| |L| only scale a residual, so they are formed
in f64: their own relative error of n u moves a metric by that fraction of
itself.

The bound of the device tests: for each metric m, m_dev <= R max(m_ref, u),
u = 2^-53, where m_ref is the same metric of LAPACK on the CPU
(torch.linalg.cholesky, solve_triangular of its factor) on the same matrix.
R is recorded in DESIGN.md section 4 with the ratios it was set from.

The families are deterministic functions of (n, seed) and share nothing with
the package or with oracle/.  The case lists at the end are what
test_gpu_chol_accuracy.py runs on the device and test_chol_restatement_cpu.py
shows well posed on the host."""
import ctypes
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

LD = np.longdouble
if not np.finfo(LD).eps < 2e-19:
    pytest.skip("np.longdouble is not the 64-bit-mantissa extended format here",
                allow_module_level=True)

U = 2.0 ** -53
# m_dev <= R max(m_ref, u).  Set from the ratios measured on the device
# ("Accuracy against an extended-precision reference").
R = 16.0
RBF, MATERN52 = 0, 1
F64 = torch.float64


def _f64(A):
    if torch.is_tensor(A):
        A = A.detach().cpu().numpy()
    A = np.asarray(A)
    assert A.dtype == np.float64
    return A


def tensor(A):
    """A writable torch copy of a (cached, read-only) case matrix."""
    return torch.from_numpy(np.array(A, dtype=np.float64))


def ld(A):
    return _f64(A).astype(LD)


def mm(A, B):
    """A B accumulated in longdouble (B column-major: both operands of the
    inner loop are then contiguous, which numpy's generic loop needs to be quick)."""
    return np.dot(np.ascontiguousarray(A, dtype=LD), np.asfortranarray(B, dtype=LD))


def ext_cholesky(A):
    A = ld(A)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        c = A[j:, j] - np.dot(L[j:, :j], L[j, :j])
        if not c[0] > 0:
            return L, j + 1
        L[j:, j] = c / np.sqrt(c[0])
    return L, 0


def ext_tri_inverse(L):
    L = np.asarray(L, dtype=LD)
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD, order="F")
    for i in range(n):
        X[i, :i] = -np.dot(L[i, :i], X[:i, :i]) / L[i, i]
        X[i, i] = LD(1) / L[i, i]
    return np.ascontiguousarray(X)


def _max_ratio(num, den):
    """max num / den over the entries; an entry whose scale is zero has to be
    exact (a zero numerator counts 0, anything else infinity)."""
    num = np.asarray(num, dtype=np.float64)
    if np.isnan(num).any() or np.isnan(den).any():
        return math.inf
    zero = den == 0
    if (num[zero] != 0).any():
        return math.inf
    q = num[~zero] / den[~zero]
    return float(q.max()) if q.size else 0.0


def omega(A, L):
    Lf = _f64(L)
    res = np.abs(ld(A) - mm(Lf, Lf.T))
    return _max_ratio(res, np.abs(Lf) @ np.abs(Lf).T)


def _fro(M):
    return np.sqrt(np.sum(np.asarray(M, dtype=LD) ** 2))


def eta(A, L):
    Lf = _f64(L)
    return float(_fro(ld(A) - mm(Lf, Lf.T)) / _fro(ld(A)))


def fwd(L, Lx):
    return float(_fro(ld(L) - Lx) / _fro(Lx))


def factor_metrics(A, L, Lx):
    """omega, eta and fwd of one factor, sharing the residual A - L L^T."""
    Lf, Al = _f64(L), ld(A)
    res = Al - mm(Lf, Lf.T)
    return {"omega": _max_ratio(np.abs(res), np.abs(Lf) @ np.abs(Lf).T),
            "eta": float(_fro(res) / _fro(Al)),
            "fwd": fwd(Lf, Lx)}


def inverse_metrics(L, X, Xx):
    """Both inv_res values of X against its own factor L, and fwd against Xx."""
    left, right = inv_res(L, X)
    return {"inv_left": left, "inv_right": right, "inv_fwd": fwd(X, Xx)}


def inv_res(L, X):
    Lf, Xf = _f64(L), _f64(X)
    n = Lf.shape[0]
    I = np.eye(n, dtype=LD)
    low = np.tril_indices(n)
    left = np.abs(mm(Xf, Lf) - I)
    right = np.abs(mm(Lf, Xf) - I)
    assert not np.triu(left, 1).any() and not np.triu(right, 1).any()
    return (_max_ratio(left[low], (np.abs(Xf) @ np.abs(Lf))[low]),
            _max_ratio(right[low], (np.abs(Lf) @ np.abs(Xf))[low]))


# ---- matrix families --------------------------------------------------------

def _points(n, seed, clustered):
    g = torch.Generator().manual_seed(seed)
    if not clustered:
        return torch.rand(n, 6, generator=g, dtype=F64)
    h = (n + 1) // 2
    base = torch.rand(h, 6, generator=g, dtype=F64)
    # each twin within 1e-3 (Euclidean) of its original
    shift = (2.0 * torch.rand(n - h, 6, generator=g, dtype=F64) - 1.0) * (1e-3 / math.sqrt(6.0))
    return torch.cat([base, base[: n - h] + shift])


def _kernel_matrix(X, kind, ls, noise):
    Z = X / ls
    r = torch.cdist(Z, Z, compute_mode="donot_use_mm_for_euclid_dist")
    r = 0.5 * (r + r.T)
    r.fill_diagonal_(0.0)
    if kind == RBF:
        K = torch.exp(-0.5 * r ** 2)
    else:
        K = (1.0 + math.sqrt(5.0) * r + (5.0 / 3.0) * r ** 2) * torch.exp(-math.sqrt(5.0) * r)
    return (K + noise * torch.eye(X.shape[0], dtype=F64)).numpy()


def gp(kind, n, ls, noise, seed=None):
    """k(X, X) + noise I on X = rand(n, 6): RBF exp(-r^2 / 2), Matern-5/2
    (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r), r = |x - x'| / ls."""
    return _kernel_matrix(_points(n, n if seed is None else seed, False), kind, ls, noise)


def gp_clustered(kind, n, ls, noise, seed=None):
    """gp with the second half of the points within 1e-3 of the first half."""
    return _kernel_matrix(_points(n, n if seed is None else seed, True), kind, ls, noise)


def _orthogonal(n, seed):
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    return Q


def _from_spectrum(Q, s):
    A = (Q * s) @ Q.T
    return 0.5 * (A + A.T)


def spectrum(n, cond, seed=None):
    """Q diag(logspace(0, -log10 cond, n)) Q^T, symmetrised."""
    s = np.logspace(0.0, -math.log10(cond), n) if n > 1 else np.ones(1)
    return _from_spectrum(_orthogonal(n, n if seed is None else seed), s)


def graded(n, seed=None):
    """D A D, D = diag(2^k_i), k_i spread over -20 .. 20 in a seeded order (the
    scaling is exact: the factor of D A D is D times the factor of A)."""
    seed = n if seed is None else seed
    k = np.round(np.linspace(-20.0, 20.0, n)) if n > 1 else np.array([20.0])
    k = np.random.default_rng(seed).permutation(k)
    D = 2.0 ** k
    return gp(RBF, n, 0.3, 1e-4, seed) * D[:, None] * D[None, :]


def fail_at(n, p, seed=None):
    """B = L0 L0^T of a gp matrix with B[p, p] lowered by 1.5 L0[p, p]^2: the
    leading minor of order p + 1 is the first non-positive one (its pivot is
    -L0[p, p]^2 / 2 up to rounding, the earlier pivots are L0's)."""
    L0 = np.linalg.cholesky(gp(RBF, n, 0.3, 1e-3, seed))
    B = L0 @ L0.T
    B = np.tril(B) + np.tril(B, -1).T
    B[p, p] -= 1.5 * L0[p, p] ** 2
    return B


def ladder_member(q, lam, seed):
    """Q diag(e_1, s_2 .. s_q) Q^T, s_i in [0.5, 2]; e_1 = -lam, or s_1 for the
    clean member (lam = 0: no negative eigenvalue -- an exactly zero one would
    leave its rung to rounding): A + j I is positive definite exactly for
    j > lam."""
    rng = np.random.default_rng(1000 * q + seed)
    s = 0.5 + 1.5 * rng.random(q)
    if lam > 0:
        s[0] = -lam
    return _from_spectrum(_orthogonal(q, 7000 * q + seed), s)


# ---- the shared case lists ----------------------------------------------------

Case = namedtuple("Case", "family n lo hi")   # lo <= cond_2 < hi is what the case covers

FAMILIES = {
    "gp_rbf": lambda n: gp(RBF, n, 0.3, 1e-4),
    "gp_matern": lambda n: gp(MATERN52, n, 0.3, 1e-4),
    "gp_hard": lambda n: gp(RBF, n, 1.5, 1e-7),
    "clustered": lambda n: gp_clustered(RBF, n, 0.3, 1e-6),
    "clustered_matern": lambda n: gp_clustered(MATERN52, n, 0.3, 1e-6),
    "spectrum1e3": lambda n: spectrum(n, 1e3),
    "spectrum1e6": lambda n: spectrum(n, 1e6),
    "spectrum1e8": lambda n: spectrum(n, 1e8),
    "spectrum1e12": lambda n: spectrum(n, 1e12),
    "graded": graded,
}


def _band(family, n):
    """The condition numbers a case is there to cover.  A 1 x 1 matrix has
    condition 1 whatever its family."""
    if n == 1:
        return 1.0, 1.0 + 1e-12
    if family.startswith("spectrum"):
        c = float(family[len("spectrum"):])
        return c * (1 - 1e-3), c * (1 + 1e-3)
    if family in ("gp_rbf", "gp_matern"):
        return 1.0, 1e6                       # benign
    if family == "gp_hard":
        return 1e9, 1e11
    if family.startswith("clustered"):
        return (1e6, 1e8) if n >= 65 else (1e5, 1e8) if n >= 16 else (1.0, 1e8)
    return 1e6, math.inf                      # graded: 2^80 by construction


def case(family, n):
    return Case(family, n, *_band(family, n))


@functools.lru_cache(maxsize=None)
def matrix(family, n):
    A = FAMILIES[family](n)
    A.setflags(write=False)
    return A


def case_id(c):
    return f"{c.family}-{c.n}"


# bo_chol_dag_tasks(T): the smallest tile counts at which a batched (nk > 1)
# column update / inverse step first appears in the task queue
# (test_chol_restatement_cpu.py holds these two numbers to the queue).
T_COLUPD, T_XSTEP = 2, 3
T_FIRST_BATCHED_COLUPD = 6
T_FIRST_BATCHED_XSTEP = 4


def dag_queue_nk(T):
    """[(task type, nk)] of the DAG's task queue for T tile rows (host only)."""
    from botorch_amd._lib import lib
    fn = lib().bo_chol_dag_tasks
    n = fn(T, None, 0)
    buf = np.zeros(4 * n, dtype=np.int32)
    assert fn(T, buf.ctypes.data_as(ctypes.c_void_p), n) == n
    return [(int(x) & 0xFF, max(1, int(x) >> 16)) for x in buf.reshape(n, 4)[:, 0]]


def first_batched(task, tmax=64):
    for T in range(1, tmax + 1):
        if any(t == task and nk > 1 for t, nk in dag_queue_nk(T)):
            return T
    return None


DAG_ORDERS = [1, 2, 16, 17, 63, 64, 65, 127, 128, 129, 191, 193, 257, 385]


def _dag_cases():
    out = []
    for i, n in enumerate(DAG_ORDERS):
        out.append(case("gp_rbf", n))
        out.append(case("spectrum1e6", n))
        # the other families in rotation, so that each meets every kind of edge
        extra = ["gp_matern", "clustered", "spectrum1e12", "graded"]
        out.append(case(extra[i % 4], n))
        if n in (65, 129, 193, 385):
            out += [case(f, n) for f in extra if f != extra[i % 4]]
    out.append(case("gp_hard", 385))
    out += [case("gp_rbf", 640), case("clustered", 640)]
    for T in sorted({T_FIRST_BATCHED_COLUPD, T_FIRST_BATCHED_XSTEP}):
        out += [case("gp_rbf", 64 * T - 1), case("spectrum1e6", 64 * T - 1)]
    return out


DAG_CASES = _dag_cases()

FAIL_CASES = [(65, 0), (129, 15), (129, 16), (193, 63), (193, 64), (193, 65), (257, 127),
              (257, 128), (300, 299)]
NAN_DIAG = [0, 64, 130]          # on a gp matrix of order 193
NAN_OFF = (150, 20)              # A[i, j] = A[j, i] = nan: info = i + 1
PAD_ORDERS = [1, 65, 129, 300]

SMALL_ORDERS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150]
SMALL_BATCH = ["spectrum1e3", "spectrum1e8", "spectrum1e12", "clustered", "clustered_matern"]
SMALL_CASES = [case(f, q) for q in SMALL_ORDERS for f in SMALL_BATCH]

LADDER_ORDERS = [3, 16, 17, 64, 65]
LADDER_LAMBDAS = [0.0, 3e-9, 3e-7, 3e-5]
LADDER_RUNGS = [0.0, 1e-8, 1e-6, 1e-4]
LADDER_JITTER0, LADDER_TRIES = 1e-8, 6


def ladder_batch(q, with_bad=False):
    """The four members of LADDER_LAMBDAS (and, with_bad, a fifth with
    lam = 1, which no rung repairs, in the middle of the batch)."""
    members = [(lam, i) for i, lam in enumerate(LADDER_LAMBDAS)]   # (lam, seed)
    if with_bad:
        members.insert(2, (1.0, len(LADDER_LAMBDAS)))
    return np.stack([ladder_member(q, lam, s) for lam, s in members]), [lam for lam, _ in members]


SCALE_CASE = ("spectrum1e6", 193)     # times 4^(+-100), exact in f64
CACHE_CASE = (193, 0.3, 1e-6)         # build_gp_cache on clustered points: n, ls, noise


def cache_inputs():
    n, ls, noise = CACHE_CASE
    X = _points(n, n, True)
    g = torch.Generator().manual_seed(n + 1)
    y = torch.sin(3.0 * X.sum(-1)) + 0.1 * torch.randn(n, generator=g, dtype=F64)
    return X, y, ls, noise


def ext_solve(A, b):
    """A^{-1} b in longdouble through ext_cholesky."""
    L, info = ext_cholesky(A)
    assert info == 0
    X = ext_tri_inverse(L)
    return np.dot(X.T, np.dot(X, ld(b)))
