"""The three ICM kernels of icm.hip against the host restatement
(tests/icm_restatement.py): bo_icm_covar elementwise, bo_icm_mll_terms through
fit.icm_mll_terms with the MLL suite's tolerances (value 1e-9 max(1, |v|),
gradient rtol 1e-6 / atol 1e-9; test_mtgp_cpu.py shows two host formulations a
hundred times closer), bo_icm_task_view against the torch formulas."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import icm_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
KIND_NAME = {R.RBF: "rbf", R.MATERN52: "matern"}


def _dev_case(X, task, y, ls, noise, F, v):
    B = R.task_covar(F, v)
    return (X.to(DEV), task.to(torch.int32).to(DEV), y.to(DEV), ls.to(DEV),
            noise.to(DEV) if torch.is_tensor(noise) else noise, B.to(DEV))


# ---- bo_icm_covar -----------------------------------------------------------------------------
@pytest.mark.parametrize("vec", [False, True], ids=["scalar", "vector"])
@pytest.mark.parametrize("kind", R.KINDS, ids=["rbf", "matern"])
@pytest.mark.parametrize("T", [1, 3, 16])
@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_icm_covar_matches_restatement(n, T, kind, vec):
    """A = o kbar * B[tau, tau] + diag(noise) on and below the diagonal, exact zeros
    above it, the identity on the padding (np = 128 or 384 here)."""
    from botorch_amd import kernels
    X, task, y, ls, noise, F, v = R.make_case(6, n, T, min(T, 2), vec)
    Xd, td, _, lsd, nd, Bd = _dev_case(X, task, y, ls, noise, F, v)
    A = kernels.icm_covar(Xd, td, lsd, Bd, kind, R.OUTPUTSCALE, 0.0 if vec else noise,
                          nd if vec else None).cpu()
    np_ = kernels.padded_order(n)
    assert A.shape == (np_, np_)
    ref = torch.tril(R.train_covar(X, task, ls, noise, R.OUTPUTSCALE, R.task_covar(F, v), kind))
    err = (A[:n, :n] - ref).abs().max().item()
    print(f"max err {err:.3e} of {1e-12 * ref.abs().max().item():.3e}")
    assert err <= 1e-12 * ref.abs().max().item()
    assert torch.equal(torch.triu(A[:n, :n], 1), torch.zeros(n, n, dtype=F64))
    pad = torch.eye(np_, dtype=F64)
    assert torch.equal(A[n:], pad[n:]) and torch.equal(A[:, n:], pad[:, n:])
    # a ladder's jitter rides in `noise` beside the observed variances
    if vec and n == 65:
        A2 = kernels.icm_covar(Xd, td, lsd, Bd, kind, R.OUTPUTSCALE, 1e-3, nd).cpu()
        torch.testing.assert_close(torch.diagonal(A2)[:n], torch.diagonal(A)[:n] + 1e-3,
                                   rtol=1e-15, atol=0)
        assert torch.equal(torch.tril(A2[:n, :n], -1), torch.tril(A[:n, :n], -1))


# ---- bo_icm_mll_terms through fit.icm_mll_terms -------------------------------------------------
TASKS = {"T1": (1, 1, ()), "T2": (2, 2, ()), "T3r1-empty": (3, 1, (2,)), "T16": (16, 16, ()),
         "T16r2": (16, 2, ())}


def _grid():
    cases = []
    for kind in R.KINDS:
        # every width: the d = 6 template instance, the runtime-d instance at 1 and 9, the limit
        cases += [(kind, d, 65, "T2", False) for d in (1, 6, 9, 64)]
        # every task layout x noise form at a template and at a runtime-d width
        cases += [(kind, d, 65, tk, vec) for d in (6, 9) for tk in TASKS for vec in (False, True)]
        # one lane, two lanes, a second wavefront, a second trip of the pair loop (i >= 256)
        cases += [(kind, d, n, "T3r1-empty", False) for d in (6, 64) for n in (1, 2, 65, 257, 300)]
        # sixteen bins in use where the pair loop wraps, fixed noise
        cases += [(kind, 64, 300, "T16", True), (kind, 9, 257, "T16r2", True)]
    return sorted(set(cases))


assert len(_grid()) < 80


def _case_id(case):
    kind, d, n, tk, vec = case
    return f"{KIND_NAME[kind]}-d{d}-n{n}-{tk}-{'fixed' if vec else 'scalar'}"


@functools.lru_cache(maxsize=None)
def _reference(kind, d, n, tk, vec):
    T, rank, empty = TASKS[tk]
    X, task, y, ls, noise, F, v = R.make_case(d, n, T, rank, vec, empty_tasks=empty)
    return R.ll_autograd(X, task, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE, F, v, kind)


def _assert_close(val, grad, ref_val, ref_grad):
    print(f"value {val!r} ref {ref_val!r}  |dv| {abs(val - ref_val):.3e}  max |dg| "
          f"{np.max(np.abs(grad - ref_grad)):.3e}  max rel "
          f"{np.max(np.abs(grad - ref_grad) / (1e-9 + 1e-6 * np.abs(ref_grad))):.3e} of tol")
    assert math.isfinite(val) and np.isfinite(grad).all()
    assert abs(val - ref_val) < 1e-9 * max(1.0, abs(ref_val))
    np.testing.assert_allclose(grad, ref_grad, rtol=1e-6, atol=1e-9)


def _run(fn, kind, d, n, T, rank, vec, empty=()):
    X, task, y, ls, noise, F, v = R.make_case(d, n, T, rank, vec, empty_tasks=empty)
    return fn(X.to(DEV), task.to(torch.int32).to(DEV), y.to(DEV), ls.numpy(),
              noise.to(DEV) if vec else noise, R.CONSTANT, R.OUTPUTSCALE, F.numpy(), v.numpy(), kind)


@pytest.mark.parametrize("case", _grid(), ids=_case_id)
def test_icm_mll_terms_match_restatement(case):
    """(ll, d ll / d [noise, constant, ls, outputscale, F, v]) of the fused route
    against Cholesky + autograd.  n >= 65 holds a coincident pair of rows in
    different tasks; a task without data has exactly zero gradient rows.  With
    fixed noise the first gradient entry is documented as meaningless."""
    from botorch_amd.fit import icm_mll_terms
    kind, d, n, tk, vec = case
    T, rank, empty = TASKS[tk]
    val, grad = _run(icm_mll_terms, kind, d, n, T, rank, vec, empty)
    ref_val, ref_grad = _reference(*case)
    assert grad.shape == (d + 3 + T * rank + T,)
    lo = 1 if vec else 0
    _assert_close(val, grad[lo:], ref_val, ref_grad[lo:])
    for t in empty:
        assert np.all(grad[3 + d:3 + d + T * rank].reshape(T, rank)[t] == 0.0)
        assert grad[3 + d + T * rank + t] == 0.0


@pytest.mark.parametrize("case", [(R.MATERN52, 6, 300, "T16", True), (R.RBF, 9, 257, "T3r1-empty", False)],
                         ids=_case_id)
def test_icm_mll_terms_are_deterministic(case):
    from botorch_amd.fit import icm_mll_terms
    kind, d, n, tk, vec = case
    T, rank, empty = TASKS[tk]
    v1, g1 = _run(icm_mll_terms, kind, d, n, T, rank, vec, empty)
    v2, g2 = _run(icm_mll_terms, kind, d, n, T, rank, vec, empty)
    assert v1 == v2 and torch.equal(torch.from_numpy(g1), torch.from_numpy(g2))


@pytest.mark.parametrize("kind", R.KINDS, ids=["rbf", "matern"])
@pytest.mark.parametrize("d,T", [(6, 17), (65, 2)], ids=["T17", "d65"])
def test_beyond_the_limits_takes_the_torch_route(kind, d, T):
    """T = 17 and d = 65: the route rule sends them to icm_mll_terms_torch, which
    meets the same bound; the fused entry refuses them on the host."""
    from botorch_amd import kernels
    from botorch_amd.fit import icm_mll_terms, icm_mll_terms_torch
    assert not kernels.icm_fused_ok(T, d)
    with pytest.raises(ValueError, match="bo_icm"):
        _run(icm_mll_terms, kind, d, 65, T, 2, False)
    val, grad = _run(icm_mll_terms_torch, kind, d, 65, T, 2, False)
    X, task, y, ls, noise, F, v = R.make_case(d, 65, T, 2, False)
    ref_val, ref_grad = R.ll_autograd(X, task, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE, F, v, kind)
    _assert_close(val, grad, ref_val, ref_grad)


@pytest.mark.parametrize("kind", R.KINDS, ids=["rbf", "matern"])
def test_torch_route_matches_restatement_within_the_limits(kind):
    """The benchmark's comparator on a shape both routes take, fixed noise included."""
    from botorch_amd.fit import icm_mll_terms_torch
    for vec in (False, True):
        val, grad = _run(icm_mll_terms_torch, kind, 6, 257, 3, 1, vec, (2,))
        ref_val, ref_grad = _reference(kind, 6, 257, "T3r1-empty", vec)
        lo = 1 if vec else 0
        _assert_close(val, grad[lo:], ref_val, ref_grad[lo:])


# ---- bo_icm_task_view ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 300])
def test_icm_task_view_matches_torch(n):
    """U' = D U, L^{-1}' = U'^T and alpha' = D alpha elementwise, exact up to one
    rounding of the product, with D holding an exact zero (task 2 uncorrelated
    with task 0) and a negative entry (task 1); the padding is the identity the
    cache build left."""
    from botorch_amd import kernels
    T = 3
    X, task, y, ls, noise, F, v = R.make_case(6, n, T, T, False, seed=1)
    F = torch.tensor([[1.0, 0.0, 0.0], [-0.8, 0.5, 0.0], [0.0, 0.0, 0.7]], dtype=F64)
    Xd, td, yd, lsd, nd, Bd = _dev_case(X, task, y, ls, noise, F, v)
    B = R.task_covar(F, v)
    assert B[0, 2] == 0.0 and B[0, 1] < 0.0
    cache, info = kernels.build_icm_cache(Xd, td, yd, lsd, Bd, noise, R.CONSTANT, kind=R.MATERN52,
                                          outputscale=R.OUTPUTSCALE)
    assert info is None and cache.jitter == 0.0
    for t in range(T):
        view = kernels.icm_task_view(cache, td, Bd, t, float(B[t, t]))
        assert view.L is None and view.outputscale == R.OUTPUTSCALE * float(B[t, t])
        assert view.beta is cache.beta and view.Xt_scaled is cache.Xt_scaled
        D = torch.ones(cache.np, dtype=F64, device=DEV)
        D[:n] = Bd[t][task.to(DEV)] / Bd[t, t]
        if t == 0:
            assert (D == 0).any() and (D < 0).any()
        U_ref = D.unsqueeze(-1) * cache.U
        one_rounding = dict(rtol=2.5e-16, atol=0.0)
        torch.testing.assert_close(view.U, U_ref, **one_rounding)
        torch.testing.assert_close(view.Linv, U_ref.mT.contiguous(), **one_rounding)
        torch.testing.assert_close(view.alpha, D[:n] * cache.alpha, **one_rounding)
        assert torch.equal(view.U[n:], cache.U[n:]) and torch.equal(view.Linv[n:], cache.Linv[n:])
        assert torch.equal(torch.tril(view.U, -1), torch.zeros_like(view.U).tril(-1))
