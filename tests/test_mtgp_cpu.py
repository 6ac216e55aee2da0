"""MultiTaskGP without a device: the two identities the ICM kernels rest on, in
torch fp64 on the host (tests/icm_restatement.py), the host-side pieces of the
model and the fit, every error the model raises, and the argument checks of the
three bo_icm_* entry points (refused before any launch)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import icm_restatement as R
from tests import mll_restatement as S

F64 = torch.float64


def _assert_host(val, grad, ref_val, ref_grad):
    """The bar between two host formulations: a hundred times inside the kernel
    tests' (value 1e-9 max(1, |v|), gradient rtol 1e-6 / atol 1e-9)."""
    print(f"|dv| {abs(val - ref_val):.3e}  max |dg| {np.max(np.abs(grad - ref_grad)):.3e}")
    assert abs(val - ref_val) < 1e-11 * max(1.0, abs(ref_val))
    np.testing.assert_allclose(grad, ref_grad, rtol=1e-8, atol=1e-11)


CASES = [(R.RBF, 1, 2, 1, 1, False, ()), (R.MATERN52, 3, 65, 2, 2, False, ()),
         (R.RBF, 6, 65, 3, 1, True, (2,)), (R.MATERN52, 6, 300, 3, 1, False, (2,)),
         (R.RBF, 9, 257, 16, 2, True, ()), (R.MATERN52, 6, 300, 4, 4, True, ())]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"k{c[0]}-d{c[1]}-n{c[2]}-T{c[3]}-r{c[4]}")
def test_closed_form_matches_autograd(case):
    """Value and every gradient entry, d ll / d F and d ll / d v among them, of the
    closed form against autograd; a task without data has exactly zero rows and
    columns in G (no pair belongs to it), hence an exactly zero gradient row in F."""
    kind, d, n, T, rank, vec, empty = case
    X, task, y, ls, noise, F, v = R.make_case(d, n, T, rank, vec, empty_tasks=empty)
    ref_val, ref_grad = R.ll_autograd(X, task, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE, F, v, kind)
    val, grad, G = R.ll_closed(X, task, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE, F, v, kind)
    lo = 1 if vec else 0
    _assert_host(val, grad[lo:], ref_val, ref_grad[lo:])
    for t in empty:
        assert torch.equal(G[t], torch.zeros(T, dtype=F64))
        assert torch.equal(G[:, t], torch.zeros(T, dtype=F64))
        gF = grad[3 + d:3 + d + T * rank].reshape(T, rank)
        assert np.all(gF[t] == 0.0) and grad[3 + d + T * rank + t] == 0.0


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n,T,rank", [(300, 1, 1), (300, 2, 2), (300, 16, 16), (300, 16, 2),
                                      (257, 3, 1), (65, 16, 16)])
def test_cases_are_well_conditioned(kind, n, T, rank):
    """make_case keeps cond(A) below 1e4 (noise >= 1e-2), so the kernel tests'
    tolerances are not spent on conditioning."""
    for d in (1, 6, 64):
        for vec in (False, True):
            X, task, y, ls, noise, F, v = R.make_case(d, n, T, rank, vec)
            nz = noise if vec else torch.tensor(noise, dtype=F64)
            assert float(nz.min()) >= 1e-2
            A = R.train_covar(X, task, ls, noise, R.OUTPUTSCALE, R.task_covar(F, v), kind)
            assert torch.linalg.cond(A).item() < 1e4


def _view_posterior(X, task, y, ls, noise, c, o, B, kind, Xq, t):
    """The posterior of task t as the single-task path computes it from the task
    view: U' = D U, alpha' = D alpha, outputscale' = o B[t, t], beta unchanged."""
    n = X.shape[0]
    A = R.train_covar(X, task, ls, noise, o, B, kind)
    L = torch.linalg.cholesky(A)
    U = torch.linalg.inv(L).T
    beta = torch.linalg.solve_triangular(L, (y - c).unsqueeze(-1), upper=False).squeeze(-1)
    alpha = U @ beta
    D = B[t][task] / B[t, t]
    Uv, alphav, osv = D.unsqueeze(-1) * U, D * alpha, o * B[t, t]
    Ks = osv * R.unit_kernel(Xq, X, ls, kind)
    Rm = Ks @ Uv
    mean_beta = c + Rm @ beta                      # the fused kernel's form of the mean
    mean_alpha = c + Ks @ alphav                   # the generic route's
    cov = osv * R.unit_kernel(Xq, Xq, ls, kind) - Rm @ Rm.mT
    # A^{-1}' = D A^{-1} D where it is formed (the quad plan): L^{-1}'^T L^{-1}'
    Ainv_v = Uv @ Uv.T
    cov_quad = osv * R.unit_kernel(Xq, Xq, ls, kind) - Ks @ Ainv_v @ Ks.mT
    return mean_beta, mean_alpha, cov, cov_quad


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("which", ["negative", "zero"])
def test_task_view_identity(kind, which):
    """Mean and covariance from the view agree with the explicit (x, task) GP for a B
    with a negative off-diagonal entry and for a B with exact zeros (F = I,
    rank = T: the other tasks' rows of D are exactly 0, so no D^{-1} exists)."""
    d, n, T = 3, 40, 3
    X, task, y, ls, noise, F, v = R.make_case(d, n, T, T, False, seed=3)
    if which == "negative":
        F = torch.tensor([[1.0, 0.0, 0.0], [-0.8, 0.5, 0.0], [0.3, 0.2, 0.6]], dtype=F64)
        assert R.task_covar(F, v)[0, 1] < 0
    else:
        F = torch.eye(T, dtype=F64)
        assert R.task_covar(F, v)[0, 1] == 0.0
    B = R.task_covar(F, v)
    g = torch.Generator().manual_seed(5)
    Xq = torch.rand(4, 3, d, generator=g, dtype=F64)
    for t in range(T):
        tq = torch.full((4, 3), t, dtype=torch.long)
        m_ref, c_ref = R.posterior_explicit(X, task, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE, B,
                                            kind, Xq, tq)
        for m in _view_posterior(X, task, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE, B, kind, Xq, t)[:2]:
            assert (m - m_ref).abs().max() <= 1e-9 * m_ref.abs().max() + 1e-10
        for cv in _view_posterior(X, task, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE, B, kind, Xq, t)[2:]:
            assert (cv - c_ref).abs().max() <= 1e-9 * c_ref.abs().max() + 1e-10


@pytest.mark.parametrize("kind", R.KINDS)
def test_single_task_is_the_single_task_model(kind):
    """T = 1: the ICM likelihood is the single-task one at outputscale o B[0, 0]."""
    X, task, y, ls, noise, F, v = R.make_case(6, 65, 1, 1, False)
    B00 = float(R.task_covar(F, v)[0, 0])
    val, grad = R.ll_autograd(X, task, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE, F, v, kind)
    ref_val, ref_grad = S.ll_autograd(X, y, ls, noise, R.CONSTANT, R.OUTPUTSCALE * B00, kind)
    assert abs(val - ref_val) < 1e-11 * max(1.0, abs(ref_val))
    d = 6
    np.testing.assert_allclose(grad[:2 + d], ref_grad[:2 + d], rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(grad[2 + d], ref_grad[2 + d] * B00, rtol=1e-8, atol=1e-11)


# ---- the model on the host --------------------------------------------------------------------
def _data(n=12, d=2, tasks=(0, 1), task_feature=-1, seed=0):
    g = torch.Generator().manual_seed(seed)
    Xd = torch.rand(n, d, generator=g, dtype=F64)
    t = torch.tensor([tasks[i % len(tasks)] for i in range(n)], dtype=F64).unsqueeze(-1)
    tf = task_feature % (d + 1)
    X = torch.cat([Xd[:, :tf], t, Xd[:, tf:]], dim=-1)
    Y = torch.sin(3 * Xd[:, :1]) + 0.1 * t
    return X, Y


def test_construction_defaults_and_remapping():
    from botorch_amd.models import (FixedNoiseGaussianLikelihood, GammaPrior, IndexKernel,
                                    MaternKernel, MultiTaskGP, ScaleKernel, SingleTaskGP, Standardize)
    X, Y = _data(tasks=(3, 7), task_feature=1)
    torch.manual_seed(0)
    m = MultiTaskGP(X, Y, task_feature=1)
    assert not isinstance(m, SingleTaskGP) and m.num_outputs == 2 and m.num_tasks == 2
    assert m._task_long.tolist() == [0, 1] * 6 and m._Xd.shape == (12, 2)
    assert torch.equal(m._Xd, X[:, [0, 2]]) and torch.equal(m.train_inputs[0], X)
    assert isinstance(m.covar_module, ScaleKernel) and isinstance(m.covar_module.base_kernel, MaternKernel)
    p = m.covar_module.base_kernel.lengthscale_prior
    assert isinstance(p, GammaPrior) and (p.concentration, p.rate) == (3.0, 6.0)
    p = m.covar_module.outputscale_prior
    assert isinstance(p, GammaPrior) and (p.concentration, p.rate) == (2.0, 0.15)
    p = m.likelihood.noise_prior
    assert isinstance(p, GammaPrior) and (p.concentration, p.rate) == (1.1, 0.05)
    assert m.likelihood.noise_lower == 1e-4 and abs(float(m.likelihood.noise.detach()) - 2.0) < 1e-12
    assert not hasattr(m, "outcome_transform") and torch.equal(m.train_targets, Y.squeeze(-1))
    tk = m.task_covar_module
    assert isinstance(tk, IndexKernel) and tk.covar_factor.shape == (2, 2) and tk.var.shape == (2,)
    # the reference's draws from the global generator: F ~ randn(T, rank), then the raw variances
    torch.manual_seed(0)
    F0 = torch.randn(2, 2).to(F64)
    v0 = torch.nn.functional.softplus(torch.randn(2).to(F64))
    assert torch.equal(tk.covar_factor.detach(), F0) and torch.equal(tk.var.detach(), v0)
    assert torch.equal(tk.covar_matrix.detach(), F0 @ F0.T + torch.diag(v0))
    # a superset of tasks, rank, one output task, fixed noise, Standardize
    m = MultiTaskGP(X, Y, task_feature=1, train_Yvar=torch.full_like(Y, 0.01), all_tasks=[7, 3, 9],
                    output_tasks=[7], rank=1, outcome_transform=Standardize(m=1))
    assert m.num_tasks == 3 and m.num_outputs == 1 and m.task_covar_module.covar_factor.shape == (3, 1)
    assert m._task_long.tolist() == [0, 1] * 6  # 3 -> 0, 7 -> 1, 9 -> 2 (no data)
    assert isinstance(m.likelihood, FixedNoiseGaussianLikelihood)
    ys = Y.std()
    torch.testing.assert_close(m.likelihood.noise, torch.full((12,), 0.01, dtype=F64) / ys ** 2)
    torch.testing.assert_close(m.train_targets, ((Y - Y.mean()) / ys).squeeze(-1))


def test_construction_errors():
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import MultiTaskGP
    X, Y = _data()
    with pytest.raises(ValueError, match="Must have that -2 <= task_feature <= 2"):
        MultiTaskGP(X, Y, task_feature=3)
    with pytest.raises(RuntimeError, match="All output tasks must be present in input data."):
        MultiTaskGP(X, Y, task_feature=-1, output_tasks=[2])
    with pytest.raises(UnsupportedError, match="does not contain all the task features"):
        MultiTaskGP(X, Y, task_feature=-1, all_tasks=[0, 2])
    with pytest.raises(UnsupportedError, match="task_covar_prior"):
        MultiTaskGP(X, Y, task_feature=-1, task_covar_prior=object())
    with pytest.raises(UnsupportedError, match="input transforms"):
        MultiTaskGP(X, Y, task_feature=-1, input_transform=object())
    with pytest.raises(ValueError, match="Unsupported shape"):
        MultiTaskGP(X.unsqueeze(0), Y.unsqueeze(0), task_feature=-1)


def test_prediction_errors():
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import MultiTaskGP
    X, Y = _data(tasks=(3, 7))
    m = MultiTaskGP(X, Y, task_feature=-1)
    Xq = torch.rand(2, 3, dtype=F64)
    Xq[:, -1] = 5.0
    with pytest.raises(ValueError, match="Received invalid raw task values"):
        m.posterior(Xq)
    with pytest.raises(ValueError, match="`output_indices` must be None when `X` includes task features."):
        m.posterior(Xq, output_indices=[3])
    with pytest.raises(ValueError, match="Received invalid raw task values"):
        m.posterior(Xq[:, :2], output_indices=[5])
    with pytest.raises(UnsupportedError, match="exactly one output task") as err:
        m.posterior(Xq[:, :2])
    assert "task column" in str(err.value)
    with pytest.raises(NotImplementedError, match="Passing a tensor of observations is not supported"):
        m.posterior(Xq, observation_noise=torch.ones(2, 1))
    with pytest.raises(UnsupportedError, match="several output tasks"):
        m.prediction_cache()
    # task values 0..T-1: the reference's range message
    X0, Y0 = _data(tasks=(0, 1))
    m0 = MultiTaskGP(X0, Y0, task_feature=-1)
    Xq[:, -1] = 2.0
    with pytest.raises(ValueError, match="Expected all task features in `X` to be between 0 and"):
        m0.posterior(Xq)


def test_check_scaling_ignores_the_task_column():
    import warnings

    from botorch_amd.exceptions import InputDataWarning
    from botorch_amd.models import MultiTaskGP
    X, Y = _data(tasks=(3, 7))
    with warnings.catch_warnings():
        warnings.simplefilter("error", InputDataWarning)
        MultiTaskGP(X, Y, task_feature=-1)     # task values 3 and 7 are no scaling problem
    X[0, 0] = 1.5
    with pytest.warns(InputDataWarning):
        MultiTaskGP(X, Y, task_feature=-1)


def test_refusals():
    from botorch_amd.acquisition import qKnowledgeGradient, qProbabilityOfImprovement
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import MultiTaskGP
    from botorch_amd.pathwise import draw_matheron_paths
    from botorch_amd.sampling import SobolQMCNormalSampler
    X, Y = _data()
    m = MultiTaskGP(X, Y, task_feature=-1, output_tasks=[1]).eval()
    with pytest.raises(UnsupportedError, match="MultiTaskGP"):
        m.fantasize(X[:2, :2], SobolQMCNormalSampler(sample_shape=torch.Size([4])))
    with pytest.raises(UnsupportedError, match="MultiTaskGP"):
        m.condition_on_observations(X[:2], Y[:2])
    with pytest.raises(UnsupportedError, match="MultiTaskGP"):
        draw_matheron_paths(m, torch.Size([4]))
    with pytest.raises(UnsupportedError, match="MultiTaskGP"):
        qKnowledgeGradient(m, num_fantasies=4)
    with pytest.raises(UnsupportedError, match="MultiTaskGP"):
        qProbabilityOfImprovement(m, best_f=0.0)


def test_icm_layout_round_trip_and_bounds():
    from botorch_amd.fit import _ICMLayout, _layout
    from botorch_amd.models import ICM_VAR_LOWER, MultiTaskGP
    X, Y = _data(d=3, tasks=(0, 1, 2))
    for yvar, rank in ((None, 2), (torch.full_like(Y, 0.02), 3)):
        m = MultiTaskGP(X, Y, task_feature=-1, train_Yvar=yvar, rank=rank)
        lay = _layout(m)
        assert isinstance(lay, _ICMLayout)
        o = 0 if yvar is not None else 1
        assert lay.size == o + 1 + 3 + 1 + 3 * rank + 3 == len(lay.bounds)
        assert [s[0] for s in lay.segments] == (["noise"] if o else []) + [
            "constant", "lengthscale", "outputscale", "covar_factor", "var"]
        x0 = lay.get()
        np.testing.assert_array_equal(x0[lay.f0:lay.v0].reshape(3, rank),
                                      m.task_covar_module.covar_factor.detach().numpy())
        x = np.arange(1, lay.size + 1, dtype=np.float64) / 7.0
        lay.set(x)
        np.testing.assert_array_equal(lay.get(), x)
        np.testing.assert_array_equal(m.task_covar_module.covar_factor.detach().numpy().reshape(-1),
                                      x[lay.f0:lay.v0])       # row-major
        np.testing.assert_array_equal(m.task_covar_module.var.detach().numpy(), x[lay.v0:])
        if o:
            assert lay.bounds[0] == (1e-4, None)
        assert lay.bounds[o] == (None, None)
        assert lay.bounds[o + 1:o + 4] == [(m.covar_module.base_kernel.lengthscale_lower, None)] * 3
        assert lay.bounds[o + 4] == (0.0, None)
        assert lay.bounds[lay.f0:lay.v0] == [(None, None)] * (3 * rank)
        assert lay.bounds[lay.v0:] == [(ICM_VAR_LOWER, None)] * 3 and ICM_VAR_LOWER == 1e-6


# ---- priors -----------------------------------------------------------------------------------
def test_gamma_prior_matches_torch():
    from botorch_amd.fit import _prior_terms
    from botorch_amd.models import GammaPrior
    x = torch.tensor([0.05, 0.4, 1.3, 6.0], dtype=F64, requires_grad=True)
    for conc, rate in ((3.0, 6.0), (2.0, 0.15), (1.1, 0.05)):
        prior = GammaPrior(conc, rate)
        ref = torch.distributions.Gamma(torch.tensor(conc, dtype=F64),
                                        torch.tensor(rate, dtype=F64)).log_prob(x)
        torch.testing.assert_close(prior.log_prob(x.detach()), ref.detach(), rtol=1e-13, atol=1e-13)
        (gref,) = torch.autograd.grad(ref.sum(), x)
        val, grad = _prior_terms(prior, x.detach().numpy())
        assert abs(val - ref.sum().item()) < 1e-12
        np.testing.assert_allclose(grad, gref.numpy(), rtol=1e-13, atol=1e-13)
        assert abs(prior.mode - (conc - 1.0) / rate) < 1e-15


def test_lognormal_prior_terms_unchanged():
    """_prior_terms on a LogNormalPrior, bit for bit what it returned before it
    learned GammaPrior (the formula written out here)."""
    from botorch_amd.fit import _prior_terms
    from botorch_amd.models import LogNormalPrior
    x = np.array([0.03, 0.4, 1.0, 2.5, 17.0])
    for loc, scale in ((-4.0, 1.0), (math.sqrt(2.0) + 0.5 * math.log(6), math.sqrt(3.0))):
        val, grad = _prior_terms(LogNormalPrior(loc, scale), x)
        lx = np.log(x)
        ref = np.sum(-((lx - loc) ** 2) / (2 * scale ** 2) - math.log(scale)
                     - 0.5 * math.log(2 * math.pi) - lx)
        assert val == float(ref)
        np.testing.assert_array_equal(grad, -(lx - loc) / (scale ** 2 * x) - 1.0 / x)
    val, grad = _prior_terms(None, x)
    assert val == 0.0 and not grad.any()


# ---- the library ------------------------------------------------------------------------------
def _records():
    from botorch_amd import _lib
    return {"bo_icm_covar": (_lib.IcmCovarArgs, dict(kind=0, d=2, T=2, n=4, np=128)),
            "bo_icm_mll_terms": (_lib.IcmMllArgs, dict(kind=0, d=2, T=2, n=4, ld=128)),
            "bo_icm_task_view": (_lib.IcmTaskViewArgs, dict(T=2, t=0, n=4, np=128))}


def test_icm_entries_refuse_bad_arguments():
    """A wrong header, T outside 1..16, d outside 1..64 and a kind that is neither
    RBF nor Matern are BO_ERR_ARG with a message naming the entry; the records
    hold null pointers, so nothing can have been launched."""
    from botorch_amd import _lib
    lib = _lib.lib()
    assert lib.bo_version() == _lib.ABI_VERSION == 12
    assert set(_lib.ICM_RECORD_ENTRIES) == set(_records())
    for cname, rec in _lib.ICM_ARG_RECORDS.items():
        assert lib.bo_struct_size(cname.encode()) == ctypes.sizeof(rec)
    for sym, (rec, ok) in _records().items():
        assert sym in _lib.exported_symbols() and _lib.ICM_RECORD_ENTRIES[sym] is rec
        fn = getattr(lib, sym)
        a = rec(**ok)
        a.abi_version = _lib.ABI_VERSION + 1
        assert fn(ctypes.byref(a), None) == _lib.BO_ERR_ARG and sym.encode() in lib.bo_last_error()
        a = rec(**ok)
        a.struct_size = ctypes.sizeof(rec) - 8
        assert fn(ctypes.byref(a), None) == _lib.BO_ERR_ARG and sym.encode() in lib.bo_last_error()
        assert fn(None, None) == _lib.BO_ERR_ARG
        bad = [dict(T=17), dict(T=0)]
        if "d" in ok:
            bad += [dict(d=65), dict(d=0), dict(kind=2)]
        for change in bad:
            a = rec(**{**ok, **change})
            assert fn(ctypes.byref(a), None) == _lib.BO_ERR_ARG, (sym, change)
            msg = lib.bo_last_error().decode()
            assert sym in msg and str(list(change.values())[0]) in msg, msg
        # valid sizes but null pointers: still refused on the host
        assert fn(ctypes.byref(rec(**ok)), None) == _lib.BO_ERR_ARG
    a = _lib.IcmTaskViewArgs(T=2, t=2, n=4, np=128)
    assert lib.bo_icm_task_view(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert _lib.ICM_MAX_TASKS == 16 and _lib.ICM_MAX_DIM == 64


def test_icm_ops_registered_with_fake_shapes():
    import botorch_amd
    from botorch_amd import kernels, ops
    for name in ("icm_covar", "icm_mll_terms", "icm_task_view"):
        assert name in ops.OPS and hasattr(torch.ops.bo, name)
    meta = dict(device="meta", dtype=F64)
    n, d, T = 300, 6, 3
    X, ls, B = torch.empty(n, d, **meta), torch.empty(d, **meta), torch.empty(T, T, **meta)
    task = torch.empty(n, device="meta", dtype=torch.int32)
    A = torch.ops.bo.icm_covar(X, task, ls, B, 1, 1.7, 0.3)
    assert A.shape == (384, 384) and A.dtype == F64
    v = torch.empty(n, **meta)
    part = torch.ops.bo.icm_mll_terms(X, task, ls, B, 1, 1.7, A, A, v, v)
    assert part.shape == (n, d + 5 + T)
    U, Linv, alpha = torch.ops.bo.icm_task_view(A, v, task, B, 1)
    assert U.shape == Linv.shape == (384, 384) and alpha.shape == (n,)
    assert kernels.icm_fused_ok(16, 64) and not kernels.icm_fused_ok(17, 6)
    assert not kernels.icm_fused_ok(2, 65)
    for name in ("MultiTaskGP", "IndexKernel", "GammaPrior", "get_matern_kernel_with_gamma_prior",
                 "get_gaussian_likelihood_with_gamma_prior", "icm_mll_terms", "icm_mll_terms_torch"):
        assert name in botorch_amd.__all__ and getattr(botorch_amd, name) is not None
