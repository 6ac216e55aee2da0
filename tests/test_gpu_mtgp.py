"""MultiTaskGP on the device: its posterior in every supported form of X against
the explicit (x, task) GP of tests/icm_restatement.py, the admitted acquisition
classes' fused routes against their own generic routes on the same model, and
fit_gpytorch_mll against scipy's L-BFGS-B over the restated loss."""
import numpy as np
import pytest
import torch

from tests import icm_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
VAL = dict(rtol=1e-6, atol=1e-8)      # the MC classes' fused-route bars (tests/test_gpu_mc_family.py)
GRAD = dict(rtol=1e-5, atol=1e-8)


def _bound(got, ref, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs().max().item()
    lim = 1e-9 * ref.abs().max().item() + 1e-10
    print(f"{what}: max err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


# name -> (points per task, d, raw task values, task_feature)
SHAPES = {"n40": ((25, 15), 3, (0, 1), -1), "n300": ((120, 100, 80), 6, (2, 5, 9), 1)}
HYPER = dict(noise=0.1, c=0.2, o=1.4)


def _problem(shape, seed=0):
    counts, d, raw, tf = SHAPES[shape]
    g = torch.Generator().manual_seed(17 * len(counts) + d + seed)
    n, T = sum(counts), len(counts)
    Xd = torch.rand(n, d, generator=g, dtype=F64)
    task = torch.cat([torch.full((c,), t, dtype=torch.long) for t, c in enumerate(counts)])
    perm = torch.randperm(n, generator=g)
    Xd, task = Xd[perm], task[perm]
    Y = (torch.sin(4 * Xd[:, 0]) + Xd[:, 1] ** 2 + 0.4 * task.to(F64) * torch.cos(3 * Xd[:, 2])
         + 0.05 * torch.randn(n, generator=g, dtype=F64)).unsqueeze(-1)
    Yvar = 0.01 + 0.02 * torch.rand(n, 1, generator=g, dtype=F64)
    ls = 0.3 + 0.5 * torch.rand(d, generator=g, dtype=F64)
    F = 0.8 * torch.randn(T, T, generator=g, dtype=F64)
    F[0] = 0.0
    F[0, :2] = torch.tensor([0.9, 0.2], dtype=F64)
    F[1, :2] = torch.tensor([-0.6, 0.5], dtype=F64)       # B[0, 1] = -0.44: anti-correlated tasks
    v = 0.2 + 0.3 * torch.rand(T, generator=g, dtype=F64)
    return Xd, task, Y, Yvar, ls, F, v


def _with_task_column(Xd, task_raw, tf):
    tf = tf % (Xd.shape[-1] + 1)
    return torch.cat([Xd[..., :tf], task_raw.to(F64).unsqueeze(-1), Xd[..., tf:]], dim=-1)


def _model(shape, kind, fixed=False, standardize=False, output_tasks=None, seed=0):
    from botorch_amd.models import MultiTaskGP, RBFKernel, ScaleKernel, Standardize
    counts, d, raw, tf = SHAPES[shape]
    Xd, task, Y, Yvar, ls, F, v = _problem(shape, seed)
    raw_t = torch.tensor(raw)[task]
    X = _with_task_column(Xd, raw_t, tf)
    m = MultiTaskGP(X.to(DEV), Y.to(DEV), task_feature=tf,
                    train_Yvar=Yvar.to(DEV) if fixed else None,
                    covar_module=ScaleKernel(RBFKernel(ard_num_dims=d)) if kind == R.RBF else None,
                    outcome_transform=Standardize(m=1) if standardize else None,
                    output_tasks=output_tasks)
    assert m.kind == kind
    m.covar_module.base_kernel.lengthscale = ls
    m.covar_module.outputscale = HYPER["o"]
    m.mean_module.constant = HYPER["c"]
    if not fixed:
        m.likelihood.noise = HYPER["noise"]
    with torch.no_grad():
        m.task_covar_module.covar_factor.copy_(F)
    m.task_covar_module.var = v
    # the model's (transformed) space on the host
    ymean, ystd = (Y.mean().item(), Y.std().item()) if standardize else (0.0, 1.0)
    y = ((Y - ymean) / ystd).squeeze(-1)
    noise = (Yvar / ystd ** 2).squeeze(-1) if fixed else HYPER["noise"]
    host = dict(X=Xd, task=task, y=y, ls=ls, noise=noise, c=HYPER["c"], o=HYPER["o"],
                B=R.task_covar(F, v), kind=kind, ymean=ymean, ystd=ystd)
    return m.eval(), host


def _reference(host, Xq, tq, observation_noise=False):
    mean, cov = R.posterior_explicit(host["X"], host["task"], host["y"], host["ls"], host["noise"],
                                     host["c"], host["o"], host["B"], host["kind"], Xq, tq)
    if observation_noise:
        nz = host["noise"]
        if torch.is_tensor(nz):  # the mean observed noise of each test point's task
            T = host["B"].shape[0]
            nz = torch.stack([nz[host["task"] == t].mean() for t in range(T)])[tq]
        else:
            nz = torch.full(tq.shape, nz, dtype=F64)
        cov = cov + torch.diag_embed(nz)
    return host["ymean"] + host["ystd"] * mean, host["ystd"] ** 2 * cov


def _force_route(monkeypatch, route):
    """The posterior's route switch: FUSED_QMAX = 0 sends every q to the generic kernels."""
    from botorch_amd import posteriors
    if route == "generic":
        monkeypatch.setattr(posteriors, "FUSED_QMAX", 0)
    else:
        def boom(*a, **k):
            raise AssertionError("the generic posterior route was taken")
        monkeypatch.setattr(posteriors._GeneralMoments, "apply", boom)


@pytest.mark.parametrize("route", ["fused", "generic"])
@pytest.mark.parametrize("kind", R.KINDS, ids=["rbf", "matern"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_posterior_matches_explicit_gp(monkeypatch, shape, kind, route):
    counts, d, raw, tf = SHAPES[shape]
    T = len(counts)
    g = torch.Generator().manual_seed(3)
    Xq = torch.rand(4, 3, d, generator=g, dtype=F64)
    Wt = torch.rand(4, 3, 3, generator=g, dtype=F64)
    raw_t = torch.tensor(raw)
    for fixed, standardize in ((False, False), (True, True)):
        m, host = _model(shape, kind, fixed=fixed, standardize=standardize)
        _force_route(monkeypatch, route)
        for t in range(T):
            tq = torch.full((4, 3), t, dtype=torch.long)
            for noise_on in (False, True):
                m_ref, c_ref = _reference(host, Xq, tq, noise_on)
                # X without the task column, the task by output_indices
                post = m.posterior(Xq.to(DEV), output_indices=[raw[t]], observation_noise=noise_on)
                assert post.mean.shape == (4, 3, 1)
                _bound(post.mean.squeeze(-1), m_ref, f"task {t} mean (no column)")
                _bound(post.covariance_matrix, c_ref, f"task {t} cov (no column)")
                # X with a uniform task column (in the middle of X for n300)
                post = m.posterior(_with_task_column(Xq, raw_t[tq], tf).to(DEV),
                                   observation_noise=noise_on)
                _bound(post.mean.squeeze(-1), m_ref, f"task {t} mean (column)")
                _bound(post.covariance_matrix, c_ref, f"task {t} cov (column)")
        # dX of the view route against autograd through the restatement
        tq = torch.full((4, 3), T - 1, dtype=torch.long)
        Xo = Xq.clone().requires_grad_(True)
        m_ref, c_ref = _reference(host, Xo, tq)
        (g_ref,) = torch.autograd.grad(m_ref.sum() + (c_ref * Wt).sum(), Xo)
        Xg = Xq.to(DEV).requires_grad_(True)
        post = m.posterior(Xg, output_indices=[raw[T - 1]])
        (g_dev,) = torch.autograd.grad(post.mean.sum() + (post.covariance_matrix * Wt.to(DEV)).sum(), Xg)
        _bound(g_dev, g_ref, "dX (view)")
        monkeypatch.undo()


@pytest.mark.parametrize("kind", R.KINDS, ids=["rbf", "matern"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_posterior_mixed_tasks_in_a_q_batch(shape, kind):
    """Task values that vary inside a q = 3 batch: the cross-task covariance blocks,
    observation noise per point's task, and dX."""
    counts, d, raw, tf = SHAPES[shape]
    T = len(counts)
    g = torch.Generator().manual_seed(4)
    Xq = torch.rand(4, 3, d, generator=g, dtype=F64)
    Wt = torch.rand(4, 3, 3, generator=g, dtype=F64)
    tq = torch.tensor([[0, 1, 0], [1, 1, 0], [T - 1, 0, 1], [0, T - 1, T - 1]])
    raw_t = torch.tensor(raw)
    for fixed, standardize in ((False, True), (True, False)):
        m, host = _model(shape, kind, fixed=fixed, standardize=standardize)
        for noise_on in (False, True):
            m_ref, c_ref = _reference(host, Xq, tq, noise_on)
            post = m.posterior(_with_task_column(Xq, raw_t[tq], tf).to(DEV), observation_noise=noise_on)
            _bound(post.mean.squeeze(-1), m_ref, "mean (mixed)")
            _bound(post.covariance_matrix, c_ref, "cov (mixed)")
        Xo = Xq.clone().requires_grad_(True)
        m_ref, c_ref = _reference(host, Xo, tq)
        (g_ref,) = torch.autograd.grad(m_ref.sum() + (c_ref * Wt).sum(), Xo)
        Xg = _with_task_column(Xq, raw_t[tq], tf).to(DEV).requires_grad_(True)
        post = m.posterior(Xg)
        (g_dev,) = torch.autograd.grad(post.mean.sum() + (post.covariance_matrix * Wt.to(DEV)).sum(), Xg)
        keep = [j for j in range(d + 1) if j != tf % (d + 1)]
        _bound(g_dev[..., keep], g_ref, "dX (mixed)")
        assert not g_dev[..., tf % (d + 1)].any()  # the task column carries no gradient


def test_prediction_cache_is_the_view_and_follows_the_parameters():
    """One output task: prediction_cache() is that task's view (no factor L); it is
    cached, and dropped with the base caches on any parameter change."""
    m, host = _model("n40", R.MATERN52, output_tasks=[1])
    c1 = m.prediction_cache()
    assert c1.L is None and c1 is m.prediction_cache() and c1.d == 3
    assert abs(c1.outputscale - HYPER["o"] * float(host["B"][1, 1])) < 1e-15
    Xq = torch.rand(2, 2, 3, dtype=F64)
    before = m.posterior(Xq.to(DEV)).mean
    m.task_covar_module.var = m.task_covar_module.var.detach() * 2.0
    c2 = m.prediction_cache()
    assert c2 is not c1 and c2.outputscale != c1.outputscale
    assert (m.posterior(Xq.to(DEV)).mean - before).abs().max() > 1e-6


# ---- the admitted acquisition classes -------------------------------------------------------------
def _value_and_grad(acqf, X):
    Xd = X.to(DEV).requires_grad_(True)
    val = acqf(Xd)
    (g,) = torch.autograd.grad(val.sum(), Xd)
    return val.detach().cpu(), g.cpu()


MC_CLASSES = ["qExpectedImprovement", "qLogExpectedImprovement", "qNoisyExpectedImprovement",
              "qLogNoisyExpectedImprovement", "qUpperConfidenceBound"]


@pytest.fixture(scope="module")
def n65_model():
    """n = 65 (40 source + 25 target points), d = 3, one output task."""
    from botorch_amd.models import MultiTaskGP, Standardize
    g = torch.Generator().manual_seed(9)
    Xd = torch.rand(65, 3, generator=g, dtype=F64)
    task = torch.cat([torch.zeros(40), torch.ones(25)])
    Y = (torch.sin(4 * Xd[:, 0]) + Xd[:, 1] ** 2 + 0.3 * task * torch.cos(3 * Xd[:, 2])
         + 0.05 * torch.randn(65, generator=g, dtype=F64)).unsqueeze(-1)
    X = torch.cat([Xd, task.to(F64).unsqueeze(-1)], dim=-1)
    torch.manual_seed(0)
    m = MultiTaskGP(X.to(DEV), Y.to(DEV), task_feature=-1, output_tasks=[1],
                    outcome_transform=Standardize(m=1))
    m.covar_module.base_kernel.lengthscale = torch.tensor([0.4, 0.6, 0.5], dtype=F64)
    m.covar_module.outputscale = 1.2
    m.likelihood.noise = 0.02
    with torch.no_grad():
        m.task_covar_module.covar_factor.copy_(torch.tensor([[0.9, 0.1], [0.7, -0.4]], dtype=F64))
    m.task_covar_module.var = torch.tensor([0.2, 0.3], dtype=F64)
    return m.eval(), Xd[task == 1], Y[task == 1]


def _make(name, model, Xb, Yb):
    from botorch_amd import acquisition as A
    from botorch_amd.sampling import SobolQMCNormalSampler
    sampler = SobolQMCNormalSampler(sample_shape=torch.Size([128]), seed=7)
    best_f = float(Yb.median())
    if name in ("qExpectedImprovement", "qLogExpectedImprovement"):
        return getattr(A, name)(model, best_f=best_f, sampler=sampler)
    if name in ("qNoisyExpectedImprovement", "qLogNoisyExpectedImprovement"):
        worst = Yb.squeeze(-1).argsort()[:10]   # a weak baseline: the improvement is not flat zero
        return getattr(A, name)(model, X_baseline=Xb[worst].to(DEV), sampler=sampler,
                                prune_baseline=False)
    return A.qUpperConfidenceBound(model, beta=2.0, sampler=sampler)


@pytest.mark.parametrize("name", MC_CLASSES)
def test_mc_fused_route_matches_generic_route(monkeypatch, name, n65_model):
    from botorch_amd.acquisition import MCAcquisitionFunction
    model, Xb, Yb = n65_model
    g = torch.Generator().manual_seed(21)
    X = torch.rand(3, 2, 3, generator=g, dtype=F64)
    acqf = _make(name, model, Xb, Yb)
    assert acqf._fused_eligible(X.to(DEV))
    with monkeypatch.context() as mp:
        def boom(*a, **k):
            raise AssertionError("the generic route was taken")
        mp.setattr(MCAcquisitionFunction, "_generic_forward", boom)
        v_f, g_f = _value_and_grad(acqf, X)
    with monkeypatch.context() as mp:
        mp.setattr(MCAcquisitionFunction, "_fused_eligible", lambda self, X: False)
        v_g, g_g = _value_and_grad(acqf, X)
    print(name, v_f.tolist(), v_g.tolist())
    assert g_g.abs().max() > 0
    torch.testing.assert_close(v_f, v_g, **VAL)
    torch.testing.assert_close(g_f, g_g, **GRAD)
    # X that carries the task column is not for the task view: the generic route
    Xt = torch.cat([X, torch.ones(3, 2, 1, dtype=F64)], dim=-1).to(DEV)
    assert not acqf._fused_eligible(Xt)
    if "Noisy" not in name:  # (X_baseline was given without the column)
        torch.testing.assert_close(acqf(Xt).cpu(), v_g, **VAL)


@pytest.mark.parametrize("name", ["ExpectedImprovement", "LogExpectedImprovement",
                                  "UpperConfidenceBound", "PosteriorMean"])
def test_analytic_fused_route_matches_generic_route(monkeypatch, name, n65_model):
    """q = 1: the route on the fused posterior (LogEI: its fused chain) against the
    generic posterior kernels (LogEI: its generic chain), the analytic suite's bound."""
    from botorch_amd import acquisition as A
    from botorch_amd import posteriors
    model, Xb, Yb = n65_model
    g = torch.Generator().manual_seed(22)
    X = torch.rand(3, 1, 3, generator=g, dtype=F64)
    args = {"ExpectedImprovement": (float(Yb.median()),), "LogExpectedImprovement": (float(Yb.median()),),
            "UpperConfidenceBound": (2.0,), "PosteriorMean": ()}[name]
    acqf = getattr(A, name)(model, *args)
    if name == "LogExpectedImprovement":
        assert acqf._fused_applies(X.to(DEV))
        acqf._route = "fused"
        v_f, g_f = _value_and_grad(acqf, X)
        acqf._route = "generic"
        v_g, g_g = _value_and_grad(acqf, X)
    else:
        v_f, g_f = _value_and_grad(acqf, X)
        with monkeypatch.context() as mp:
            mp.setattr(posteriors, "FUSED_QMAX", 0)
            v_g, g_g = _value_and_grad(acqf, X)
    assert g_g.abs().max() > 0
    _bound(v_f, v_g, f"{name} value")
    _bound(g_f, g_g, f"{name} dX")


def test_optimize_acqf_with_qlognei(n65_model):
    from botorch_amd.optim import optimize_acqf
    model, Xb, Yb = n65_model
    acqf = _make("qLogNoisyExpectedImprovement", model, Xb, Yb)
    bounds = torch.stack([torch.zeros(3, dtype=F64), torch.ones(3, dtype=F64)]).to(DEV)
    cand, val = optimize_acqf(acqf, bounds, q=2, num_restarts=4, raw_samples=32,
                              options={"maxiter": 20})
    assert cand.shape == (2, 3) and torch.isfinite(val).all()
    assert (cand >= 0).all() and (cand <= 1).all()


# ---- the fit --------------------------------------------------------------------------------------
def fit_problem():
    """n = 96 (64 source + 32 target points), d = 3: two correlated smooth tasks
    (the target is the source plus a small smooth shift) with 0.05 noise."""
    g = torch.Generator().manual_seed(11)
    Xd = torch.rand(96, 3, generator=g, dtype=F64)
    task = torch.cat([torch.zeros(64, dtype=torch.long), torch.ones(32, dtype=torch.long)])
    f = torch.sin(6 * Xd[:, 0]) * torch.cos(4 * Xd[:, 1]) + Xd[:, 2] ** 2
    Y = 0.3 * (f + 0.3 * task.to(F64) * torch.sin(3 * Xd[:, 1])) \
        + 0.05 * torch.randn(96, generator=g, dtype=F64)
    return Xd, task, Y.unsqueeze(-1)


def test_fit_reaches_restated_optimum():
    """fit_gpytorch_mll of a default MultiTaskGP (Standardize) from an explicit seeded
    start against scipy's L-BFGS-B over the restated loss from the same start and
    bounds: the fitted loss is within 1e-6 relative of scipy's or below it, the
    gradient at the fitted point matches the restated gradient with the MLL
    tolerances, and the fitted B correlates the tasks positively.  (B, not F: the
    factor is determined up to sign and rotation.)"""
    from scipy.optimize import minimize

    from botorch_amd.fit import (ExactMarginalLogLikelihood, _ICMLayout,
                                 fit_gpytorch_mll, icm_mll_value_and_grad)
    from botorch_amd.models import MultiTaskGP, Standardize
    Xd, task, Y = fit_problem()
    X = torch.cat([Xd, task.to(F64).unsqueeze(-1)], dim=-1)
    torch.manual_seed(5)
    m = MultiTaskGP(X.to(DEV), Y.to(DEV), task_feature=-1, outcome_transform=Standardize(m=1))
    lay = _ICMLayout(m)
    x0 = lay.get()
    x0[0] = 0.1                                  # noise: off the prior mode 2.0 (a far, flat start)
    x0[lay.f0:lay.v0] = [0.8, 0.1, 0.6, 0.4]     # F
    x0[lay.v0:] = [0.3, 0.3]                     # v
    lay.set(x0)
    fit_gpytorch_mll(ExactMarginalLogLikelihood(m.likelihood, m))
    x1 = lay.get()
    y = ((Y - Y.mean()) / Y.std()).squeeze(-1)

    def f(x):
        return R.neg_mll_flat(x, Xd, task, y, R.MATERN52, 2, 2)

    ref = minimize(f, x0, jac=True, method="L-BFGS-B", bounds=lay.bounds)
    v1, g1 = f(x1)
    v_dev, g_dev = icm_mll_value_and_grad(m, x1, lay)
    B = m.task_covar_module.covar_matrix.detach().cpu()
    Fr = torch.tensor(ref.x[lay.f0:lay.v0]).reshape(2, 2)
    B_ref = Fr @ Fr.T + torch.diag(torch.tensor(ref.x[lay.v0:]))
    print(f"x1 {x1}\nf(x1) {v1!r}  ref.fun {ref.fun!r}  B {B.tolist()}  B_ref {B_ref.tolist()}\n"
          f"max |g_dev - g1| {np.max(np.abs(g_dev - g1)):.3e}")
    assert v1 <= ref.fun + 1e-6 * abs(ref.fun)
    assert abs(v_dev - v1) < 1e-9 * max(1.0, abs(v1))
    np.testing.assert_allclose(g_dev, g1, rtol=1e-6, atol=1e-9)
    assert B[0, 1] > 0
