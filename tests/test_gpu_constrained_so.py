"""Outcome constraints on the public single-objective MC acquisitions
(qExpectedImprovement, qLogExpectedImprovement, qNoisyExpectedImprovement,
qLogNoisyExpectedImprovement with ``constraints=``) on the fused route, against
the CPU oracle.

Setup as tests/test_gpu_constrained_mobo.py: DTLZ2, n = 60, d = 6, fixed
hyperparameters; a model list of Mt in {2, 3} members, the last one fitted to a
smooth constraint function whose sign changes across the cube, one
ExactGPOracle per member, ``LinearMCObjective`` over the members.  The
reference samples all members as the oracle does (oracle.sampling's
multi-output base samples for qEI / qLogEI; QNEHVIOracle's baseline and
new-point samples for qNEI / qLogNEI) and feeds them to the torch restatement
tests/constrained_so_restatement.py.

Bars (those of test_gpu_generic.py and test_gpu_logei.py): plain values rtol
1e-6 / atol 1e-10, log values rtol 1e-6 / atol 1e-8, gradients w.r.t. X rtol
1e-5 / atol 1e-8.  In the route tests ``_generic_forward`` raises, so a silent
fall-back fails."""
import functools

import pytest
import torch

from tests.constrained_so_restatement import constrained_acq_from_samples

DEV = "cuda"
F64 = torch.float64
GRAD = dict(rtol=1e-5, atol=1e-8)
WEIGHTS = {2: [1.0, 0.0], 3: [1.0, -0.5, 0.0]}


def _val(log):
    return dict(rtol=1e-6, atol=1e-8 if log else 1e-10)


def _last(Z):
    return Z[..., -1]


def _mix(Z):
    return 0.5 * Z[..., 0] + Z[..., 1] - 1.2


def constraint_sets(Mt):
    """name -> (linear (A, b) or None, the same constraints as plain callables, eta)."""
    e_last = [0.0] * (Mt - 1) + [1.0]
    one = (torch.tensor([e_last], dtype=F64), torch.zeros(1, 1, dtype=F64))
    sets = {"one": (one, [_last], 1e-3)}
    if Mt == 3:
        two = (torch.tensor([e_last, [0.5, 1.0, 0.0]], dtype=F64), torch.tensor([[0.0], [1.2]], dtype=F64))
        sets["two"] = (two, [_last, _mix], torch.tensor([0.05, 0.1], dtype=F64))
    return sets


@functools.lru_cache(maxsize=None)
def _data(Mt, seed=0, n=60):
    """(X, Y (n x Mt), oracles), all on the CPU."""
    from botorch_amd.test_functions import DTLZ2
    from oracle.gp import ExactGPOracle, GPHyper
    m = Mt - 1
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, 6, generator=g, dtype=F64)
    Y = DTLZ2(dim=6, num_objectives=max(m, 2)).evaluate_true(X)[:, :m]
    Y = Y + 0.05 * torch.randn(n, m, generator=g, dtype=F64)
    c = X[:, 0] + 0.5 * torch.sin(3.0 * X[:, 1]) - 0.8 + 0.02 * torch.randn(n, generator=g, dtype=F64)
    assert 0.2 < (c <= 0).double().mean() < 0.8
    Y = torch.cat([Y, c.unsqueeze(-1)], dim=-1)
    oracles = [ExactGPOracle(X, Y[:, t:t + 1], GPHyper(torch.full((6,), 0.6, dtype=F64), 1e-2, 0.0))
               for t in range(Mt)]
    return X, Y, oracles


@functools.lru_cache(maxsize=None)
def _model(Mt):
    from botorch_amd.models import ModelListGP, SingleTaskGP
    X, Y, _ = _data(Mt)
    models = []
    for t in range(Mt):
        mm = SingleTaskGP(X.to(DEV), Y[:, t:t + 1].to(DEV))
        mm.covar_module.lengthscale = torch.full((1, 6), 0.6, dtype=F64)
        mm.likelihood.noise = torch.tensor([1e-2], dtype=F64)
        models.append(mm.eval())
    return ModelListGP(*models)


def _best_f(Mt):
    _, Y, _ = _data(Mt)
    return float((Y @ torch.tensor(WEIGHTS[Mt], dtype=F64)).median())


def _points(B, q, seed):
    return torch.rand(B, q, 6, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ---- references (CPU only) -----------------------------------------------------------
def qei_samples(Mt, S, seed):
    """X (b x q x d) -> the members' samples S x b x q x Mt, as the oracle draws them."""
    from oracle.acquisition import mc_samples
    from oracle.sampling import base_samples_multi_output
    oracles = _data(Mt)[2]

    def f(X):
        Z = base_samples_multi_output(S, X.shape[-2], Mt, seed)
        return torch.stack([mc_samples(*orc.posterior(X), Z[:, t]) for t, orc in enumerate(oracles)], dim=-1)
    return f


def nei_oracle(Mt, Xb, S, seed):
    """QNEHVIOracle over all members (its initial hypervolumes are not read: skipped)."""
    import oracle.acquisition as oacq
    orig = oacq.hypervolume
    oacq.hypervolume = lambda Y, ref: Y.new_zeros(())
    try:
        return oacq.QNEHVIOracle(_data(Mt)[2], Xb, [-1e6] * Mt, S, seed=seed)
    finally:
        oacq.hypervolume = orig


def nei_best_f(Mt, orc, cons):
    """The per-sample best feasible baseline objective (S), as the classes compute it."""
    from botorch_amd.objective import compute_best_feasible_objective
    w = torch.tensor(WEIGHTS[Mt], dtype=F64)
    return compute_best_feasible_objective(orc.Y_base, orc.Y_base @ w, cons)


def reference(samples_fn, Mt, best_f, cons, eta, log, fat, tau_max=1e-2):
    def ref(X):
        return constrained_acq_from_samples(samples_fn(X), WEIGHTS[Mt], best_f, cons, eta, log=log,
                                            fat=fat, tau_max=tau_max)
    return ref


def check_not_vacuous(samples_fn, Mt, best_f, cons, eta, Xc, fat=False):
    """The reference alone: plain value positive on at least half of the
    t-batches, weights below 0.1 and above 0.9 among the samples, gradient nonzero."""
    from botorch_amd.objective import compute_smoothed_feasibility_indicator
    Xo = Xc.clone().requires_grad_(True)
    f = samples_fn(Xo)
    plain = constrained_acq_from_samples(f, WEIGHTS[Mt], best_f, cons, eta)
    (g,) = torch.autograd.grad(plain.sum(), Xo)
    w = compute_smoothed_feasibility_indicator(cons, f.detach(), eta, fat=fat)
    assert (plain > 0).sum() * 2 >= plain.numel(), plain
    assert (w < 0.1).any() and (w > 0.9).any()
    assert g.abs().max() > 0


def _value_and_grad(acqf, Xc, dtype=F64):
    Xd = Xc.to(DEV, dtype).requires_grad_(True)
    v = acqf(Xd)
    (g,) = torch.autograd.grad(v.sum(), Xd)
    return v.detach().cpu(), g.cpu()


def _compare(acqf, Xc, ref_fn, log):
    v, gx = _value_and_grad(acqf, Xc)
    Xo = Xc.clone().requires_grad_(True)
    rv = ref_fn(Xo)
    (go,) = torch.autograd.grad(rv.sum(), Xo)
    print(f"value max|diff| = {(v - rv.detach()).abs().max().item():.3e} of {rv.abs().max().item():.3e}; "
          f"gradient max|diff| = {(gx - go).abs().max().item():.3e} of {go.abs().max().item():.3e}")
    assert torch.isfinite(rv).all() and go.abs().max() > 0
    torch.testing.assert_close(v, rv.detach(), **_val(log))
    torch.testing.assert_close(gx, go, **GRAD)
    with torch.no_grad():   # forward-only calls take the same kernels
        torch.testing.assert_close(acqf(Xc.to(DEV)).cpu(), v, rtol=0, atol=0)
    return v, gx


def _no_generic(monkeypatch):
    from botorch_amd.acquisition import MCAcquisitionFunction

    def boom(self, X):
        raise AssertionError("the generic route was taken")
    monkeypatch.setattr(MCAcquisitionFunction, "_generic_forward", boom)


def _make(kind, Mt, S, seed, cons, eta, Xb=None, sampler="single", **kw):
    from botorch_amd import acquisition as A
    from botorch_amd.objective import LinearMCObjective
    from botorch_amd.sampling import ListSampler, SobolQMCNormalSampler
    if sampler == "single":
        sampler = SobolQMCNormalSampler(torch.Size([S]), seed=seed)
    elif sampler == "list":
        sampler = ListSampler(*[SobolQMCNormalSampler(torch.Size([S]), seed=seed + t) for t in range(Mt)])
    common = dict(sampler=sampler, objective=LinearMCObjective(torch.tensor(WEIGHTS[Mt], dtype=F64, device=DEV)),
                  constraints=cons, eta=eta, **kw)
    if kind == "qEI":
        return A.qExpectedImprovement(_model(Mt), _best_f(Mt), **common)
    if kind == "qLogEI":
        return A.qLogExpectedImprovement(_model(Mt), _best_f(Mt), **common)
    cls = A.qNoisyExpectedImprovement if kind == "qNEI" else A.qLogNoisyExpectedImprovement
    kw2 = dict(prune_baseline=False)
    kw2.update(common)
    return cls(_model(Mt), Xb.to(DEV), **kw2)


CONFIGS = [(2, 1, 64, "one"), (3, 3, 128, "one"), (3, 3, 64, "two")]


def test_references_are_not_vacuous():
    """CPU: every configuration below, by the reference alone."""
    from botorch_amd.objective import get_outcome_constraint_transforms
    for Mt, q, S, cset in CONFIGS:
        lin, cons, eta = constraint_sets(Mt)[cset]
        Xc = _points(5, q, 10 * Mt + q)
        check_not_vacuous(qei_samples(Mt, S, 4), Mt, _best_f(Mt), cons, eta, Xc)
        orc = nei_oracle(Mt, _data(Mt)[0][:15], S, 3)
        check_not_vacuous(orc.samples, Mt, nei_best_f(Mt, orc, cons), cons, eta, Xc)
        # the linear callables are the same constraints
        f = qei_samples(Mt, S, 4)(Xc)
        for a, b in zip(get_outcome_constraint_transforms(lin), cons):
            torch.testing.assert_close(a(f), b(f), rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("Mt,q,S,cset", CONFIGS)
@pytest.mark.parametrize("kind", ["qEI", "qLogEI"])
def test_qei_constrained_matches_oracle(kind, Mt, q, S, cset, monkeypatch):
    from botorch_amd.objective import get_outcome_constraint_transforms
    _no_generic(monkeypatch)
    log = kind == "qLogEI"
    lin, cons, eta = constraint_sets(Mt)[cset]
    Xc = _points(5, q, 10 * Mt + q)
    ref = reference(qei_samples(Mt, S, 4), Mt, _best_f(Mt), cons, eta, log, fat=log)
    # in the kernel, and the same constraints as plain callables (the torch weight tensor)
    v_lin, g_lin = _compare(_make(kind, Mt, S, 4, get_outcome_constraint_transforms(lin), eta), Xc, ref, log)
    v_lam, g_lam = _compare(_make(kind, Mt, S, 4, cons, eta), Xc, ref, log)
    torch.testing.assert_close(v_lin, v_lam, **_val(log))
    torch.testing.assert_close(g_lin, g_lam, **GRAD)


@pytest.mark.gpu
@pytest.mark.parametrize("Mt,q,S,cset", CONFIGS)
@pytest.mark.parametrize("kind", ["qNEI", "qLogNEI"])
def test_qnei_constrained_matches_oracle(kind, Mt, q, S, cset, monkeypatch):
    """Over a model list with a single sampler: per-member cached baseline roots."""
    from botorch_amd.objective import get_outcome_constraint_transforms
    _no_generic(monkeypatch)
    log = kind == "qLogNEI"
    lin, cons, eta = constraint_sets(Mt)[cset]
    Xb = _data(Mt)[0][:15]
    orc = nei_oracle(Mt, Xb, S, 3)
    bf = nei_best_f(Mt, orc, cons)
    Xc = _points(5, q, 10 * Mt + q)
    ref = reference(orc.samples, Mt, bf, cons, eta, log, fat=log)
    a_lin = _make(kind, Mt, S, 3, get_outcome_constraint_transforms(lin), eta, Xb=Xb)
    torch.testing.assert_close(a_lin.baseline_samples.cpu(), orc.Y_base, rtol=1e-8, atol=1e-10)
    torch.testing.assert_close(a_lin._baseline_best_f.cpu(), bf, rtol=1e-8, atol=1e-10)
    v_lin, g_lin = _compare(a_lin, Xc, ref, log)
    v_lam, g_lam = _compare(_make(kind, Mt, S, 3, cons, eta, Xb=Xb), Xc, ref, log)
    torch.testing.assert_close(v_lin, v_lam, **_val(log))
    torch.testing.assert_close(g_lin, g_lam, **GRAD)


@pytest.mark.gpu
def test_qnei_constrained_batched_roots_match_per_member(monkeypatch):
    """As test_qnehvi_members_batched_roots_match_per_member, for constrained
    qNEI: at a size whose one-model plan splits k (n = 1024) the members'
    cached-root terms go as GEMMs batched over the members; value,
    forward-only value and gradient equal the per-member route (s^2 folded
    into the operands: rounding only)."""
    from botorch_amd import acquisition, kernels
    from botorch_amd.models import ModelListGP, SingleTaskGP
    from botorch_amd.objective import LinearMCObjective, get_outcome_constraint_transforms
    from botorch_amd.sampling import SobolQMCNormalSampler
    _no_generic(monkeypatch)
    Mt, n, r, B, q, S = 2, 1024, 40, 32, 4, 64
    assert kernels.split_plan(B, q, n)[0] != 0  # stream-K: the members' route applies
    g = torch.Generator().manual_seed(3)
    X = torch.rand(n, 6, generator=g, dtype=F64)
    Y = torch.stack([torch.sin(3.0 * X[:, 0]) + X[:, 1:].pow(2).sum(-1),
                     X[:, 0] + 0.5 * torch.sin(3.0 * X[:, 1]) - 0.8], dim=-1)
    Y = Y + 0.05 * torch.randn(n, Mt, generator=g, dtype=F64)
    models = []
    for t in range(Mt):
        mm = SingleTaskGP(X.to(DEV), Y[:, t:t + 1].to(DEV))
        mm.covar_module.lengthscale = torch.full((1, 6), 0.6, dtype=F64)
        mm.likelihood.noise = torch.tensor([1e-2], dtype=F64)
        models.append(mm.eval())
    lin, _, eta = constraint_sets(Mt)["one"]
    acqf = acquisition.qNoisyExpectedImprovement(
        ModelListGP(*models), X[:r].to(DEV), sampler=SobolQMCNormalSampler(torch.Size([S]), seed=0),
        objective=LinearMCObjective(torch.tensor(WEIGHTS[Mt], dtype=F64, device=DEV)),
        constraints=get_outcome_constraint_transforms(lin), eta=eta, prune_baseline=False)
    Xc = _points(B, q, 1).to(DEV)
    calls = []
    orig = acquisition._roots_forward_batched

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    monkeypatch.setattr(acquisition, "_roots_forward_batched", spy)

    def run():
        v, gx = _value_and_grad(acqf, Xc)
        with torch.no_grad():
            v2 = acqf(Xc).cpu()
        kernels.check_ladder_status(DEV)
        return v, gx, v2

    v1, g1, w1 = run()
    assert calls, "the batched roots route did not run"
    monkeypatch.setattr(acquisition, "_roots_batched", lambda *a, **k: False)
    n1 = len(calls)
    v0, g0, w0 = run()
    assert len(calls) == n1, "the per-member route was not taken"
    assert (v0 > 0).sum() > 5
    torch.testing.assert_close(v1, v0, rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(w1, w0, rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(g1, g0, rtol=1e-8, atol=1e-11)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["qEI", "qLogEI"])
def test_list_sampler_draws_the_generic_routes_samples(kind):
    """A ListSampler of Mt samplers: the fused value is the generic route's on
    the very same sampler."""
    from botorch_amd.objective import get_outcome_constraint_transforms
    Mt, q, S = 3, 3, 64
    log = kind == "qLogEI"
    lin, cons, eta = constraint_sets(Mt)["two"]
    acqf = _make(kind, Mt, S, 11, get_outcome_constraint_transforms(lin), eta, sampler="list")
    Xc = _points(5, q, 21)
    v, g = _value_and_grad(acqf, Xc)
    Xd = Xc.to(DEV).requires_grad_(True)
    vg = acqf._generic_forward(Xd)
    (gg,) = torch.autograd.grad(vg.sum(), Xd)
    assert vg.abs().max() > 0 and gg.abs().max() > 0
    torch.testing.assert_close(v, vg.detach().cpu(), **_val(log))
    torch.testing.assert_close(g, gg.cpu(), **GRAD)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["qEI", "qLogNEI"])
def test_x_pending(kind, monkeypatch):
    from botorch_amd.objective import get_outcome_constraint_transforms
    _no_generic(monkeypatch)
    Mt, q, S = 2, 2, 64
    log = kind == "qLogNEI"
    lin, cons, eta = constraint_sets(Mt)["one"]
    Xb = _data(Mt)[0][:15]
    Xp = _points(1, 1, 77)[0]                  # one pending point
    acqf = _make(kind, Mt, S, 5, get_outcome_constraint_transforms(lin), eta, Xb=Xb)
    acqf.set_X_pending(Xp.to(DEV))
    if kind == "qEI":
        samples, bf = qei_samples(Mt, S, 5), _best_f(Mt)
    else:
        orc = nei_oracle(Mt, Xb, S, 5)
        samples, bf = orc.samples, nei_best_f(Mt, orc, cons)
    inner = reference(samples, Mt, bf, cons, eta, log, fat=log)

    def ref(X):
        return inner(torch.cat([X, Xp.expand(X.shape[0], 1, 6)], dim=-2))
    _compare(acqf, _points(5, q, 31), ref, log)


@pytest.mark.gpu
def test_qnei_prune_baseline(monkeypatch):
    from botorch_amd.objective import get_outcome_constraint_transforms
    Mt, q, S = 2, 3, 64
    lin, cons, eta = constraint_sets(Mt)["one"]
    torch.manual_seed(0)
    acqf = _make("qNEI", Mt, S, 9, get_outcome_constraint_transforms(lin), eta, Xb=_data(Mt)[0][:30],
                 prune_baseline=True)
    _no_generic(monkeypatch)
    Xb = acqf.X_baseline.cpu()
    assert 0 < Xb.shape[0] < 30
    orc = nei_oracle(Mt, Xb, S, 9)
    torch.testing.assert_close(acqf.baseline_samples.cpu(), orc.Y_base, rtol=1e-8, atol=1e-10)
    # the class's own baseline best: a sample without a feasible pruned point
    # takes the model's (randomised) lower bound, which no oracle restates
    bf = acqf._baseline_best_f.cpu()
    if (orc.Y_base[..., -1] <= 0).any(-1).all():
        torch.testing.assert_close(bf, nei_best_f(Mt, orc, cons), rtol=1e-8, atol=1e-10)
    _compare(acqf, _points(5, q, 41), reference(orc.samples, Mt, bf, cons, eta, False, False), False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["qLogEI", "qNEI"])
def test_fp32_x_in_and_out(kind, monkeypatch):
    """fp32 X: the model computes in fp64 on the same inputs; value and
    gradient return in fp32 (their own rounding: 6e-8 relative)."""
    from botorch_amd.objective import get_outcome_constraint_transforms
    _no_generic(monkeypatch)
    Mt, q, S = 2, 3, 64
    lin, cons, eta = constraint_sets(Mt)["one"]
    acqf = _make(kind, Mt, S, 2, get_outcome_constraint_transforms(lin), eta, Xb=_data(Mt)[0][:15])
    X32 = _points(5, q, 51).float()
    v32, g32 = _value_and_grad(acqf, X32, torch.float32)
    v64, g64 = _value_and_grad(acqf, X32.double())
    assert v32.dtype == torch.float32 and g32.dtype == torch.float32
    torch.testing.assert_close(v32.double(), v64, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(g32.double(), g64, rtol=1e-6, atol=1e-7)


@pytest.mark.gpu
def test_optimize_acqf_constrained_qlognei():
    """4 restarts, q = 2: L-BFGS-B never ends below its start and the
    initialisation keeps the best raw sample, so the returned value is at least
    the best raw-sample value (up to the rounding between two batch shapes)."""
    from botorch_amd.objective import get_outcome_constraint_transforms
    from botorch_amd.optim import optimize_acqf
    from botorch_amd.utils_sampling import draw_sobol_samples
    Mt, S = 2, 64
    lin, cons, eta = constraint_sets(Mt)["one"]
    acqf = _make("qLogNEI", Mt, S, 6, get_outcome_constraint_transforms(lin), eta, Xb=_data(Mt)[0][:15])
    bounds = torch.stack([torch.zeros(6, dtype=F64), torch.ones(6, dtype=F64)]).to(DEV)
    raw = draw_sobol_samples(bounds=bounds.cpu(), n=16, q=2, seed=0).to(DEV)
    with torch.no_grad():
        best_raw = float(acqf(raw).max())
    torch.manual_seed(0)
    cand, val = optimize_acqf(acqf, bounds, q=2, num_restarts=4, raw_samples=16,
                              options={"maxiter": 20, "seed": 0})
    assert cand.shape == (2, 6) and (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
    assert float(val) >= best_raw - 1e-9 * abs(best_raw)


@pytest.mark.gpu
def test_graph_capture_declines_the_fused_route(monkeypatch):
    """Under a graph capture the constrained acquisition takes the route it
    took before this one existed (the generic forward); the eager warm-up
    calls around it take the fused kernels."""
    from botorch_amd import graphs, kernels
    from botorch_amd.acquisition import MCAcquisitionFunction
    from botorch_amd.objective import get_outcome_constraint_transforms
    Mt, q, S = 2, 2, 64
    lin, cons, eta = constraint_sets(Mt)["one"]
    acqf = _make("qLogEI", Mt, S, 8, get_outcome_constraint_transforms(lin), eta)
    calls = {"fused": [], "generic": []}
    real = kernels.qmc_feas

    def spy(*a, **k):
        calls["fused"].append(kernels._dev_index(a[0].device) in kernels._CAPTURE)
        return real(*a, **k)

    def generic(self, X):
        calls["generic"].append(kernels._dev_index(X.device) in kernels._CAPTURE)
        return X.new_zeros(X.shape[:-2])
    monkeypatch.setattr(kernels, "qmc_feas", spy)
    monkeypatch.setattr(MCAcquisitionFunction, "_generic_forward", generic)
    X = _points(4, q, 61).to(DEV)
    graphs.graphed(acqf, X)(X)
    assert calls["fused"] and not any(calls["fused"])      # the warm-up calls, eager
    assert calls["generic"] == [True]                      # the captured call


@pytest.mark.gpu
def test_other_configurations_keep_their_route(monkeypatch):
    """A ListSampler on qNEI, and a call without constraints on a model list,
    go where they went: the generic forward."""
    from botorch_amd.acquisition import MCAcquisitionFunction
    Mt, q, S = 2, 2, 32
    lin, cons, eta = constraint_sets(Mt)["one"]
    seen = []
    real = MCAcquisitionFunction._generic_forward

    def generic(self, X):
        seen.append(type(self).__name__)
        return real(self, X)
    monkeypatch.setattr(MCAcquisitionFunction, "_generic_forward", generic)
    X = _points(3, q, 71).to(DEV)
    with pytest.warns(RuntimeWarning, match="cache_root"):
        nei = _make("qLogNEI", Mt, S, 1, cons, eta, Xb=_data(Mt)[0][:10], sampler="list")
    assert torch.isfinite(nei(X)).all()
    assert torch.isfinite(_make("qEI", Mt, S, 1, None, eta, sampler="list")(X)).all()
    assert seen == ["qLogNoisyExpectedImprovement", "qExpectedImprovement"]
