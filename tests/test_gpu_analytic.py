"""LogExpectedImprovement, LogProbabilityOfImprovement, PosteriorStandardDeviation
and the constrained (Log)EI on the device: the fused route (posterior moments ->
bo::analytic) against the generic route (the safe_math chain on model.posterior)
and against the restatement (tests/analytic_restatement.py) on the CPU posterior of
tests/jes_restatement.py's GP, values and dX.

n = 24 (17 and 30 for the other members of the model list), d = 3 (9 for the
generic posterior underneath), targets with mean != 0 and std != 1,
hyperparameters set by hand (lengthscale 0.35, noise 1e-2, mean constant 0.1).
Bound (the project's kernel bound): max|got - ref| <= 1e-9 max|ref| + 1e-10.
The route under test has the other one raise, so a silent fall-back fails."""
import functools

import pytest
import torch

from tests import analytic_restatement as ar
from tests import jes_restatement as jr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
LS, NOISE, CONST, OSCALE = 0.35, 1e-2, 0.1, 1.4
SHAPES = [(1,), (17,), (300,), (3, 5)]
SINGLE = ["LogExpectedImprovement", "LogProbabilityOfImprovement", "PosteriorStandardDeviation"]
CONSTRAINED = ["LogConstrainedExpectedImprovement", "ConstrainedExpectedImprovement"]


def _bound(got, ref, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs().max().item()
    lim = 1e-9 * ref.abs().max().item() + 1e-10
    print(f"{what}: max err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def _data(n, d, t):
    g = torch.Generator().manual_seed(40 + 7 * t + n + d)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = (torch.sin(5 * X[:, :1] + t) * torch.cos(3 * X[:, 1:2]) + X[:, 2:3] ** 2) * 2.5 + 1.7 - t
    return X, Y


def _set_hypers(mm, d, matern):
    base = mm.covar_module.base_kernel if matern else mm.covar_module
    base.lengthscale = torch.full((1, d), LS, dtype=F64)
    mm.likelihood.noise = torch.tensor([NOISE], dtype=F64)
    mm.mean_module.constant = CONST


def _oracle(mm, X, d, matern):
    """(the CPU GP of the member, its outcome mean and std)."""
    ymean, ystd = mm.outcome_stats()
    gp = jr.make_gp(X, mm.train_targets.detach().cpu(), torch.full((d,), LS, dtype=F64), NOISE,
                    const=CONST, kind=jr.MATERN52 if matern else jr.RBF,
                    o=OSCALE if matern else 1.0)
    return gp, float(ymean), float(ystd)


@functools.lru_cache(maxsize=None)
def _setup(variant):
    """(model on the device, [(gp, ymean, ystd)] of its outputs on the CPU, d)."""
    from botorch_amd.models import MaternKernel, ModelListGP, ScaleKernel, SingleTaskGP
    d = 9 if variant == "d9" else 3
    matern = variant == "matern"
    if variant in ("rbf", "matern", "d9"):
        X, Y = _data(24, d, 0)
        kw = {"covar_module": ScaleKernel(MaternKernel(ard_num_dims=d), outputscale=OSCALE)} \
            if matern else {}
        model = SingleTaskGP(X.to(DEV), Y.to(DEV), **kw)
        members, Xs = [model], [X]
    elif variant == "mo3":
        X = _data(24, d, 0)[0]
        Y = torch.cat([_data(24, d, t)[1] for t in range(3)], dim=-1)
        model = SingleTaskGP(X.to(DEV), Y.to(DEV))
        members, Xs = list(model.models), [X] * 3
    else:  # "list3": different n per member
        pairs = [_data(n, d, t) for t, n in enumerate((24, 17, 30))]
        members = [SingleTaskGP(X.to(DEV), Y.to(DEV)) for X, Y in pairs]
        model, Xs = ModelListGP(*members), [p[0] for p in pairs]
    for mm in members:
        _set_hypers(mm, d, matern)
    model.eval()
    return model, [_oracle(mm, X, d, matern) for mm, X in zip(members, Xs)], d


def _points(shape, d):
    g = torch.Generator().manual_seed(200 + len(shape) + shape[0])
    return torch.rand(*shape, 1, d, generator=g, dtype=F64)


def _cpu_moments(oracles, X):
    """(mean, var), Mt x R, in outcome space, differentiable in X (CPU)."""
    X3 = X.reshape(-1, 1, X.shape[-1])
    means, variances = [], []
    for gp, ymean, ystd in oracles:
        mu, Sigma = jr.posterior(gp, X3)
        means.append(ymean + ystd * mu.reshape(-1))
        variances.append(ystd * ystd * Sigma.reshape(-1))
    return torch.stack(means), torch.stack(variances)


def _best_f(shape, base=1.9):
    """A scalar for one batch dimension, per last batch dimension otherwise."""
    return base if len(shape) == 1 else base + 0.1 * torch.arange(shape[-1], dtype=F64)


def _best_f_rows(best_f, shape):
    if not torch.is_tensor(best_f):
        return torch.tensor(best_f, dtype=F64)
    return torch.broadcast_to(best_f, shape).reshape(-1)


def _only(monkeypatch, acqf, route):
    """Force ``route`` and make the other one raise."""
    other = "_generic" if route == "fused" else "_fused"

    def boom(*a, **k):
        raise AssertionError(f"the {other[1:]} route was taken")
    monkeypatch.setattr(acqf, other, boom)
    acqf._route = route


def _value_and_grad(acqf, X):
    Xd = X.to(DEV).requires_grad_(True)
    val = acqf(Xd)
    (g,) = torch.autograd.grad(val.sum(), Xd)
    return val.detach(), g


def _check(monkeypatch, acqf, X, restate, what):
    Xo = X.clone().requires_grad_(True)
    ref = restate(Xo).reshape(X.shape[:-2])
    (gref,) = torch.autograd.grad(ref.sum(), Xo)
    assert gref.abs().max() > 0
    for route in ("fused", "generic"):
        with monkeypatch.context() as mp:
            _only(mp, acqf, route)
            val, g = _value_and_grad(acqf, X)
        _bound(val, ref, f"{what} {route} value")
        _bound(g, gref, f"{what} {route} dX")
    acqf._route = None
    assert acqf._fused_applies(X.reshape(-1, 1, X.shape[-1]).to(DEV))


@pytest.mark.parametrize("variant", ["rbf", "matern", "d9"])
@pytest.mark.parametrize("name", SINGLE)
def test_single_output_classes(monkeypatch, name, variant):
    from botorch_amd import acquisition
    model, oracles, d = _setup(variant)
    mode = {"LogExpectedImprovement": ar.LOG_EI, "LogProbabilityOfImprovement": ar.LOG_PI,
            "PosteriorStandardDeviation": ar.STD}[name]
    for shape in SHAPES if variant == "rbf" else SHAPES[1:2] + SHAPES[3:]:
        for maximize in (True, False):
            best_f = _best_f(shape)
            args = () if mode == ar.STD else (best_f,)
            acqf = getattr(acquisition, name)(model, *args, maximize=maximize)
            X = _points(shape, d)
            rows = _best_f_rows(best_f, shape)

            def restate(Xo):
                mean, var = _cpu_moments(oracles, Xo)
                return ar.analytic(mean, var, rows, mode, w=1.0 if maximize else -1.0)
            _check(monkeypatch, acqf, X, restate, f"{name} {variant} {shape} max={maximize}")


@pytest.mark.parametrize("variant", ["mo3", "list3"])
@pytest.mark.parametrize("name", CONSTRAINED)
def test_constrained_classes(monkeypatch, name, variant):
    from botorch_amd import acquisition
    model, oracles, d = _setup(variant)
    mode = ar.LOG_EI if name.startswith("Log") else ar.EI
    cases = [({0: (0.5, None), 2: (-2.0, 1.5)}, [(0, 0.5, 0.0, ar.LOWER), (2, -2.0, 1.5, ar.BOTH)]),
             ({2: (None, 0.4)}, [(2, 0.0, 0.4, ar.UPPER)])]
    for constraints, table in cases:
        for shape in SHAPES:
            maximize = len(shape) == 1
            best_f = _best_f(shape, 0.6)  # (within the objective's range: the plain CEI is not tiny)
            acqf = getattr(acquisition, name)(model, best_f, 1, constraints, maximize=maximize)
            X = _points(shape, d)
            rows = _best_f_rows(best_f, shape)

            def restate(Xo):
                mean, var = _cpu_moments(oracles, Xo)
                return ar.analytic(mean, var, rows, mode, obj=1, w=1.0 if maximize else -1.0,
                                   constraints=table)
            _check(monkeypatch, acqf, X, restate, f"{name} {variant} {sorted(constraints)} {shape}")


def test_posterior_transform_takes_the_generic_route(monkeypatch):
    from botorch_amd.acquisition import LogExpectedImprovement
    from botorch_amd.objective import ScalarizedPosteriorTransform
    model, oracles, d = _setup("mo3")
    wts = torch.tensor([0.5, -1.0, 0.25], dtype=F64)
    acqf = LogExpectedImprovement(model, 0.3,
                                  posterior_transform=ScalarizedPosteriorTransform(wts.to(DEV)))
    X = _points((17,), d)
    assert not acqf._fused_applies(X.to(DEV))

    def boom(*a, **k):
        raise AssertionError("the fused route was taken")
    monkeypatch.setattr(acqf, "_fused", boom)
    val, g = _value_and_grad(acqf, X)
    Xo = X.clone().requires_grad_(True)
    mean, var = _cpu_moments(oracles, Xo)
    ref = ar.analytic((wts[:, None] * mean).sum(0, keepdim=True),
                      (wts[:, None] ** 2 * var).sum(0, keepdim=True),
                      torch.tensor(0.3, dtype=F64), ar.LOG_EI)
    (gref,) = torch.autograd.grad(ref.sum(), Xo)
    _bound(val, ref, "scalarized value")
    _bound(g, gref, "scalarized dX")


def test_float32_and_far_point():
    """float32 X returns float32; far from the data, where EI is exactly 0, LogEI
    on the fused route is finite with a finite non-zero gradient."""
    from botorch_amd.acquisition import ExpectedImprovement, LogExpectedImprovement
    model, _, d = _setup("rbf")
    acqf = LogExpectedImprovement(model, 1.9)
    X = _points((17,), d)
    out = acqf(X.to(DEV).to(torch.float32))
    assert out.dtype == torch.float32 and out.shape == (17,)
    _bound(out.to(F64), acqf(X.to(torch.float32).to(F64).to(DEV)).to(torch.float32).to(F64), "fp32")
    far = torch.full((1, 1, d), 1.0 + 10 * LS, dtype=F64)
    best_f = 1.7 + 50 * 2.5
    ei, gei = _value_and_grad(ExpectedImprovement(model, best_f), far)
    assert ei.item() == 0.0 and not gei.any()
    lei, g = _value_and_grad(LogExpectedImprovement(model, best_f), far)
    assert torch.isfinite(lei).all() and lei.item() < -700
    assert torch.isfinite(g).all() and g.abs().max().item() > 0


@pytest.mark.parametrize("device_gen", [False, True])
@pytest.mark.parametrize("name", ["LogExpectedImprovement", "LogConstrainedExpectedImprovement"])
def test_optimize_acqf(name, device_gen):
    from botorch_amd import acquisition, optim
    from botorch_amd.exceptions import UnsupportedError
    variant = "rbf" if name == "LogExpectedImprovement" else "list3"
    model, _, d = _setup(variant)
    if name == "LogExpectedImprovement":
        acqf = acquisition.LogExpectedImprovement(model, 1.9)
    else:
        acqf = acquisition.LogConstrainedExpectedImprovement(model, 1.9, 1, {0: (0.5, None),
                                                                            2: (-2.0, 1.5)})
    bounds = torch.stack([torch.zeros(d, dtype=F64), torch.ones(d, dtype=F64)]).to(DEV)
    gen = optim.gen_candidates_device if device_gen else optim.gen_candidates_scipy
    torch.manual_seed(0)
    cand, val = optim.optimize_acqf(acqf, bounds, q=1, num_restarts=4, raw_samples=64,
                                    options={"seed": 11}, gen_candidates=gen)
    raw = optim.draw_raw_samples(bounds, 64, 1, seed=11)
    best_raw = optim.evaluate_raw_samples(acqf, raw).max().item()
    print(f"{name} device={device_gen}: {val.item():.6f} (best raw sample {best_raw:.6f})")
    assert cand.shape == (1, d) and torch.isfinite(val).all()
    assert val.item() >= best_raw
    assert (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
    assert abs(acqf(cand.unsqueeze(0)).item() - val.item()) <= 1e-9 * abs(val.item()) + 1e-10
    with pytest.raises(UnsupportedError, match="do not account for X_pending"):
        optim.optimize_acqf(acqf, bounds, q=2, num_restarts=2, raw_samples=16,
                            options={"seed": 11}, gen_candidates=gen, sequential=True)
