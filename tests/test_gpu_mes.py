"""qMaxValueEntropy and qLowerBoundMaxValueEntropy (GIBBON) on the device against
autograd through the restatement (tests/mes_restatement.py on the posterior of
tests/jes_restatement.py's GP), fed the same max values and base samples:
values and dX.

n = 48, d = 3, targets with mean != 0 and std != 1, hyperparameters set by hand
(lengthscale 0.35, noise 1e-2, mean constant 0.1).  Bars (the project's
end-to-end bars, those of tests/test_gpu_jes.py): values rtol 1e-7, gradients
rtol 1e-5, each with the absolute floor 1e-8.  The fused tests make ``_generic``
raise, so a silent fall-back fails; the reference gradient is asserted non-zero
before the device is asked."""
import functools
import warnings

import pytest
import torch

from tests import jes_restatement as jr
from tests import mes_restatement as mr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
VAL = dict(rtol=1e-7, atol=1e-8)
GRAD = dict(rtol=1e-5, atol=1e-8)
N, D = 48, 3
LS, NOISE, CONST, OSCALE = 0.35, 1e-2, 0.1, 1.4
BS = [1, 5, 130]
NAMES = ["qMaxValueEntropy", "qLowerBoundMaxValueEntropy"]


# ---- data, model, restatement ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _setup(variant="homo"):
    """(model on the device, the restatement's GP on the CPU, (ymean, ystd, tau2))."""
    from botorch_amd.models import MaternKernel, ScaleKernel, SingleTaskGP
    g = torch.Generator().manual_seed(3)
    X = torch.rand(N, D, generator=g, dtype=F64)
    Y = (torch.sin(5 * X[:, :1]) * torch.cos(3 * X[:, 1:2]) + X[:, 2:] ** 2) * 2.5 + 1.7
    Yvar = (0.5 + torch.rand(N, 1, generator=g, dtype=F64)) * 0.02 if variant == "fixed" else None
    kw = {}
    if variant == "notransform":
        kw["outcome_transform"] = None
    if variant == "matern":
        kw["covar_module"] = ScaleKernel(MaternKernel(ard_num_dims=D), outputscale=OSCALE)
    m = SingleTaskGP(X.to(DEV), Y.to(DEV), None if Yvar is None else Yvar.to(DEV), **kw)
    base = m.covar_module.base_kernel if variant == "matern" else m.covar_module
    base.lengthscale = torch.full((1, D), LS, dtype=F64)
    if variant != "fixed":
        m.likelihood.noise = torch.tensor([NOISE], dtype=F64)
    m.mean_module.constant = CONST
    m.eval()
    ymean, ystd = m.outcome_stats()
    assert variant == "notransform" or (abs(ymean) > 0.05 and abs(ystd - 1) > 0.1)
    noise = m.likelihood.noise.detach().cpu().reshape(-1) if variant == "fixed" else NOISE
    gp = jr.make_gp(X, m.train_targets.detach().cpu(), torch.full((D,), LS, dtype=F64), noise,
                    const=CONST, kind=jr.MATERN52 if variant == "matern" else jr.RBF,
                    o=OSCALE if variant == "matern" else 1.0)
    return m, gp, (float(ymean), float(ystd), float(gp.tau2) * float(ystd) ** 2)


def _candidates():
    return torch.rand(200, D, generator=torch.Generator().manual_seed(21), dtype=F64)


@functools.lru_cache(maxsize=None)
def _pool():
    """130 random points, the one with the largest posterior mean + 2 sigma of the
    restatement's GP first: far below the max values both acquisition functions
    are flat to rounding, and the B = 1 case must have a gradient to compare."""
    X = torch.rand(130, 1, D, generator=torch.Generator().manual_seed(101), dtype=F64)
    mu, Sigma = jr.posterior(_setup("homo")[1], X)
    best = (mu[:, 0] + 2.0 * Sigma[:, 0, 0].sqrt()).argmax()
    return torch.cat([X[best:best + 1], X[:best], X[best + 1:]])


def _points(B):
    return _pool()[:B].clone()


def _pending(m):
    return torch.rand(m, D, generator=torch.Generator().manual_seed(77 + m), dtype=F64)


@functools.lru_cache(maxsize=None)
def _acqf(name, variant="homo", maximize=True, use_gumbel=True, m=0):
    """One acquisition function per configuration, built once (its max values
    and base samples are what the restatement is fed)."""
    from botorch_amd import acquisition
    torch.manual_seed(5)
    kw = dict(maximize=maximize, use_gumbel=use_gumbel)
    if m:
        kw["X_pending"] = _pending(m).to(DEV)
    return getattr(acquisition, name)(_setup(variant)[0], _candidates().to(DEV), **kw)


def _outcome_moments(variant, X):
    """(mu B, Sigma B x q x q) in outcome space of the restatement's GP."""
    _, gp, (ymean, ystd, _) = _setup(variant)
    mu, Sigma = jr.posterior(gp, X)
    return ymean + ystd * mu, ystd * ystd * Sigma


def _restate(acqf, variant, X):
    """The restatement's value at X (B x 1 x d, CPU) with acqf's max values,
    base samples and pending points."""
    tau2 = _setup(variant)[2][2]
    fstar = acqf.posterior_max_values.detach().cpu().reshape(-1).to(F64)
    w = 1.0 if acqf.maximize else -1.0
    if type(acqf).__name__ == "qMaxValueEntropy":
        mu, Sigma = _outcome_moments(variant, X)
        return mr.mes(mu[:, 0], Sigma[:, 0, 0], fstar, acqf.base_samples.cpu(), tau2, w).ig
    if acqf.X_pending is None:
        mu, Sigma = _outcome_moments(variant, X)
        return mr.gibbon(mu[:, 0], Sigma[:, 0, 0], fstar, tau2, w).acq
    Xp = acqf.X_pending.detach().cpu().to(F64)
    m = Xp.shape[0]
    mu, Sigma = _outcome_moments(variant, torch.cat([X, Xp.expand(X.shape[0], m, D)], dim=1))
    Binv = torch.linalg.inv(Sigma[0, 1:, 1:].detach() + tau2 * torch.eye(m, dtype=F64))
    return mr.gibbon(mu[:, 0], Sigma[:, 0, 0], fstar, tau2, w, Sigma[:, 0, 1:], Binv).acq


def _reference(acqf, variant, X):
    Xo = X.clone().requires_grad_(True)
    val = _restate(acqf, variant, Xo)
    (g,) = torch.autograd.grad(val.sum(), Xo)
    assert g.abs().max() > 1e-6
    return val.detach(), g


def _no_route(monkeypatch, name, route):
    from botorch_amd import acquisition

    def boom(self, *a):
        raise AssertionError(f"the {route[1:]} route was taken")
    monkeypatch.setattr(getattr(acquisition, name), route, boom)


def _value_and_grad(acqf, X):
    Xd = X.to(DEV).requires_grad_(True)
    val = acqf(Xd)
    (g,) = torch.autograd.grad(val.sum(), Xd)
    return val.detach().cpu(), g.cpu()


def _report(what, got, ref):
    err = ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    print(f"{what}: max rel err {err:.3e}, max abs err {(got - ref).abs().max().item():.3e}")


def _check(acqf, variant, X, what):
    ref, gref = _reference(acqf, variant, X)
    val, g = _value_and_grad(acqf, X)
    assert val.shape == X.shape[:1]
    _report(f"value {what}", val, ref)
    _report(f"dX    {what}", g, gref)
    torch.testing.assert_close(val, ref, **VAL)
    torch.testing.assert_close(g, gref, **GRAD)
    return val, g


# ---- the fused route --------------------------------------------------------------------
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", NAMES)
def test_fused_value_and_gradient(name, B, monkeypatch):
    _no_route(monkeypatch, name, "_generic")
    acqf = _acqf(name)
    val, _ = _check(acqf, "homo", _points(B), f"{name} B={B}")
    with torch.no_grad():  # the forward-only call gives the same value
        torch.testing.assert_close(acqf(_points(B).to(DEV)).cpu(), val, rtol=0, atol=0)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name, m", [(NAMES[0], 0), (NAMES[1], 0), (NAMES[1], 4)])
def test_routes_agree(name, m, B):
    acqf = _acqf(name, m=m)
    X = _points(B)
    out = {}
    try:
        for route in ("fused", "generic"):
            acqf._route = route
            out[route] = _value_and_grad(acqf, X)
    finally:
        acqf._route = None
    _report(f"fused vs generic value {name} m={m} B={B}", out["fused"][0], out["generic"][0])
    torch.testing.assert_close(out["fused"][0], out["generic"][0], **VAL)
    torch.testing.assert_close(out["fused"][1], out["generic"][1], **GRAD)
    ref, gref = _reference(acqf, "homo", X)
    torch.testing.assert_close(out["generic"][0], ref, **VAL)
    torch.testing.assert_close(out["generic"][1], gref, **GRAD)


def test_forced_route_is_taken(monkeypatch):
    _no_route(monkeypatch, NAMES[0], "_fused")
    acqf = _acqf(NAMES[0])
    acqf._route = "generic"
    try:
        with torch.no_grad():
            acqf(_points(2).to(DEV))
    finally:
        acqf._route = None


def test_wrong_q_raises_the_shape_error():
    with pytest.raises(AssertionError, match="Expected X to be `batch_shape x q=1 x d`"):
        _acqf(NAMES[1])(torch.rand(2, 2, D, dtype=F64, device=DEV))


# ---- GIBBON's pending points -----------------------------------------------------------
@pytest.mark.parametrize("m", [1, 4, 15])
def test_gibbon_pending_fused(m, monkeypatch):
    _no_route(monkeypatch, NAMES[1], "_generic")
    acqf = _acqf(NAMES[1], m=m)
    val, _ = _check(acqf, "homo", _points(5), f"GIBBON m={m}")
    plain = _restate(_acqf(NAMES[1]), "homo", _points(5))
    assert (val - plain).abs().max() > 1e-4  # the pending points matter


def test_gibbon_sixteen_pending_takes_the_generic_route(monkeypatch):
    _no_route(monkeypatch, NAMES[1], "_fused")
    acqf = _acqf(NAMES[1], m=16)
    _check(acqf, "homo", _points(5), "GIBBON m=16 (generic)")


def test_gibbon_repulsion_is_the_posterior_logdet_identity():
    """One row on a model without outcome transform: the value with pending
    points minus the value without (same max values) is
    (logdet V - logdet B - log vm) / 2 for V the noisy joint posterior
    covariance of [x; X_pending], B its pending block and vm = V[0, 0]."""
    from botorch_amd.acquisition import qLowerBoundMaxValueEntropy
    model = _setup("notransform")[0]
    torch.manual_seed(1)
    acqf = qLowerBoundMaxValueEntropy(model, _candidates().to(DEV))
    fstar = acqf.posterior_max_values.clone()
    x, Xp = _points(1).to(DEV), _pending(4).to(DEV)
    with torch.no_grad():
        plain = acqf(x)
        acqf.set_X_pending(Xp)
        assert not torch.equal(acqf.posterior_max_values, fstar)  # redrawn
        acqf.posterior_max_values = fstar
        full = acqf(x)
        V = model.posterior(torch.cat([x[0], Xp]), observation_noise=True).distribution \
            .covariance_matrix
    want = 0.5 * (torch.logdet(V) - torch.logdet(V[1:, 1:]) - torch.log(V[0, 0]))
    print(f"repulsion {(full - plain).item():.12e}, log-determinant identity {want.item():.12e}")
    assert want.abs() > 1e-4
    torch.testing.assert_close((full - plain).reshape(()), want, rtol=1e-7, atol=1e-10)


# ---- variants -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_minimize(name, monkeypatch):
    _no_route(monkeypatch, name, "_generic")
    acqf = _acqf(name, maximize=False)
    X = _points(5)
    val, _ = _check(acqf, "homo", X, f"{name} minimize")
    # the max values are those of -f: not far below the largest negated training target
    ymean, ystd, _ = _setup("homo")[2]
    y = ymean + ystd * _setup("homo")[0].train_targets.detach().cpu()
    assert acqf.posterior_max_values.cpu().min() > (-y).max() - 1.0


@pytest.mark.parametrize("variant", ["notransform", "matern", "fixed"])
@pytest.mark.parametrize("name", NAMES)
def test_model_variants(name, variant, monkeypatch):
    """No outcome transform, ScaleKernel(MaternKernel), fixed noise (the
    default variant of every other test has Standardize)."""
    _no_route(monkeypatch, name, "_generic")
    _check(_acqf(name, variant), variant, _points(5), f"{name} {variant}")


@pytest.mark.parametrize("name", NAMES)
def test_fp32_inputs(name, monkeypatch):
    """fp32 X is computed in fp64 and returned in fp32: the reference is the
    restatement at the rounded points, the bars those of fp32's rounding."""
    _no_route(monkeypatch, name, "_generic")
    acqf = _acqf(name)
    X32 = _points(5).float()
    ref, gref = _reference(acqf, "homo", X32.double())
    Xd = X32.to(DEV).requires_grad_(True)
    val = acqf(Xd)
    (g,) = torch.autograd.grad(val.sum(), Xd)
    assert val.dtype == torch.float32 and g.dtype == torch.float32
    torch.testing.assert_close(val.cpu(), ref.float(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(g.cpu(), gref.float(), rtol=1e-5, atol=1e-6)


# ---- the max values -----------------------------------------------------------------------
@pytest.mark.parametrize("maximize", [True, False])
def test_gumbel_max_values(maximize):
    from botorch_amd import ops  # noqa: F401
    from botorch_amd.acquisition import _mv_moments
    acqf = _acqf(NAMES[1], maximize=maximize)
    mv = acqf.posterior_max_values
    assert mv.shape == (10, 1) and torch.isfinite(mv).all()
    assert acqf.candidate_set.shape == (200 + N, D)  # the training inputs are appended
    with torch.no_grad():
        mu, sigma = _mv_moments(acqf.model, acqf.candidate_set, maximize)
    y, status = torch.ops.bo.mv_quantiles(mu, sigma, False, 0.0, 0.0)
    assert status.tolist() == [0, 0, 0] and y[0] < y[1] < y[2]
    # against the restatement's bisection on the same moments
    ref, _ = mr.quantiles(mu.cpu(), sigma.cpu())
    torch.testing.assert_close(y.cpu(), ref, rtol=0, atol=1e-11)
    assert y[1] > mu.max() - 1e-9  # the median of the maximum lies above every mean


@pytest.mark.parametrize("maximize", [True, False])
def test_thompson_max_values(maximize):
    from botorch_amd.acquisition import _mv_moments
    acqf = _acqf(NAMES[1], maximize=maximize, use_gumbel=False)
    mv = acqf.posterior_max_values
    assert mv.shape == (10, 1) and torch.isfinite(mv).all()
    model = acqf.model
    with torch.no_grad():
        mu, sigma = _mv_moments(model, model.train_inputs[0], maximize)
    i = mu.argmax()
    assert mv.min() >= mu[i] - 6.0 * sigma[i]


def test_mes_refuses_pending_points():
    from botorch_amd.exceptions import UnsupportedError
    with pytest.raises(UnsupportedError, match="GIBBON"):
        _acqf(NAMES[0]).set_X_pending(_pending(1).to(DEV))


# ---- the pipeline -------------------------------------------------------------------------
def _bounds():
    return torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)]).to(DEV)


@pytest.mark.parametrize("name, q, sequential", [(NAMES[0], 1, False), (NAMES[1], 1, False),
                                                 (NAMES[1], 3, True)])
def test_optimize_acqf(name, q, sequential):
    """optimize_acqf with gen_candidates_scipy: candidates inside the bounds, the
    returned values equal to a re-evaluation (with the max values of the greedy
    step they were computed at), the max values redrawn after each greedy step."""
    from botorch_amd import acquisition
    from botorch_amd.optim import gen_candidates_scipy, optimize_acqf
    model, bounds = _setup("homo")[0], _bounds()
    torch.manual_seed(0)
    acqf = getattr(acquisition, name)(model, _candidates().to(DEV))
    drawn = [acqf.posterior_max_values.clone()]
    set_pending = acqf.set_X_pending

    def logged(X_pending=None):
        set_pending(X_pending)
        drawn.append(acqf.posterior_max_values.clone())
    acqf.set_X_pending = logged
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cand, val = optimize_acqf(acqf, bounds, q=q, num_restarts=4, raw_samples=32,
                                  options={"maxiter": 10}, sequential=sequential,
                                  gen_candidates=gen_candidates_scipy)
    assert cand.shape == (q, D) and (cand >= 0).all() and (cand <= 1).all()
    assert acqf.X_pending is None
    with torch.no_grad():
        if sequential:
            assert val.shape == (q,)
            # one draw at construction, one after each pick, one at the final reset
            assert len(drawn) == q + 2
            assert all(not torch.equal(drawn[i], drawn[i + 1]) for i in range(q + 1))
            for i in range(q):
                set_pending(cand[:i] if i else None)
                acqf.posterior_max_values = drawn[i]
                torch.testing.assert_close(acqf(cand[i:i + 1]).reshape(()), val[i],
                                           rtol=1e-9, atol=1e-12)
            set_pending(None)
        else:
            assert len(drawn) == 1
            torch.testing.assert_close(acqf(cand).reshape(()), val.reshape(()),
                                       rtol=1e-9, atol=1e-12)
