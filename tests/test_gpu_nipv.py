"""qNegIntegratedPosteriorVariance on the device against autograd through the
restatement (tests/nipv_restatement.py): values and dX.

The set-up is test_gpu_jes.py's: n = 48, d = 3, targets with mean != 0 and
std != 1, hyperparameters set by hand (lengthscale 0.35, noise 1e-2, mean
constant 0.1); N = 64 Sobol integration points.  Bars (the project's end-to-end
bars): values rtol 1e-7, atol 1e-8; gradients rtol 1e-5, atol 1e-8.  The fused
tests make ``_generic`` raise, so a silent fall-back fails; the reference
gradient is asserted above 1e-6 before the device is asked."""
import functools

import pytest
import torch

from tests import nipv_restatement as nr
from tests.test_gpu_jes import D, _setup

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
VAL = dict(rtol=1e-7, atol=1e-8)
GRAD = dict(rtol=1e-5, atol=1e-8)
NZ = 64
SHAPES = [(3, 1), (2, 3), (1, 8)]


@functools.lru_cache(maxsize=None)
def _mc_points():
    from botorch_amd.utils_sampling import draw_sobol_samples
    bounds = torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)])
    return draw_sobol_samples(bounds, NZ, 1, seed=5).squeeze(1).to(F64).cpu()


def _points(B, q):
    return torch.rand(B, q, D, generator=torch.Generator().manual_seed(B * 100 + q), dtype=F64)


def _restate(variant, X, Xp=None):
    """The restatement in outcome space: ystd^2 nipv."""
    _, gp, (_, ystd) = _setup(variant)
    if Xp is not None:
        X = torch.cat([X, Xp.expand(X.shape[0], *Xp.shape)], dim=1)
    return (ystd * ystd) * nr.nipv(gp, _mc_points(), X)


@functools.lru_cache(maxsize=None)
def reference(variant, B, q, pending=False):
    """(X, Xp, value, dX) of the restatement, computed once and shared."""
    X = _points(B, q)
    Xp = torch.rand(2, D, generator=torch.Generator().manual_seed(77), dtype=F64) if pending else None
    Xo = X.clone().requires_grad_(True)
    val = _restate(variant, Xo, Xp)
    (g,) = torch.autograd.grad(val.sum(), Xo)
    assert g.abs().max() > 1e-6
    return X, Xp, val.detach(), g


def _acqf(variant, **kw):
    from botorch_amd.acquisition import qNegIntegratedPosteriorVariance
    return qNegIntegratedPosteriorVariance(_setup(variant)[0], _mc_points().to(DEV), **kw)


def _no_generic(monkeypatch):
    from botorch_amd.acquisition import qNegIntegratedPosteriorVariance

    def boom(self, *a):
        raise AssertionError("the generic route was taken")
    monkeypatch.setattr(qNegIntegratedPosteriorVariance, "_generic", boom)


def _value_and_grad(acqf, X):
    Xd = X.to(DEV).requires_grad_(True)
    val = acqf(Xd)
    (g,) = torch.autograd.grad(val.sum(), Xd)
    return val.detach().cpu(), g.cpu()


def _report(what, got, ref):
    err = ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    print(f"{what}: max rel err {err:.3e}, max abs err {(got - ref).abs().max().item():.3e}")


def _check(what, acqf, X, ref, gref):
    val, g = _value_and_grad(acqf, X)
    assert val.shape == ref.shape
    _report(f"value {what}", val, ref)
    _report(f"dX    {what}", g, gref)
    torch.testing.assert_close(val, ref, **VAL)
    torch.testing.assert_close(g, gref, **GRAD)


# ---- the fused route --------------------------------------------------------------------
@pytest.mark.parametrize("B, q", SHAPES)
def test_fused_value_and_gradient(B, q, monkeypatch):
    _no_generic(monkeypatch)
    X, _, ref, gref = reference("homo", B, q)
    acqf = _acqf("homo")
    assert acqf._route is None  # the default route on the device is the fused one
    _check(f"homo B={B} q={q}", acqf, X, ref, gref)
    with torch.no_grad():  # the forward-only call gives the graph-mode value
        torch.testing.assert_close(acqf(X.to(DEV)).cpu(), ref, **VAL)


@pytest.mark.parametrize("variant", ["fixed", "matern", "notransform"])
def test_fused_variants(variant, monkeypatch):
    _no_generic(monkeypatch)
    B, q = 2, 3
    X, _, ref, gref = reference(variant, B, q)
    _check(f"{variant} B={B} q={q}", _acqf(variant), X, ref, gref)


def test_fused_with_pending_points(monkeypatch):
    _no_generic(monkeypatch)
    X, Xp, ref, gref = reference("homo", 2, 3, pending=True)
    _check("pending B=2 q=3+2", _acqf("homo", X_pending=Xp.to(DEV)), X, ref, gref)


@pytest.mark.parametrize("B, q", SHAPES)
def test_generic_route_forced(B, q):
    X, _, ref, gref = reference("homo", B, q)
    acqf = _acqf("homo")
    acqf._route = "generic"
    _check(f"generic B={B} q={q}", acqf, X, ref, gref)


def test_generic_route_in_chunks(monkeypatch):
    """The integration points in chunks of 16 + 16 + 16 + 16 (the transient
    bound lowered), on the same reference."""
    from botorch_amd import acquisition
    monkeypatch.setattr(acquisition, "NIPV_GENERIC_TRANSIENT", 4)
    X, _, ref, gref = reference("homo", 2, 3)
    acqf = _acqf("homo")
    acqf._route = "generic"
    _check("generic, chunked", acqf, X, ref, gref)


def test_q17_takes_the_generic_route(monkeypatch):
    from botorch_amd.acquisition import qNegIntegratedPosteriorVariance

    def boom(self, *a):
        raise AssertionError("the fused route was taken")
    monkeypatch.setattr(qNegIntegratedPosteriorVariance, "_fused", boom)
    X, _, ref, gref = reference("homo", 2, 17)
    _check("q=17", _acqf("homo"), X, ref, gref)


def test_model_list_with_scalarization(monkeypatch):
    """ModelListGP of two members, weights (0.7, -1.3): sum_t w_t^2 acq_t; and a
    single-output model with one weight: w^2 acq."""
    from botorch_amd.models import ModelListGP
    from botorch_amd.objective import ScalarizedPosteriorTransform
    from botorch_amd.acquisition import qNegIntegratedPosteriorVariance
    _no_generic(monkeypatch)
    B, q = 2, 3
    X = _points(B, q)
    Xo = X.clone().requires_grad_(True)
    ref = 0.49 * _restate("homo", Xo) + 1.69 * _restate("matern", Xo)
    (gref,) = torch.autograd.grad(ref.sum(), Xo)
    assert gref.abs().max() > 1e-6
    model = ModelListGP(_setup("homo")[0], _setup("matern")[0]).eval()
    pt = ScalarizedPosteriorTransform(torch.tensor([0.7, -1.3], dtype=F64, device=DEV), offset=3.0)
    acqf = qNegIntegratedPosteriorVariance(model, _mc_points().to(DEV), posterior_transform=pt)
    _check("model list", acqf, X, ref.detach(), gref)
    one = ScalarizedPosteriorTransform(torch.tensor([-1.3], dtype=F64, device=DEV))
    _, _, r1, g1 = reference("homo", B, q)
    _check("w^2 acq", _acqf("homo", posterior_transform=one), X, 1.69 * r1, 1.69 * g1)


@pytest.mark.parametrize("variant", ["homo", "fixed"])
def test_fused_value_equals_conditioned_model(variant, monkeypatch):
    """The closed form against the repository's own explicit model on the
    device: condition_on_observations(X_b, Y, noise) followed by
    posterior(mc_points).variance.mean(), one t-batch at a time."""
    _no_generic(monkeypatch)
    model = _setup(variant)[0]
    acqf = _acqf(variant)
    Z = _mc_points().to(DEV)
    for B, q in SHAPES:
        X = _points(B, q).to(DEV)
        with torch.no_grad():
            val = acqf(X)
            for b in range(B):
                Y = torch.full((q, 1), 0.3, dtype=F64, device=DEV)
                noise = None
                if variant == "fixed":  # the mean of the (transformed) fixed variances
                    noise = model.likelihood.noise.mean().expand(q, 1).clone()
                cond = model.condition_on_observations(X[b], Y, noise=noise)
                want = -cond.posterior(Z.unsqueeze(-2)).variance.mean()
                print(f"{variant} B={B} q={q} b={b}: fused {val[b].item():.12e} "
                      f"conditioned {want.item():.12e}")
                torch.testing.assert_close(val[b], want, rtol=1e-7, atol=0.0)


def test_optimize_acqf_end_to_end():
    from botorch_amd.optim import draw_raw_samples, optimize_acqf
    acqf = _acqf("homo")
    bounds = torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)]).to(DEV)
    cand, value = optimize_acqf(acqf, bounds, q=2, num_restarts=4, raw_samples=32,
                                options={"seed": 0})
    assert cand.shape == (2, D)
    assert (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
    with torch.no_grad():
        torch.testing.assert_close(acqf(cand.unsqueeze(0)).reshape(()), value.reshape(()), **VAL)
        best_raw = acqf(draw_raw_samples(bounds, 32, 2, seed=0)).max()  # the optimiser's own
    print(f"optimised {value.item():.6e}, best of 32 raw samples {best_raw.item():.6e}")
    assert value.item() >= best_raw.item() - 1e-12
