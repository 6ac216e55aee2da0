"""qKnowledgeGradient (one-shot, posterior mean as inner value) on the device
against autograd through the oracle restatement (tests/kg_restatement.py):
values and dX over all q + N_f rows.

n = 200, d = 6, negated Hartmann targets (mean != 0, std != 1), the
hyperparameters set as tests/test_gpu_mc_family.py sets them.  Bars (the
project's): fused values rtol 1e-6 / atol 1e-8, gradients rtol 1e-5 / atol 1e-8;
the generic route rtol 1e-5.  The fused tests make ``_generic`` raise, so a
silent fall-back fails; the reference gradient is asserted non-zero on the
actual and on the fantasy rows before the device is asked."""
import functools
import warnings

import pytest
import torch

from tests.kg_restatement import kg_values

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
VAL = dict(rtol=1e-6, atol=1e-8)
GRAD = dict(rtol=1e-5, atol=1e-8)
GENERIC = dict(rtol=1e-5, atol=1e-8)
SEED = 5
LS, NOISE, CONST = 0.35, 1e-3, 0.1


# ---- data, model, restatement ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(d=6, fixed=False, n=200):
    """(X, Y, Yvar or None, oracle) on the CPU."""
    from botorch_amd.test_functions import Hartmann
    from oracle.gp import ExactGPOracle, GPHyper, standardize_fit
    from oracle.sampling import draw_sobol_samples
    lo = torch.zeros(d, dtype=F64)
    X = draw_sobol_samples(lo, lo + 1, n, 1, 0).squeeze(1)
    Y = Hartmann(negate=True)(X[:, :6]).unsqueeze(-1)
    ymean, ystd = standardize_fit(Y)
    assert abs(ymean.item()) > 0.05 and abs(ystd.item() - 1) > 0.1
    Yvar, noise = None, NOISE
    if fixed:
        g = torch.Generator().manual_seed(4)
        Yvar = (0.5 + torch.rand(n, 1, generator=g, dtype=F64)) * 2e-3 * ystd.item() ** 2
        noise = (Yvar / ystd ** 2).squeeze(-1)
    orc = ExactGPOracle(X, Y, GPHyper(torch.full((d,), LS, dtype=F64), noise, CONST))
    return X, Y, Yvar, orc


@functools.lru_cache(maxsize=None)
def _model(d=6, fixed=False):
    from botorch_amd.models import SingleTaskGP
    X, Y, Yvar, _ = _data(d, fixed)
    m = SingleTaskGP(X.to(DEV), Y.to(DEV), None if Yvar is None else Yvar.to(DEV))
    m.covar_module.lengthscale = torch.full((1, d), LS, dtype=F64)
    if not fixed:
        m.likelihood.noise = torch.tensor([NOISE], dtype=F64)
    m.mean_module.constant = CONST
    return m.eval()


def _outcome_noise(orc):
    n = orc.h.noise
    return float(n.mean() if torch.is_tensor(n) else n) * float(orc.ystd) ** 2


def restatement(orc, X, N_f, Xp=None, seed=SEED):
    """KG without current_value of X (b x (q + N_f) x d), pending points Xp."""
    from oracle.sampling import draw_sobol_normal_samples
    Xa, Xf = X[:, :-N_f], X[:, -N_f:]
    if Xp is not None:
        Xa = torch.cat([Xa, Xp.expand(X.shape[0], *Xp.shape)], dim=1)
    q_a = Xa.shape[1]
    Z = draw_sobol_normal_samples(q_a, N_f, seed)
    mean, cov = orc.posterior(torch.cat([Xa, Xf], dim=1))
    return kg_values(mean, cov, Z, _outcome_noise(orc), q_a).mean(dim=-1)


def _points(b, q, N_f, d=6):
    return torch.rand(b, q + N_f, d, generator=torch.Generator().manual_seed(b * 100 + q), dtype=F64)


@functools.lru_cache(maxsize=None)
def reference(b, q, N_f, d=6, fixed=False, pending=False):
    """(X, Xp, value, dX) of the restatement, computed once and shared."""
    orc = _data(d, fixed)[3]
    X = _points(b, q, N_f, d)
    Xp = torch.rand(1, d, generator=torch.Generator().manual_seed(77), dtype=F64) if pending else None
    Xo = X.clone().requires_grad_(True)
    val = restatement(orc, Xo, N_f, Xp)
    (g,) = torch.autograd.grad(val.sum(), Xo)
    assert g[:, :q].abs().max() > 1e-6 and g[:, q:].abs().max() > 1e-6
    return X, Xp, val.detach(), g


def _acqf(N_f, d=6, fixed=False, **kw):
    from botorch_amd.acquisition import qKnowledgeGradient
    from botorch_amd.sampling import SobolQMCNormalSampler
    return qKnowledgeGradient(_model(d, fixed), num_fantasies=N_f,
                              sampler=SobolQMCNormalSampler(torch.Size([N_f]), seed=SEED), **kw)


def _no_generic(monkeypatch):
    from botorch_amd.acquisition import qKnowledgeGradient

    def boom(self, *a):
        raise AssertionError("the generic route was taken")
    monkeypatch.setattr(qKnowledgeGradient, "_generic", boom)


def _value_and_grad(acqf, X):
    Xd = X.to(DEV).requires_grad_(True)
    val = acqf(Xd)
    (g,) = torch.autograd.grad(val.sum(), Xd)
    return val.detach().cpu(), g.cpu()


# ---- the fused route --------------------------------------------------------------------
@pytest.mark.parametrize("b, q, N_f", [(3, 2, 5), (2, 1, 16), (2, 4, 13), (1, 8, 8)])
def test_fused_value_and_gradient(b, q, N_f, monkeypatch):
    _no_generic(monkeypatch)
    X, _, ref, gref = reference(b, q, N_f)
    acqf = _acqf(N_f)
    val, g = _value_and_grad(acqf, X)
    assert val.shape == (b,)
    torch.testing.assert_close(val, ref, **VAL)
    torch.testing.assert_close(g, gref, **GRAD)
    with torch.no_grad():  # the forward-only call gives the same value
        torch.testing.assert_close(acqf(X.to(DEV)).cpu(), ref, **VAL)


@pytest.mark.parametrize("b, q, N_f, d", [(2, 9, 5, 6), (2, 2, 5, 10)])
def test_generic_route(b, q, N_f, d, monkeypatch):
    from botorch_amd.acquisition import qKnowledgeGradient

    def boom(self, *a):
        raise AssertionError("the fused route was taken")
    monkeypatch.setattr(qKnowledgeGradient, "_fused", boom)
    X, _, ref, gref = reference(b, q, N_f, d)
    val, g = _value_and_grad(_acqf(N_f, d), X)
    torch.testing.assert_close(val, ref, **GENERIC)
    torch.testing.assert_close(g, gref, **GENERIC)


def test_routes_agree(monkeypatch):
    """The in-library cross-check: both routes on one input."""
    X = _points(2, 3, 7).to(DEV)
    acqf = _acqf(7)
    with torch.no_grad():
        fused = acqf._fused(X[:, :3], X[:, 3:], acqf.sampler.base_samples_2d(3, X.device))
        generic = acqf._generic(X[:, :3], X[:, 3:], acqf.sampler.base_samples_2d(3, X.device))
    torch.testing.assert_close(fused, generic, **GENERIC)


def test_x_pending(monkeypatch):
    _no_generic(monkeypatch)
    X, Xp, ref, gref = reference(2, 2, 5, pending=True)
    acqf = _acqf(5, X_pending=Xp.to(DEV))
    val, g = _value_and_grad(acqf, X)
    plain = reference(2, 2, 5)[2]
    assert (ref - plain).abs().max() > 1e-4  # the pending point matters
    torch.testing.assert_close(val, ref, **VAL)
    torch.testing.assert_close(g, gref, **GRAD)


def test_current_value(monkeypatch):
    _no_generic(monkeypatch)
    X, _, ref, gref = reference(3, 2, 5)
    for cv in (0.7, torch.tensor(0.7, dtype=F64, device=DEV)):
        val, g = _value_and_grad(_acqf(5, current_value=cv), X)
        torch.testing.assert_close(val, ref - 0.7, **VAL)
        torch.testing.assert_close(g, gref, **GRAD)


def test_fixed_noise_model(monkeypatch):
    _no_generic(monkeypatch)
    X, _, ref, gref = reference(2, 2, 5, fixed=True)
    homo = reference(2, 2, 5)[2]
    assert (ref - homo).abs().max() > 1e-5  # another model, another value
    val, g = _value_and_grad(_acqf(5, fixed=True), X)
    torch.testing.assert_close(val, ref, **VAL)
    torch.testing.assert_close(g, gref, **GRAD)


def test_fp32_inputs(monkeypatch):
    """fp32 X is computed in fp64 and returned in fp32: the reference is the
    restatement at the rounded points, the bars those of fp32's rounding."""
    _no_generic(monkeypatch)
    orc = _data()[3]
    X32 = _points(2, 2, 5).float()
    Xo = X32.double().requires_grad_(True)
    ref = restatement(orc, Xo, 5)
    (gref,) = torch.autograd.grad(ref.sum(), Xo)
    Xd = X32.to(DEV).requires_grad_(True)
    val = _acqf(5)(Xd)
    (g,) = torch.autograd.grad(val.sum(), Xd)
    assert val.dtype == torch.float32 and g.dtype == torch.float32
    torch.testing.assert_close(val.cpu(), ref.detach().float(), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(g.cpu(), gref.float(), rtol=1e-5, atol=1e-6)


def test_scalarizing_transform(monkeypatch):
    from botorch_amd.objective import ScalarizedPosteriorTransform
    _no_generic(monkeypatch)
    X, _, ref, gref = reference(3, 2, 5)
    pt = ScalarizedPosteriorTransform(torch.tensor([-1.0], dtype=F64, device=DEV), offset=0.25)
    val, g = _value_and_grad(_acqf(5, posterior_transform=pt), X)
    torch.testing.assert_close(val, 0.25 - ref, **VAL)
    torch.testing.assert_close(g, -gref, **GRAD)


def test_definition_through_condition_on_observations(monkeypatch):
    """b = 1, q = 2, N_f = 3, one fantasy at a time through the product's own
    condition_on_observations: Y_i = mu(X) + L z_i under observation noise,
    the conditioned model's posterior mean at x'_i."""
    _no_generic(monkeypatch)
    q, N_f = 2, 3
    model = _model()
    acqf = _acqf(N_f)
    X = _points(1, q, N_f).to(DEV)
    with torch.no_grad():
        got = acqf(X)
        Z = acqf.sampler.base_samples_2d(q, X.device)
        post = model.posterior(X[0, :q])
        mu, Sigma = post.mean.reshape(q), post.distribution.covariance_matrix.reshape(q, q)
        ystd = model.outcome_stats()[1]
        s2 = model.hyper()[2] * ystd * ystd
        L = torch.linalg.cholesky(Sigma + s2 * torch.eye(q, dtype=F64, device=DEV))
        vals = []
        for i in range(N_f):
            cond = model.condition_on_observations(X[0, :q], (mu + L @ Z[i]).unsqueeze(-1))
            vals.append(cond.posterior(X[0, q + i:q + i + 1]).mean.reshape(()))
        ref = torch.stack(vals).mean()
    torch.testing.assert_close(got.reshape(()), ref, rtol=1e-6, atol=1e-8)


# ---- optimisation -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_model(n=30, d=2):
    from botorch_amd.models import SingleTaskGP
    g = torch.Generator().manual_seed(2)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = torch.sin(6 * X[:, :1]) * torch.cos(4 * X[:, 1:]) + 0.5
    m = SingleTaskGP(X.to(DEV), Y.to(DEV))
    m.covar_module.lengthscale = torch.full((1, d), 0.3, dtype=F64)
    m.likelihood.noise = torch.tensor([1e-3], dtype=F64)
    return m.eval()


_OPT = {"maxiter": 5, "num_inner_restarts": 4, "raw_inner_samples": 16, "seed": 0}


def _small_acqf(N_f=4):
    from botorch_amd.acquisition import qKnowledgeGradient
    return qKnowledgeGradient(_small_model(), num_fantasies=N_f)


def _bounds(d=2):
    return torch.stack([torch.zeros(d, dtype=F64), torch.ones(d, dtype=F64)]).to(DEV)


def test_optimize_acqf_one_shot():
    from botorch_amd.optim import optimize_acqf
    q, N_f, d = 2, 4, 2
    acqf, bounds = _small_acqf(N_f), _bounds(d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scipy is told of options it does not know
        torch.manual_seed(0)
        cand, val = optimize_acqf(acqf, bounds, q=q, num_restarts=4, raw_samples=16, options=_OPT)
        torch.manual_seed(0)
        tree, tval = optimize_acqf(acqf, bounds, q=q, num_restarts=4, raw_samples=16,
                                   options=_OPT, return_full_tree=True)
    assert cand.shape == (q, d) and val.shape == ()
    assert (cand >= 0).all() and (cand <= 1).all()
    assert tree.shape == (q + N_f, d) and (tree >= 0).all() and (tree <= 1).all()
    with torch.no_grad():
        torch.testing.assert_close(acqf(tree).reshape(()), tval, rtol=1e-9, atol=1e-12)
    with pytest.raises(NotImplementedError, match="one-shot"):
        optimize_acqf(acqf, bounds, q=q, num_restarts=4, raw_samples=16, sequential=True)


def test_one_shot_initial_conditions():
    from botorch_amd.optim import gen_one_shot_kg_initial_conditions
    q, N_f, d, restarts = 2, 4, 2, 3
    acqf, bounds = _small_acqf(N_f), _bounds(d)
    torch.manual_seed(1)
    ics = gen_one_shot_kg_initial_conditions(
        acqf, bounds, q=q, num_restarts=restarts, raw_samples=8,
        options={"frac_random": 0.3, "num_inner_restarts": 4, "raw_inner_samples": 16, "seed": 1})
    assert ics.shape == (restarts, q + N_f, d) and ics.device.type == "cuda"
    assert (ics >= 0).all() and (ics <= 1).all()


def test_sharded_driver_refuses_one_shot():
    from botorch_amd.distributed import _optimize_acqf_batch_sharded
    from botorch_amd.exceptions import UnsupportedError
    with pytest.raises(UnsupportedError, match="one-shot"):
        _optimize_acqf_batch_sharded(
            acq_function=_small_acqf(), bounds=_bounds(), q=2, num_restarts=2, raw_samples=4,
            options=None, fixed_features=None, post_processing_func=None,
            batch_initial_conditions=None, return_best_only=True, gen_candidates=None,
            ic_generator=None, timeout_sec=None, retry_on_optimization_warning=True,
            ic_gen_kwargs={})
