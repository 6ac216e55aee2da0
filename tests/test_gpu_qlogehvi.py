"""qLogExpectedHypervolumeImprovement / qLogNoisyExpectedHypervolumeImprovement
on the fused gfx950 route against CPU fp64 autograd through the oracle's
posterior and sample pieces (oracle.gp.ExactGPOracle, oracle.acquisition.
mc_samples / QNEHVIOracle, imported as they are) followed by the torch
restatement of the log-space reduction (tests/logehvi_restatement.py, pinned to
the reference by tests/test_logehvi_golden.py).

Setup: DTLZ2, n = 64, d = 3, fixed hyperparameters, a ModelListGP of two or
three SingleTaskGPs (plus one constraint member where constraints are tested;
three objectives are DTLZ2's on the slice x_4 = 0.5 of its four inputs, since
DTLZ2 needs more inputs than objectives).
Values: rtol 1e-7 / atol 1e-10; gradients w.r.t. X: rtol 1e-5 / atol 1e-8 (the
project's qEHVI / qNEHVI bars)."""
import functools
import math

import pytest
import torch

from tests.logehvi_restatement import log_qehvi_from_samples

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
VAL = dict(rtol=1e-7, atol=1e-10)
GRAD = dict(rtol=1e-5, atol=1e-8)
D = 3


def _last(Z):
    return Z[..., -1]


@functools.lru_cache(maxsize=None)
def _setup(m, constrained=False, seed=0, n=64):
    """(X, Y, ModelListGP on the device, oracles); with ``constrained`` one more
    member, fitted to a smooth function whose sign changes across the cube."""
    from botorch_amd.models import ModelListGP, SingleTaskGP
    from botorch_amd.test_functions import DTLZ2
    from oracle.gp import ExactGPOracle, GPHyper
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, D, generator=g, dtype=F64)
    # DTLZ2 needs more inputs than objectives: its d = 3 slice x_4 = 0.5 for m = 3
    Xe = X if m < D else torch.cat([X, torch.full((n, m + 1 - D), 0.5, dtype=F64)], dim=-1)
    Y = DTLZ2(dim=Xe.shape[-1], num_objectives=m).evaluate_true(Xe)
    Y = Y + 0.05 * torch.randn(n, m, generator=g, dtype=F64)
    if constrained:
        c = X[:, 0] + 0.5 * torch.sin(3.0 * X[:, 1]) - 0.8 + 0.02 * torch.randn(n, generator=g, dtype=F64)
        assert 0.2 < (c <= 0).double().mean() < 0.8
        Y = torch.cat([Y, c.unsqueeze(-1)], dim=-1)
    models, oracles = [], []
    for t in range(Y.shape[-1]):
        mm = SingleTaskGP(X.to(DEV), Y[:, t:t + 1].to(DEV))
        mm.covar_module.lengthscale = torch.full((1, D), 0.6, dtype=F64)
        mm.likelihood.noise = torch.tensor([1e-2], dtype=F64)
        models.append(mm.eval())
        oracles.append(ExactGPOracle(X, Y[:, t:t + 1], GPHyper(torch.full((D,), 0.6, dtype=F64), 1e-2, 0.0)))
    return X, Y, ModelListGP(*models), oracles


def _logw(cons, f, eta, fat):
    from botorch_amd.objective import compute_smoothed_feasibility_indicator
    if cons is None:
        return None
    return compute_smoothed_feasibility_indicator(cons, f, torch.as_tensor(eta, dtype=F64).reshape(-1),
                                                  log=True, fat=fat)


def _value_and_grad(acqf, Xc):
    Xd = Xc.to(DEV).requires_grad_(True)
    v = acqf(Xd)
    (g,) = torch.autograd.grad(v.sum(), Xd)
    return v.detach().cpu(), g.cpu()


def _compare(acqf, Xc, ref_fn):
    v, gx = _value_and_grad(acqf, Xc)
    Xo = Xc.clone().requires_grad_(True)
    rv = ref_fn(Xo)
    (go,) = torch.autograd.grad(rv.sum(), Xo)
    print(f"value max|diff| = {(v - rv.detach()).abs().max().item():.3e} of {rv.abs().max().item():.3e}; "
          f"gradient max|diff| = {(gx - go).abs().max().item():.3e} of {go.abs().max().item():.3e}")
    assert torch.isfinite(rv).all() and torch.isfinite(go).all() and go.abs().max() > 0
    torch.testing.assert_close(v, rv.detach(), **VAL)
    torch.testing.assert_close(gx, go, **GRAD)
    return v, gx


# ---- qLogEHVI --------------------------------------------------------------------------
def _qlogehvi(m, S, seed, cons=None, nfront=15, plain=False, **kw):
    from botorch_amd.acquisition import (IdentityMCMultiOutputObjective,
                                         qExpectedHypervolumeImprovement,
                                         qLogExpectedHypervolumeImprovement)
    from botorch_amd.multi_objective import FastNondominatedPartitioning
    from botorch_amd.sampling import SobolQMCNormalSampler
    X, Y, model, oracles = _setup(m, cons is not None)
    ref_point = torch.zeros(m, dtype=F64)
    part = FastNondominatedPartitioning(ref_point, Y[:nfront, :m])
    objective = IdentityMCMultiOutputObjective(outcomes=list(range(m))) if cons is not None else None
    cls = qExpectedHypervolumeImprovement if plain else qLogExpectedHypervolumeImprovement
    acqf = cls(model, ref_point.tolist(), part, sampler=SobolQMCNormalSampler(torch.Size([S]), seed=seed),
               objective=objective, constraints=cons, **kw)
    lo, hi = part.get_hypercell_bounds()
    return acqf, oracles, lo.to(F64), hi.to(F64)


def _oracle_samples(oracles, X, S, seed):
    from oracle.acquisition import mc_samples
    from oracle.sampling import base_samples_multi_output
    Z = base_samples_multi_output(S, X.shape[-2], len(oracles), seed)
    return torch.stack([mc_samples(*orc.posterior(X), Z[:, t]) for t, orc in enumerate(oracles)], dim=-1)


def _qlogehvi_reference(oracles, m, S, seed, cons, eta, fat, tau_relu, tau_max, lo, hi):
    def ref(X):
        f = _oracle_samples(oracles, X, S, seed)
        return log_qehvi_from_samples(f[..., :m], lo, hi, _logw(cons, f, eta, fat), fat, tau_relu, tau_max)
    return ref


@pytest.mark.parametrize("m,q,S,fat", [(2, 1, 32, True), (2, 3, 16, True), (3, 2, 16, True),
                                       (2, 2, 16, False)])
def test_qlogehvi_matches_oracle(m, q, S, fat):
    acqf, oracles, lo, hi = _qlogehvi(m, S, 4, fat=fat)
    assert (acqf.tau_relu, acqf.tau_max) == (1e-6, 1e-2)
    Xc = torch.rand(5, q, D, generator=torch.Generator().manual_seed(10 * m + q), dtype=F64)
    v, _ = _compare(acqf, Xc, _qlogehvi_reference(oracles, m, S, 4, None, None, fat, 1e-6, 1e-2, lo, hi))
    with torch.no_grad():   # forward-only calls take the same kernel
        torch.testing.assert_close(acqf(Xc.to(DEV)).cpu(), v, rtol=0, atol=0)
    # t-batch shapes are kept
    assert acqf(Xc.to(DEV).reshape(5, 1, q, D)).shape == (5, 1)


def test_qlogehvi_with_pending_point():
    m, q, S = 2, 2, 16
    acqf, oracles, lo, hi = _qlogehvi(m, S, 5)
    Xp = torch.rand(1, D, generator=torch.Generator().manual_seed(2), dtype=F64)
    acqf.set_X_pending(Xp.to(DEV))
    Xc = torch.rand(4, q, D, generator=torch.Generator().manual_seed(3), dtype=F64)
    inner = _qlogehvi_reference(oracles, m, S, 5, None, None, True, 1e-6, 1e-2, lo, hi)
    _compare(acqf, Xc, lambda X: inner(torch.cat([X, Xp.expand(X.shape[0], 1, D)], dim=-2)))


def test_qlogehvi_one_outcome_constraint():
    m, q, S = 2, 3, 16
    cons, eta = [_last], 1e-2
    acqf, oracles, lo, hi = _qlogehvi(m, S, 6, cons=cons, eta=eta)
    Xc = torch.rand(5, q, D, generator=torch.Generator().manual_seed(7), dtype=F64)
    ref = _qlogehvi_reference(oracles, m, S, 6, cons, eta, True, 1e-6, 1e-2, lo, hi)
    v, _ = _compare(acqf, Xc, ref)
    free = _qlogehvi_reference(oracles, m, S, 6, None, None, True, 1e-6, 1e-2, lo, hi)(Xc)
    assert (v < free - 1e-3).any()   # the feasibility weights matter


# ---- qLogNEHVI -------------------------------------------------------------------------
def _qlognehvi(m, S, seed, r=15, Xb=None, **kw):
    from botorch_amd.acquisition import qLogNoisyExpectedHypervolumeImprovement
    from botorch_amd.sampling import SobolQMCNormalSampler
    from oracle.acquisition import QNEHVIOracle
    X, Y, model, oracles = _setup(m)
    Xb = X[:r] if Xb is None else Xb
    acqf = qLogNoisyExpectedHypervolumeImprovement(
        model, [0.0] * m, Xb.to(DEV), sampler=SobolQMCNormalSampler(torch.Size([S]), seed=seed), **kw)
    return acqf, QNEHVIOracle(oracles, acqf.X_baseline.cpu(), [0.0] * m, S, seed=seed)


def _qlognehvi_reference(orc, lo, hi, fat=True, tau_relu=1e-6, tau_max=1e-3, joint=False, prev=None):
    from botorch_amd.safe_math import logplusexp

    def ref(X):
        f = orc.samples_joint(X) if joint else orc.samples(X)
        v = log_qehvi_from_samples(f, lo, hi, None, fat, tau_relu, tau_max)
        return v if prev is None else logplusexp(v, prev.log().expand_as(v))
    return ref


@pytest.mark.parametrize("cache_root", [True, False])
@pytest.mark.parametrize("m,q", [(2, 2), (3, 1)])
def test_qlognehvi_matches_oracle(m, q, cache_root):
    S = 16
    acqf, orc = _qlognehvi(m, S, 3, cache_root=cache_root)
    assert (acqf.tau_relu, acqf.tau_max, acqf.fat) == (1e-6, 1e-3, True)
    torch.testing.assert_close(acqf.baseline_samples, orc.Y_base, rtol=1e-8, atol=1e-10)
    lo, hi = acqf.cell_lower_bounds.cpu(), acqf.cell_upper_bounds.cpu()
    pad = ((lo == 0).all(-1) & (hi == 0).all(-1)).sum(-1)
    assert (pad > 0).any() and (pad == 0).any()   # the padding cells are exercised
    Xc = torch.rand(4, q, D, generator=torch.Generator().manual_seed(m * 10 + q), dtype=F64)
    _compare(acqf, Xc, _qlognehvi_reference(orc, lo, hi, joint=not cache_root))


def test_qlognehvi_not_incremental_with_pending_points():
    """incremental_nehvi=False: two pending points join the baseline, their
    hypervolume mean_s (HV_s(after) - HV_s(before))+ joins the value as
    logplusexp(value, log prev_nehvi) (logei.py:471)."""
    from oracle.acquisition import QNEHVIOracle
    m, q, S, seed = 2, 2, 16, 9
    X, _, _, oracles = _setup(m)
    acqf, orc0 = _qlognehvi(m, S, seed, incremental_nehvi=False)
    acqf.set_X_pending(X[45:47].to(DEV))
    assert acqf.X_baseline.shape[0] == 17 and acqf.X_pending is None
    orc = QNEHVIOracle(oracles, torch.cat([X[:15], X[45:47]]), [0.0] * m, S, seed=seed)
    prev = (orc.initial_hv - orc0.initial_hv).clamp_min(0.0).mean()
    assert prev > 0
    torch.testing.assert_close(acqf._prev_nehvi.cpu(), prev, rtol=1e-9, atol=1e-12)
    lo, hi = acqf.cell_lower_bounds.cpu(), acqf.cell_upper_bounds.cpu()
    Xc = torch.rand(4, q, D, generator=torch.Generator().manual_seed(21), dtype=F64)
    v, _ = _compare(acqf, Xc, _qlognehvi_reference(orc, lo, hi, prev=prev))
    assert (v > prev.log()).all()
    inc = _qlognehvi_reference(orc, lo, hi)(Xc)
    assert not torch.allclose(v, inc, rtol=1e-6)   # prev_nehvi matters


@pytest.mark.parametrize("kind", ["qlogehvi", "qlognehvi"])
def test_q_above_eight_is_unsupported(kind):
    from botorch_amd.exceptions import UnsupportedError
    X = _setup(2)[0]
    if kind == "qlogehvi":
        acqf = _qlogehvi(2, 8, 0)[0]
        acqf.set_X_pending(X[50:55].to(DEV))
    else:
        acqf = _qlognehvi(2, 8, 0, cache_pending=False)[0]
        acqf.set_X_pending(X[50:55].to(DEV))
    Xc = torch.rand(2, 4, D, generator=torch.Generator().manual_seed(0), dtype=F64).to(DEV)
    with pytest.raises(UnsupportedError, match="q <= 8"):
        acqf(Xc)                      # 4 + 5 pending points
    assert torch.isfinite(acqf(Xc[:, :3])).all()   # 3 + 5 = 8 runs


# ---- what the log formulation is for ---------------------------------------------------
def _hopeless(plain, S=16, seed=1):
    """A front far above anything the models can reach."""
    from botorch_amd.acquisition import (qExpectedHypervolumeImprovement,
                                         qLogExpectedHypervolumeImprovement)
    from botorch_amd.multi_objective import FastNondominatedPartitioning
    from botorch_amd.sampling import SobolQMCNormalSampler
    _, _, model, _ = _setup(2)
    ref_point = torch.zeros(2, dtype=F64)
    part = FastNondominatedPartitioning(ref_point, torch.tensor([[6.0, 7.0], [7.0, 6.0]], dtype=F64))
    cls = qExpectedHypervolumeImprovement if plain else qLogExpectedHypervolumeImprovement
    return cls(model, ref_point.tolist(), part, sampler=SobolQMCNormalSampler(torch.Size([S]), seed=seed))


def test_optimize_acqf_from_a_hopeless_start():
    from botorch_amd.optim import optimize_acqf
    from botorch_amd.utils_sampling import draw_sobol_samples
    bounds = torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)]).to(DEV)
    raw = draw_sobol_samples(bounds=bounds.cpu(), n=16, q=2, seed=0).to(DEV)
    with torch.no_grad():
        plain0 = _hopeless(True)(raw).cpu()
        log0 = _hopeless(False)(raw).cpu()
    assert (plain0 == 0).all()                       # the plateau plain qEHVI starts on
    assert torch.isfinite(log0).all() and log0.max() - log0.min() > 1e-6
    torch.manual_seed(0)
    cand, val = optimize_acqf(_hopeless(False), bounds, q=2, num_restarts=4, raw_samples=16,
                              options={"maxiter": 20, "seed": 0})
    assert cand.shape == (2, D)
    assert (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
    assert math.isfinite(float(val))


def test_exp_qlogehvi_against_plain_qehvi():
    """On a mixed case |exp(qLogEHVI) - qEHVI| is the smoothing of the default
    temperatures, not error: it equals the same difference formed by the CPU
    restatements on the same samples."""
    from oracle.acquisition import qehvi_from_samples
    m, q, S, seed = 2, 2, 32, 8
    acqf, oracles, lo, hi = _qlogehvi(m, S, seed)
    plain = _qlogehvi(m, S, seed, plain=True)[0]
    Xc = torch.rand(6, q, D, generator=torch.Generator().manual_seed(4), dtype=F64)
    with torch.no_grad():
        lv, pv = acqf(Xc.to(DEV)).cpu(), plain(Xc.to(DEV)).cpu()
    f = _oracle_samples(oracles, Xc, S, seed)
    ref_log = log_qehvi_from_samples(f, lo, hi, None, True, 1e-6, 1e-2)
    ref_plain = qehvi_from_samples(f, lo, hi)
    assert (ref_plain > 0).any()
    got, ref = (lv.exp() - pv).abs(), (ref_log.exp() - ref_plain).abs()
    print("smoothing |exp(qLogEHVI) - qEHVI|: device", got.tolist(), "reference", ref.tolist())
    torch.testing.assert_close(lv, ref_log, **VAL)
    torch.testing.assert_close(pv, ref_plain, **VAL)
    assert ref.max() > 0
    # both values are within VAL of their references, so the differences agree
    # to the sum of the two bounds
    bound = VAL["rtol"] * (ref_log.exp() + ref_plain.abs()) + 2 * VAL["atol"]
    assert ((got - ref).abs() <= bound).all(), ((got - ref).abs().tolist(), bound.tolist())
