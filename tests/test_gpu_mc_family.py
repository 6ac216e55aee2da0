"""qSimpleRegret, qProbabilityOfImprovement and qUpperConfidenceBound
(acquisition/monte_carlo.py:648-871) on the fused gfx950 path against a torch
restatement over the oracle's samples: values and dX.

Shapes (B, q, S): (5, 1, 64) and (7, 3, 128) take the one-sample-per-thread
form of the finalisation kernel, (6, 8, 320) its groups of 8 lanes and a second,
partial chunk of the backward, (3, 16, 320) the groups of 16.  n = 256, d = 6.

Bars (tests/test_gpu_logei.py): fused values rtol 1e-6 / atol 1e-8, gradients
rtol 1e-5 / atol 1e-8; the generic route's values rtol 1e-5 / atol 1e-8 (its
q > 16 test there).  The fused tests make ``_generic_forward`` raise, so a
silent fall-back fails.

What keeps the comparisons from passing vacuously is asserted on the reference
before the device is asked: negative qSR / qUCB values with targets below -2 (a
q-maximum that starts at 0 fails there), qPI's best_f at the median of the
reference qSR values so that its values are not all 0 or 1, non-zero reference
gradients."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
VAL = dict(rtol=1e-6, atol=1e-8)
GRAD = dict(rtol=1e-5, atol=1e-8)
GENERIC = dict(rtol=1e-5, atol=1e-8)
SHAPES = [(5, 1, 64), (7, 3, 128), (6, 8, 320), (3, 16, 320)]
SEED = 5


# ---- data, model, restatement ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(shifted: bool, n=256, d=6, ls=0.35, noise=1e-3, const=0.1):
    """(X, Y, oracle) on the CPU, as tests/test_gpu_acquisition._setup; ``shifted``
    moves the negated Hartmann targets below -2."""
    from botorch_amd.test_functions import Hartmann
    from oracle.gp import ExactGPOracle, GPHyper
    from oracle.sampling import draw_sobol_samples
    lo = torch.zeros(d, dtype=F64)
    X = draw_sobol_samples(lo, lo + 1, n, 1, 0).squeeze(1)
    Y = Hartmann(negate=True)(X[:, :6]).unsqueeze(-1)
    if shifted:
        Y = Y - (Y.max() + 2.5)
        assert (Y < -2).all()
    orc = ExactGPOracle(X, Y, GPHyper(torch.full((d,), ls, dtype=F64), noise, const))
    return X, Y, orc


@functools.lru_cache(maxsize=None)
def _model(shifted: bool, ls=0.35, noise=1e-3, const=0.1):
    from botorch_amd.models import SingleTaskGP
    X, Y, _ = _data(shifted)
    m = SingleTaskGP(X.to(DEV), Y.to(DEV))
    m.covar_module.lengthscale = torch.full((1, X.shape[1]), ls, dtype=F64)
    m.likelihood.noise = torch.tensor([noise], dtype=F64)
    m.mean_module.constant = const
    return m.eval()


def _points(B, q, d=6):
    return torch.rand(B, q, d, generator=torch.Generator().manual_seed(B * 100 + q), dtype=F64)


def utility(name, s, best_f=None, tau=None, beta=None):
    """The three utilities on samples s (S x ... x q)."""
    if name == "qSR":
        return s
    if name == "qPI":
        return torch.sigmoid((s - best_f) / tau)
    mean = s.mean(dim=0)
    return mean + math.sqrt(beta * math.pi / 2) * (s - mean).abs()


def restatement(name, orc, X, S, seed=SEED, **params):
    from oracle.acquisition import mc_samples
    from oracle.sampling import draw_sobol_normal_samples
    Z = draw_sobol_normal_samples(X.shape[-2], S, seed)
    s = mc_samples(*orc.posterior(X), Z)
    return utility(name, s, **params).amax(-1).mean(0)


@functools.lru_cache(maxsize=None)
def reference(name, shifted, B, q, S, pending=False, **params):
    """(X, pending point or None, value, dX) of the restatement, computed once."""
    orc = _data(shifted)[2]
    X = _points(B, q)
    Xp = torch.rand(1, 6, generator=torch.Generator().manual_seed(77), dtype=F64) if pending else None
    Xo = X.clone().requires_grad_(True)
    Xj = Xo if Xp is None else torch.cat([Xo, Xp.expand(B, 1, 6)], dim=-2)
    val = restatement(name, orc, Xj, S, **params)
    (g,) = torch.autograd.grad(val.sum(), Xo)
    return X, Xp, val.detach(), g


def _no_generic(monkeypatch):
    from botorch_amd.acquisition import MCAcquisitionFunction

    def boom(self, X):
        raise AssertionError("the generic route was taken")
    monkeypatch.setattr(MCAcquisitionFunction, "_generic_forward", boom)


def _sampler(S, seed=SEED):
    from botorch_amd.sampling import SobolQMCNormalSampler
    return SobolQMCNormalSampler(torch.Size([S]), seed=seed)


def _compare(acqf, X, val, g):
    Xd = X.to(DEV).requires_grad_(True)
    v = acqf(Xd)
    (gd,) = torch.autograd.grad(v.sum(), Xd)
    with torch.no_grad():  # the forward-only call is the same value
        v0 = acqf(X.to(DEV))
    print("value  max |d - ref|", float((v.detach().cpu() - val).abs().max()),
          " grad max |d - ref|", float((gd.cpu() - g).abs().max()), " |ref grad| max", float(g.abs().max()))
    assert g.abs().max() > 0
    torch.testing.assert_close(v.detach().cpu(), val, **VAL)
    torch.testing.assert_close(v0.cpu(), val, **VAL)
    torch.testing.assert_close(gd.cpu(), g, **GRAD)


# ---- the fused route ----------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("B,q,S", SHAPES)
def test_qsr_matches_restatement(B, q, S, shifted, monkeypatch):
    from botorch_amd.acquisition import qSimpleRegret
    _no_generic(monkeypatch)
    X, _, val, g = reference("qSR", shifted, B, q, S)
    if shifted:
        assert val.max() < 0
    _compare(qSimpleRegret(_model(shifted), sampler=_sampler(S)), X, val, g)


def _qpi_best_f(B, q, S):
    """The median over the t-batches of the reference qSR value at the same X and Z."""
    return float(reference("qSR", False, B, q, S)[2].median())


@pytest.mark.parametrize("tau", [0.1, 1e-3])
@pytest.mark.parametrize("B,q,S", SHAPES)
def test_qpi_matches_restatement(B, q, S, tau, monkeypatch):
    from botorch_amd.acquisition import qProbabilityOfImprovement
    _no_generic(monkeypatch)
    best_f = _qpi_best_f(B, q, S)
    X, _, val, g = reference("qPI", False, B, q, S, best_f=best_f, tau=tau)
    assert int(((val > 0.05) & (val < 0.95)).sum()) >= 2, val
    kw = {} if tau == 1e-3 else dict(tau=tau)  # 1e-3 is the default
    acqf = qProbabilityOfImprovement(_model(False), torch.tensor(best_f, dtype=F64, device=DEV),
                                     sampler=_sampler(S), **kw)
    _compare(acqf, X, val, g)


@pytest.mark.parametrize("beta,shifted", [(0.2, True), (4.0, False)])
@pytest.mark.parametrize("B,q,S", SHAPES)
def test_qucb_matches_restatement(B, q, S, beta, shifted, monkeypatch):
    from botorch_amd.acquisition import qUpperConfidenceBound
    _no_generic(monkeypatch)
    X, _, val, g = reference("qUCB", shifted, B, q, S, beta=beta)
    if shifted:
        assert val.max() < 0
    _compare(qUpperConfidenceBound(_model(shifted), beta, sampler=_sampler(S)), X, val, g)


@pytest.mark.parametrize("name", ["qSR", "qPI", "qUCB"])
def test_x_pending(name, monkeypatch):
    """One pending point: the q-maximum, and qUCB's sample mean, span q + 1 rows."""
    from botorch_amd import acquisition as A
    _no_generic(monkeypatch)
    B, q, S = 7, 3, 128
    params = {"qSR": {}, "qUCB": dict(beta=0.2),
              "qPI": dict(best_f=_qpi_best_f(B, q, S), tau=0.1)}[name]
    X, Xp, val, g = reference(name, False, B, q, S, pending=True, **params)
    m, kw = _model(False), dict(sampler=_sampler(S), X_pending=Xp.to(DEV))
    acqf = {"qSR": lambda: A.qSimpleRegret(m, **kw),
            "qUCB": lambda: A.qUpperConfidenceBound(m, 0.2, **kw),
            "qPI": lambda: A.qProbabilityOfImprovement(m, params.get("best_f"), tau=0.1, **kw)}[name]()
    _compare(acqf, X, val, g)


def test_qucb_sample_mean_is_kept_with_the_base_samples():
    """zbar is computed when the base samples are made, not per forward."""
    s = _sampler(64)
    a = s.base_sample_mean_2d(3, torch.device(DEV))
    assert a is s.base_sample_mean_2d(3, torch.device(DEV))
    torch.testing.assert_close(a, s.base_samples_2d(3, torch.device(DEV)).mean(dim=0), rtol=0, atol=0)
    b = s.base_sample_mean_2d(4, torch.device(DEV))  # another q: new samples, new mean
    assert b.shape == (4,)


def test_fp32_x_in_and_out(monkeypatch):
    from botorch_amd.acquisition import qUpperConfidenceBound
    _no_generic(monkeypatch)
    X, _, val, _ = reference("qUCB", False, 7, 3, 128, beta=4.0)
    acqf = qUpperConfidenceBound(_model(False), 4.0, sampler=_sampler(128))
    with torch.no_grad():
        v = acqf(X.to(DEV, torch.float32))
    assert v.dtype == torch.float32
    ref32 = restatement("qUCB", _data(False)[2], X.float().double(), 128, beta=4.0)
    torch.testing.assert_close(v.cpu(), ref32.float(), rtol=1e-5, atol=1e-6)


# ---- the generic route ------------------------------------------------------------------
def test_generic_route_q_gt_16():
    """q = 20 leaves the fused kernel: device posterior + sampler + torch reductions."""
    from botorch_amd.acquisition import qSimpleRegret
    B, q, S = 3, 20, 64
    orc = _data(True)[2]
    X = _points(B, q)
    ref = restatement("qSR", orc, X, S, seed=4)
    assert ref.max() < 0
    with torch.no_grad():
        v = qSimpleRegret(_model(True), sampler=_sampler(S, 4))(X.to(DEV)).cpu()
    torch.testing.assert_close(v, ref, **GENERIC)


def test_generic_route_qpi_constrained_model_list():
    """qPI with one linear outcome constraint on a two-member ModelListGP,
    objective on output 0 (data and members of tests/test_gpu_constrained_so.py);
    a ListSampler, whose member t draws Sobol samples of dimension q at seed + t."""
    from botorch_amd.acquisition import qProbabilityOfImprovement
    from botorch_amd.objective import LinearMCObjective, get_outcome_constraint_transforms
    from botorch_amd.sampling import ListSampler
    from oracle.acquisition import mc_samples, smoothed_feasibility
    from oracle.sampling import draw_sobol_normal_samples
    from tests.test_gpu_constrained_so import _data as so_data, _model as so_model
    Mt, B, q, S, seed, tau, eta = 2, 3, 3, 64, 11, 0.1, 1e-2
    oracles = so_data(Mt)[2]
    X = _points(B, q)
    f = torch.stack([mc_samples(*orc.posterior(X), draw_sobol_normal_samples(q, S, seed + t))
                     for t, orc in enumerate(oracles)], dim=-1)            # S x B x q x Mt
    best_f = float(f[..., 0].amax(-1).mean(0).median())
    w = smoothed_feasibility([lambda Z: Z[..., 1]], f, eta)
    ref = (utility("qPI", f[..., 0], best_f=best_f, tau=tau) * w).amax(-1).mean(0)
    assert ((ref > 0.01) & (ref < 0.99)).any(), ref
    lin = (torch.tensor([[0.0, 1.0]], dtype=F64), torch.zeros(1, 1, dtype=F64))
    acqf = qProbabilityOfImprovement(
        so_model(Mt), best_f, sampler=ListSampler(*[_sampler(S, seed + t) for t in range(Mt)]),
        objective=LinearMCObjective(torch.tensor([1.0, 0.0], dtype=F64, device=DEV)), tau=tau,
        constraints=get_outcome_constraint_transforms(lin), eta=eta)
    with torch.no_grad():
        v = acqf(X.to(DEV)).cpu()
    torch.testing.assert_close(v, ref, **GENERIC)


def test_generic_route_qucb_saas():
    """qUCB over a SAAS ensemble: per member the restatement, averaged over the members."""
    from botorch_amd.acquisition import qUpperConfidenceBound
    from botorch_amd.models import SaasFullyBayesianSingleTaskGP, sample_saas_prior
    from botorch_amd.test_functions import Hartmann
    from oracle.acquisition import saas_members
    from oracle.sampling import draw_sobol_samples
    d, M, q, n, S, B, beta = 10, 3, 2, 64, 64, 3, 0.2
    lo = torch.zeros(d, dtype=F64)
    X = draw_sobol_samples(lo, lo + 1, n, 1, 0).squeeze(1)
    Y = Hartmann(negate=True)(X[:, :6]).unsqueeze(-1)
    Y = (Y - Y.mean()) / Y.std()
    smp = sample_saas_prior(d, M, seed=1)
    m = SaasFullyBayesianSingleTaskGP(X.to(DEV), Y.to(DEV))
    m.load_mcmc_samples({k: v.to(DEV) for k, v in smp.items()})
    m.eval()
    Xc = draw_sobol_samples(lo, lo + 1, B, q, 3)
    ref = torch.stack([restatement("qUCB", mm, Xc, S, seed=2, beta=beta)
                       for mm in saas_members(X, Y, smp)], dim=-1).mean(dim=-1)
    with torch.no_grad():
        v = qUpperConfidenceBound(m, beta, sampler=_sampler(S, 2))(Xc.to(DEV)).cpu()
    assert v.shape == (B,)
    torch.testing.assert_close(v, ref, **GENERIC)


# ---- the device optimiser ---------------------------------------------------------------
def test_optimize_acqf_device_qucb():
    """q = 2, 4 restarts, 16 raw samples through the device L-BFGS-B: candidates
    in bounds, the returned value is the acquisition at the candidates and is not
    below the best raw sample (L-BFGS-B never ends below its start and the
    initialisation keeps the best raw sample)."""
    from botorch_amd.acquisition import qUpperConfidenceBound
    from botorch_amd.optim import _fused_qei, gen_candidates_device, optimize_acqf
    from botorch_amd.utils_sampling import draw_sobol_samples
    acqf = qUpperConfidenceBound(_model(True), 0.2, sampler=_sampler(64))
    bounds = torch.stack([torch.zeros(6, dtype=F64), torch.ones(6, dtype=F64)]).to(DEV)
    raw = draw_sobol_samples(bounds=bounds.cpu(), n=16, q=2, seed=0).to(DEV)
    assert _fused_qei(acqf, raw)  # the eager two-call evaluation, no graph in "auto"
    with torch.no_grad():
        best_raw = float(acqf(raw).max())
    torch.manual_seed(0)
    cand, val = optimize_acqf(acqf, bounds, q=2, num_restarts=4, raw_samples=16,
                              options={"maxiter": 20, "seed": 0}, gen_candidates=gen_candidates_device)
    assert gen_candidates_device.last_graphed_evals == 0
    assert cand.shape == (2, 6) and (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
    with torch.no_grad():
        again = float(acqf(cand))
    assert abs(float(val) - again) <= 1e-9 * max(1.0, abs(again))
    assert float(val) >= best_raw - 1e-9 * abs(best_raw)
