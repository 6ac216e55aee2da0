"""qBayesianActiveLearningByDisagreement end to end on the device against the
torch restatement (tests/bald_restatement.py) on oracle.acquisition.saas_members:
values (rtol 1e-7, atol 1e-8) and dX (rtol 1e-5, atol 1e-8).

The three problems (d, M, q, n, S, B) are the restatement's CASES, with and
without Standardize, with and without two pending points and with an extra
leading batch dimension.  The members' noise in these draws is 2e-3 at the least
(M = 16) and 1e-2 or more in the two small problems, far above the ladder's
first rung, and the Cholesky ladder adds no jitter: every evaluation runs with
NumericalWarning turned into an error.
The fused tests replace ``_generic`` by a function that raises, the generic ones
do the same to the fused node, so neither route can stand in for the other."""
import warnings

import pytest
import torch

from tests import bald_restatement as br

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
VAL = dict(rtol=1e-7, atol=1e-8)
GRAD = dict(rtol=1e-5, atol=1e-8)


def _setup(case, standardize=False):
    """(model on the device, oracle members, candidates, base samples, sampler)."""
    from botorch_amd.models import SaasFullyBayesianSingleTaskGP, Standardize
    from botorch_amd.sampling import SobolQMCNormalSampler
    from oracle.acquisition import saas_members
    X, Y, smp, Xc, Z = br.problem(*case, standardize=standardize)
    assert float(smp["noise"].min()) >= 2e-3  # (jitter itself is an error in _value_and_grad)
    m = SaasFullyBayesianSingleTaskGP(X.to(DEV), Y.to(DEV),
                                      outcome_transform=Standardize(m=1) if standardize else None)
    m.load_mcmc_samples({k: v.to(DEV) for k, v in smp.items()})
    m.eval()
    members = saas_members(X, Y, smp, standardize=standardize)
    return m, members, Xc, Z, SobolQMCNormalSampler(torch.Size([case[4]]), seed=2)


def _no_route(name):
    def raiser(*a, **k):
        raise AssertionError(f"the {name} route was taken")
    return raiser


def _value_and_grad(acqf, X):
    from botorch_amd.exceptions import NumericalWarning
    Xd = X.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error", NumericalWarning)
        v = acqf(Xd)
        (g,) = torch.autograd.grad(v.sum(), Xd)
    return v.detach().cpu(), g.cpu()


def _reference(members, X, Z, Xp=None):
    """The restatement's value and dX at X (... x q x d), pending points joined."""
    Xr = X.clone().requires_grad_(True)
    Xf = Xr if Xp is None else torch.cat([Xr, Xp.expand(*X.shape[:-2], *Xp.shape)], dim=-2)
    q, d = Xf.shape[-2:]
    ref = br.bald_members(members, Xf.reshape(-1, q, d), Z).reshape(X.shape[:-2])
    (g,) = torch.autograd.grad(ref.sum(), Xr)
    return ref.detach(), g


def _report(what, v, ref, g, gref):
    print(f"{what}: value err {(v - ref).abs().max():.3e} (max |ref| {ref.abs().max():.3e}), "
          f"dX err {(g - gref).abs().max():.3e} (max |dX| {gref.abs().max():.3e})")


@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("standardize", [False, True])
@pytest.mark.parametrize("case", br.CASES)
def test_fused_matches_restatement(case, standardize, pending, monkeypatch):
    from botorch_amd.acquisition import qBayesianActiveLearningByDisagreement as BALD
    from oracle.sampling import base_samples_single_output
    m, members, Xc, Z, sampler = _setup(case, standardize)
    monkeypatch.setattr(BALD, "_generic", _no_route("generic"))
    d, q, S = case[0], case[2], case[4]
    Xp = None
    if pending:
        Xp = torch.rand(2, d, generator=torch.Generator().manual_seed(9), dtype=F64)
        if q + 2 > 16:
            Xc = Xc[:, :q - 2]
        Z = base_samples_single_output(S, Xc.shape[-2] + 2, 2)
    acqf = BALD(m, sampler=sampler, X_pending=None if Xp is None else Xp.to(DEV))
    v, g = _value_and_grad(acqf, Xc)
    ref, gref = _reference(members, Xc, Z, Xp)
    assert v.shape == (case[5],) and g.shape == Xc.shape
    _report(f"{case} standardize={standardize} pending={pending}", v, ref, g, gref)
    assert gref.abs().max() > 1e-6
    torch.testing.assert_close(v, ref, **VAL)
    torch.testing.assert_close(g, gref, **GRAD)


def test_fused_extra_batch_dimension_and_empty(monkeypatch):
    from botorch_amd.acquisition import qBayesianActiveLearningByDisagreement as BALD
    case = br.CASES[0]
    m, members, Xc, Z, sampler = _setup(case)
    monkeypatch.setattr(BALD, "_generic", _no_route("generic"))
    acqf = BALD(m, sampler=sampler)
    X4 = torch.stack([Xc, Xc.flip(0) * 0.9], dim=0)                   # 2 x B x q x d
    v, g = _value_and_grad(acqf, X4)
    ref, gref = _reference(members, X4, Z)
    assert v.shape == (2, case[5])
    _report("extra batch dimension", v, ref, g, gref)
    torch.testing.assert_close(v, ref, **VAL)
    torch.testing.assert_close(g, gref, **GRAD)
    with torch.no_grad():
        assert acqf(torch.empty(0, case[2], case[0], dtype=F64, device=DEV)).shape == (0,)
        one = acqf(Xc[1].to(DEV))                                     # q x d
    torch.testing.assert_close(one.cpu(), ref[0, 1].reshape(1), **VAL)


@pytest.mark.parametrize("case", br.CASES[:2])
def test_routes_agree(case):
    from botorch_amd.acquisition import qBayesianActiveLearningByDisagreement as BALD
    m, _, Xc, _, sampler = _setup(case, standardize=True)
    acqf = BALD(m, sampler=sampler)
    v, g = _value_and_grad(acqf, Xc)
    vg, gg = _value_and_grad(acqf._generic, Xc)
    _report(f"{case} fused against generic", v, vg, g, gg)
    torch.testing.assert_close(v, vg, **VAL)
    torch.testing.assert_close(g, gg, **GRAD)


def test_generic_route_q17_and_posterior_transform(monkeypatch):
    """q = 17 and a posterior transform are outside the fused route; the generic
    one matches the restatement (the transform w f + c scales every component
    alike, which the restatement applies to its moments)."""
    from botorch_amd import acquisition
    from botorch_amd.acquisition import qBayesianActiveLearningByDisagreement as BALD
    from botorch_amd.objective import ScalarizedPosteriorTransform
    from botorch_amd.sampling import SobolQMCNormalSampler
    from oracle.sampling import base_samples_single_output, draw_sobol_samples
    case = br.CASES[0]
    d, S = case[0], case[4]
    m, members, Xc, Z, sampler = _setup(case)
    monkeypatch.setattr(acquisition._FusedBALD, "forward", staticmethod(_no_route("fused")))
    lo = torch.zeros(d, dtype=F64)
    X17 = draw_sobol_samples(lo, lo + 1, 2, 17, 5)
    v, g = _value_and_grad(BALD(m, sampler=SobolQMCNormalSampler(torch.Size([S]), seed=2)), X17)
    ref, gref = _reference(members, X17, base_samples_single_output(S, 17, 2))
    _report("q = 17", v, ref, g, gref)
    torch.testing.assert_close(v, ref, **VAL)
    torch.testing.assert_close(g, gref, **GRAD)
    w, c = 2.0, 0.5
    tf = ScalarizedPosteriorTransform(torch.tensor([w], dtype=F64, device=DEV), offset=c)
    v, g = _value_and_grad(BALD(m, sampler=sampler, posterior_transform=tf), Xc)
    Xr = Xc.clone().requires_grad_(True)
    mean, cov = br.member_moments(members, Xr)
    ref = br.bald(w * mean + c, (w * w) * cov, Z)
    (gref,) = torch.autograd.grad(ref.sum(), Xr)
    _report("posterior transform", v, ref.detach(), g, gref)
    torch.testing.assert_close(v, ref.detach(), **VAL)
    torch.testing.assert_close(g, gref, **GRAD)


def test_optimize_acqf_bald():
    """q = 2, 4 restarts, 16 raw samples, a few iterations: finite candidates in
    the bounds whose value is the acquisition at the candidates and is not below
    the best raw sample's (L-BFGS-B never ends below its start and the
    initialisation keeps the best raw sample)."""
    from botorch_amd.acquisition import qBayesianActiveLearningByDisagreement as BALD
    from botorch_amd.optim import optimize_acqf
    from botorch_amd.utils_sampling import draw_sobol_samples
    case = br.CASES[0]
    d = case[0]
    m, _, _, _, sampler = _setup(case)
    acqf = BALD(m, sampler=sampler)
    bounds = torch.stack([torch.zeros(d, dtype=F64), torch.ones(d, dtype=F64)]).to(DEV)
    raw = draw_sobol_samples(bounds=bounds.cpu(), n=16, q=2, seed=0).to(DEV)
    with torch.no_grad():
        best_raw = float(acqf(raw).max())
    torch.manual_seed(0)
    cand, val = optimize_acqf(acqf, bounds, q=2, num_restarts=4, raw_samples=16,
                              options={"maxiter": 5, "seed": 0})
    assert cand.shape == (2, d) and torch.isfinite(cand).all()
    assert (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
    with torch.no_grad():
        again = float(acqf(cand))
    print(f"best raw {best_raw:.6e}, optimised {float(val):.6e}")
    assert abs(float(val) - again) <= 1e-9 * max(1.0, abs(again))
    assert float(val) >= best_raw - 1e-9 * abs(best_raw)
