"""The ParEGO family on a ModelListGP: the fused Chebyshev-scalarization route against the
same object's generic route, and one optimize_acqf call.
Bars: those tests/test_gpu_constrained_so.py holds the routes of _FusedSOFeas to."""
import pytest
import torch

from tests.test_gpu_constrained_so import GRAD, _val

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64 = torch.float64
N, D, MT, S, B, Q = 40, 3, 3, 32, 4, 2


@pytest.fixture(scope="module")
def setup():
    from botorch_amd.models import ModelListGP, SingleTaskGP
    g = torch.Generator().manual_seed(5)
    X = torch.rand(N, D, dtype=F64, generator=g)
    Y = torch.stack([torch.sin(3.0 * X.sum(-1)), -((X - 0.4) ** 2).sum(-1), X[:, 0] * X[:, 1]],
                    dim=-1) + 0.02 * torch.randn(N, MT, dtype=F64, generator=g)
    model = ModelListGP(*[SingleTaskGP(X.to(DEV), Y[:, t:t + 1].to(DEV)) for t in range(MT)])
    return model.eval(), X.to(DEV), Y.to(DEV), torch.rand(B, Q, D, dtype=F64, generator=g).to(DEV)


def _make(kind, model, Xb, Y, cons):
    from botorch_amd import acquisition as A, get_chebyshev_scalarization
    from botorch_amd.objective import GenericMCObjective
    from botorch_amd.sampling import ListSampler, SobolQMCNormalSampler
    w = torch.tensor([0.5, -0.3, 0.2], dtype=F64, device=DEV)
    one = SobolQMCNormalSampler(torch.Size([S]), seed=2)
    if kind == "qLogNParEGO":
        return A.qLogNParEGO(model, Xb, scalarization_weights=w, sampler=one, constraints=cons)
    obj = GenericMCObjective(get_chebyshev_scalarization(w, Y))
    if kind == "qNoisyExpectedImprovement":
        return A.qNoisyExpectedImprovement(model, Xb, objective=obj, prune_baseline=False,
                                           sampler=one, constraints=cons)
    # a sampler per member: the samples the generic route draws on a model list
    per = ListSampler(*[SobolQMCNormalSampler(torch.Size([S]), seed=2 + t) for t in range(MT)])
    return getattr(A, kind)(model, best_f=-0.45, objective=obj, sampler=per, constraints=cons)


def _linear():
    from botorch_amd.objective import get_outcome_constraint_transforms
    A = torch.tensor([[0.5, 0.0, 1.0], [0.0, -1.0, 0.2]], dtype=F64, device=DEV)
    return get_outcome_constraint_transforms((A, torch.tensor([[0.9], [1.2]], dtype=F64, device=DEV)))


@pytest.mark.parametrize("kind,constrained", [("qLogNParEGO", False), ("qLogNParEGO", True),
                                              ("qNoisyExpectedImprovement", False),
                                              ("qLogExpectedImprovement", True),
                                              ("qExpectedImprovement", False)])
def test_fused_route_matches_generic(setup, kind, constrained):
    """Value and dX of the two routes of one object: same baseline, same base samples (the
    cached-root classes' generic route draws each member's joint samples from the one Sobol
    sampler's interleaved columns)."""
    model, Xb, Y, X = setup
    acqf = _make(kind, model, Xb, Y, _linear() if constrained else None)
    out = []
    for route in ("fused", "generic"):
        acqf.cheb_route = route
        Xr = X.clone().requires_grad_(True)
        val = acqf(Xr)
        val.sum().backward()
        out.append((val.detach().cpu(), Xr.grad.cpu()))
    print("max |dv|, |dg|:", float((out[0][0] - out[1][0]).abs().max()),
          float((out[0][1] - out[1][1]).abs().max()))
    torch.testing.assert_close(out[0][0], out[1][0], **_val(acqf._log))
    torch.testing.assert_close(out[0][1], out[1][1], **GRAD)


def test_default_construction_off_the_fused_route(setup):
    """sampler=None: one Sobol sampler only where the fused route applies.  Beyond it (d = 9:
    no member roots; q = 17; cheb_route = "generic") the generic route returns a value."""
    from botorch_amd import qLogNParEGO
    from botorch_amd.models import ModelListGP, SingleTaskGP
    from botorch_amd.sampling import SobolQMCNormalSampler
    model, Xb, Y, X = setup
    acqf = qLogNParEGO(model, Xb)
    assert type(acqf.sampler) is SobolQMCNormalSampler and acqf._roots is not None
    g = torch.Generator().manual_seed(9)
    wide = torch.rand(B, 17, D, dtype=F64, generator=g).to(DEV)
    assert torch.isfinite(acqf(wide)).all()
    fused = acqf(X)
    acqf.cheb_route = "generic"
    torch.testing.assert_close(acqf(X), fused, **_val(True))
    X9 = torch.rand(20, 9, dtype=F64, generator=g).to(DEV)
    m9 = ModelListGP(*[SingleTaskGP(X9, Y[:20, t:t + 1]) for t in range(MT)]).eval()
    with pytest.warns(RuntimeWarning, match="cache_root"):
        a9 = qLogNParEGO(m9, X9)
    assert a9.sampler is None and a9._roots is None
    assert torch.isfinite(a9(torch.rand(2, Q, 9, dtype=F64, generator=g).to(DEV))).all()


def test_optimize_acqf_parego(setup):
    """One restart: L-BFGS-B never ends below its start and the initialisation keeps the best
    raw sample, so the returned value is at least the best raw-sample value up to the
    rounding between two batch shapes, the bar of test_optimize_acqf_constrained_qlognei.
    (Several restarts are optimised as one sum, which does not bound each restart's own.)"""
    from botorch_amd import qLogNParEGO
    from botorch_amd.optim import optimize_acqf
    from botorch_amd.utils_sampling import draw_sobol_samples
    model, Xb, Y, _ = setup
    acqf = qLogNParEGO(model, Xb)  # the default construction: weights drawn, one Sobol sampler
    acqf.cheb_route = "fused"
    bounds = torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)]).to(DEV)
    raw = draw_sobol_samples(bounds=bounds.cpu(), n=16, q=Q, seed=0).to(DEV)
    with torch.no_grad():
        best_raw = float(acqf(raw).max())
    torch.manual_seed(0)
    cand, val = optimize_acqf(acqf, bounds, q=Q, num_restarts=1, raw_samples=16,
                              options={"seed": 0, "maxiter": 20})
    assert cand.shape == (Q, D) and (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
    assert float(val) >= best_raw - 1e-9 * abs(best_raw)
