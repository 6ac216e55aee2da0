"""Risk-averse qSR / qEI / qLogEI over a perturbed SingleTaskGP: the fused route against
the same object's generic route."""
import pytest
import torch

from tests.test_gpu_risk_kernels import ACQ_TOL, DL_TOL, _err

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N_W = 8


@pytest.fixture(scope="module")
def model():
    from botorch_amd.models import SingleTaskGP
    from botorch_amd.transforms import InputPerturbation
    g = torch.Generator().manual_seed(3)
    X = torch.rand(40, 3, dtype=torch.float64, generator=g)
    Y = torch.sin(3.0 * X.sum(-1, keepdim=True)) + 0.05 * torch.randn(40, 1, dtype=torch.float64,
                                                                      generator=g)
    P = 0.15 * torch.randn(N_W, 3, dtype=torch.float64, generator=g)
    tf = InputPerturbation(P.to(DEV), bounds=torch.tensor([[0.0] * 3, [1.0] * 3], device=DEV))
    return SingleTaskGP(X.to(DEV), Y.to(DEV), input_transform=tf).eval()


@pytest.mark.parametrize("measure", ["CVaR", "VaR"])
@pytest.mark.parametrize("name", ["qSimpleRegret", "qExpectedImprovement",
                                  "qLogExpectedImprovement"])
def test_fused_route_matches_generic(model, name, measure):
    from botorch_amd import acquisition as A, risk_measures
    from botorch_amd.sampling import SobolQMCNormalSampler
    kw = {} if name == "qSimpleRegret" else {"best_f": 0.1}
    acqf = getattr(A, name)(model, sampler=SobolQMCNormalSampler(torch.Size([64]), seed=1),
                            objective=getattr(risk_measures, measure)(0.75, N_W), **kw)
    X = torch.rand(3, 2, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    assert A._risk_fused_ok(acqf, X.to(DEV), getattr(acqf, "_fused_mode", 1))  # (1: QMC_QEI)
    acqf.risk_route = "fused"  # (the default takes it only where it was measured faster)
    out = []
    for route in (acqf, acqf._generic_forward):
        Xr = X.to(DEV).requires_grad_(True)
        val = route(Xr)
        val.sum().backward()
        out.append((val.detach().cpu(), Xr.grad.cpu()))
    errs = _err(out[0][0], out[1][0]), _err(out[0][1], out[1][1])
    print("errors (acq, X.grad):", errs)
    assert errs[0] <= ACQ_TOL and errs[1] <= DL_TOL


def test_refusals(model):
    from botorch_amd import acquisition as A
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import SingleTaskGP
    from botorch_amd.transforms import Normalize
    with pytest.raises(UnsupportedError, match="qUpperConfidenceBound.*InputPerturbation"):
        A.qUpperConfidenceBound(model, beta=2.0)
    X = model.train_inputs[0]
    plain = SingleTaskGP(X, model._raw_train_Y, input_transform=Normalize(3))
    with pytest.raises(UnsupportedError, match="input_transform"):
        A.qSimpleRegret(plain)
