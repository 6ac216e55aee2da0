"""bo_pairwise_laplace (csrc/pairwise.hip) against tests/pairwise_restatement.py, and
PairwiseGP on the fused route against its torch route.

Bounds: 10 x the largest disagreement of the restatement's two forms (plain and on
permuted datapoints) over this file's own cases, where the 144 of
test_kernel_against_restatement dominate; measured once on the CPU,
relative to max(1, largest magnitude of the quantity)."""
import pytest
import torch

from tests.pairwise_restatement import kernel, make_case, restate
from tests.test_pairwise_cpu import F64, _model, rel

# 10 x (4.4e-10, 3.2e-9, 3.4e-9, 6.3e-9, 1.4e-10), the measured disagreements
BOUND = dict(psi=4.4e-9, f=3.2e-8, grad=3.4e-8, mean=6.3e-8, cov=1.4e-9)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _window(t):
    """t inside a NaN-filled buffer (reads outside the window poison the result)."""
    buf = torch.full((t.numel() + 64,), float("nan") if t.is_floating_point() else -1,
                     dtype=t.dtype, device=DEV)
    buf[32:32 + t.numel()] = t.reshape(-1).to(DEV)
    return buf[32:32 + t.numel()].view(t.shape)


def _launch(X, comp, hyper, kind, **kw):
    from botorch_amd import kernels
    n, d = X.shape
    hyper = hyper.reshape(-1, d + 1)
    inc = tuple(_window(t) for t in kernels.pairwise_incidence(comp, n))
    work = torch.full((kernels.pairwise_laplace_work(n, comp.shape[0], d, hyper.shape[0]),),
                      float("nan"), dtype=F64, device=DEV)
    kw.setdefault("jitter", 1e-6)
    return kernels.pairwise_laplace(_window(X), inc, _window(hyper), kind, work=work, **kw)


def _check(X, comp, hyper, kind, o, row=0):
    Xq = torch.rand(4, X.shape[1], dtype=F64, generator=torch.Generator().manual_seed(5))
    ref = restate(X, comp, hyper, kind, 1e-6, Xq=Xq)
    kx = kernel(Xq, X, hyper, kind)
    got = dict(psi=o["psi"][row].cpu(), f=o["f"][row].cpu(), grad=o["grad"][row].cpu(),
               mean=kx @ o["alpha"][row].cpu(),
               cov=kernel(Xq, Xq, hyper, kind) - kx @ o["R"][row].cpu() @ kx.T)
    for k, bound in BOUND.items():
        print(k, rel(got[k], ref[k]))
        assert rel(got[k], ref[k]) <= bound, k


@pytest.mark.parametrize("d", [1, 3, 65])
@pytest.mark.parametrize("many", [False, True])
@pytest.mark.parametrize("n", [2, 15, 16, 17, 33, 129])
def test_kernel_against_restatement(n, many, d):
    for kind in (0, 1):
        for scale in (1, 6):
            X, comp, hyper = make_case(n, 3 * n if many else 1, d, scale)
            o = _launch(X, comp, hyper, kind)
            assert o["status"].tolist() == [0]
            _check(X, comp, hyper, kind, o)


@pytest.mark.parametrize("comp", [[[0, 1], [0, 1], [2, 3]], [[0, 1], [1, 0], [4, 2]], [[0, 1]]],
                         ids=["repeated", "contradictory", "isolated"])
def test_special_comparisons(comp):
    X, _, hyper = make_case(17, 1, 3, 1)
    comp = torch.tensor(comp)
    _check(X, comp, hyper, 1, _launch(X, comp, hyper, 1))


def test_warm_start_determinism_and_rows():
    X, comp, hyper = make_case(33, 100, 3, 6)
    o = _launch(X, comp, hyper, 0)
    warm = _launch(X, comp, hyper, 0, f_init=o["f"].clone())
    assert warm["iters"].tolist() == [1] and warm["status"].tolist() == [0]
    hy3 = torch.stack([hyper, 0.7 * hyper, 1.2 * hyper])
    a, b = _launch(X, comp, hy3, 0), _launch(X, comp, hy3, 0)
    one = _launch(X, comp, hy3[1], 0)
    for k in ("f", "alpha", "psi", "grad", "R", "iters"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k][1], one[k][0]), k
    _check(X, comp, hy3[2], 0, a, row=2)


def test_status():
    X, comp, hyper = make_case(17, 40, 3, 1)
    hy3 = torch.stack([hyper, hyper, hyper])
    hy3[1, 2] = float("nan")
    o = _launch(X, comp, hy3, 1)
    assert o["status"].tolist() == [0, 1, 0] and float(o["psi"][1]) == -float("inf")
    assert not o["grad"][1].any() and torch.equal(o["f"][0], o["f"][2])
    X2 = X.clone()
    X2[5] = X2[9]
    assert _launch(X2, comp, hyper, 0, jitter=0.0)["status"].tolist() == [2]
    capped = _launch(X, comp, hyper, 0, maxfev=1)
    assert capped["status"].tolist() == [3] and torch.isfinite(capped["f"]).all()


def test_model_fused_against_torch_route():
    from botorch_amd import AnalyticExpectedUtilityOfBestOption, qExpectedUtilityOfBestOption
    models = []
    from botorch_amd.sampling import SobolQMCNormalSampler
    for route in ("fused", "torch"):  # (both on the device: the Sobol sampler lives there)
        m, X, comp, hyper = _model(33, 100, 3, 1.0, kind=1)
        m.set_train_data(X.to(DEV), comp.to(DEV))
        m._route = route
        models.append(m)
    g = torch.Generator().manual_seed(11)
    Xq = torch.rand(6, 2, 3, dtype=F64, generator=g)
    out = []
    for m in models:
        Xg = Xq.to(m.datapoints.device).requires_grad_(True)
        post = m.posterior(Xg)
        eubo = AnalyticExpectedUtilityOfBestOption(m)(Xg)
        qeubo = qExpectedUtilityOfBestOption(
            m, sampler=SobolQMCNormalSampler(torch.Size([64]), seed=3))(Xg)
        (post.mean.sum() + post.distribution.covariance_matrix.sum() + eubo.sum()).backward()
        out.append([t.detach().cpu() for t in (post.mean, post.distribution.covariance_matrix,
                                               Xg.grad, eubo, qeubo)])
    for got, want, key in zip(out[0], out[1], ("mean", "cov", "mean", "mean", "mean")):
        assert rel(got, want) <= BOUND[key]


def test_mc_acquisitions_admit_the_model():
    from botorch_amd import acquisition as acq, qExpectedUtilityOfBestOption
    from botorch_amd.sampling import SobolQMCNormalSampler
    m, X, comp, _ = _model(33, 100, 3, 1.0)
    m.set_train_data(X.to(DEV), comp.to(DEV))
    Xq = torch.rand(4, 2, 3, dtype=F64, generator=torch.Generator().manual_seed(4)).to(DEV)
    sampler = lambda: SobolQMCNormalSampler(torch.Size([64]), seed=3)
    for a in (acq.qExpectedImprovement(m, 0.1, sampler()), acq.qLogExpectedImprovement(m, 0.1, sampler()),
              acq.qNoisyExpectedImprovement(m, X.to(DEV)[:5], sampler()),
              acq.qLogNoisyExpectedImprovement(m, X.to(DEV)[:5], sampler()),
              acq.qUpperConfidenceBound(m, 2.0, sampler())):
        assert torch.isfinite(a(Xq)).all(), type(a).__name__
    assert torch.equal(acq.qSimpleRegret(m, sampler())(Xq),
                       qExpectedUtilityOfBestOption(m, sampler=sampler())(Xq))


def test_fit_on_the_device_matches_the_torch_route():
    """Both fits stop on L-BFGS-B's relative-reduction criterion (ftol 2.2e-9): bound
    100 ftol max(1, |loss|), as tests/test_pairwise_cpu.py."""
    from botorch_amd.fit import _layout, fit_gpytorch_mll
    from botorch_amd.models import PairwiseGP, PairwiseLaplaceMarginalLogLikelihood
    X, comp, _ = make_case(33, 100, 3, 1.0)
    losses = []
    for route, dev in (("fused", DEV), ("torch", "cpu")):
        m = PairwiseGP(X.to(dev), comp.to(dev))
        m._route = route
        fit_gpytorch_mll(PairwiseLaplaceMarginalLogLikelihood(m.likelihood, m))
        m._route, lay = "torch", _layout(m)
        m.set_train_data(X, comp)
        losses.append(lay.value_and_grad(lay.get())[0])
    print(losses)
    assert abs(losses[0] - losses[1]) <= 2.2e-7 * max(1.0, abs(losses[1]))
