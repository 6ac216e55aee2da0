"""SingleTaskGP with Normalize / Warp input transforms on the device: the fit's closure, the
posterior, the admitted acquisition classes and a fit that has to learn a known warp."""
import numpy as np
import pytest
import torch

from tests import warp_restatement as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LO, HI = -1.0, 3.0


def _model(n, d, idx, seed=0, device=DEV):
    from botorch_amd.models import LogNormalPrior, SingleTaskGP
    from botorch_amd.transforms import ChainedInputTransform, Normalize, Warp
    g = torch.Generator().manual_seed(seed)
    X = LO + (HI - LO) * torch.rand(n, d, dtype=torch.float64, generator=g)
    Y = torch.sin(2.0 * X.sum(-1, keepdim=True)) + 0.1 * torch.randn(n, 1, dtype=torch.float64,
                                                                    generator=g)
    bounds = torch.tensor([[LO] * d, [HI] * d], dtype=torch.float64)
    tf = ChainedInputTransform(
        normalize=Normalize(d, bounds=bounds),
        warp=Warp(idx, concentration1_prior=LogNormalPrior(0.0, 0.75 ** 0.5),
                  concentration0_prior=LogNormalPrior(0.1, 0.5)))
    model = SingleTaskGP(X.to(device), Y.to(device), input_transform=tf)
    tf["warp"].concentration1 = torch.linspace(0.6, 1.8, len(idx), dtype=torch.float64)
    tf["warp"].concentration0 = torch.linspace(1.4, 0.7, len(idx), dtype=torch.float64)
    return model, X, Y


def _twin(model):
    """A plain SingleTaskGP on the pre-transformed inputs with the same hyperparameters."""
    from botorch_amd.models import SingleTaskGP
    twin = SingleTaskGP(model.transformed_train_inputs(), model._raw_train_Y)
    twin.covar_module.lengthscale = model.covar_module.lengthscale.detach()
    twin.likelihood.noise = model.likelihood.noise.detach()
    twin.mean_module.constant = float(model.mean_module.constant.detach())
    return twin.eval()


@pytest.mark.parametrize("n,d,idx", [(17, 3, [0, 2]), (130, 6, [1, 2, 5])])
def test_closure_matches_restatement(n, d, idx):
    from botorch_amd import fit
    model, X, _ = _model(n, d, idx)
    layout = fit._layout(model)
    assert [s[0] for s in layout.segments][-2:] == ["concentration0", "concentration1"]
    x = layout.get()
    x[0], x[1] = 0.05, 0.1
    loss, grad = fit.mll_value_and_grad(model, x, layout, sync_model=False)
    k = len(idx)
    t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    noise, const, ls, b, a = t[0], t[1], t[2:2 + d], t[2 + d:2 + d + k], t[2 + d + k:]
    flag = torch.zeros(d, dtype=torch.bool)
    flag[idx] = True
    one = torch.ones(d, dtype=torch.float64)
    A, B = one.index_put((torch.tensor(idx),), a), one.index_put((torch.tensor(idx),), b)
    Xt = ref.warp_reference(X, torch.full((d,), LO, dtype=torch.float64),
                            torch.full((d,), 1.0 / (HI - LO), dtype=torch.float64), A, B, flag)
    warp = model.input_transform["warp"]
    lsp, np_ = model.covar_module.lengthscale_prior, model.likelihood.noise_prior
    ll = (ref.mll(Xt, model.train_targets.cpu(), ls, noise, const, 1.0, 0)
          + ref.lognormal_logpdf(ls, lsp.loc, lsp.scale)
          + ref.lognormal_logpdf(noise, np_.loc, np_.scale)
          + ref.lognormal_logpdf(a, warp.concentration1_prior.loc, warp.concentration1_prior.scale)
          + ref.lognormal_logpdf(b, warp.concentration0_prior.loc, warp.concentration0_prior.scale))
    (-ll / n).backward()
    np.testing.assert_allclose(loss, float(-ll / n), rtol=1e-9)
    np.testing.assert_allclose(grad, t.grad.numpy(), rtol=1e-6, atol=1e-9)


def test_posterior_matches_pretransformed_twin():
    model, X, _ = _model(40, 3, [0, 2])
    model.eval()
    twin = _twin(model)
    Xq = (LO + (HI - LO) * torch.rand(5, 4, 3, dtype=torch.float64)).to(DEV).requires_grad_(True)
    post = model.posterior(Xq)
    Xq_tf = model.input_transform.eval_transform(Xq.detach()).detach()
    want = twin.posterior(Xq_tf)
    torch.testing.assert_close(post.mean, want.mean, rtol=1e-6, atol=1e-8)
    torch.testing.assert_close(post.covariance_matrix, want.covariance_matrix, rtol=1e-4, atol=1e-9)
    w = torch.randn(post.mean.shape, dtype=torch.float64, device=DEV)
    (post.mean * w).sum().backward()
    # chain rule through the restatement: d mean / d X = d mean / d X~ . d X~ / d X
    Xt = Xq_tf.clone().requires_grad_(True)
    (twin.posterior(Xt).mean * w).sum().backward()
    Xc = Xq.detach().cpu().requires_grad_(True)
    (_warp_restated(model, Xc) * Xt.grad.cpu()).sum().backward()
    torch.testing.assert_close(Xq.grad.cpu(), Xc.grad, rtol=1e-6, atol=1e-9)


def _warp_restated(model, X):
    """The model's Normalize + Warp chain on X through the restatement (CPU)."""
    d = X.shape[-1]
    warp = model.input_transform["warp"]
    idx = (warp.indices.cpu(),)
    flag = torch.zeros(d, dtype=torch.bool).index_put(idx, torch.tensor(True))
    one = torch.ones(d, dtype=torch.float64)
    return ref.warp_logspace(X, torch.full((d,), LO, dtype=torch.float64),
                             torch.full((d,), 1.0 / (HI - LO), dtype=torch.float64),
                             one.index_put(idx, warp.concentration1.detach().cpu()),
                             one.index_put(idx, warp.concentration0.detach().cpu()), flag)


def _acqf(name, model, best_f, X_baseline=None):
    from botorch_amd import acquisition as A
    from botorch_amd.sampling import SobolQMCNormalSampler
    cls = getattr(A, name)
    kw = {}
    if name.startswith("q"):
        kw["sampler"] = SobolQMCNormalSampler(torch.Size([64]), seed=3)
    if "Noisy" in name:
        return cls(model, X_baseline=X_baseline, prune_baseline=False, **kw)
    if "UpperConfidenceBound" in name:
        return cls(model, beta=2.0, **kw)
    if name == "PosteriorMean":
        return cls(model)
    return cls(model, best_f=best_f, **kw)


@pytest.mark.parametrize("name,q", [(n, q) for n in ("qExpectedImprovement", "qLogExpectedImprovement",
                                                     "qNoisyExpectedImprovement",
                                                     "qLogNoisyExpectedImprovement",
                                                     "qUpperConfidenceBound") for q in (1, 4)]
                         + [(n, 1) for n in ("ExpectedImprovement", "LogExpectedImprovement",
                                             "UpperConfidenceBound", "PosteriorMean")])
def test_admitted_acquisition_matches_twin(name, q):
    model, X, Y = _model(40, 3, [0, 2])
    model.eval()
    twin = _twin(model)
    tf = model.input_transform
    best_f = float(Y.median())
    Xb = X[:7].to(DEV)
    acq = _acqf(name, model, best_f, Xb)
    acq_twin = _acqf(name, twin, best_f, tf.eval_transform(Xb).detach())
    if name.startswith("q"):
        Xp = (LO + (HI - LO) * torch.rand(2, 3, dtype=torch.float64)).to(DEV)
        acq.set_X_pending(Xp)
        acq_twin.set_X_pending(tf.eval_transform(Xp))
    Xq = (LO + (HI - LO) * torch.rand(6, q, 3, dtype=torch.float64)).to(DEV).requires_grad_(True)
    val = acq(Xq)
    val.sum().backward()
    Xt = tf.eval_transform(Xq.detach()).detach().requires_grad_(True)
    want = acq_twin(Xt)
    want.sum().backward()
    Xc = Xq.detach().cpu().requires_grad_(True)  # the chain rule through the restatement
    (_warp_restated(model, Xc) * Xt.grad.cpu()).sum().backward()
    torch.testing.assert_close(val, want, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(Xq.grad.cpu(), Xc.grad, rtol=1e-6, atol=1e-9)
    if "Noisy" in name:
        assert torch.equal(acq.X_baseline, Xb)  # raw again after the call
    if name.startswith("q"):
        assert torch.equal(acq.X_pending, Xp)  # the raw pending points are back in place


@pytest.mark.parametrize("name,q", [("qExpectedImprovement", 4), ("qLogNoisyExpectedImprovement", 4),
                                    ("qUpperConfidenceBound", 1), ("ExpectedImprovement", 1),
                                    ("LogExpectedImprovement", 1), ("PosteriorMean", 1)])
def test_model_list_of_transformed_members_matches_twin_list(name, q):
    """A ModelListGP of two warped members under a scalarising posterior transform: each
    member's posterior transforms its own input.  The members' warps differ in their
    parameters' storage but hold the same values, so the list of pre-transformed twins,
    called at the transformed points, is the reference."""
    from botorch_amd.models import ModelListGP
    from botorch_amd.objective import ScalarizedPosteriorTransform
    members = [_model(30, 3, [0, 2], seed=s)[0].eval() for s in (1, 2)]
    X = members[0].train_inputs[0].cpu()
    tf = members[0].input_transform
    model, twin = ModelListGP(*members), ModelListGP(*[_twin(m) for m in members])
    pt = ScalarizedPosteriorTransform(torch.tensor([0.7, -0.4], dtype=torch.float64, device=DEV))

    def build(mdl, Xb):
        from botorch_amd import acquisition as A
        from botorch_amd.sampling import SobolQMCNormalSampler
        kw = dict(posterior_transform=pt)
        if name.startswith("q"):
            kw["sampler"] = SobolQMCNormalSampler(torch.Size([64]), seed=3)
        if "Noisy" in name:
            return A.qLogNoisyExpectedImprovement(mdl, X_baseline=Xb, **kw)
        if "UpperConfidenceBound" in name:
            return getattr(A, name)(mdl, beta=2.0, **kw)
        if name == "PosteriorMean":
            return A.PosteriorMean(mdl, **kw)
        return getattr(A, name)(mdl, best_f=0.1, **kw)

    Xb = X[:5].to(DEV)
    acq, acq_twin = build(model, Xb), build(twin, tf.eval_transform(Xb))
    Xq = (LO + (HI - LO) * torch.rand(6, q, 3, dtype=torch.float64)).to(DEV).requires_grad_(True)
    val = acq(Xq)
    val.sum().backward()
    Xt = tf.eval_transform(Xq.detach()).detach().requires_grad_(True)
    want = acq_twin(Xt)
    want.sum().backward()
    Xc = Xq.detach().cpu().requires_grad_(True)
    (_warp_restated(members[0], Xc) * Xt.grad.cpu()).sum().backward()
    torch.testing.assert_close(val, want, rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(Xq.grad.cpu(), Xc.grad, rtol=1e-6, atol=1e-9)


def test_refusals_name_the_transform():
    from botorch_amd import acquisition as A
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.sampling import SobolQMCNormalSampler
    model, X, _ = _model(20, 3, [0])
    with pytest.raises(UnsupportedError, match="input_transform"):
        A.qSimpleRegret(model)
    with pytest.raises(UnsupportedError, match="input_transform"):
        model.fantasize(X[:2].to(DEV), SobolQMCNormalSampler(torch.Size([4])))


def test_every_column_warped_at_d_64_through_the_model():
    """Column 63's flag is bit 63 of the mask: the transform, the constructor and posterior
    on the device against the restatement and a pre-transformed twin."""
    from botorch_amd.models import SingleTaskGP
    from botorch_amd.transforms import Warp
    g = torch.Generator().manual_seed(5)
    X = torch.rand(20, 64, dtype=torch.float64, generator=g)
    Y = torch.sin(X[:, :3].sum(-1, keepdim=True))
    warp = Warp(list(range(64)))
    warp.concentration1 = torch.linspace(0.5, 2.0, 64, dtype=torch.float64)
    warp.concentration0 = torch.linspace(1.5, 0.6, 64, dtype=torch.float64)
    model = SingleTaskGP(X.to(DEV), Y.to(DEV), input_transform=warp).eval()
    flag = torch.ones(64, dtype=torch.bool)
    want = ref.warp_logspace(X, torch.zeros(64, dtype=torch.float64),
                             torch.ones(64, dtype=torch.float64), warp.concentration1.detach().cpu(),
                             warp.concentration0.detach().cpu(), flag)
    Z = warp.transform(X.to(DEV))
    torch.testing.assert_close(Z.detach().cpu(), want, rtol=0, atol=1e-14)
    twin = _twin(model)
    Xq = torch.rand(3, 2, 64, dtype=torch.float64, generator=g).to(DEV)
    post, ptwin = model.posterior(Xq), twin.posterior(warp.transform(Xq).detach())
    torch.testing.assert_close(post.mean, ptwin.mean, rtol=1e-6, atol=1e-8)
    torch.testing.assert_close(post.covariance_matrix, ptwin.covariance_matrix, rtol=1e-4, atol=1e-9)


def test_fit_learns_a_known_warp():
    """y = f(kumaraswamy_cdf(x; 2, 0.5)): freeing the concentrations must lower the loss."""
    from botorch_amd import fit
    from botorch_amd.models import SingleTaskGP
    from botorch_amd.transforms import Warp
    x = torch.linspace(0.01, 0.99, 40, dtype=torch.float64).unsqueeze(-1)
    z = 1.0 - (1.0 - x ** 2.0) ** 0.5
    y = torch.sin(6.0 * z) + z
    losses = {}
    for free in (False, True):
        model = SingleTaskGP(x.to(DEV), y.to(DEV), input_transform=Warp([0]))
        mll = fit.ExactMarginalLogLikelihood(model.likelihood, model)
        bounds = None if free else {"input_transform.concentration0": (1.0, 1.0),
                                       "input_transform.concentration1": (1.0, 1.0)}
        fit.fit_gpytorch_mll(mll, optimizer_kwargs={"bounds": bounds} if bounds else None)
        layout = fit._layout(model)
        losses[free] = fit.mll_value_and_grad(model, layout.get(), layout)[0]
    print("loss with the concentrations at 1:", losses[False], "fitted:", losses[True])
    assert losses[True] < losses[False]
