"""PairwiseGP on the torch route against tests/pairwise_restatement.py: the Laplace
evidence, the MAP utility, the gradient, the posterior and dX; consolidation, the
prior-only model, the refusals, EUBO against the reference's formula, and the fit.

Bounds: 10 x the largest disagreement of the restatement's two forms (plain and on
datapoints permuted with seeds 0, 1, 2) over this file's own cases (the four of
test_torch_route_against_restatement and the n = 20 model of test_posterior_and_dx),
measured once on the CPU, relative to max(1, largest magnitude of
the quantity)."""
import math

import numpy as np
import pytest
import torch
from tests.pairwise_restatement import kernel, make_case, posterior_at, restate

# 10 x (1.3e-12, 9.9e-11, 6.1e-10, 2.2e-10, 6.5e-13), the measured disagreements
BOUND = dict(psi=1.3e-11, f=9.9e-10, grad=6.1e-9, mean=2.2e-9, cov=6.5e-12)
# dX of the mean's and of the covariance's sum at n = 20: 10 x (3.6e-12, 2.4e-13)
BOUND_DX = dict(mean=3.6e-11, cov=2.4e-12)
F64 = torch.float64


def rel(a, b):
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def _model(n=20, m=60, d=2, scale=1.0, kind=0):
    from botorch_amd.models import MaternKernel, PairwiseGP, RBFKernel, ScaleKernel
    X, comp, hyper = make_case(n, m, d, scale)
    base = (RBFKernel if kind == 0 else MaternKernel)(ard_num_dims=d)
    model = PairwiseGP(X, comp, covar_module=ScaleKernel(base), jitter=1e-6)
    model.covar_module.base_kernel.lengthscale = hyper[1:]
    model.covar_module.outputscale = float(hyper[0])
    return model, X, comp, hyper


@pytest.mark.parametrize("n,m,d,scale,kind", [(12, 20, 2, 1, 0), (17, 40, 3, 4, 1),
                                              (33, 100, 3, 6, 0), (33, 100, 3, 1, 1)])
def test_torch_route_against_restatement(n, m, d, scale, kind):
    from botorch_amd.models import pairwise_laplace_torch
    X, comp, hyper = make_case(n, m, d, scale)
    Xq = torch.rand(4, d, dtype=F64, generator=torch.Generator().manual_seed(5))
    ref = restate(X, comp, hyper, kind, 1e-6, Xq=Xq)
    o = pairwise_laplace_torch(X, comp, hyper.reshape(1, -1), kind, jitter=1e-6)
    assert int(o["status"][0]) == 0
    kx = kernel(Xq, X, hyper, kind)
    got = dict(psi=o["psi"][0], f=o["f"][0], grad=o["grad"][0], mean=kx @ o["alpha"][0],
               cov=kernel(Xq, Xq, hyper, kind) - kx @ o["R"][0] @ kx.T)
    for k, bound in BOUND.items():
        print(k, rel(got[k], ref[k]))
        assert rel(got[k], ref[k]) <= bound, k


def test_posterior_and_dx():
    model, X, comp, hyper = _model(kind=1)
    Xq = torch.rand(3, 2, 2, dtype=F64, generator=torch.Generator().manual_seed(7))
    state = restate(X, comp, hyper, 1, 0.0)["state"]
    post = model.posterior(Xq)
    ref = dict(zip(("mean", "cov"), posterior_at(state, Xq)))
    assert rel(post.mean.squeeze(-1), ref["mean"]) <= BOUND["mean"]
    assert rel(post.distribution.covariance_matrix, ref["cov"]) <= BOUND["cov"]
    # dX against autograd through the restatement's kernel expressions
    for k, pick in (("mean", lambda p: p[0]), ("cov", lambda p: p[1])):
        Xr, Xm = Xq.clone().requires_grad_(True), Xq.clone().requires_grad_(True)
        pick(posterior_at(state, Xr)).sum().backward()
        p = model.posterior(Xm)
        pick((p.mean, p.distribution.covariance_matrix)).sum().backward()
        print(k, rel(Xm.grad, Xr.grad))
        assert rel(Xm.grad, Xr.grad) <= BOUND_DX[k], k


def test_consolidation_prior_only_and_refusals():
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import PairwiseGP, PairwiseLogitLikelihood
    X = torch.tensor([[0.1, 0.2], [0.5, 0.5], [0.1, 0.2], [0.9, 0.3]], dtype=F64)
    model = PairwiseGP(X, torch.tensor([[0, 1], [2, 3], [3, 1]]))
    assert model.datapoints.shape[0] == 3 and model.comparisons.tolist() == [[0, 1], [0, 2], [2, 1]]
    assert model.utility.shape == (3,)
    new = model.condition_on_observations(torch.rand(2, 2, dtype=F64), torch.tensor([[0, 1]]))
    assert new.datapoints.shape[0] == 5 and new.comparisons.shape[0] == 4
    prior = PairwiseGP(None, None, covar_module=model.covar_module)
    post = prior.posterior(X[:2])
    assert float(post.mean.abs().max()) == 0.0
    torch.testing.assert_close(post.variance.reshape(-1), torch.ones(2, dtype=F64))
    with pytest.raises(UnsupportedError, match="PairwiseLogitLikelihood"):
        PairwiseLogitLikelihood()
    with pytest.raises(UnsupportedError, match="input_transform"):
        PairwiseGP(X, torch.tensor([[0, 1]]), input_transform=object())
    with pytest.raises(UnsupportedError, match="batched datapoints"):
        PairwiseGP(X.expand(2, 4, 2), torch.tensor([[0, 1]]))
    with pytest.raises(RuntimeError, match="output_indices"):
        model.posterior(X[:2], output_indices=[0])


def test_acquisition_admission():
    """The classes that reach a model through ``posterior`` alone take a PairwiseGP (the
    analytic ones are evaluated); the others refuse it by name."""
    from botorch_amd import acquisition as acq
    from botorch_amd.exceptions import UnsupportedError
    model, X, *_ = _model()
    Xq = torch.rand(3, 1, 2, dtype=F64, generator=torch.Generator().manual_seed(2))
    for a in (acq.ExpectedImprovement(model, 0.1), acq.LogExpectedImprovement(model, 0.1),
              acq.UpperConfidenceBound(model, 2.0), acq.PosteriorMean(model)):
        assert torch.isfinite(a(Xq)).all()
    torch.testing.assert_close(acq.PosteriorMean(model)(Xq), model.posterior(Xq).mean.reshape(3))
    acq.qSimpleRegret(model), acq.qUpperConfidenceBound(model, 2.0)
    acq.qExpectedImprovement(model, 0.1), acq.qLogExpectedImprovement(model, 0.1)
    # (qNEI and qLogNEI sample at construction: tests/test_gpu_pairwise.py, on the device)
    for refused in (lambda: acq.qProbabilityOfImprovement(model, 0.1),
                    lambda: acq.ProbabilityOfImprovement(model, 0.1),
                    lambda: acq.qKnowledgeGradient(model)):
        with pytest.raises(UnsupportedError, match="PairwiseGP is not on the accelerated path"):
            refused()
    with pytest.raises(UnsupportedError, match="needs a PairwiseGP"):
        from botorch_amd import AnalyticExpectedUtilityOfBestOption
        AnalyticExpectedUtilityOfBestOption(object())


@pytest.mark.parametrize("winner", [False, True])
def test_eubo_against_formula(winner):
    from botorch_amd import AnalyticExpectedUtilityOfBestOption
    model, *_ = _model()
    g = torch.Generator().manual_seed(3)
    X = torch.rand(5, 1 if winner else 2, 2, dtype=F64, generator=g)
    prev = torch.rand(1, 2, dtype=F64, generator=g) if winner else None
    got = AnalyticExpectedUtilityOfBestOption(model, previous_winner=prev)(X)
    Y = torch.cat([X, prev.expand(5, 1, 2)], dim=-2) if winner else X
    post = model.posterior(Y)
    mean, cov = post.mean.squeeze(-1), post.distribution.covariance_matrix
    delta = mean[:, 0] - mean[:, 1]
    sigma = torch.sqrt((cov[:, 0, 0] + cov[:, 1, 1] - 2 * cov[:, 0, 1]).clamp_min(1e-8))
    u = delta / sigma
    normal = torch.distributions.Normal(0.0, 1.0)
    want = mean[:, 1] + sigma * torch.exp(normal.log_prob(u)) + delta * normal.cdf(u)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_fit_reaches_the_restatements_optimum():
    """fit_gpytorch_mll at n = 20, d = 2: the restatement's loss at the fitted parameters
    against what scipy L-BFGS-B reaches on the restatement from the same start.  Both stop
    on L-BFGS-B's relative-reduction criterion (ftol 2.2e-9); bound 100 ftol max(1, |loss|)."""
    from scipy.optimize import minimize

    from botorch_amd.fit import fit_gpytorch_mll
    from botorch_amd.models import PairwiseGP, PairwiseLaplaceMarginalLogLikelihood
    X, comp, _ = make_case(20, 60, 2, 1.0)
    model = PairwiseGP(X, comp)
    lp, op = model.covar_module.base_kernel.lengthscale_prior, model.covar_module.outputscale_prior

    def loss(x):  # x: lengthscales, outputscale
        r = restate(X, comp, torch.as_tensor(np.concatenate([x[2:], x[:2]])), 0, 0.0)
        xt = torch.as_tensor(x)
        val = float(r["psi"]) + float(lp.log_prob(xt[:2]).sum()) + float(op.log_prob(xt[2:]).sum())
        g = np.concatenate([r["grad"][1:].numpy(), r["grad"][:1].numpy()])
        g[:2] += (lp.concentration - 1.0) / x[:2] - lp.rate
        g[2:] += op.terms(x[2:])[1]
        return -val, -g

    x0 = np.array([lp.mode, lp.mode, 1.0])
    ref = minimize(loss, x0, jac=True, method="L-BFGS-B", bounds=[(1e-4, None)] * 2 + [(0.005, 200.0)])
    fit_gpytorch_mll(PairwiseLaplaceMarginalLogLikelihood(model.likelihood, model))
    cm = model.covar_module
    x = np.array(cm.lengthscale.detach().reshape(-1).tolist() + [float(cm.outputscale)])
    print(loss(x)[0], ref.fun)
    assert abs(loss(x)[0] - ref.fun) <= 2.2e-7 * max(1.0, abs(ref.fun))
