"""SingleTaskMultiFidelityGP on the torch route and the multi-fidelity utilities: what
needs no GPU (the fused kernels: tests/test_gpu_ltf_kernels.py, test_gpu_ltf_model.py)."""
import math
import warnings

import pytest
import torch

from tests import ltf_restatement as R

F64 = dict(dtype=torch.float64)


def _data(n=12, d=4):
    g = torch.Generator().manual_seed(3)
    X = torch.rand(n, d, generator=g, **F64)
    return X, torch.sin(3.0 * X.sum(-1, keepdim=True))


def test_constructor_validation_and_messages():
    from botorch_amd import SingleTaskMultiFidelityGP as GP
    from botorch_amd.exceptions import UnsupportedError
    X, Y = _data()
    with pytest.raises(UnsupportedError, match="requires at least one fidelity parameter"):
        GP(X, Y)
    with pytest.raises(ValueError, match="Cannot specify both `data_fidelity` and `data_fidelities`"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            GP(X, Y, data_fidelity=3, data_fidelities=[3])
    with pytest.warns(DeprecationWarning, match="`data_fidelity` argument is deprecated"):
        m = GP(X, Y, data_fidelity=3)
    assert m.fidelity_kernels[0].fidelity_dims == [3]
    m = GP(X, Y, iteration_fidelity=-2, data_fidelities=[-1])
    assert m.fidelity_kernels[0].fidelity_dims == [2, 3]
    assert len(GP(X, Y, data_fidelities=[2, 3]).fidelity_kernels) == 2
    for kw, word in ((dict(nu=1.5), "nu"), (dict(input_transform=object()), "input_transform")):
        with pytest.raises(UnsupportedError, match=word):
            GP(X, Y, data_fidelities=[3], **kw)
    with pytest.raises(UnsupportedError, match="m > 1"):
        GP(X, torch.cat([Y, Y], -1), data_fidelities=[3])
    with pytest.raises(UnsupportedError, match="batched"):
        GP(X.unsqueeze(0), Y.unsqueeze(0), data_fidelities=[3])
    m = GP(X, Y, data_fidelities=[3])
    with pytest.raises(UnsupportedError, match="condition_on_observations"):
        m.condition_on_observations(X, Y)
    with pytest.raises(UnsupportedError, match="fantasize"):
        m.fantasize(X, None)


def test_default_priors_bounds_and_route():
    from botorch_amd import SingleTaskMultiFidelityGP as GP
    from botorch_amd.fit import _layout
    from botorch_amd.models import FixedNoiseGaussianLikelihood, Standardize
    X, Y = _data()
    m = GP(X, Y, data_fidelities=[3])
    k = m.fidelity_kernels[0]
    pri = [(p.concentration, p.rate) for p in (
        k.covar_module_unbiased.lengthscale_prior, k.covar_module_biased.lengthscale_prior,
        k.power_prior, m.outputscale_prior)]
    assert pri == [(3.0, 6.0), (6.0, 2.0), (3.0, 3.0), (2.0, 0.15)]
    assert isinstance(m.outcome_transform, Standardize)
    lay = _layout(m)
    assert lay.size == 2 + 3 + 3 + 1 + 1
    assert [b[0] for b in lay.bounds] == [1e-4, None] + [0.025] * 6 + [1e-4, 1e-6]
    assert torch.allclose(torch.as_tensor(lay.get()[2:]), torch.full((8,), math.log(2.0), **F64))
    assert isinstance(GP(X, Y, Y * 0 + 0.01, data_fidelities=[3]).likelihood,
                      FixedNoiseGaussianLikelihood)
    assert not m.fused()          # CPU tensors: the torch route
    m._route = "fused"
    assert m.fused()
    m._route = "torch"
    assert not m.fused()


@pytest.mark.parametrize("nf", (1, 2))
def test_torch_route_matches_the_restatement(nf):
    from botorch_amd import SingleTaskMultiFidelityGP as GP
    from botorch_amd.fit import _layout
    Z, y, p, noise, c = R.make_case(nf, 3, 14)
    m = GP(Z, y.unsqueeze(-1), outcome_transform=None, **(
        dict(data_fidelities=[0]) if nf == 1 else dict(iteration_fidelity=0, data_fidelities=[p["fc"][1]])))
    lay = _layout(m)
    x = torch.cat([noise.reshape(1), torch.tensor([c], **F64), p["l0"], p["l1"], p["pw"].reshape(1),
                   p["o"].reshape(1)]).numpy()
    lay.set(x)
    X = R.make_queries(Z, p, 3, 2).requires_grad_(True)
    mean, cov = m.moments(X)
    (mean.sum() + (cov * cov).sum()).backward()
    Xr = X.detach().clone().requires_grad_(True)
    mr, cr = R.posterior(Z, y, p, noise, c, Xr)
    (mr.sum() + (cr * cr).sum()).backward()
    torch.testing.assert_close(mean, mr, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(cov, cr, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(X.grad, Xr.grad, rtol=1e-9, atol=1e-10)
    # the closure's data term and gradient against the restatement's autograd
    ll, g = R.ll_autograd(Z, y, p, noise, c)
    m.likelihood.noise_prior = None
    for k in m.fidelity_kernels:
        k.covar_module_unbiased.lengthscale_prior = k.covar_module_biased.lengthscale_prior = None
        k.power_prior = None
    m.outputscale_prior = None
    lay = _layout(m)
    v, gv = lay.value_and_grad(x)
    n = Z.shape[0]
    ref = torch.cat([g["noise"].reshape(1), g["const"].reshape(1), g["l0"], g["l1"],
                     g["pw"].reshape(1), g["o"].reshape(1)])
    assert abs(v + float(ll) / n) < 1e-12
    torch.testing.assert_close(torch.as_tensor(gv), -ref / n, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("it,dfs", ((None, [3]), (2, []), (2, [1, 3])))
def test_not_truncated_product_kernel_on_the_torch_route(it, dfs):
    """linear_truncated=False: its priors, closure and posterior against the restatement."""
    from botorch_amd import SingleTaskMultiFidelityGP as GP
    from botorch_amd.fit import _layout
    g = torch.Generator().manual_seed(9)
    Z = torch.rand(14, 4, generator=g, **F64)
    y = torch.sin(3.0 * Z.sum(-1))
    m = GP(Z, y.unsqueeze(-1), iteration_fidelity=it, data_fidelities=dfs or None,
           linear_truncated=False, outcome_transform=None)
    assert not m.fused()
    lay = _layout(m)
    xc = [j for j in range(4) if j != it and j not in dfs]
    nh = len(xc) + (3 if it is not None else 0) + 2 * len(dfs)
    assert lay.size == 2 + nh + 1 and all(pr.concentration == 3.0 and pr.rate == 6.0
                                          for pr, _, _ in lay.priors[:-1])
    x = torch.cat([torch.tensor([0.05, 0.3], **F64), 0.4 + torch.rand(nh + 1, generator=g, **F64)])
    lay.set(x.numpy())
    assert torch.equal(torch.as_tensor(lay.get()), x)

    def ref(t, X1, X2):
        h, at = t[2:], len(xc)
        q = dict(xc=xc, ls=h[:at], o=h[-1], it=it, dfs=dfs, ed=None, ds=[])
        if it is not None:
            q["ed"], at = (h[at], h[at + 1], h[at + 2]), at + 3
        q["ds"] = [(h[at + 2 * i], h[at + 2 * i + 1]) for i in range(len(dfs))]
        return R.kernel_product(X1, X2, q)

    t = x.clone().requires_grad_(True)
    L = torch.linalg.cholesky(ref(t, Z, Z) + t[0] * torch.eye(14, **F64))
    b = torch.linalg.solve_triangular(L, (y - t[1]).unsqueeze(-1), upper=False)
    ll = -0.5 * (b * b).sum() - torch.log(torch.diagonal(L)).sum() - 7 * math.log(2 * math.pi)
    h = t[2:]
    prior = (3 * math.log(6.0) + 2 * torch.log(h[:-1]) - 6 * h[:-1] - math.lgamma(3.0)).sum() \
        + 2 * math.log(0.15) + torch.log(h[-1]) - 0.15 * h[-1] - math.lgamma(2.0)
    lx = torch.log(t[0])
    prior = prior - 0.5 * (lx + 4.0) ** 2 - 0.5 * math.log(2 * math.pi) - lx
    loss = -(ll + prior) / 14
    (gr,) = torch.autograd.grad(loss, t)
    v, gv = lay.value_and_grad(x.numpy())
    assert abs(v - float(loss.detach())) < 1e-12
    torch.testing.assert_close(torch.as_tensor(gv), gr, rtol=1e-9, atol=1e-11)
    X = torch.rand(3, 2, 4, generator=g, **F64)
    mean, cov = m.moments(X)
    A, Kx = ref(x, Z, Z) + x[0] * torch.eye(14, **F64), ref(x, X, Z)
    torch.testing.assert_close(mean, x[1] + Kx @ torch.linalg.solve(A, y - x[1]), rtol=1e-9, atol=1e-10)
    torch.testing.assert_close(cov, ref(x, X, X) - Kx @ torch.linalg.solve(A, Kx.mT), rtol=1e-8, atol=1e-10)


def test_utilities_by_hand():
    from botorch_amd import (AffineFidelityCostModel, InverseCostWeightedUtility,
                             expand_trace_observations, project_to_target_fidelity)
    from botorch_amd.exceptions import UnsupportedError
    X = torch.tensor([[[0.1, 0.2, 0.5], [0.3, 0.4, 1.0]]], **F64, requires_grad=True)
    cm = AffineFidelityCostModel({2: 2.0}, fixed_cost=5.0)
    assert cm(X).tolist() == [[[6.0], [7.0]]]
    assert AffineFidelityCostModel()(X).squeeze(-1).tolist() == [[0.51, 1.01]]
    util = InverseCostWeightedUtility(cm)
    deltas = torch.tensor([[2.6], [-1.0]], **F64)  # N_f x b: divided where positive, multiplied otherwise
    assert util(X=X, deltas=deltas).tolist() == [[0.2], [-13.0]]
    with pytest.raises(UnsupportedError, match="deterministic"):
        InverseCostWeightedUtility(object())
    P = project_to_target_fidelity(X)
    assert P[..., 2].tolist() == [[1.0, 1.0]] and torch.equal(P[..., :2], X[..., :2])
    P.sum().backward()
    assert X.grad[..., 2].tolist() == [[0.0, 0.0]] and (X.grad[..., :2] == 1).all()
    P = project_to_target_fidelity(X.detach()[..., :2], {1: 0.7}, d=3)
    assert P[0, 0].tolist() == [0.1, 0.7, 0.2]
    E = expand_trace_observations(X.detach(), num_trace_obs=2)
    assert E.shape == (1, 6, 3) and torch.equal(E[:, :2], X.detach())
    torch.testing.assert_close(E[0, :, 2], torch.tensor([0.5, 1.0, 1 / 3, 2 / 3, 1 / 6, 1 / 3], **F64))
    assert torch.equal(E[0, 2:, :2], X.detach()[0, :, :2].repeat(2, 1))


def test_augmented_hartmann_optimum():
    from botorch_amd.multi_fidelity import AugmentedHartmann
    from botorch_amd.test_functions import Hartmann
    f = AugmentedHartmann()
    x = torch.tensor(f._optimizers[0], **F64)
    assert abs(float(f(x)) - f._optimal_value) < 1e-5
    assert float(f(x)) == float(Hartmann()(x[:6]))       # at full fidelity: Hartmann-6
    lo = x.clone()
    lo[6] = 0.0
    assert float(f(lo)) > float(f(x)) and float(AugmentedHartmann(negate=True)(x)) == -float(f(x))


def test_kg_and_audit_refusals():
    from botorch_amd import (AffineFidelityCostModel, InverseCostWeightedUtility,
                             SingleTaskMultiFidelityGP, project_to_target_fidelity,
                             qMultiFidelityKnowledgeGradient as MFKG)
    from botorch_amd import acquisition as A
    from botorch_amd.pathwise import draw_matheron_paths
    from botorch_amd.exceptions import UnsupportedError
    X, Y = _data()
    m = SingleTaskMultiFidelityGP(X, Y, data_fidelities=[3])
    util = InverseCostWeightedUtility(AffineFidelityCostModel({3: 1.0}, fixed_cost=0.2))
    with pytest.raises(UnsupportedError, match="Cost-aware KG requires current_value."):
        MFKG(m, num_fantasies=4, cost_aware_utility=util)
    with pytest.raises(UnsupportedError, match="valfunc_cls"):
        MFKG(m, num_fantasies=4, valfunc_cls=object)
    for call in (lambda: A.qNegIntegratedPosteriorVariance(m, X),
                 lambda: draw_matheron_paths(m, torch.Size([2]))):
        with pytest.raises(UnsupportedError, match="SingleTaskMultiFidelityGP"):
            call()
    ei = A.LogExpectedImprovement(m, best_f=float(Y.max()))  # an admitted class: through posterior
    assert torch.isfinite(ei(X[:6].reshape(6, 1, 4))).all()
    acq = MFKG(m, num_fantasies=4, current_value=0.1, cost_aware_utility=util,
               project=project_to_target_fidelity)       # (the forward: tests/test_gpu_ltf_model.py)
    assert acq.get_augmented_q_batch_size(2) == 6 and acq.extract_candidates(X[:6]).shape == (2, 4)
