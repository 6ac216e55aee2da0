"""MixedSingleTaskGP and optimize_acqf_mixed without a GPU: the restatement's two
forms agree, the torch route equals the restatement, constructor errors and
refusals, the mixed optimiser on a deterministic acquisition function."""
import numpy as np
import pytest
import torch

from tests import mixed_restatement as R

FLOOR = 1e-15  # ll_closed against ll_autograd relative to sum |summand|: 9.6e-16 measured


def _model(kind=1, dc=3, dk=2, n=30, fixed=False, **kw):
    from botorch_amd.models import MixedSingleTaskGP, RBFKernel
    Z, y, p, noise, c = R.make_case(kind, dc, dk, n, fixed_noise=fixed)
    if kind == 0:
        kw["cont_kernel_factory"] = lambda batch_shape, ard_num_dims, active_dims: RBFKernel(
            ard_num_dims=ard_num_dims, lengthscale_lower=1e-4, initial=0.5)
    m = MixedSingleTaskGP(Z, y.unsqueeze(-1), [j - Z.shape[1] for j in p["cat"]],
                          train_Yvar=noise.unsqueeze(-1) if fixed else None, **kw)
    return m, Z, y, p, noise


@pytest.mark.parametrize("kind,dims,n", [(0, (1, 1), 17), (1, (3, 2), 70), (1, (8, 8), 130)])
def test_restatement_forms_agree(kind, dims, n):
    Z, y, p, noise, c = R.make_case(kind, *dims, n, fixed_noise=True)
    ll_a, ga = R.ll_autograd(Z, y, p, noise, c)
    ll_c, gc, S, _ = R.ll_closed(Z, y, p, noise, c)
    assert abs(float(ll_a - ll_c)) <= 1e-12 * abs(float(ll_a))
    for k in R.NAMES:
        assert ((gc[k] - ga[k]).abs() <= FLOOR * S[k].abs().sum(dim=(0, 1))).all(), k
    torch.testing.assert_close(gc["noise"], ga["noise"], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("kind,dims,fixed", [(1, (3, 2), False), (0, (2, 3), True), (1, (9, 2), False)])
def test_torch_route_equals_restatement(kind, dims, fixed):
    """(9, 2) is the shape beyond the fused limits: the torch route on any device."""
    from botorch_amd import fit, kernels
    m, Z, y, p, noise = _model(kind, *dims, fixed=fixed)
    assert m.cat_dims == p["cat"] and m.cont_dims == p["cont"] and not m.fused()
    assert kernels.mixed_fused_ok(*dims) == (dims[0] <= 8)
    lay = fit._layout(m)
    x = lay.get()
    x[lay.h0:] = np.linspace(0.4, 1.3, lay.size - lay.h0)
    v, g = lay.value_and_grad(x)
    if not fixed:
        v_ref, g_ref = R.neg_mll_flat(x, Z, y, kind, p["cont"], p["cat"])
        np.testing.assert_allclose(v, v_ref, rtol=1e-12)
        np.testing.assert_allclose(g, g_ref, rtol=1e-9, atol=1e-12)
    lay.set(x)
    np.testing.assert_array_equal(lay.get(), x)
    h = torch.as_tensor(x[lay.h0:])
    dc, dk = dims
    pp = dict(p, l1=h[:dc], lam1=h[dc:dc + dk], l2=h[dc + dk:2 * dc + dk], lam2=h[2 * dc + dk:-3],
              os=h[-3], oc=h[-2], op=h[-1])
    X = R.make_queries(Z, p, 3, 4).requires_grad_(True)
    nz = noise if fixed else torch.tensor(float(x[0]))
    post = m.posterior(X)
    mean, cov = R.posterior_explicit(Z, y, pp, nz, float(x[lay.o]), X)
    # two orders of the same solves: cond(A) ~ n o / noise ~ 1e5, so eps cond ~ 1e-11 per entry
    torch.testing.assert_close(post.mean.squeeze(-1), mean, rtol=1e-8, atol=1e-9)
    torch.testing.assert_close(post.mvn.covariance_matrix, cov, rtol=1e-8, atol=1e-9)
    (dX,) = torch.autograd.grad(post.mean.sum() + post.variance.sum(), X)
    assert (dX[..., p["cat"]] == 0).all() and torch.isfinite(dX).all()


def test_defaults_errors_and_refusals():
    from botorch_amd import MixedSingleTaskGP, acquisition as A
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import Standardize
    from botorch_amd.pathwise import draw_matheron_paths
    m, Z, y, p, _ = _model(outcome_transform=Standardize(m=1))
    ln2 = np.log(2.0)
    assert float(m.likelihood.noise.detach()) == 1e-3 and m.likelihood.noise_lower == 1e-6
    assert (m.likelihood.noise_prior.concentration, m.likelihood.noise_prior.rate) == (0.9, 10.0)
    assert torch.allclose(m.hyper_vector(), torch.full((10,), ln2, dtype=torch.float64))
    assert torch.allclose(m.outputscales, torch.full((3,), ln2, dtype=torch.float64))
    assert m.kind == 1 and m.cont_kernel_sum.lengthscale_prior is None
    assert not hasattr(m, "prediction_cache")
    Y = y.unsqueeze(-1)
    with pytest.raises(ValueError, match="Must specify categorical dimensions for MixedSingleTaskGP"):
        MixedSingleTaskGP(Z, Y, [])
    for kw, pat in ((dict(train_X=Z, train_Y=Y, input_transform=object()), "input_transform"),
                    (dict(train_X=Z, train_Y=torch.cat([Y, Y], -1)), "m > 1"),
                    (dict(train_X=Z.unsqueeze(0), train_Y=Y.unsqueeze(0)), "batched")):
        with pytest.raises(UnsupportedError, match=pat):
            MixedSingleTaskGP(cat_dims=[0], **kw)
    for call in (lambda: m.condition_on_observations(Z[:1], Y[:1]), lambda: m.fantasize(Z[:1], None),
                 lambda: A.qKnowledgeGradient(m, num_fantasies=2),
                 lambda: A.qNegIntegratedPosteriorVariance(m, Z), lambda: draw_matheron_paths(m, torch.Size([2]))):
        with pytest.raises(UnsupportedError, match="MixedSingleTaskGP"):
            call()
    only_cat = MixedSingleTaskGP(Z[:, p["cat"]], Y, [0, 1])  # d_c = 0: os * kap, torch route
    assert only_cat.posterior(Z[:4, p["cat"]]).mean.shape == (4, 1) and not only_cat.fused()
    ei = A.LogExpectedImprovement(m, best_f=float(y.max()))
    assert torch.isfinite(ei(Z[:3].unsqueeze(1))).all()


class _Peak(torch.nn.Module):
    """sum over q of 0.1 c - (x0 - c / 4)^2: deterministic, maximised at x0 = c / 4,
    best for the largest category c = 2 (value 0.2 per point)."""
    X_pending = None
    seen = []

    def set_X_pending(self, X):
        self.X_pending = X
        self.seen.append(None if X is None else X.clone())

    def forward(self, X):
        c = X[..., 1]
        return (0.1 * c - (X[..., 0] - 0.25 * c) ** 2).sum(-1)


def test_optimize_acqf_mixed():
    from botorch_amd.optim import optimize_acqf_mixed
    acq = _Peak()
    bounds = torch.tensor([[0.0, 0.0], [1.0, 3.0]], dtype=torch.float64)
    ffl = [{1: 0.0}, {1: 2.0}, {1: 1.0}]
    with pytest.raises(ValueError, match="non-empty"):
        optimize_acqf_mixed(acq, bounds, 1, 2, [], raw_samples=8)
    cand, val = optimize_acqf_mixed(acq, bounds, 1, 2, ffl, raw_samples=8)
    assert cand.shape == (1, 2) and cand[0, 1] == 2.0
    assert abs(float(cand[0, 0]) - 0.5) < 1e-5 and abs(float(val) - 0.2) < 1e-9
    pend = torch.tensor([[0.9, 1.0]], dtype=torch.float64)
    acq.X_pending, acq.seen = pend, []
    cand, val = optimize_acqf_mixed(acq, bounds, 2, 2, ffl, raw_samples=8)
    assert cand.shape == (2, 2) and set(cand[:, 1].tolist()) <= {0.0, 1.0, 2.0}
    assert [None if s is None else s.shape[0] for s in acq.seen] == [2, 3, 1] and acq.X_pending is pend
    assert torch.equal(acq.seen[0][1:], cand[:1]) and torch.equal(val, acq(cand))
