"""SingleTaskMultiFidelityGP and qMultiFidelityKnowledgeGradient on the fused route
(n = 33, d_x = 3, one and two fidelity columns) against tests/ltf_restatement.py.
Tolerances are 10 x the largest disagreement of two references on these same cases,
measured once on the CPU: posterior (Cholesky) against posterior_inverse (linalg.inv)
differ by 8.9e-17 of sum |summand| in the mean, 3.5e-17 in the covariance and 1.2e-14 of
max |dX| in the gradient; ll_closed against ll_autograd by 2.25e-15 of sum |summand|
(test_gpu_ltf_kernels).  The knowledge gradient's four cases (_mfkg_reference on the two
sets of moments, base samples from randn since the Sobol ones come from the device)
differ by 4.4e-14 of max |acq| and 3.1e-14 of max |gradient|."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import ltf_restatement as R

pytestmark = pytest.mark.gpu
MEAN_TOL, COV_TOL = 8.9e-16, 3.5e-16   # of sum |summand|
GRAD_TOL = 1.2e-13                     # of max |dX|
KG_TOL, KG_GRAD_TOL = 4.4e-13, 3.1e-13 # of max |acq|, of max |gradient|
SUM_TOL = 2.3e-14                      # of sum |summand|
DEV = "cuda"
N, NFANT, PEND = 33, 4, 0.35   # (PEND: every coordinate of the pending point)


@functools.lru_cache(maxsize=None)
def _case(nf, fixed=False):
    from botorch_amd import SingleTaskMultiFidelityGP, fit
    Z, y, p, noise, c = R.make_case(nf, 3, N, fixed_noise=fixed)
    kw = dict(data_fidelities=[0]) if nf == 1 else dict(iteration_fidelity=0, data_fidelities=[p["fc"][1]])
    m = SingleTaskMultiFidelityGP(Z.to(DEV), y.unsqueeze(-1).to(DEV), outcome_transform=None,
                                  train_Yvar=noise.unsqueeze(-1).to(DEV) if fixed else None, **kw)
    lay = fit._layout(m)
    x = np.concatenate([[] if fixed else [float(noise)], [c], p["l0"], p["l1"], [float(p["pw"]), float(p["o"])]])
    lay.set(x)
    return m, lay, x, Z, y, p, noise, c


def _queries(Z, p):
    """3 x 2 x d: fidelities at 0, 1, inside, beyond both ends; distinct points."""
    X = torch.rand(3, 2, Z.shape[1], dtype=torch.float64, generator=torch.Generator().manual_seed(11))
    f = torch.tensor([[0.0, 1.0], [0.4, 1.3], [-0.2, 0.7]], dtype=torch.float64)
    X[..., p["fc"]] = f.unsqueeze(-1).expand(3, 2, len(p["fc"]))
    return X


def _gamma(x, a, b):
    return a * math.log(b) + (a - 1.0) * torch.log(x) - b * x - math.lgamma(a)


@pytest.mark.parametrize("nf,fixed", ((1, False), (2, False), (2, True)))
def test_mll_value_and_grad(nf, fixed):
    """The fit's loss, priors included, against autograd on the restatement."""
    from botorch_amd import fit
    m, lay, x, Z, y, p, noise, c = _case(nf, fixed)
    assert m.fused()
    v, g = fit.ltf_mll_value_and_grad(m, x, lay)
    t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    o = 0 if fixed else 1
    h = t[o + 1:]
    pp = dict(p, l0=h[:3], l1=h[3:6], pw=h[6], o=h[7])
    A = R.kernel(Z, Z, pp) + (torch.diag(noise) if fixed else t[0] * torch.eye(N, dtype=torch.float64))
    L = torch.linalg.cholesky(A)
    b = torch.linalg.solve_triangular(L, (y - t[o]).unsqueeze(-1), upper=False)
    ll = -0.5 * (b * b).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * N * math.log(2 * math.pi)
    prior = _gamma(h[:3], 3.0, 6.0).sum() + _gamma(h[3:6], 6.0, 2.0).sum() + _gamma(h[6], 3.0, 3.0) \
        + _gamma(h[7], 2.0, 0.15)
    if not fixed:  # LogNormal(-4, 1) on the noise
        lx = torch.log(t[0])
        prior = prior - 0.5 * (lx + 4.0) ** 2 - 0.5 * math.log(2 * math.pi) - lx
    loss = -(ll + prior) / N
    (gr,) = torch.autograd.grad(loss, t)
    _, _, S, W = R.ll_closed(Z, y, p, noise, c)
    alpha = torch.cholesky_solve((y - c).unsqueeze(-1), L.detach()).squeeze(-1)
    mass = ([] if fixed else [0.5 * float(W.diagonal().abs().sum())]) + [float(alpha.abs().sum())] + [
        float(s) for k in R.NAMES for s in S[k].abs().sum(dim=(0, 1)).reshape(-1)]
    # the priors' own gradient terms join the mass: |(a - 1) / x| + b (Gamma), |.| of the LogNormal's
    ab = [(3.0, 6.0)] * 3 + [(6.0, 2.0)] * 3 + [(3.0, 3.0), (2.0, 0.15)]
    pm = ([] if fixed else [abs(float(torch.log(t[0])) + 4.0) / x[0] + 1.0 / x[0]]) + [0.0] + [
        abs(a - 1.0) / xv + bb for (a, bb), xv in zip(ab, x[o + 1:])]
    scale = (np.asarray(mass) + np.asarray(pm)) / N
    mass_v = float(0.5 * ((y - c) * alpha).abs().sum() + L.detach().diagonal().log().abs().sum()
                   + abs(float(prior))) / N
    ev, eg = abs(v - float(loss)) / mass_v, np.abs(g - gr.numpy()) / scale
    print("mll: value", ev, "gradient", eg.max())
    assert ev <= SUM_TOL and (eg <= SUM_TOL).all()


@pytest.mark.parametrize("nf", (1, 2))
def test_fit_lowers_the_loss_and_routes_agree(nf):
    from botorch_amd import SingleTaskMultiFidelityGP
    from botorch_amd.fit import ExactMarginalLogLikelihood, _layout, fit_gpytorch_mll
    _, _, _, Z, y, p, _, _ = _case(nf)
    kw = dict(data_fidelities=[0]) if nf == 1 else dict(iteration_fidelity=0, data_fidelities=[p["fc"][1]])
    final = {}
    for route in ("fused", "torch"):
        m = SingleTaskMultiFidelityGP(Z.to(DEV), y.unsqueeze(-1).to(DEV), **kw)
        m._route = route
        lay = _layout(m)
        start = lay.value_and_grad(lay.get())[0]
        fit_gpytorch_mll(ExactMarginalLogLikelihood(m.likelihood, m))
        final[route] = lay.value_and_grad(lay.get())[0]
        print("fit:", route, start, "->", final[route])
        assert final[route] < start
    assert abs(final["fused"] - final["torch"]) <= 100 * 2.2e-9 * max(1.0, abs(final["torch"]))


@pytest.mark.parametrize("nf", (1, 2))
def test_posterior_and_gradient(nf):
    m, lay, x, Z, y, p, noise, c = _case(nf)
    X = _queries(Z, p)
    Xd = X.to(DEV).requires_grad_(True)
    post = m.posterior(Xd)
    Xr = X.clone().requires_grad_(True)
    mean, cov = R.posterior(Z, y, p, noise, c, Xr)
    _, _, mass_m, mass_c = R.posterior_inverse(Z, y, p, noise, c, X)
    em = (post.mean.squeeze(-1).cpu() - mean).abs() / mass_m
    ec = (post.mvn.covariance_matrix.cpu() - cov).abs() / mass_c
    print("posterior: mean", float(em.max()), "cov", float(ec.max()))
    assert em.max() <= MEAN_TOL and ec.max() <= COV_TOL
    (dX,) = torch.autograd.grad(post.mean.sum() + post.mvn.covariance_matrix.sum(), Xd)
    (dXr,) = torch.autograd.grad(mean.sum() + cov.sum(), Xr)
    eg = (dX.cpu() - dXr).abs().max() / dXr.abs().max()
    print("posterior: dX", float(eg))
    assert eg <= GRAD_TOL
    assert (dXr[..., p["fc"]] != 0).any() and (dX.cpu()[1, 1, p["fc"]] == 0).all()   # (s = 1.3: clamped)
    noisy = m.posterior(X.to(DEV), observation_noise=True).mvn.covariance_matrix
    assert torch.allclose((noisy - post.mvn.covariance_matrix).detach().cpu(),
                          float(noise) * torch.eye(2, dtype=torch.float64).expand(3, 2, 2), atol=1e-15)


def _mfkg_reference(post, case, Xa, Xf, Zb, extras):
    """R.mfkg on the moments ``post`` gives: the fantasy observations at the candidates
    (with ``extras``: plus the pending point, then one trace observation of each at
    half the last fidelity), the fantasy points projected to fidelity 1, the cost of
    the candidates alone.  Returns (acq, mean-first variant, d acq.sum() / d [Xa, Xf])."""
    _, _, _, Z, y, p, noise, c = case
    fid, d = p["fc"][-1], Z.shape[1]
    Xar, Xfr = Xa.clone().requires_grad_(True), Xf.clone().requires_grad_(True)
    Xp = torch.stack([Xfr[..., i] if i not in p["fc"] else torch.ones_like(Xfr[..., i])
                      for i in range(d)], dim=-1)
    Xe = Xar
    if extras:
        Xe = torch.cat([Xar, torch.full((Xa.shape[0], 1, d), PEND, dtype=torch.float64)], dim=1)
        scale = torch.ones(d, dtype=torch.float64)
        scale[fid] = 0.5
        Xe = torch.cat([Xe, Xe * scale], dim=1)
    out = post(Z, y, p, noise, c, torch.cat([Xe, Xp], dim=1))
    cost = (0.2 + Xar[..., fid]).clamp_min(0.01).sum(-1)
    ref, early = R.mfkg(out[0], out[1], Zb, float(noise), Xe.shape[1], 0.1, cost)
    return ref.detach(), early.detach(), torch.cat(torch.autograd.grad(ref.sum(), [Xar, Xfr]), dim=1)


@pytest.mark.parametrize("extras", (False, True), ids=("plain", "pending+trace"))
@pytest.mark.parametrize("nf", (1, 2))
def test_mfkg_value_gradient_and_order(nf, extras):
    from botorch_amd import (AffineFidelityCostModel, InverseCostWeightedUtility,
                             expand_trace_observations, project_to_target_fidelity,
                             qMultiFidelityKnowledgeGradient)
    case = _case(nf)
    m, _, _, Z, y, p, noise, c = case
    fid = p["fc"][-1]
    target = {j: 1.0 for j in p["fc"]}
    kw = dict(X_pending=torch.full((1, Z.shape[1]), PEND, dtype=torch.float64, device=DEV),
              expand=lambda X: expand_trace_observations(X, fidelity_dims=[fid], num_trace_obs=1)) if extras else {}
    acq = qMultiFidelityKnowledgeGradient(
        m, num_fantasies=NFANT, current_value=torch.tensor(0.1, dtype=torch.float64, device=DEV),
        cost_aware_utility=InverseCostWeightedUtility(AffineFidelityCostModel({fid: 1.0}, fixed_cost=0.2)),
        project=lambda X: project_to_target_fidelity(X, target), **kw)
    Xa = _queries(Z, p)
    Xf = torch.rand(3, NFANT, Z.shape[1], dtype=torch.float64, generator=torch.Generator().manual_seed(21))
    Xd = torch.cat([Xa, Xf], dim=1).to(DEV).requires_grad_(True)
    val = acq(Xd)
    (dX,) = torch.autograd.grad(val.sum(), Xd)
    Zb = acq.sampler.base_samples_2d(6 if extras else 2, torch.device(DEV)).cpu()
    ref, early, dXr = _mfkg_reference(R.posterior, case, Xa, Xf, Zb, extras)
    ev = float((val.detach().cpu() - ref).abs().max() / ref.abs().max())
    ed = float((dX.cpu() - dXr).abs().max() / dXr.abs().max())
    print("mfkg: value", ev, "gradient", ed)
    assert ev <= KG_TOL and ed <= KG_GRAD_TOL
    assert (dX.cpu()[:, 2:, p["fc"]] == 0).all()            # projected: no gradient to the fantasies' fidelities
    assert (ref - early).abs().max() > 1e-3 * ref.abs().max()   # the order matters


def test_optimize_acqf_on_the_mfkg():
    from botorch_amd import (AffineFidelityCostModel, InverseCostWeightedUtility,
                             project_to_target_fidelity, qMultiFidelityKnowledgeGradient)
    from botorch_amd.optim import optimize_acqf
    m, lay, x, Z, y, p, noise, c = _case(1)
    d = Z.shape[1]
    acq = qMultiFidelityKnowledgeGradient(
        m, num_fantasies=NFANT, current_value=torch.tensor(0.1, dtype=torch.float64, device=DEV),
        cost_aware_utility=InverseCostWeightedUtility(AffineFidelityCostModel({0: 1.0}, fixed_cost=0.2)),
        project=lambda X: project_to_target_fidelity(X, {0: 1.0}))
    bounds = torch.stack([torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)]).to(DEV)
    torch.manual_seed(2)
    cand, val = optimize_acqf(acq, bounds, q=2, num_restarts=2, raw_samples=8, options={"maxiter": 10})
    assert cand.shape == (2, d) and torch.isfinite(val).all()
    assert (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
