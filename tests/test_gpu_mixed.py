"""MixedSingleTaskGP on the fused route (n = 70, d_c = 3, d_k = 2) against
tests/mixed_restatement.py.  Tolerances are 10 x the largest disagreement of two
references on these same cases, measured once on the CPU: posterior_explicit
(Cholesky) against posterior_inverse (linalg.inv) differ by 2.3e-16 of sum |summand|
in the mean, 2.9e-17 in the covariance, and by 1.8e-13 of max |dX| in the gradient;
ll_closed against ll_autograd by 9.6e-16 of sum |summand| (test_gpu_mixed_kernels)."""
import functools
import math

import numpy as np
import pytest
import torch
from scipy.optimize import minimize

from tests import mixed_restatement as R

pytestmark = pytest.mark.gpu
POST_TOL = 2.3e-15   # of sum |summand|: 10 x 2.3e-16
GRAD_TOL = 1.8e-12   # of max |dX|: 10 x 1.8e-13
SUM_TOL = 1e-14      # of sum |summand|: 10 x 9.6e-16
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(kind=1, fixed=False, dims=(3, 2)):
    from botorch_amd.models import MixedSingleTaskGP, RBFKernel
    Z, y, p, noise, c = R.make_case(kind, *dims, 70, fixed_noise=fixed)
    kw = {}
    if kind == 0:
        kw["cont_kernel_factory"] = lambda batch_shape, ard_num_dims, active_dims: RBFKernel(
            ard_num_dims=ard_num_dims, lengthscale_lower=1e-4)
    m = MixedSingleTaskGP(Z.to(DEV), y.unsqueeze(-1).to(DEV), p["cat"],
                          train_Yvar=noise.unsqueeze(-1).to(DEV) if fixed else None, **kw)
    from botorch_amd import fit
    lay = fit._layout(m)
    x = np.concatenate([[] if fixed else [float(noise)], [c], p["l1"], p["lam1"], p["l2"], p["lam2"],
                        [float(p["os"]), float(p["oc"]), float(p["op"])]])
    lay.set(x)
    return m, lay, x, Z, y, p, noise, c


@pytest.mark.parametrize("q", (1, 3, 17))
@pytest.mark.parametrize("kind,fixed", ((1, False), (0, True)))
def test_posterior_and_gradient(kind, fixed, q):
    m, lay, x, Z, y, p, noise, c = _case(kind, fixed)
    assert m.fused()
    X = R.make_queries(Z, p, 4, q)
    Xd = X.to(DEV).requires_grad_(True)
    post = m.posterior(Xd)
    Xr = X.clone().requires_grad_(True)
    mean, cov = R.posterior_explicit(Z, y, p, noise, c, Xr)
    _, _, mass_m, mass_c = R.posterior_inverse(Z, y, p, noise, c, X)
    em = (post.mean.squeeze(-1).cpu() - mean).abs() / mass_m
    ec = (post.mvn.covariance_matrix.cpu() - cov).abs() / mass_c
    print("posterior: mean", float(em.max()), "cov", float(ec.max()))
    assert em.max() <= POST_TOL and ec.max() <= POST_TOL
    w = torch.linspace(0.5, 1.5, q, dtype=torch.float64)
    (dX,) = torch.autograd.grad((post.mean.squeeze(-1) * w.to(DEV)).sum() + post.mvn.covariance_matrix.sum(), Xd)
    (dXr,) = torch.autograd.grad((mean * w).sum() + cov.sum(), Xr)
    assert (dX.cpu()[..., p["cat"]] == 0.0).all()
    eg = (dX.cpu()[..., p["cont"]] - dXr[..., p["cont"]]).abs().max() / dXr.abs().max()
    print("posterior: dX", float(eg))
    assert eg <= GRAD_TOL


@pytest.mark.parametrize("kind,fixed", ((1, False), (0, True)))
def test_mll_value_and_grad(kind, fixed):
    from botorch_amd import fit
    m, lay, x, Z, y, p, noise, c = _case(kind, fixed)
    v, g = fit.mixed_mll_value_and_grad(m, x, lay)
    ll, gr, S, _ = R.ll_closed(Z, y, p, noise, c)
    n = 70
    ref = [] if fixed else [float(gr["noise"]) + (0.9 - 1) / x[0] - 10.0]
    ref += [float(gr["const"])] + [float(t) for k in R.NAMES for t in gr[k].reshape(-1)]
    prior = 0.0 if fixed else 0.9 * np.log(10.0) + (0.9 - 1) * np.log(x[0]) - 10.0 * x[0] - math.lgamma(0.9)
    _, _, _, W = R.ll_closed(Z, y, p, noise, c)
    Lr = torch.linalg.cholesky(R.kernel(Z, Z, p) + R._noise_matrix(noise, n))
    alpha = torch.cholesky_solve((y - c).unsqueeze(-1), Lr).squeeze(-1)
    mass_v = float(0.5 * ((y - c) * alpha).abs().sum() + Lr.diagonal().log().abs().sum()) + abs(prior)
    mass = [] if fixed else [0.5 * float(W.diagonal().abs().sum()) + abs((0.9 - 1) / x[0]) + 10.0]
    mass += [float(alpha.abs().sum())] + [float(t) for k in R.NAMES
                                          for t in S[k].abs().sum(dim=(0, 1)).reshape(-1)]
    scale = np.asarray(mass) / n
    ev, eg = abs(v + (float(ll) + prior) / n) / (mass_v / n), np.abs(g + np.asarray(ref) / n) / scale
    print("mll: value", ev, "gradient", eg.max())
    assert ev <= SUM_TOL and (eg <= SUM_TOL).all()
    m._route = "torch"
    try:
        vt, gt = fit.mixed_mll_value_and_grad(m, x, lay)
    finally:
        m._route = None
    assert abs(v - vt) <= SUM_TOL * mass_v / n and (np.abs(g - gt) <= SUM_TOL * scale).all()


def test_fit_reaches_scipy_optimum():
    """Loss at the fit minus scipy L-BFGS-B's on neg_mll_flat from the same start: <= 100 ftol."""
    from botorch_amd.fit import (ExactMarginalLogLikelihood, _layout, fit_gpytorch_mll,
                                 fit_gpytorch_mll_scipy)
    from botorch_amd.models import MixedSingleTaskGP
    Z, y, p, _, _ = R.make_case(1, 3, 2, 70)
    m = MixedSingleTaskGP(Z.to(DEV), y.unsqueeze(-1).to(DEV), p["cat"])
    lay = _layout(m)
    x0 = lay.get()
    f = lambda x: R.neg_mll_flat(x, Z, y, 1, p["cont"], p["cat"])  # noqa: E731
    res = minimize(f, x0, jac=True, method="L-BFGS-B", bounds=lay.bounds)
    stops = [str(res.message)]

    def optimizer(mll, **kw):
        out = fit_gpytorch_mll_scipy(mll, **kw)
        stops.append(out.message)
        return out

    fit_gpytorch_mll(ExactMarginalLogLikelihood(m.likelihood, m), optimizer=optimizer, max_attempts=1)
    assert len(stops) == 2 and all("REDUCTION OF F" in s.upper().replace("_", " ") for s in stops), stops
    ours = f(lay.get())[0]
    print("fit: ours", ours, "scipy", res.fun, "difference", ours - res.fun)
    assert ours - res.fun <= 100 * 2.2e-9 * max(1.0, abs(res.fun))


@pytest.mark.parametrize("name", ("qLogNoisyExpectedImprovement", "LogExpectedImprovement"))
def test_acquisition_fused_equals_torch_route(name):
    from botorch_amd import acquisition as A
    m, lay, x, Z, y, p, noise, c = _case()
    q = 1 if name == "LogExpectedImprovement" else 3
    # distinct points (at a repeated one the joint covariance is singular and the Cholesky's
    # derivative unbounded); best_f at the median of y, so that EI is not tiny
    g = torch.Generator().manual_seed(3)
    X = torch.rand(5, q, Z.shape[1], dtype=torch.float64, generator=g)
    X[..., p["cat"]] = torch.randint(0, 3, (5, q, 2), generator=g).to(torch.float64) * 0.5 + 0.25
    X = X.to(DEV)
    out = []
    for route in ("fused", "torch"):
        m._route = route
        try:
            torch.manual_seed(0)
            acq = (A.LogExpectedImprovement(m, best_f=float(y.median())) if q == 1 else
                   A.qLogNoisyExpectedImprovement(m, Z[:20].to(DEV)))
            Xr = X.clone().requires_grad_(True)
            val = acq(Xr)
            (dX,) = torch.autograd.grad(val.sum(), Xr)
            out.append((val.detach(), dX))
        finally:
            m._route = None
    (v0, d0), (v1, d1) = out
    ev = float((v0 - v1).abs().max() / v1.abs().max().clamp_min(1.0))
    ed = float((d0 - d1).abs().max() / d1.abs().max())
    print("acquisition:", name, "value", ev, "dX", ed)
    assert ev <= GRAD_TOL and ed <= GRAD_TOL   # the posterior's (gradient) tolerance
    assert (d0[..., p["cat"]] == 0).all()


def test_optimize_acqf_mixed_on_the_model():
    from botorch_amd import acquisition as A
    from botorch_amd.optim import optimize_acqf_mixed
    m, lay, x, Z, y, p, noise, c = _case()
    d = Z.shape[1]
    bounds = torch.stack([torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)]).to(DEV)
    bounds[1, p["cat"]] = 1.25
    ffl = [{p["cat"][0]: a, p["cat"][1]: b} for a in (0.25, 0.75) for b in (0.25, 1.25)]
    torch.manual_seed(1)
    acq = A.qLogExpectedImprovement(m, best_f=float(y.max()))
    cand, val = optimize_acqf_mixed(acq, bounds, 2, 2, ffl, raw_samples=16, options={"maxiter": 20})
    assert cand.shape == (2, d) and acq.X_pending is None
    for row in cand.cpu():
        assert {p["cat"][0]: float(row[p["cat"][0]]), p["cat"][1]: float(row[p["cat"][1]])} in ffl
    assert (cand >= bounds[0]).all() and (cand <= bounds[1]).all()
    with torch.no_grad():
        assert torch.allclose(val, acq(cand), rtol=0, atol=0)


def test_beyond_the_fused_limits_takes_the_torch_route():
    m, lay, x, Z, y, p, noise, c = _case(1, False, (9, 2))
    assert not m.fused()
    X = R.make_queries(Z, p, 2, 3)
    mean, cov = R.posterior_explicit(Z, y, p, noise, c, X)
    post = m.posterior(X.to(DEV))
    _, _, mass_m, mass_c = R.posterior_inverse(Z, y, p, noise, c, X)
    assert ((post.mean.squeeze(-1).cpu() - mean).abs() <= POST_TOL * mass_m).all()
    assert ((post.mvn.covariance_matrix.cpu() - cov).abs() <= POST_TOL * mass_c).all()
