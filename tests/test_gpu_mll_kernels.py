"""bo_mll_terms (mll.hip) through fit.mll_terms, and both routes of
fit.mll_value_and_grad, against the host restatement of the exact MLL
(tests/mll_restatement.py): Matern-5/2 and RBF, with and without an
outputscale, scalar and fixed noise, the d = 6 and d = 8 template instances and
the runtime-d instance from d = 1 to its limit d = 64, n from one row to rows
whose pair loop takes a second trip.

Tolerances are the ones the suite already uses for the MLL (value
1e-9 max(1, |v|); gradient rtol 1e-6, atol 1e-9); test_mll_restatement_cpu.py
shows that two independent host formulations agree a hundred times closer on
the same inputs."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import mll_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
KIND_NAME = {R.RBF: "rbf", R.MATERN52: "matern"}


def _grid():
    cases = []
    for kind in R.KINDS:
        # every width: d = 6 / 8 template instances, the runtime-d instance at 1,
        # just above a specialisation (7, 9), the SAAS width 50 and the limit 64
        cases += [(kind, d, 65, 1.7, False) for d in R.DIMS]
        # noise form x outputscale at a template and at a runtime-d width
        cases += [(kind, d, 65, o, vec) for d in (6, 9) for o in R.OUTPUTSCALES
                  for vec in (False, True)]
        # one lane, two lanes, a second wavefront, a second k-loop trip (i >= 256)
        cases += [(kind, d, n, 1.7, False) for d in (6, 64) for n in R.SIZES]
        # fixed noise where every slot is in use and the k-loop wraps
        cases += [(kind, 64, 300, 1.0, True), (kind, 50, 257, 1.7, True)]
    return sorted(set(cases))


def _case_id(case):
    kind, d, n, o, vec = case
    return f"{KIND_NAME[kind]}-d{d}-n{n}-o{o}-{'fixed' if vec else 'scalar'}"


@functools.lru_cache(maxsize=None)
def _reference(kind, d, n, o, vec):
    X, y, ls, noise = R.make_case(d, n, vec)
    return R.ll_autograd(X, y, ls, noise, R.CONSTANT, o, kind)


def _assert_close(val, grad, ref_val, ref_grad):
    print(f"value {val!r} ref {ref_val!r}  |dv| {abs(val - ref_val):.3e}  max |dg| "
          f"{np.max(np.abs(grad - ref_grad)):.3e}  max rel "
          f"{np.max(np.abs(grad - ref_grad) / (1e-9 + 1e-6 * np.abs(ref_grad))):.3e} of tol")
    assert math.isfinite(val) and np.isfinite(grad).all()
    assert abs(val - ref_val) < 1e-9 * max(1.0, abs(ref_val))
    np.testing.assert_allclose(grad, ref_grad, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("case", _grid(), ids=_case_id)
def test_mll_terms_match_restatement(case):
    """(ll, d ll / d [noise, constant, ls_1..d, outputscale]) of fit.mll_terms
    against the Cholesky + autograd restatement.  n >= 65 holds a coincident
    pair of rows (r = 0 off the diagonal: the Matern branch must stay finite
    and contribute a zero lengthscale gradient).  With fixed noise the first
    gradient entry is documented as meaningless and left out."""
    from botorch_amd.fit import mll_terms
    kind, d, n, o, vec = case
    X, y, ls, noise = R.make_case(d, n, vec)
    noise_d = noise.to(DEV) if vec else noise
    val, grad = mll_terms(X.to(DEV), y.to(DEV), ls, noise_d, R.CONSTANT, o, kind)
    ref_val, ref_grad = _reference(*case)
    assert grad.shape == (d + 3,)
    lo = 1 if vec else 0
    _assert_close(val, grad[lo:], ref_val, ref_grad[lo:])


@pytest.mark.parametrize("kind", R.KINDS, ids=["rbf", "matern"])
def test_d_above_limit_is_refused(kind):
    """d = 65 is an argument error on the host (nothing is launched with it)."""
    from botorch_amd.fit import mll_terms
    X, y, ls, noise = R.make_case(65, 8, False)
    with pytest.raises(ValueError) as err:
        mll_terms(X.to(DEV), y.to(DEV), ls, noise, R.CONSTANT, 1.0, kind)
    if "bo_mll_terms" in str(err.value):
        assert "64" in str(err.value)


# ---- fit.mll_value_and_grad: the public op route and the fit's direct route -------------------
NOISE_PRIOR = (-4.0, 1.0)                      # LogNormal(-4, 1)


def _dim_scaled_prior(d):
    return (math.sqrt(2.0) + 0.5 * math.log(d), math.sqrt(3.0))


def _model_data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=torch.float64)
    Y = (torch.sin(3 * X[:, 0]) + X[:, 1] ** 2 - 0.5 * X[:, 2]
         + 0.05 * torch.randn(n, generator=g, dtype=torch.float64)).unsqueeze(-1)
    Yvar = 1e-3 + 0.02 * torch.rand(n, 1, generator=g, dtype=torch.float64)
    return X, Y, Yvar


def _standardize(Y, Yvar=None):
    sd = Y.std(dim=0, keepdim=True)
    y = ((Y - Y.mean(dim=0, keepdim=True)) / sd).squeeze(-1)
    return y, (None if Yvar is None else (Yvar / sd ** 2).squeeze(-1))


def _configs():
    from botorch_amd.models import (MaternKernel, ScaleKernel,
                                    get_covar_module_with_dim_scaled_prior)
    # name -> (covariance module, fixed noise, restatement keywords, flat vector)
    return {
        "scale_matern": (lambda: ScaleKernel(MaternKernel(ard_num_dims=3)), False,
                         dict(kind=R.MATERN52, has_os=True, ls_prior=None, noise_prior=NOISE_PRIOR),
                         [0.02, 0.3, 0.4, 0.55, 0.7, 1.7]),
        "scale_rbf_yvar": (lambda: ScaleKernel(get_covar_module_with_dim_scaled_prior(3)), True,
                           dict(kind=R.RBF, has_os=True, ls_prior=_dim_scaled_prior(3),
                                noise_prior=NOISE_PRIOR),  # ignored: the noise is fixed
                           [0.3, 0.4, 0.55, 0.7, 1.7]),
        "bare_matern": (lambda: MaternKernel(ard_num_dims=3), False,
                        dict(kind=R.MATERN52, has_os=False, ls_prior=None, noise_prior=NOISE_PRIOR),
                        [0.02, 0.3, 0.4, 0.55, 0.7]),
    }


@pytest.mark.parametrize("name", ["scale_matern", "scale_rbf_yvar", "bare_matern"])
def test_op_route_and_direct_route_agree(name):
    """torch.ops.bo.mll (sync_model=True) and the fit's direct fit.mll_terms
    call (sync_model=False) run the same kernels in the same order: bit-equal
    loss and gradient, both equal to the restated -(ll + priors) / n of the
    standardised targets in the layout's order."""
    from botorch_amd.fit import _Layout, mll_value_and_grad
    from botorch_amd.models import RBFKernel, SingleTaskGP
    make_covar, fixed, kw, x = _configs()[name]
    X, Y, Yvar = _model_data(65, 3, seed=5)
    m = SingleTaskGP(X.to(DEV), Y.to(DEV), Yvar.to(DEV) if fixed else None,
                     covar_module=make_covar())
    lay = _Layout(m)
    assert lay.has_os == kw["has_os"] and lay.fixed == fixed
    if name == "scale_rbf_yvar":
        assert isinstance(lay.base, RBFKernel) and lay.base.lengthscale_prior is not None
    else:
        assert lay.base.lengthscale_prior is None
    x = np.asarray(x)
    assert lay.size == len(x)
    v_op, g_op = mll_value_and_grad(m, x, lay)
    v_direct, g_direct = mll_value_and_grad(m, x, lay, sync_model=False)
    assert v_op == v_direct
    np.testing.assert_array_equal(g_op, g_direct)
    y, nv = _standardize(Y, Yvar if fixed else None)
    ref_v, ref_g = R.neg_mll_flat(x, X, y, noise_vec=nv, **kw)
    _assert_close(v_op, g_op, ref_v, ref_g)


def fit_problem():
    """The end-to-end fit's data: n = 96, d = 3, smooth plus 0.05 noise.  The
    signal's amplitude (0.3) keeps the standardised noise near 0.06, where the
    optimum is well determined: on the host, L-BFGS-B over the restated loss
    ends after 22 iterations at noise 0.060, lengthscales (0.33, 0.55, 1.09),
    outputscale 1.72, every parameter off its bound, with a largest gradient
    entry of 9e-6; relative gradient perturbations of 1e-8 move its final loss
    by 3e-12 relative.  (With an O(1) signal the noise entry, near 2e-3, is so
    stiff that the same optimiser stops anywhere within 1e-2 of stationarity,
    whatever computes the gradient.)"""
    g = torch.Generator().manual_seed(11)
    X = torch.rand(96, 3, generator=g, dtype=torch.float64)
    Y = 0.3 * (torch.sin(6 * X[:, 0]) * torch.cos(4 * X[:, 1]) + X[:, 2] ** 2) \
        + 0.05 * torch.randn(96, generator=g, dtype=torch.float64)
    return X, Y.unsqueeze(-1)


def test_scale_matern_fit_reaches_restated_optimum():
    """fit_gpytorch_mll of a ScaleKernel(MaternKernel) model against scipy's
    L-BFGS-B over the restated loss from the same start and bounds: the fit's
    optimum is no worse than the reference's and stationary in the restated
    gradient off the bounds.  (No parameter equality: the outputscale /
    lengthscale ridge of a Matern fit is flat.)"""
    from scipy.optimize import minimize

    from botorch_amd.fit import ExactMarginalLogLikelihood, _Layout, fit_gpytorch_mll
    from botorch_amd.models import MaternKernel, ScaleKernel, SingleTaskGP
    X, Y = fit_problem()
    m = SingleTaskGP(X.to(DEV), Y.to(DEV), covar_module=ScaleKernel(MaternKernel(ard_num_dims=3)))
    lay = _Layout(m)
    x0 = lay.get()
    fit_gpytorch_mll(ExactMarginalLogLikelihood(m.likelihood, m))
    x1 = lay.get()
    y, _ = _standardize(Y)

    def f(x):
        return R.neg_mll_flat(x, X, y, R.MATERN52, has_os=True, noise_prior=NOISE_PRIOR)

    ref = minimize(f, x0, jac=True, method="L-BFGS-B", bounds=lay.bounds)
    v1, g1 = f(x1)
    lower = np.array([-np.inf if b[0] is None else b[0] for b in lay.bounds])
    free = x1 > lower + 1e-10
    print(f"x1 {x1}  f(x1) {v1!r}  ref.x {ref.x}  ref.fun {ref.fun!r}  |g1| free "
          f"{np.abs(g1[free]).max():.3e}")
    assert v1 <= ref.fun + 1e-6 * abs(ref.fun)
    assert np.all(np.abs(g1[free]) < 1e-3)
