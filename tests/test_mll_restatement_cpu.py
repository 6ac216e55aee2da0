"""The two host formulations of the exact MLL in mll_restatement.py (Cholesky +
autograd; explicit inverse + closed-form gradient) agree over the case grid the
device tests draw from, to one hundredth of the tolerances the device tests
use (value 1e-9 max(1, |v|); gradient rtol 1e-6, atol 1e-9).  That margin is
what the kernel's own summation order has to fit into."""
import numpy as np
import pytest
import torch

from tests import mll_restatement as R

VALUE_TOL = 1e-9 / 100
GRAD_RTOL, GRAD_ATOL = 1e-6 / 100, 1e-9 / 100


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("d", R.DIMS)
@pytest.mark.parametrize("kind", R.KINDS, ids=["rbf", "matern"])
def test_formulations_agree(kind, d, n):
    for vector_noise in (False, True):
        X, y, ls, noise = R.make_case(d, n, vector_noise)
        assert len(set(ls.tolist())) == d
        for o in R.OUTPUTSCALES:
            va, ga = R.ll_autograd(X, y, ls, noise, R.CONSTANT, o, kind)
            vc, gc = R.ll_closed(X, y, ls, noise, R.CONSTANT, o, kind)
            assert ga.shape == gc.shape == (d + 3,)
            assert np.isfinite(va) and np.isfinite(ga).all()
            assert abs(va - vc) < VALUE_TOL * max(1.0, abs(vc))
            np.testing.assert_allclose(ga, gc, rtol=GRAD_RTOL, atol=GRAD_ATOL)


def test_gradient_is_not_degenerate():
    """Every gradient entry of the grid's inputs is well above the absolute
    tolerance, and distinct per dimension: a swapped, dropped or mis-scaled
    entry cannot hide under atol."""
    for kind in R.KINDS:
        X, y, ls, noise = R.make_case(9, 65, False)
        _, g = R.ll_autograd(X, y, ls, noise, R.CONSTANT, 1.7, kind)
        assert (np.abs(g) > 1e-4).all()
        assert len(set(np.round(g[2:-1], 6))) == 9


def test_neg_mll_flat_layouts():
    """neg_mll_flat is -(ll + priors) / n of the same data term in each of the
    fit's layouts, and its gradient picks the matching entries."""
    X, y, ls, nv = R.make_case(3, 65, True)
    n, c, o = 65, R.CONSTANT, 1.7
    lp, npr = (0.9, 1.1), (-4.0, 1.0)
    pl = R.lognormal_log_prob(ls, *lp)
    dpl = (-(ls.log() - lp[0]) / lp[1] ** 2 - 1.0) / ls
    # learned noise, outputscale, both priors
    x = np.concatenate([[2e-2, c], ls.numpy(), [o]])
    v, g = R.neg_mll_flat(x, X, y, R.MATERN52, ls_prior=lp, noise_prior=npr)
    ll, gl = R.ll_closed(X, y, ls, 2e-2, c, o, R.MATERN52)
    pn = R.lognormal_log_prob(torch.tensor(2e-2, dtype=R.F64), *npr).item()
    dpn = (-(np.log(2e-2) - npr[0]) / npr[1] ** 2 - 1.0) / 2e-2
    assert abs(v + (ll + pl.sum().item() + pn) / n) < 1e-12 * max(1.0, abs(v))
    ref = gl.copy()
    ref[0] += dpn
    ref[2:-1] += dpl.numpy()
    np.testing.assert_allclose(g, -ref / n, rtol=1e-8, atol=1e-11)
    # fixed noise (a noise prior must be ignored), no outputscale, no lengthscale prior
    x = np.concatenate([[c], ls.numpy()])
    v, g = R.neg_mll_flat(x, X, y, R.RBF, noise_vec=nv, has_os=False, noise_prior=npr)
    ll, gl = R.ll_closed(X, y, ls, nv, c, 1.0, R.RBF)
    assert abs(v + ll / n) < 1e-12 * max(1.0, abs(v))
    np.testing.assert_allclose(g, -gl[1:-1] / n, rtol=1e-8, atol=1e-11)
