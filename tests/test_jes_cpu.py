"""qJointEntropySearch without a GPU: the ABI record and symbols, the ABI's
refusals, the rank-one identities of the restatement (tests/jes_restatement.py)
against an explicit dense solve on the n + 1 points, a known answer, and every
constructor error with the native library made to raise."""
import ctypes
import math

import pytest
import torch

from tests import jes_restatement as jr

F64 = torch.float64


def test_jes_record_and_symbols():
    from botorch_amd import _lib, ops
    lib = _lib.lib()
    assert "BoJesArgs" in _lib.ARG_RECORDS
    assert lib.bo_struct_size(b"BoJesArgs") == ctypes.sizeof(_lib.JesArgs)
    for sym in ("bo_jes_v", "bo_jes_backward_v"):
        assert sym in _lib.exported_symbols()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert "jes" in ops.OPS and "jes_backward" in ops.OPS
    assert lib.bo_version() == _lib.ABI_VERSION == 12  # a pure addition


def test_jes_abi_refusals():
    """Header discipline and argument errors, refused before any launch."""
    from botorch_amd import _lib
    lib = _lib.lib()
    a = _lib.JesArgs(kind=0, d=3, P=1, R=1)
    a.abi_version = _lib.ABI_VERSION + 1
    assert lib.bo_jes_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    dummy = torch.zeros(16, dtype=F64)
    ok = dict(kind=0, d=3, P=1, R=1, n=0, X=dummy, lengthscale=dummy, Xopt_scaled=dummy, g=dummy,
              sinv=dummy, wf=dummy, tau2=dummy, mu=dummy, var=dummy, outputscale=1.0, w=1.0,
              out=dummy, dout=dummy, dX=dummy, dmu=dummy, dvar=dummy)
    bads = [(dict(d=129), "d <= 128"), (dict(d=0), "d <= 128"), (dict(P=0), "P >= 1"),
            (dict(R=0), "R >= 1"), (dict(kind=2), "kernel kind"), (dict(n=2), "Xt_scaled and V"),
            (dict(w=0.5), "+1 or -1")]
    bads += [({name: None}, "required") for name in
             ("X", "lengthscale", "Xopt_scaled", "g", "sinv", "wf", "tau2", "mu", "var")]
    for bad, text in bads:
        for fn in (lib.bo_jes_v, lib.bo_jes_backward_v):
            assert fn(ctypes.byref(_lib.JesArgs(**{**ok, **bad})), None) == _lib.BO_ERR_ARG, bad
            assert text in lib.bo_last_error().decode(), (bad, lib.bo_last_error())
    assert lib.bo_jes_v(ctypes.byref(_lib.JesArgs(**{**ok, "out": None})), None) == _lib.BO_ERR_ARG
    for name in ("dout", "dX", "dmu", "dvar"):
        assert lib.bo_jes_backward_v(ctypes.byref(_lib.JesArgs(**{**ok, name: None})),
                                     None) == _lib.BO_ERR_ARG


def test_jes_op_fake_shapes():
    meta = dict(device="meta", dtype=F64)
    R, d, P, n = 37, 5, 7, 11
    e = lambda *s: torch.empty(*s, **meta)  # noqa: E731
    args = (e(R, d), e(R), e(R), e(d), e(n, d), e(P, d), e(P, n), e(P), e(P), e(P), e(P), 0, 1.0,
            1.0)
    assert torch.ops.bo.jes(*args).shape == (R,)
    dX, dmu, dvar = torch.ops.bo.jes_backward(e(R), *args)
    assert dX.shape == (R, d) and dmu.shape == (R,) and dvar.shape == (R,)


def _problem(case, n=20, d=3, P=5, q=3, seed=11):
    g = torch.Generator().manual_seed(seed)
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    y = torch.randn(n, generator=g, dtype=F64)
    ls = 0.3 + 0.4 * torch.rand(d, generator=g, dtype=F64)
    noise = 1e-2 * (1.0 + torch.rand(n, generator=g, dtype=F64)) if case == "fixed" else 1e-2
    kind = jr.MATERN52 if case == "matern" else jr.RBF
    gp = jr.make_gp(Xt, y, ls, noise, const=0.2, kind=kind, o=1.3)
    Xo = torch.rand(P, d, generator=g, dtype=F64)
    X = torch.rand(q, d, generator=g, dtype=F64)
    f = jr.posterior(gp, Xo)[0] + 1.0 + torch.rand(P, generator=g, dtype=F64)
    return gp, jr.make_optima(gp, Xo, f, condition_noiseless=True), X


@pytest.mark.parametrize("case", ["homoskedastic", "fixed", "matern"])
def test_rank_one_moments_equal_dense_refit(case):
    """mu_ji, s2_ji and tau2_j of the rank-one form against the GP refitted on
    the n + 1 points with noise diag(s2, ..., s2, nu_j): 1e-10."""
    gp, opt, X = _problem(case)
    n = gp.Xt.shape[0]
    mu, Sigma = jr.posterior(gp, X)
    c = jr.cross_cov(gp, opt, X)
    mu_j, s2_j = jr.rank_one_moments(c, mu, Sigma.diagonal(), opt)
    worst = 0.0
    for j in range(opt.Xo.shape[0]):
        m_ref, v_ref = jr.explicit_conditioned(gp, opt, j, X)
        worst = max(worst, (mu_j[:, j] - m_ref).abs().max().item(),
                    (s2_j[:, j] - v_ref).abs().max().item())
        # the conditioned model's observation noise by the project's rule
        noise_j = torch.cat([gp.noise, opt.nu[j:j + 1]])
        want = noise_j.mean() if gp.fixed else gp.noise[0]
        assert abs(opt.tau2[j].item() - want.item()) <= 1e-15
    print("rank-one vs dense refit, max abs error:", worst)
    assert worst <= 1e-10
    assert (c.abs() > 1e-3).any()  # the optima do move the posterior
    if gp.fixed:
        assert abs(opt.tau2[0].item() - (n * gp.tau2.item() + 1e-4) / (n + 1)) <= 1e-15


def test_known_answer_far_optimum():
    """P = 1 and f* so far above the posterior that z > 30: the truncation
    vanishes and acq = logdet(A) / 2 - sum_i log(Sigma_ii - c_i^2 / s + tau2) / 2."""
    gp, _, X = _problem("homoskedastic", P=1)
    Xo = torch.full((1, 3), 0.4, dtype=F64)
    opt = jr.make_optima(gp, Xo, torch.tensor([500.0], dtype=F64))
    mu, Sigma = jr.posterior(gp, X)
    ch = jr.conditional_entropy(gp, opt, X, mu, Sigma.diagonal())
    assert (ch.z > 30).all()
    c = jr.cross_cov(gp, opt, X)[:, 0]
    A = Sigma + gp.tau2 * torch.eye(X.shape[0], dtype=F64)
    want = 0.5 * torch.logdet(A) - (0.5 * torch.log(Sigma.diagonal() - c * c / opt.s[0]
                                                    + gp.tau2)).sum()
    got = jr.jes_lower_bound(gp, opt, X)
    assert abs(got.item() - want.item()) <= 1e-12, (got.item(), want.item())


def test_chain_matches_package_formula():
    """The package's torch chain (the generic route's) is the restatement's."""
    from botorch_amd.acquisition import _jes_chain
    gp, opt, X = _problem("matern")
    mu, Sigma = jr.posterior(gp, X)
    c = jr.cross_cov(gp, opt, X)
    for w in (1.0, -1.0):
        ref = jr.chain(c, mu, Sigma.diagonal(), opt.g, 1.0 / opt.s, w * opt.f, opt.tau2, w).H
        got = _jes_chain(c, mu, Sigma.diagonal(), opt.g, 1.0 / opt.s, w * opt.f, opt.tau2, w)
        assert torch.equal(got, ref)


@pytest.fixture
def no_native(monkeypatch):
    """Any use of the native library fails the test."""
    from botorch_amd import _lib, kernels

    def boom(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(kernels, "lib", boom)


def _model(n=6, d=2, m=1, fixed=False):
    from botorch_amd.models import SingleTaskGP
    g = torch.Generator().manual_seed(0)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = torch.stack([(X.sum(-1) + t).sin() for t in range(m)], dim=-1)
    return SingleTaskGP(X, Y, torch.full_like(Y, 1e-3) if fixed else None)


def test_constructor_errors_before_native(no_native):
    from botorch_amd.acquisition import qJointEntropySearch
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import ModelListGP, SaasFullyBayesianSingleTaskGP
    from botorch_amd.objective import ScalarizedPosteriorTransform
    Xo, fo = torch.rand(4, 2, dtype=F64), torch.rand(4, 1, dtype=F64)
    g = torch.Generator().manual_seed(1)
    X = torch.rand(6, 2, generator=g, dtype=F64)
    saas = SaasFullyBayesianSingleTaskGP(X, X.sum(-1, keepdim=True))
    with pytest.raises(NotImplementedError, match="JES is not yet available with Fully Bayesian"):
        qJointEntropySearch(saas, Xo, fo)
    with pytest.raises(UnsupportedError, match="multi-output"):
        qJointEntropySearch(_model(m=2).eval(), Xo, fo)
    with pytest.raises(UnsupportedError, match="ModelListGP"):
        qJointEntropySearch(ModelListGP(_model().eval(), _model().eval()), Xo, fo)
    model = _model()
    assert model.training
    with pytest.raises(UnsupportedError, match="eval mode"):
        qJointEntropySearch(model, Xo, fo)
    model.eval()
    pt = ScalarizedPosteriorTransform(torch.tensor([1.0], dtype=F64))
    with pytest.raises(UnsupportedError, match="posterior_transform"):
        qJointEntropySearch(model, Xo, fo, posterior_transform=pt)
    with pytest.raises(UnsupportedError, match="not on the accelerated path"):
        qJointEntropySearch(model, Xo, fo, estimation_type="MC")
    with pytest.raises(ValueError, match=r"Estimation type XX is not valid. Please specify any of "
                                         r"\['MC', 'LB'\]"):
        qJointEntropySearch(model, Xo, fo, estimation_type="XX")
    with pytest.raises(ValueError, match="optimal_inputs"):
        qJointEntropySearch(model, torch.rand(4, 3, dtype=F64), fo)
    with pytest.raises(ValueError, match="optimal_outputs"):
        qJointEntropySearch(model, Xo, fo.squeeze(-1))
    with pytest.raises(RuntimeError, match="requires a `noise` kwarg"):
        qJointEntropySearch(_model(fixed=True).eval(), Xo, fo, condition_noiseless=False)


def test_kernel_wrapper_checks_before_native(no_native):
    from botorch_amd import kernels
    with pytest.raises(ValueError, match="d <= 128"):
        kernels.jes_check(129, 1)
    with pytest.raises(ValueError, match="P >= 1"):
        kernels.jes_check(3, 0)
    with pytest.raises(ValueError, match="R >= 1"):
        kernels.jes_check(3, 1, 0)
    kernels.jes_check(128, 1, 1)
    assert math.isclose(kernels.JES_DMAX, 128)
