"""Max-value entropy search without a GPU: the three ABI records and five
symbols, the ABI's refusals, the restatement (tests/mes_restatement.py) against
closed forms, the quantile restatement against brentq on the reference's own
objective, and every constructor error with the native library made to raise."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import mes_restatement as mr

F64 = torch.float64
SYMBOLS = ("bo_mes_v", "bo_mes_backward_v", "bo_gibbon_v", "bo_gibbon_backward_v",
           "bo_mv_quantiles_v")


def test_mes_records_and_symbols():
    from botorch_amd import _lib, ops
    lib = _lib.lib()
    for cname, rec in (("BoMesArgs", _lib.MesArgs), ("BoGibbonArgs", _lib.GibbonArgs),
                       ("BoMvQuantilesArgs", _lib.MvQuantilesArgs)):
        assert _lib.ARG_RECORDS[cname] is rec
        assert lib.bo_struct_size(cname.encode()) == ctypes.sizeof(rec)
    for sym in SYMBOLS:
        assert sym in _lib.exported_symbols()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    for op in ("mes", "mes_backward", "gibbon", "gibbon_backward", "mv_quantiles"):
        assert op in ops.OPS
    assert lib.bo_version() == _lib.ABI_VERSION == 12  # a pure addition


def test_mes_abi_refusals():
    """Header discipline and argument errors, refused before any launch."""
    from botorch_amd import _lib
    lib = _lib.lib()
    d = torch.zeros(16, dtype=F64)
    for fn, rec in ((lib.bo_mes_v, _lib.MesArgs), (lib.bo_gibbon_v, _lib.GibbonArgs),
                    (lib.bo_mv_quantiles_v, _lib.MvQuantilesArgs)):
        a = rec()
        a.abi_version = _lib.ABI_VERSION + 1
        assert fn(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    ok = dict(S_M=3, S_m=4, R=2, mu=d, var=d, fstar=d, z=d, kappa=0.1, var_h0=0.5, zsq_mean=1.0,
              tau2=0.1, w=1.0, out=d, dout=d, dmu=d, dvar=d)
    bads = [(dict(S_m=1), "2 <= S_m"), (dict(S_m=4097), "2 <= S_m"), (dict(S_M=0), "1 <= S_M"),
            (dict(S_M=1025), "1 <= S_M"), (dict(R=0), "1 <= R"), (dict(w=0.5), "+1 or -1"),
            (dict(var_h0=0.0), "var_h0 > 0"), (dict(tau2=-1.0), "tau2 >= 0")]
    bads += [({name: None}, "required") for name in ("mu", "var", "fstar", "z")]
    for bad, text in bads:
        for fn in (lib.bo_mes_v, lib.bo_mes_backward_v):
            assert fn(ctypes.byref(_lib.MesArgs(**{**ok, **bad})), None) == _lib.BO_ERR_ARG, bad
            assert text in lib.bo_last_error().decode(), (bad, lib.bo_last_error())
    assert lib.bo_mes_v(ctypes.byref(_lib.MesArgs(**{**ok, "out": None})), None) == _lib.BO_ERR_ARG
    for name in ("dout", "dmu", "dvar"):
        assert lib.bo_mes_backward_v(ctypes.byref(_lib.MesArgs(**{**ok, name: None})),
                                     None) == _lib.BO_ERR_ARG
    ok = dict(S_M=3, m=2, R=2, mu=d, var=d, A=d, Binv=d, fstar=d, tau2=0.1, w=1.0, out=d, dout=d,
              dmu=d, dvar=d, dA=d)
    bads = [(dict(m=16), "m <= 15"), (dict(m=-1), "m <= 15"), (dict(S_M=0), "S_M >= 1"),
            (dict(R=0), "1 <= R"), (dict(w=2.0), "+1 or -1"), (dict(A=None), "A and Binv"),
            (dict(Binv=None), "A and Binv")]
    bads += [({name: None}, "required") for name in ("mu", "var", "fstar")]
    for bad, text in bads:
        for fn in (lib.bo_gibbon_v, lib.bo_gibbon_backward_v):
            assert fn(ctypes.byref(_lib.GibbonArgs(**{**ok, **bad})), None) == _lib.BO_ERR_ARG, bad
            assert text in lib.bo_last_error().decode(), (bad, lib.bo_last_error())
    assert lib.bo_gibbon_v(ctypes.byref(_lib.GibbonArgs(**{**ok, "out": None})),
                           None) == _lib.BO_ERR_ARG
    for name in ("dout", "dmu", "dvar", "dA"):
        assert lib.bo_gibbon_backward_v(ctypes.byref(_lib.GibbonArgs(**{**ok, name: None})),
                                        None) == _lib.BO_ERR_ARG
    ok = dict(N=4, mu=d, sigma=d, out=d, status=d)
    for bad in (dict(N=0), dict(mu=None), dict(sigma=None), dict(out=None), dict(status=None),
                dict(have_bounds=1, lo=1.0, hi=1.0)):
        assert lib.bo_mv_quantiles_v(ctypes.byref(_lib.MvQuantilesArgs(**{**ok, **bad})),
                                     None) == _lib.BO_ERR_ARG, bad


def test_mes_op_fake_shapes():
    e = lambda *s: torch.empty(*s, device="meta", dtype=F64)  # noqa: E731
    R, SM, Sm, m = 37, 5, 11, 4
    args = (e(R), e(R), e(SM), e(Sm), 0.1, 0.5, 1.0, 0.2, 1.0)
    assert torch.ops.bo.mes(*args).shape == (R,)
    assert [t.shape for t in torch.ops.bo.mes_backward(e(R), *args)] == [(R,), (R,)]
    args = (e(R), e(R), e(R, m), e(m, m), e(SM), 0.2, -1.0)
    assert torch.ops.bo.gibbon(*args).shape == (R,)
    assert [t.shape for t in torch.ops.bo.gibbon_backward(e(R), *args)] == [(R,), (R,), (R, m)]
    y, st = torch.ops.bo.mv_quantiles(e(9), e(9), False, 0.0, 0.0)
    assert y.shape == (3,) and st.shape == (3,) and st.dtype == torch.int32


@pytest.mark.parametrize("S_M, S_m", [(3, 7), (10, 128)])
@pytest.mark.parametrize("w", [1.0, -1.0])
def test_mes_closed_form_far_max_values(S_M, S_m, w):
    """Every f*_j 50 sigma above the posterior: Z = 1, h1 = h0 and
    ig = (beta - 1) kappa with beta = (1 / S_m) / sqrt(S_M / ((S_m - 1)(S_M S_m - 1)))
    and kappa = (mean z^2 - 1) / 2, to 1e-12."""
    g = torch.Generator().manual_seed(S_M + S_m)
    R = 5
    mu = torch.randn(R, generator=g, dtype=F64)
    var = 0.1 + torch.rand(R, generator=g, dtype=F64)
    z = torch.randn(S_m, generator=g, dtype=F64)
    tau2 = 0.05
    fstar = (w * mu).max() + 50.0 * (var.max() + tau2).sqrt() * (1.0 + torch.rand(S_M, generator=g,
                                                                                  dtype=F64))
    out = mr.mes(mu, var, fstar, z, tau2, w)
    kappa, var_h0, zsq = mr.host_constants(z)
    assert abs(kappa - 0.5 * ((z * z).mean().item() - 1.0)) <= 1e-15
    assert abs(var_h0 - (0.5 * z * z).var().item()) <= 1e-15
    beta = (1.0 / S_m) / math.sqrt(S_M / ((S_m - 1.0) * (S_M * S_m - 1.0)))
    want = (beta - 1.0) * kappa
    err = (out.ig - want).abs().max().item()
    print(f"S_M={S_M} S_m={S_m} w={w}: ig {out.ig[0].item():.6e}, closed form {want:.6e}, "
          f"err {err:.2e}")
    assert err <= 1e-12
    assert (out.beta - beta).abs().max().item() <= 1e-12


def test_mes_sign_of_the_base_samples():
    """mean_new_k = m + t sqrt(vm) w z_k: against the reference's lines 440-448
    spelled out -- samples_m = w (mu + sqrt(vm) z), mean_m = w mu, and
    temp_term = covar_mM / variance_m with covar_mM = variance_M."""
    g = torch.Generator().manual_seed(2)
    mu, var = torch.randn(4, generator=g, dtype=F64), 0.2 + torch.rand(4, generator=g, dtype=F64)
    z = torch.randn(6, generator=g, dtype=F64)
    tau2 = 0.3
    for w in (1.0, -1.0):
        mean_M = w * mu
        samples_m = w * (mu[None] + (var + tau2).sqrt()[None] * z[:, None])   # S_m x R
        mean_m = w * mu
        mean_new = (var / (var + tau2))[None] * (samples_m - mean_m[None]) + mean_M[None]
        mine = (w * mu)[None] + (var / (var + tau2) * (var + tau2).sqrt())[None] * (w * z)[:, None]
        assert (mean_new - mine).abs().max().item() <= 1e-14
        # and the value does depend on that sign
        fstar = (w * mu).max() + torch.tensor([0.3, 0.9], dtype=F64)
        a = mr.mes(mu, var, fstar, z, tau2, w).ig
        b = mr.mes(mu, var, fstar, -z, tau2, w).ig
        assert (a - b).abs().max().item() > 1e-6


@pytest.mark.parametrize("w", [1.0, -1.0])
def test_gibbon_restatement_against_numpy(w):
    """No pending points, tau2 = 0: the same expression evaluated directly in
    numpy (scipy.stats.norm for Phi and phi)."""
    from scipy.stats import norm
    g = torch.Generator().manual_seed(4)
    R, S_M = 9, 6
    mu = torch.randn(R, generator=g, dtype=F64)
    var = 0.1 + torch.rand(R, generator=g, dtype=F64)
    fstar = (w * mu).max() + 0.1 + torch.rand(S_M, generator=g, dtype=F64)
    got = mr.gibbon(mu, var, fstar, 0.0, w).acq.numpy()
    gam = (fstar.numpy()[None, :] - w * mu.numpy()[:, None]) / np.sqrt(var.numpy())[:, None]
    r = norm.pdf(gam) / norm.cdf(gam)
    want = -0.5 * np.log(1.0 - r * (gam + r)).mean(axis=1)   # rho2 = 1 at tau2 = 0
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (want > 0).all()


def test_gibbon_repulsion_is_the_logdet_identity():
    """(log(vm - qf) - log vm) / 2 = (logdet V - logdet B - log vm) / 2 for
    V = [[vm, A], [A^T, B]]."""
    g = torch.Generator().manual_seed(5)
    m = 4
    G = torch.randn(m + 1, m + 1, generator=g, dtype=F64)
    V = G @ G.T + 0.5 * torch.eye(m + 1, dtype=F64)
    vm, A, B = V[0, 0], V[0, 1:], V[1:, 1:]
    tau2 = 0.05
    var, mu = (vm - tau2).reshape(1), torch.zeros(1, dtype=F64)
    fstar = torch.tensor([3.0, 4.0], dtype=F64)
    plain = mr.gibbon(mu, var, fstar, tau2).acq
    full = mr.gibbon(mu, var, fstar, tau2, A=A[None], Binv=torch.linalg.inv(B)).acq
    want = 0.5 * (torch.logdet(V) - torch.logdet(B) - torch.log(vm))
    assert abs((full - plain).item() - want.item()) <= 1e-12


@pytest.mark.parametrize("N", [1, 2, 257, 1500])
def test_quantile_restatement_against_brentq(N):
    """The bisection of the restatement against scipy.optimize.brentq on the
    reference's own objective, exp(sum logcdf) - p (lines 1003-1008):
    1e-11 + 1e-14 |y| (brentq's xtol 2e-12 and rtol 4 eps, times five)."""
    from scipy.optimize import brentq
    from scipy.stats import norm
    g = torch.Generator().manual_seed(N)
    mu = torch.randn(N, generator=g, dtype=F64) * 2.0
    sigma = 10.0 ** (-4.0 + 5.0 * torch.rand(N, generator=g, dtype=F64))
    y, status = mr.quantiles(mu, sigma)
    assert status == [0, 0, 0]
    lo, hi = (mu - 3 * sigma).min().item(), (mu + 5 * sigma).max().item()
    dist = norm(mu.numpy(), sigma.numpy())
    for p, got in zip(mr.QUANTILE_P, y.tolist()):
        want = brentq(lambda t: np.exp(np.sum(dist.logcdf(t))) - p, lo, hi)
        assert abs(got - want) <= 1e-11 + 1e-14 * abs(want), (p, got, want)
    assert y[0] < y[1] < y[2]
    _, status = mr.quantiles(mu, sigma, bounds=(hi + 1.0, hi + 2.0))
    assert status == [1, 1, 1]


def test_quantile_status_raises_brentqs_error(no_native):
    from botorch_amd import kernels
    kernels.mv_quantiles_raise([0, 0, 0])
    with pytest.raises(ValueError, match=r"f\(a\) and f\(b\) must have different signs"):
        kernels.mv_quantiles_raise([0, 1, 0])


def test_package_formulas_match_restatement():
    """The generic route's torch formulas are the restatement's."""
    from botorch_amd.acquisition import _gibbon_chain, _mes_chain
    g = torch.Generator().manual_seed(6)
    R, m = 7, 3
    mu, var = torch.randn(R, generator=g, dtype=F64), 0.1 + torch.rand(R, generator=g, dtype=F64)
    z = torch.randn(9, generator=g, dtype=F64)
    G = torch.randn(m, m, generator=g, dtype=F64)
    Binv = torch.linalg.inv(G @ G.T + torch.eye(m, dtype=F64))
    A = 0.2 * torch.randn(R, m, generator=g, dtype=F64)
    for w in (1.0, -1.0):
        fstar = (w * mu).max() + 0.1 + torch.rand(4, generator=g, dtype=F64)
        assert torch.equal(_mes_chain(mu, var, fstar, z, 0.3, w),
                           mr.mes(mu, var, fstar, z, 0.3, w).ig)
        assert torch.equal(_gibbon_chain(mu, var, fstar, 0.3, w, A, Binv),
                           mr.gibbon(mu, var, fstar, 0.3, w, A, Binv).acq)
        assert torch.equal(_gibbon_chain(mu, var, fstar, 0.3, w),
                           mr.gibbon(mu, var, fstar, 0.3, w).acq)


def test_gpu_kernel_references_meet_the_clamp_cap():
    """The seeds of tests/test_gpu_mes_kernels.py: on the restatement alone, at
    most a tenth of each reference's generated rows lie within 1 % of a clamp
    boundary (asserted where the rows are chosen)."""
    from tests import test_gpu_mes_kernels as gk
    gk.reference_rows_meet_the_cap()


@pytest.fixture
def no_native(monkeypatch):
    """Any use of the native library fails the test."""
    from botorch_amd import _lib, kernels

    def boom(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "torch_ops", boom)
    monkeypatch.setattr(kernels, "lib", boom)


def _model(n=6, d=2, m=1):
    from botorch_amd.models import SingleTaskGP
    g = torch.Generator().manual_seed(0)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = torch.stack([(X.sum(-1) + t).sin() for t in range(m)], dim=-1)
    return SingleTaskGP(X, Y)


@pytest.mark.parametrize("name", ["qMaxValueEntropy", "qLowerBoundMaxValueEntropy"])
def test_constructor_errors_before_native(name, no_native):
    from botorch_amd import acquisition
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import ModelListGP, SaasFullyBayesianSingleTaskGP
    from botorch_amd.objective import ScalarizedPosteriorTransform
    cls = getattr(acquisition, name)
    cand = torch.rand(8, 2, dtype=F64)
    g = torch.Generator().manual_seed(1)
    X = torch.rand(6, 2, generator=g, dtype=F64)
    saas = SaasFullyBayesianSingleTaskGP(X, X.sum(-1, keepdim=True))
    with pytest.raises(UnsupportedError, match="SaasFullyBayesianSingleTaskGP"):
        cls(saas, cand)
    with pytest.raises(UnsupportedError, match="multi-output"):
        cls(_model(m=2).eval(), cand)
    with pytest.raises(UnsupportedError, match="ModelListGP"):
        cls(ModelListGP(_model().eval(), _model().eval()), cand)
    model = _model()
    assert model.training
    with pytest.raises(UnsupportedError, match="eval mode"):
        cls(model, cand)
    model.eval()
    pt = ScalarizedPosteriorTransform(torch.tensor([1.0], dtype=F64))
    with pytest.raises(UnsupportedError, match="posterior_transform"):
        cls(model, cand, posterior_transform=pt)
    with pytest.raises(NotImplementedError, match=r"Batch GP models \(e.g. fantasized models\) "
                                                  "are not yet supported by `MaxValueBase`"):
        cls(model, cand, train_inputs=torch.rand(2, 6, 2, dtype=F64))
    if name == "qMaxValueEntropy":
        with pytest.raises(UnsupportedError, match="GIBBON.*|fantasy"):
            cls(model, cand, X_pending=torch.rand(1, 2, dtype=F64))
        with pytest.raises(ValueError, match="num_y_samples >= 2"):
            cls(model, cand, num_y_samples=1)
        with pytest.raises(ValueError, match="S_M"):
            cls(model, cand, num_mv_samples=0)


def test_mes_set_x_pending_refused(no_native, monkeypatch):
    """qMaxValueEntropy.set_X_pending with points raises before any native call
    (the instance is built without its constructor's sampling)."""
    from botorch_amd.acquisition import MES_PENDING_MSG, qMaxValueEntropy
    from botorch_amd.exceptions import UnsupportedError
    assert "GIBBON" in MES_PENDING_MSG and "fantasy" in MES_PENDING_MSG
    acqf = qMaxValueEntropy.__new__(qMaxValueEntropy)
    with pytest.raises(UnsupportedError, match="GIBBON"):
        acqf.set_X_pending(torch.rand(1, 2, dtype=F64))


def test_kernel_wrapper_checks_before_native(no_native):
    from botorch_amd import kernels
    with pytest.raises(ValueError, match="2 <= S_m"):
        kernels.mes_check(3, 1)
    with pytest.raises(ValueError, match="1 <= S_M"):
        kernels.mes_check(0, 4)
    with pytest.raises(ValueError, match="1 <= R"):
        kernels.mes_check(3, 4, 0)
    with pytest.raises(ValueError, match="m <= 15"):
        kernels.gibbon_check(3, 16)
    with pytest.raises(ValueError, match="R >= 1"):
        kernels.gibbon_check(3, 0, 0)
    kernels.mes_check(1, 2, 1)
    kernels.gibbon_check(1, 15, 1)
    assert kernels.GIBBON_MMAX == 15
    z = torch.tensor([0.5, -1.5, 2.0], dtype=F64)
    assert kernels.mes_host_constants(z) == pytest.approx(mr.host_constants(z), abs=1e-15)
