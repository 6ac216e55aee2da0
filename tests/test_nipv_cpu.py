"""qNegIntegratedPosteriorVariance without a GPU: the ABI record and symbols,
the ABI's refusals, the fake shapes of the ops, the rank-q identity of the
restatement (tests/nipv_restatement.py) against an explicit dense refit on the
n + q points, a closed-form known answer, every constructor error with the
native library made to raise, and the generic route's torch formula on host
tensors (values and dX) against the restatement."""
import ctypes

import pytest
import torch

from tests import nipv_restatement as nr

F64 = torch.float64
RBF, M52 = 0, 1


def test_nipv_record_and_symbols():
    from botorch_amd import _lib, ops
    lib = _lib.lib()
    assert "BoNipvArgs" in _lib.ARG_RECORDS
    assert lib.bo_struct_size(b"BoNipvArgs") == ctypes.sizeof(_lib.NipvArgs)
    for sym in ("bo_nipv_gram_v", "bo_nipv_gram_backward_v"):
        assert sym in _lib.exported_symbols()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert "nipv_gram" in ops.OPS and "nipv_gram_backward" in ops.OPS
    assert lib.bo_version() == _lib.ABI_VERSION == 12  # a pure addition


def test_nipv_abi_refusals():
    """Header discipline and argument errors, refused before any launch."""
    from botorch_amd import _lib
    lib = _lib.lib()
    a = _lib.NipvArgs(kind=0, d=3, q=1, R=1, N=1)
    a.abi_version = _lib.ABI_VERSION + 1
    assert lib.bo_nipv_gram_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert "ABI" in lib.bo_last_error().decode()
    a = _lib.NipvArgs(kind=0, d=3, q=1, R=1, N=1)
    a.struct_size -= 8
    assert lib.bo_nipv_gram_backward_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    dummy = torch.zeros(64, dtype=F64)
    ok = dict(kind=0, d=3, q=2, split=0, R=4, n=0, N=5, X=dummy, lengthscale=dummy, Z_scaled=dummy,
              outputscale=1.0, G=dummy, dG=dummy, dX=dummy)
    bads = [(dict(d=129), "d <= 128"), (dict(d=0), "d <= 128"), (dict(N=0), "N >= 1"),
            (dict(R=0), "R >= 1"), (dict(q=0), "q <= 16"), (dict(q=17, R=17), "q <= 16"),
            (dict(q=3), "q must divide R"), (dict(kind=2), "kernel kind"),
            (dict(n=2), "Xt_scaled and V"), (dict(n=2, Xt_scaled=dummy), "Xt_scaled and V"),
            (dict(n=2, V=dummy), "Xt_scaled and V"), (dict(split=-1), "split"),
            (dict(split=1025), "split")]
    bads += [({name: None}, "required") for name in ("X", "lengthscale", "Z_scaled")]
    for bad, text in bads:
        for fn in (lib.bo_nipv_gram_v, lib.bo_nipv_gram_backward_v):
            assert fn(ctypes.byref(_lib.NipvArgs(**{**ok, **bad})), None) == _lib.BO_ERR_ARG, bad
            assert text in lib.bo_last_error().decode(), (bad, lib.bo_last_error())
    assert lib.bo_nipv_gram_v(ctypes.byref(_lib.NipvArgs(**{**ok, "G": None})),
                              None) == _lib.BO_ERR_ARG
    assert "G is required" in lib.bo_last_error().decode()
    for name in ("dG", "dX"):
        assert lib.bo_nipv_gram_backward_v(ctypes.byref(_lib.NipvArgs(**{**ok, name: None})),
                                           None) == _lib.BO_ERR_ARG
        assert "dG and dX are required" in lib.bo_last_error().decode()


def test_nipv_op_fake_shapes():
    meta = dict(device="meta", dtype=F64)
    B, q, d, N, n = 7, 3, 5, 19, 11
    e = lambda *s: torch.empty(*s, **meta)  # noqa: E731
    args = (e(B * q, d), q, e(d), e(n, d), e(N, d), e(N, n), 0, 1.0, 0)
    assert torch.ops.bo.nipv_gram(*args).shape == (B, q, q)
    assert torch.ops.bo.nipv_gram_backward(e(B, q, q), *args).shape == (B * q, d)
    args0 = (e(B * q, d), q, e(d), None, e(N, d), None, 1, 1.0, 2)
    assert torch.ops.bo.nipv_gram(*args0).shape == (B, q, q)


def _problem(case, n=20, d=3, N=40, q=3, seed=11):
    g = torch.Generator().manual_seed(seed)
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    y = torch.randn(n, generator=g, dtype=F64)
    ls = 0.3 + 0.4 * torch.rand(d, generator=g, dtype=F64)
    noise = 1e-2 * (1.0 + torch.rand(n, generator=g, dtype=F64)) if case == "fixed" else 1e-2
    kind = M52 if case == "matern" else RBF
    gp = nr.make_gp(Xt, y, ls, noise, const=0.2, kind=kind, o=1.3)
    Z = torch.rand(N, d, generator=g, dtype=F64)
    X = torch.rand(q, d, generator=g, dtype=F64)
    return gp, Z, X


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("case", ["homoskedastic", "fixed", "matern"])
def test_rank_q_identity_equals_dense_refit(case, q):
    gp, Z, X = _problem(case, q=q)
    got, ref = nr.nipv(gp, Z, X), nr.explicit_refit(gp, Z, X)
    vbar = nr.posterior(gp, Z.unsqueeze(-2))[1].mean()
    print(f"{case} q={q}: nipv {got.item():.15e} refit {ref.item():.15e} "
          f"reduction {(1 + got / vbar).item():.3f} of vbar")
    assert abs(1 + got / vbar) > 1e-3  # the observations do lower the variance
    torch.testing.assert_close(got, ref, rtol=1e-10, atol=0.0)


def test_known_answer_without_data():
    """n = 0, q = 1: acq = -(o - sum_z (o k(x, z))^2 / ((o + tau2) N)); through
    the restatement (tau2 = 0 without data) and through the package's formula
    with tau2 = 0.3."""
    from botorch_amd.acquisition import _nipv_value
    d, N, o = 3, 33, 1.7
    g = torch.Generator().manual_seed(3)
    ls = 0.3 + 0.4 * torch.rand(d, generator=g, dtype=F64)
    gp = nr.make_gp(torch.zeros(0, d, dtype=F64), torch.zeros(0, dtype=F64), ls, 0.25, o=o)
    Z = torch.rand(N, d, generator=g, dtype=F64)
    X = torch.rand(1, d, generator=g, dtype=F64)
    k2 = (nr.kernel(X, Z, ls, RBF, o) ** 2).sum()
    want0 = -(o - k2 / (o * N))
    assert abs(nr.nipv(gp, Z, X).item() - want0.item()) <= 1e-14
    G = nr.gram(gp, Z, nr.make_V(gp, Z), X)
    assert abs(G.item() - k2.item()) <= 1e-14
    got = _nipv_value(torch.full((1, 1), o, dtype=F64), G, 0.3, o, N)
    assert abs(got.item() + (o - k2.item() / ((o + 0.3) * N))) <= 1e-14


def test_generic_formula_on_host_tensors():
    """The package's torch formula (what both routes apply to Sigma and G) on
    host tensors, from the restatement's Sigma and C taken in two chunks of the
    integration points as the generic route takes them: values and dX against
    the restatement."""
    from botorch_amd.acquisition import _nipv_value
    gp, Z, _ = _problem("fixed", N=40)
    g = torch.Generator().manual_seed(5)
    X = torch.rand(4, 3, 3, generator=g, dtype=F64)
    V = nr.make_V(gp, Z)
    vbar = nr.posterior(gp, Z.unsqueeze(-2))[1].mean().item()
    Xr = X.clone().requires_grad_(True)
    ref = nr.nipv(gp, Z, Xr)
    (dref,) = torch.autograd.grad(ref.sum(), Xr)
    assert dref.abs().max() > 1e-6
    Xg = X.clone().requires_grad_(True)
    G = sum(C @ C.mT for C in (nr.cross_cov(gp, Z[s], V[s], Xg)
                               for s in (slice(0, 17), slice(17, 40))))
    got = _nipv_value(nr.posterior(gp, Xg)[1], G, gp.tau2.item(), vbar, 40)
    (dgot,) = torch.autograd.grad(got.sum(), Xg)
    torch.testing.assert_close(got, ref, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(dgot, dref, rtol=1e-9, atol=1e-12)


@pytest.fixture
def no_native(monkeypatch):
    """Any use of the native library fails the test."""
    from botorch_amd import _lib, kernels

    def boom(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(kernels, "lib", boom)


def _model(n=6, d=2, m=1):
    from botorch_amd.models import SingleTaskGP
    g = torch.Generator().manual_seed(0)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = torch.stack([(X.sum(-1) + t).sin() for t in range(m)], dim=-1)
    return SingleTaskGP(X, Y)


def test_constructor_errors_before_native(no_native):
    from botorch_amd.acquisition import qNegIntegratedPosteriorVariance as NIPV
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import ModelListGP, SaasFullyBayesianSingleTaskGP
    from botorch_amd.objective import ScalarizedPosteriorTransform
    Z = torch.rand(9, 2, dtype=F64)
    g = torch.Generator().manual_seed(1)
    X = torch.rand(6, 2, generator=g, dtype=F64)
    saas = SaasFullyBayesianSingleTaskGP(X, X.sum(-1, keepdim=True))
    with pytest.raises(UnsupportedError, match="SaasFullyBayesianSingleTaskGP is not supported"):
        NIPV(saas, Z)
    with pytest.raises(UnsupportedError, match="is not supported \\(SingleTaskGP"):
        NIPV(torch.nn.Linear(1, 1), Z)
    with pytest.raises(UnsupportedError, match="Must specify a posterior transform"):
        NIPV(_model(m=2).eval(), Z)
    with pytest.raises(UnsupportedError, match="Must specify a posterior transform"):
        NIPV(ModelListGP(_model().eval(), _model().eval()), Z)
    with pytest.raises(UnsupportedError, match="every member .* single-output SingleTaskGP"):
        NIPV(ModelListGP(_model(m=2).eval(), _model().eval()), Z)
    two = ScalarizedPosteriorTransform(torch.tensor([1.0, 2.0], dtype=F64))
    with pytest.raises(ValueError, match="2 weights for a model with 1 outputs"):
        NIPV(_model().eval(), Z, posterior_transform=two)
    with pytest.raises(UnsupportedError, match="only a ScalarizedPosteriorTransform"):
        NIPV(_model().eval(), Z, posterior_transform=lambda p: p)
    model = _model()
    assert model.training
    with pytest.raises(UnsupportedError, match="eval mode"):
        NIPV(model, Z)
    with pytest.raises(UnsupportedError, match="eval mode"):
        NIPV(ModelListGP(_model().eval(), _model()), Z, posterior_transform=two)
    model.eval()
    with pytest.raises(UnsupportedError, match="without batch dimensions"):
        NIPV(model, torch.rand(2, 9, 2, dtype=F64))
    with pytest.raises(UnsupportedError, match="mc_points must be `N x 2`"):
        NIPV(model, torch.rand(9, 3, dtype=F64))


def test_kernel_wrapper_checks_before_native(no_native):
    from botorch_amd import kernels
    for args, text in (((129, 1, 1), "d <= 128"), ((0, 1, 1), "d <= 128"), ((3, 0, 1), "q <= 16"),
                       ((3, 17, 1), "q <= 16"), ((3, 1, 0), "N >= 1"), ((3, 3, 5, 7), "divide R"),
                       ((3, 3, 5, 0), "R >= 1"), ((3, 3, 5, 6, 1025), "split")):
        with pytest.raises(ValueError, match=text):
            kernels.nipv_check(*args)
    kernels.nipv_check(128, 16, 1, 32, 3)
    z = lambda *s: torch.zeros(*s, dtype=F64)  # noqa: E731
    with pytest.raises(ValueError, match="go together"):
        kernels.nipv_gram(z(4, 3), 2, z(3), z(5, 3), z(7, 3), None)
    with pytest.raises(ValueError, match="V must be 7 x n"):
        kernels.nipv_gram(z(4, 3), 2, z(3), z(5, 3), z(7, 3), z(6, 5))
    with pytest.raises(ValueError, match="dG must be"):
        kernels.nipv_gram_backward(z(2, 2, 3), z(4, 3), 2, z(3), None, z(7, 3), None)
