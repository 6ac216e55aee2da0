"""Pathwise sampling without a GPU: the ABI record and symbols, the exact
interpolation identity of the restatement (tests/pathwise_restatement.py),
argument errors that must be raised before the native library is touched, and
MaxPosteriorSampling.maximize_samples on hand-made samples (the known answers
of the reference's test/generation/test_sampling.py:48-101)."""
import ctypes
import itertools

import pytest
import torch

from tests import pathwise_restatement as pr

F64 = torch.float64


def test_paths_record_and_symbols():
    from botorch_amd import _lib
    lib = _lib.lib()
    assert "BoPathsArgs" in _lib.ARG_RECORDS
    assert lib.bo_struct_size(b"BoPathsArgs") == ctypes.sizeof(_lib.PathsArgs)
    for sym in ("bo_paths_eval_v", "bo_paths_eval_backward_v"):
        assert sym in _lib.exported_symbols()
    # header discipline and argument errors, refused before any launch
    a = _lib.PathsArgs(kind=0, d=3, S=1, M=4, R=1)
    a.abi_version = _lib.ABI_VERSION + 1
    assert lib.bo_paths_eval_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    dummy = torch.zeros(16, dtype=F64)
    ok = dict(kind=0, d=3, S=1, M=4, R=1, X=dummy, lengthscale=dummy, Omega=dummy, W=dummy,
              out=dummy, dout=dummy, dX=dummy)
    for bad, text in ((dict(M=3), "even"), (dict(d=129), "d <= 128"), (dict(d=0), "d <= 128"),
                      (dict(S=0), "S >= 1"), (dict(kind=2), "kernel kind"),
                      (dict(n=2), "Xt_scaled and V"), (dict(W=None), "W are required")):
        for fn in (lib.bo_paths_eval_v, lib.bo_paths_eval_backward_v):
            assert fn(ctypes.byref(_lib.PathsArgs(**{**ok, **bad})), None) == _lib.BO_ERR_ARG
            assert text in lib.bo_last_error().decode()
    assert lib.bo_paths_eval_v(ctypes.byref(_lib.PathsArgs(**{**ok, "out": None})),
                               None) == _lib.BO_ERR_ARG
    assert lib.bo_paths_eval_backward_v(ctypes.byref(_lib.PathsArgs(**{**ok, "dX": None})),
                                        None) == _lib.BO_ERR_ARG


def test_paths_op_fake_shapes():
    from botorch_amd import ops
    assert "paths_eval" in ops.OPS and "paths_eval_backward" in ops.OPS
    meta = dict(device="meta", dtype=F64)
    R, d, S, M, n = 37, 5, 3, 8, 11
    e = lambda *s: torch.empty(*s, **meta)  # noqa: E731
    args = (e(R, d), e(d), e(M // 2, d), e(S, M), e(n, d), e(S, n), 0, 1.0)
    assert torch.ops.bo.paths_eval(*args, 0.0, 0.0, 1.0, 0).shape == (S, R)
    assert torch.ops.bo.paths_eval(*args, 0.0, 0.0, 1.0, 4).shape == (R,)
    assert torch.ops.bo.paths_eval_backward(e(S, R), *args, 1.0, 0).shape == (R, d)


@pytest.mark.parametrize("kind", [pr.RBF, pr.MATERN52])
@pytest.mark.parametrize("fixed", [False, True])
def test_restatement_interpolates(kind, fixed):
    """g_s(Xt) = y_tf - eps_s - noise V_s exactly (A V = y - prior - eps),
    whatever the quality of the random features."""
    g = torch.Generator().manual_seed(3 + kind + 2 * fixed)
    n, d, S, M = 30, 3, 5, 16
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    ls = 0.3 + 0.4 * torch.rand(d, generator=g, dtype=F64)
    o, c = 1.3, 0.2
    noise = 1e-2 * (1.0 + torch.rand(n, generator=g, dtype=F64)) if fixed else 1e-2
    y = torch.randn(n, generator=g, dtype=F64)
    Omega = torch.randn(M // 2, d, generator=g, dtype=F64)
    W = torch.randn(S, M, generator=g, dtype=F64)
    nz = torch.as_tensor(noise, dtype=F64).expand(n)
    eps = torch.randn(S, n, generator=g, dtype=F64) * nz.sqrt()
    prior = pr.prior_values(Xt, Omega, W, ls, o, c)
    V = pr.update_weights(kind, Xt, ls, o, noise, y, prior, eps)
    got = pr.path_values(kind, Xt, Xt, ls, o, c, 0.0, 1.0, Omega, W, V)
    want = y.unsqueeze(0) - eps - nz * V
    err = (got - want).abs().max().item()
    assert err <= 1e-10 * want.abs().max().item(), err
    # the mapped form picks row r of path (r // inner) % S
    m = pr.mapped_values(kind, Xt, 2, Xt, ls, o, c, 0.0, 1.0, Omega, W, V)
    assert torch.equal(m[7], got[(7 // 2) % S, 7])


@pytest.fixture
def no_native(monkeypatch):
    """Any use of the native library fails the test."""
    from botorch_amd import _lib, kernels

    def boom(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(kernels, "lib", boom)


def _model(n=6, d=2, **kw):
    from botorch_amd.models import SingleTaskGP
    g = torch.Generator().manual_seed(0)
    X = torch.rand(n, d, generator=g, dtype=F64)
    return SingleTaskGP(X, X.sum(-1, keepdim=True).sin(), **kw)


def test_argument_errors_before_native(no_native):
    from botorch_amd import pathwise
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import ModelListGP, SaasFullyBayesianSingleTaskGP
    shape = torch.Size([2])
    model = _model()
    assert model.training
    for draw in (pathwise.draw_matheron_paths, pathwise.draw_kernel_feature_paths):
        with pytest.raises(UnsupportedError, match="eval mode"):
            draw(model, shape)
    with pytest.raises(UnsupportedError, match="eval mode"):
        pathwise.gaussian_update(model, torch.zeros(2, 6, dtype=F64))
    with pytest.raises(UnsupportedError, match="eval mode"):
        pathwise.get_matheron_path_model(ModelListGP(_model(), _model()))
    model.eval()
    with pytest.raises(UnsupportedError, match="even number of output features"):
        pathwise.draw_kernel_feature_paths(model, shape, num_features=7)
    wide = _model(d=129).eval()
    with pytest.raises(UnsupportedError, match="d <= 128"):
        pathwise.draw_matheron_paths(wide, shape)
    g = torch.Generator().manual_seed(1)
    X = torch.rand(6, 2, generator=g, dtype=F64)
    saas = SaasFullyBayesianSingleTaskGP(X, X.sum(-1, keepdim=True))
    with pytest.raises(NotImplementedError):
        pathwise.draw_matheron_paths(saas, shape)
    from botorch_amd.acquisition import PathwiseThompsonSampling
    with pytest.raises(NotImplementedError, match="fully Bayesian"):
        PathwiseThompsonSampling(saas)


def test_kernel_wrapper_checks_before_native(no_native):
    from botorch_amd import kernels
    with pytest.raises(ValueError, match="even"):
        kernels.paths_check(3, 5, 1)
    with pytest.raises(ValueError, match="d <= 128"):
        kernels.paths_check(129, 4, 1)
    kernels.paths_check(128, 2, 1)


def test_max_posterior_sampling_known_answers():
    from botorch_amd.generation import MaxPosteriorSampling
    from botorch_amd.objective import IdentityMCObjective
    mps = MaxPosteriorSampling(model=None)
    assert mps.replacement and isinstance(mps.objective, IdentityMCObjective)
    shapes = (torch.Size(), torch.Size([3]), torch.Size([3, 2]))
    g = torch.Generator().manual_seed(5)
    for batch_shape, N, num_samples, d in itertools.product(shapes, (5, 6), (1, 2), (1, 2)):
        X = torch.randn(*batch_shape, N, d, generator=g, dtype=F64)
        samples = torch.zeros(num_samples, *batch_shape, N, 1, dtype=F64)
        samples[..., 0, :] = 1.0
        s = MaxPosteriorSampling(None).maximize_samples(X, samples, num_samples)
        assert torch.equal(s, X[..., [0] * num_samples, :])
        samples[..., 1, 0] = 1e-6
        mps = MaxPosteriorSampling(None, replacement=False)
        if len(batch_shape) > 1:
            with pytest.raises(NotImplementedError, match="single batch dimension"):
                mps.maximize_samples(X, samples, num_samples)
        else:
            s = mps.maximize_samples(X, samples, num_samples)
            assert s.shape == batch_shape + torch.Size([num_samples, d])
            assert torch.equal(torch.sort(s, dim=-2).values,
                               torch.sort(X[..., :num_samples, :], dim=-2).values)


def test_max_posterior_sampling_without_replacement_order():
    """Sample i takes its best candidate not taken by the samples before it."""
    from botorch_amd.generation import MaxPosteriorSampling
    X = torch.arange(4, dtype=F64).unsqueeze(-1)
    obj = torch.tensor([[0.1, 0.9, 0.5, 0.0], [0.2, 0.8, 0.7, 0.0], [0.3, 0.9, 0.8, 0.0]], dtype=F64)
    s = MaxPosteriorSampling(None, replacement=False).maximize_samples(X, obj.unsqueeze(-1), 3)
    assert s.squeeze(-1).tolist() == [1.0, 2.0, 0.0]
    s = MaxPosteriorSampling(None).maximize_samples(X, obj.unsqueeze(-1), 3)
    assert s.squeeze(-1).tolist() == [1.0, 1.0, 1.0]


def test_deterministic_model_posterior():
    from botorch_amd.acquisition import PosteriorMean
    from botorch_amd.models import GenericDeterministicModel
    from botorch_amd.objective import ScalarizedPosteriorTransform
    m = GenericDeterministicModel(lambda X: torch.stack([X.sum(-1), X.prod(-1)], dim=-1), 2)
    X = torch.rand(4, 1, 3, dtype=F64)
    post = m.posterior(X)
    assert post.mean.shape == (4, 1, 2) and not post.variance.any()
    assert torch.equal(post.rsample(torch.Size([5])), post.mean.expand(5, 4, 1, 2))
    w = torch.tensor([2.0, -1.0], dtype=F64)
    acq = PosteriorMean(m, posterior_transform=ScalarizedPosteriorTransform(w))
    assert torch.allclose(acq(X), (2.0 * X.sum(-1) - X.prod(-1)).squeeze(-1))
