"""condition_on_observations without a device: the custom op's meta shapes, the
C entry points' argument checks, and the model layer on CPU tensors with the
source model in training mode (no cache is built or extended there).
Reference: botorch/models/gpytorch.py:468-531, models/model.py:149,
models/model_list_gp_regression.py:58-129."""
import ctypes

import pytest
import torch

F64 = torch.float64


def test_gp_cache_extend_meta_shapes():
    from botorch_amd import ops
    assert "gp_cache_extend" in ops.OPS
    meta = dict(device="meta", dtype=F64)
    for n, k, order in ((300, 16, 384), (380, 16, 512)):  # the second crosses a padded order
        np_ = (n + 127) // 128 * 128
        Xs = torch.empty(n, 8, **meta)
        L = torch.empty(np_, np_, **meta)
        beta = torch.empty(n, **meta)
        ls = torch.empty(6, **meta)
        Xn, yn = torch.empty(k, 6, **meta), torch.empty(k, **meta)
        Lo, Linvo, Uo, betao, alphao, Xso, info = torch.ops.bo.gp_cache_extend(
            Xs, L, L, beta, beta, ls, Xn, yn, 1.0, 1e-2, 0.0, 0)
        assert Lo.shape == Linvo.shape == Uo.shape == (order, order)
        assert betao.shape == alphao.shape == (n + k,)
        assert Xso.shape == (n + k, 8)
        assert info.shape == (1,) and info.dtype == torch.int32


def _extend_args(n=100, k=5, ld=128, ld_out=128, d=4, null_out=False):
    P = ctypes.c_void_p
    a = P(0x10000)  # aligned, never dereferenced: the checks come before any launch
    return [0, a, a, a, a, a, ld, n, d, a, 1.0, 0.0, a, a, k, 1e-2, P(0), a,
            P(0) if null_out else a, a, a, a, a, ld_out, a, a, P(0)]


def test_gp_cache_extend_refuses_bad_arguments():
    from botorch_amd import _lib
    lib = _lib.lib()
    for kw in (dict(k=0), dict(n=120, k=16, ld_out=128), dict(null_out=True), dict(d=9)):
        status = lib.bo_gp_cache_extend(*_extend_args(**kw))
        assert status == _lib.BO_ERR_ARG, kw
        assert lib.bo_last_error().decode(), kw
    we = ctypes.c_int64(0)
    assert lib.bo_gp_cache_extend_work(4096, 16, ctypes.byref(we)) == _lib.BO_OK
    assert we.value > 0


def _data(n, m=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, 4, generator=g, dtype=F64)
    cols = [torch.sin(3 * X[:, 0] + t) + X[:, 1] * (t + 1) - X[:, 2] ** 2 for t in range(m)]
    Y = torch.stack(cols, dim=-1) + 0.05 * torch.randn(n, m, generator=g, dtype=F64)
    Yvar = 1e-3 + 0.02 * torch.rand(n, m, generator=g, dtype=F64)
    return X, Y, Yvar


def test_single_output_model_layer():
    from botorch_amd.models import SingleTaskGP
    X, Y, _ = _data(30)
    X2, Y2, _ = _data(5, seed=1)
    m = SingleTaskGP(X, Y)
    m.covar_module.lengthscale = torch.tensor([[0.5, 0.6, 0.7, 0.8]], dtype=F64)
    mean, std = m.outcome_transform.means.clone(), m.outcome_transform.stdvs.clone()
    old_targets, old_X = m.train_targets.clone(), m.train_inputs[0].clone()
    assert m.training
    c = m.condition_on_observations(X2, Y2)
    assert isinstance(c, SingleTaskGP) and not c.training and c._cache is None
    assert c.train_inputs[0].shape == (35, 4) and c.train_targets.shape == (35,)
    assert torch.equal(c.train_inputs[0], torch.cat([X, X2]))
    # the old statistics, not refitted on 35 points
    assert torch.equal(c.train_targets[:30], old_targets)
    torch.testing.assert_close(c.train_targets[30:], ((Y2 - mean) / std).squeeze(-1),
                               rtol=0, atol=0)
    assert torch.equal(c._raw_train_Y, torch.cat([Y, Y2]))
    assert torch.equal(c.outcome_transform.means, mean)
    assert torch.equal(c.outcome_transform.stdvs, std)
    # the source is unchanged (its transform still in its own mode, same statistics)
    assert m.training and m.outcome_transform.training
    assert torch.equal(m.train_targets, old_targets) and torch.equal(m.train_inputs[0], old_X)
    assert torch.equal(m.outcome_transform.means, mean)
    # distinct modules with equal values
    for name in ("covar_module", "mean_module", "likelihood", "outcome_transform"):
        assert getattr(c, name) is not getattr(m, name)
    assert torch.equal(c.covar_module.lengthscale, m.covar_module.lengthscale)
    assert torch.equal(c.likelihood.noise, m.likelihood.noise)
    m.covar_module.lengthscale = torch.full((1, 4), 0.3, dtype=F64)
    assert float(c.covar_module.lengthscale.detach()[0, 0]) == 0.5
    # k = 0: an unchanged copy
    c0 = m.condition_on_observations(X2[:0], Y2[:0])
    assert torch.equal(c0.train_inputs[0], X) and torch.equal(c0.train_targets, old_targets)


def test_fixed_noise_model_layer():
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import FixedNoiseGaussianLikelihood, SingleTaskGP
    X, Y, Yvar = _data(30)
    X2, Y2, Yvar2 = _data(5, seed=1)
    m = SingleTaskGP(X, Y, Yvar)
    with pytest.raises(RuntimeError, match="requires a `noise` kwarg"):
        m.condition_on_observations(X2, Y2)
    c = m.condition_on_observations(X2, Y2, noise=Yvar2)  # taken as already transformed
    assert isinstance(c.likelihood, FixedNoiseGaussianLikelihood)
    assert torch.equal(c.likelihood.noise, torch.cat([m.likelihood.noise, Yvar2.squeeze(-1)]))
    assert m.likelihood.noise.shape == (30,)
    with pytest.raises(UnsupportedError):
        SingleTaskGP(X, Y).condition_on_observations(X2, Y2, noise=Yvar2)


def test_multi_output_and_list_model_layer():
    from botorch_amd.models import ModelListGP, SingleTaskGP
    X, Y, _ = _data(30, m=2)
    X2, Y2, _ = _data(5, m=2, seed=1)
    m = SingleTaskGP(X, Y)
    c = m.condition_on_observations(X2, Y2)
    assert c.num_outputs == 2 and c.train_targets.shape == (2, 35)
    assert c.train_inputs[0].shape == (35, 4)
    assert c.likelihood.noise.shape == (2, 1) and c.covar_module.lengthscale.shape == (2, 1, 4)
    for t in range(2):
        mean, std = m.outcome_transform.means[0, t], m.outcome_transform.stdvs[0, t]
        assert torch.equal(c.models[t].train_targets[:30], m.models[t].train_targets)
        torch.testing.assert_close(c.models[t].train_targets[30:], (Y2[:, t] - mean) / std,
                                   rtol=0, atol=0)
        assert torch.equal(c.train_targets[t], c.models[t].train_targets)
        assert c.models[t].train_inputs[0] is c.train_inputs[0]
        assert c.models[t] is not m.models[t]
    assert m.train_targets.shape == (2, 30)

    lst = ModelListGP(SingleTaskGP(X, Y[:, :1]), SingleTaskGP(X[:20], Y[:20, 1:]))
    X3 = torch.rand(5, 4, generator=torch.Generator().manual_seed(5), dtype=F64)
    cl = lst.condition_on_observations([X2, X3], Y2)
    assert isinstance(cl, ModelListGP) and len(cl.models) == 2
    assert cl.models[0].train_inputs[0].shape == (35, 4)
    assert cl.models[1].train_inputs[0].shape == (25, 4)
    assert torch.equal(cl.models[1].train_inputs[0][20:], X3)
    assert torch.equal(cl.models[1]._raw_train_Y[20:], Y2[:, 1:])
    with pytest.raises(ValueError, match="number of inputs"):
        lst.condition_on_observations([X2], Y2)
    with pytest.raises(ValueError, match="number of outputs"):
        lst.condition_on_observations([X2, X3], Y2[:, :1])
    with pytest.raises(ValueError, match="observation noise"):
        lst.condition_on_observations([X2, X3], Y2, noise=torch.ones(5, 1, dtype=F64))


def test_condition_errors():
    from botorch_amd import settings
    from botorch_amd.exceptions import InputDataError, UnsupportedError
    from botorch_amd.models import SaasFullyBayesianSingleTaskGP, SingleTaskGP
    X, Y, _ = _data(30)
    X2, Y2, _ = _data(5, seed=1)
    m = SingleTaskGP(X, Y)
    with pytest.raises(UnsupportedError):  # batched fantasies
        m.condition_on_observations(X2.unsqueeze(0), Y2.unsqueeze(0))
    with pytest.raises(UnsupportedError):
        m.condition_on_observations(X2, Y2.expand(3, 5, 1))
    with pytest.raises(ValueError):  # wrong d
        m.condition_on_observations(X2[:, :3], Y2)
    with pytest.raises(ValueError):  # wrong m
        m.condition_on_observations(X2, torch.cat([Y2, Y2], dim=-1))
    with pytest.raises(ValueError):  # mismatched lengths
        m.condition_on_observations(X2, Y2[:4])
    bad = X2.clone()
    bad[2, 1] = float("nan")
    with pytest.raises(InputDataError):
        m.condition_on_observations(bad, Y2)
    with pytest.raises(InputDataError):
        m.condition_on_observations(X2, Y2 * float("nan"))
    with settings.propagate_grads(True):
        with pytest.raises(UnsupportedError, match="propagate_grads"):
            m.condition_on_observations(X2.clone().requires_grad_(True), Y2)
    saas = SaasFullyBayesianSingleTaskGP(X, Y)
    with pytest.raises(UnsupportedError):
        saas.condition_on_observations(X2, Y2)
