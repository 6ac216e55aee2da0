"""One-shot qKnowledgeGradient, the parts that need no device: the closed form
against an explicit refit, the tile plan, the constructor's and forward's
errors, the one-shot interface, bo_kg_v's argument checks, the operator's fake
shapes and the initial-condition generator's option check."""
import ctypes
import math

import pytest
import torch

from .kg_restatement import kg_by_refit, kg_values, pack, tile_plan

F64 = torch.float64


def _cpu_model(n=12, d=3, m=1, seed=0):
    from botorch_amd.models import SingleTaskGP
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = torch.randn(n, m, generator=g, dtype=F64)
    return SingleTaskGP(X, Y)


def test_closed_form_equals_refit():
    """n = 40, d = 3, q = 3, N_f = 5, b = 2: the fantasy model's posterior mean
    by an explicit exact GP on the n + q points against the closed form in the
    current model's joint posterior (measured difference 1.2e-14 at value
    scale 4.8; bound 1e-10 absolute)."""
    from oracle.gp import ExactGPOracle, GPHyper
    n, d, q, N_f, b = 40, 3, 3, 5, 2
    g = torch.Generator().manual_seed(11)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = 3.0 + 2.0 * torch.sin(3 * X.sum(-1, keepdim=True)) + 0.1 * torch.randn(n, 1, generator=g, dtype=F64)
    orc = ExactGPOracle(X, Y, GPHyper(torch.full((d,), 0.4, dtype=F64), 1e-2, 0.1))
    assert abs(float(orc.ymean)) > 1 and abs(float(orc.ystd) - 1) > 0.1
    Xa = torch.rand(b, q, d, generator=g, dtype=F64)
    Xf = torch.rand(b, N_f, d, generator=g, dtype=F64)
    Z = torch.randn(N_f, q, generator=g, dtype=F64)
    mean, cov = orc.posterior(torch.cat([Xa, Xf], dim=1))
    noise = orc.h.noise * float(orc.ystd) ** 2
    got = kg_values(mean, cov, Z, noise, q)
    ref = kg_by_refit(orc, Xa, Xf, Z)
    diff = (got - ref).abs().max().item()
    print(f"closed form vs refit: max abs diff {diff:.3e}, value scale {ref.abs().max().item():.3g}")
    assert (ref - mean[:, q:]).abs().max() > 1e-3  # the fantasies do move the mean
    assert diff <= 1e-10


def test_tile_plan_matches_the_formula():
    from botorch_amd import kernels
    for q_a in range(1, 16):
        for N_f in (1, 15, 16, 64, 70):
            T, slots = kernels.kg_tile_plan(q_a, N_f)
            assert T == math.ceil(N_f / (16 - q_a)) and slots == math.ceil(N_f / T), (q_a, N_f)
            assert (T, slots) == tile_plan(q_a, N_f)
            assert q_a + slots <= 16 and T * slots >= N_f and (T - 1) * slots < N_f
    assert kernels.kg_tile_plan(4, 64) == (6, 11)  # 2 spare slots
    assert kernels.kg_tile_plan(8, 64) == (8, 8)   # none
    for bad in ((0, 4), (16, 4), (2, 0)):
        with pytest.raises(ValueError):
            kernels.kg_tile_plan(*bad)
    assert kernels.KG_FUSED_QMAX <= 8


def test_packing_restatement():
    Xa = torch.arange(2 * 2 * 1, dtype=F64).view(2, 2, 1)
    Xf = 100 + torch.arange(2 * 5 * 1, dtype=F64).view(2, 5, 1)
    tiles = pack(Xa, Xf, 2)  # T = 3, one spare slot
    assert tiles.shape == (2, 3, 4, 1)
    assert tiles[1, :, :, 0].tolist() == [[2, 3, 105, 106], [2, 3, 107, 108], [2, 3, 109, 109]]


def test_constructor_errors():
    from botorch_amd.acquisition import (MCAcquisitionFunction, OneShotAcquisitionFunction,
                                         qKnowledgeGradient)
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import ModelListGP, SaasFullyBayesianSingleTaskGP
    from botorch_amd.objective import IdentityMCObjective, ScalarizedPosteriorTransform
    from botorch_amd.sampling import SobolQMCNormalSampler
    model = _cpu_model()
    with pytest.raises(ValueError, match="Must specify `num_fantasies` if no `sampler` is provided."):
        qKnowledgeGradient(model, num_fantasies=None)
    with pytest.raises(ValueError, match="The sampler shape must match num_fantasies=4."):
        qKnowledgeGradient(model, num_fantasies=4, sampler=SobolQMCNormalSampler(torch.Size([8])))
    acqf = qKnowledgeGradient(model, num_fantasies=None, sampler=SobolQMCNormalSampler(torch.Size([8])))
    assert acqf.num_fantasies == 8
    acqf = qKnowledgeGradient(model)
    assert acqf.num_fantasies == 64 and acqf.sampler.sample_shape == torch.Size([64])
    assert isinstance(acqf.sampler, SobolQMCNormalSampler)
    assert isinstance(acqf, OneShotAcquisitionFunction) and isinstance(acqf, MCAcquisitionFunction)
    with pytest.raises(UnsupportedError, match="objective"):
        qKnowledgeGradient(model, num_fantasies=4, objective=IdentityMCObjective())
    with pytest.raises(UnsupportedError, match="multi-output"):
        qKnowledgeGradient(_cpu_model(m=2), num_fantasies=4,
                           objective=None, posterior_transform=None)
    with pytest.raises(UnsupportedError, match="ModelListGP"):
        qKnowledgeGradient(ModelListGP(_cpu_model(), _cpu_model(seed=1)), num_fantasies=4)
    X, Y = model.train_inputs[0], model._raw_train_Y
    with pytest.raises(UnsupportedError, match="fully Bayesian"):
        qKnowledgeGradient(SaasFullyBayesianSingleTaskGP(X, Y), num_fantasies=4)
    with pytest.raises(UnsupportedError, match="ScalarizedPosteriorTransform"):
        qKnowledgeGradient(model, num_fantasies=4,
                           posterior_transform=ScalarizedPosteriorTransform(torch.ones(2, dtype=F64)))
    with pytest.raises(UnsupportedError, match="evaluate"):
        qKnowledgeGradient(model, num_fantasies=4).evaluate(X[:2], torch.stack([X[0] * 0, X[0] * 0 + 1]))


def test_forward_shape_error_and_one_shot_interface():
    from botorch_amd.acquisition import qKnowledgeGradient
    acqf = qKnowledgeGradient(_cpu_model(), num_fantasies=5)
    with pytest.raises(ValueError, match=r"n_f \(5\) must be less than the q-batch dimension of X \(4\)"):
        acqf(torch.rand(2, 4, 3, dtype=F64))
    with pytest.raises(ValueError, match="no candidate"):
        acqf(torch.rand(2, 5, 3, dtype=F64))
    assert acqf.get_augmented_q_batch_size(3) == 8
    X_full = torch.rand(4, 8, 3, dtype=F64)
    assert torch.equal(acqf.extract_candidates(X_full), X_full[:, :3])
    assert torch.equal(acqf.extract_candidates(X_full[0]), X_full[0, :3])


def test_posterior_mean_is_analytic_q1():
    from botorch_amd.acquisition import AnalyticAcquisitionFunction, PosteriorMean
    from botorch_amd.exceptions import UnsupportedError
    pm = PosteriorMean(_cpu_model(), maximize=False)
    assert isinstance(pm, AnalyticAcquisitionFunction) and pm.maximize is False
    with pytest.raises(AssertionError):
        pm(torch.rand(2, 2, 3, dtype=F64))  # q = 1 only
    with pytest.raises(UnsupportedError):
        pm.set_X_pending(torch.rand(1, 3, dtype=F64))


def _kg_args(**kw):
    from botorch_amd import _lib
    fake = 64  # never dereferenced: the checks return before any launch
    base = dict(B=1, T=2, q_a=2, slots=3, N_f=5, max_tries=6, noise=1e-2, jitter0=1e-8, mean=fake,
                cov=fake, Z=fake, acq=fake, values=fake, L=fake, W=fake, info=fake, jitter=fake,
                dacq=fake, dmean=fake, dcov=fake)
    base.update(kw)
    return _lib.KgArgs(**base)


@pytest.mark.parametrize("bad, text", [
    (dict(q_a=0), "q_a >= 1"),
    (dict(q_a=8, slots=9), "q_a + slots <= 16"),
    (dict(T=1), "holds fewer than N_f"),
    (dict(acq=None), "acq and values are required"),
    (dict(values=None), "acq and values are required"),
    (dict(L=None), "L and W are required"),
    (dict(W=None), "L and W are required"),
])
def test_bo_kg_refuses_bad_arguments(bad, text):
    from botorch_amd import _lib
    lib = _lib.lib()
    assert "BoKgArgs" in _lib.ARG_RECORDS
    assert lib.bo_struct_size(b"BoKgArgs") == ctypes.sizeof(_lib.KgArgs)
    a = _kg_args(**bad)
    assert lib.bo_kg_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert text in lib.bo_last_error().decode()


def test_bo_kg_backward_refuses_bad_arguments():
    from botorch_amd import _lib
    lib = _lib.lib()
    for bad, text in ((dict(q_a=0), "q_a >= 1"), (dict(q_a=15, slots=2), "q_a + slots <= 16"),
                      (dict(T=1), "holds fewer than N_f"), (dict(dmean=None), "dmean and dcov"),
                      (dict(dcov=None), "dmean and dcov"), (dict(dacq=None), "dacq")):
        a = _kg_args(**bad)
        assert lib.bo_kg_backward_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG, bad
        assert text in lib.bo_last_error().decode()
    a = _kg_args()
    a.abi_version = _lib.ABI_VERSION + 1  # the header discipline of every _v entry point
    assert lib.bo_kg_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    for sym in ("bo_kg_v", "bo_kg_backward_v"):
        assert sym in _lib.exported_symbols()


def test_kg_op_fake_shapes():
    from botorch_amd import ops
    assert "kg" in ops.OPS and "kg_backward" in ops.OPS
    meta = dict(device="meta", dtype=F64)
    B, q_a, N_f = 3, 4, 13
    T, slots = tile_plan(q_a, N_f)
    qp = q_a + slots
    mean, cov = torch.empty(B * T, qp, **meta), torch.empty(B * T, qp, qp, **meta)
    Z = torch.empty(N_f, q_a, **meta)
    acq, values, L, W, jit, info = torch.ops.bo.kg(mean, cov, Z, 1e-2, q_a, slots)
    assert acq.shape == (B,) and values.shape == (B, N_f) and L.shape == (B, q_a, q_a)
    assert W.shape == (B, N_f, q_a) and jit.shape == (B,)
    assert info.shape == (B,) and info.dtype == torch.int32
    dmean, dcov = torch.ops.bo.kg_backward(acq, None, cov, L, W, slots)
    assert dmean.shape == mean.shape and dcov.shape == cov.shape


def test_frac_random_validation_and_standardize():
    from botorch_amd.acquisition import qKnowledgeGradient
    from botorch_amd.optim import gen_one_shot_kg_initial_conditions, standardize
    acqf = qKnowledgeGradient(_cpu_model(), num_fantasies=4)
    bounds = torch.stack([torch.zeros(3, dtype=F64), torch.ones(3, dtype=F64)])
    for frac in (0.0, 1.0, -0.2, 1.5):
        with pytest.raises(ValueError, match=r"frac_random must take on values in \(0,1\)"):
            gen_one_shot_kg_initial_conditions(acqf, bounds, q=2, num_restarts=2, raw_samples=4,
                                               options={"frac_random": frac})
    y = torch.tensor([1.0, 2.0, 4.0, 9.0], dtype=F64)
    s = standardize(y)
    assert abs(s.mean().item()) < 1e-15 and abs(s.std().item() - 1) < 1e-15
    assert torch.equal(standardize(torch.full((3,), 2.0, dtype=F64)), torch.zeros(3, dtype=F64))
    Y2 = torch.rand(2, 5, 3, dtype=F64)
    torch.testing.assert_close(standardize(Y2), (Y2 - Y2.mean(-2, keepdim=True)) / Y2.std(-2, keepdim=True))


def test_sequential_and_sharded_refuse_one_shot():
    from botorch_amd.acquisition import qKnowledgeGradient
    from botorch_amd.distributed import _optimize_acqf_batch_sharded
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.optim import optimize_acqf
    acqf = qKnowledgeGradient(_cpu_model(), num_fantasies=4)
    bounds = torch.stack([torch.zeros(3, dtype=F64), torch.ones(3, dtype=F64)])
    with pytest.raises(NotImplementedError, match="sequential optimization currently not supported "
                                                   "for one-shot acquisition functions"):
        optimize_acqf(acqf, bounds, q=2, num_restarts=2, raw_samples=4, sequential=True)
    with pytest.raises(UnsupportedError, match="one-shot"):
        _optimize_acqf_batch_sharded(
            acq_function=acqf, bounds=bounds, q=2, num_restarts=2, raw_samples=4, options=None,
            fixed_features=None, post_processing_func=None, batch_initial_conditions=None,
            return_best_only=True, gen_candidates=None, ic_generator=None, timeout_sec=None,
            retry_on_optimization_warning=True, ic_gen_kwargs={})
