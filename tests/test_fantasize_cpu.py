"""Model.fantasize, the parts that need no device: the conditioning formulas
against an explicit refit, the tile plan, the refusals and argument errors, the
fantasy model's shapes, bo_fantasy_posterior's argument and header checks and the operator's fake
shapes."""
import ctypes

import pytest
import torch

from .fantasy_restatement import (fantasy_by_refit, fantasy_moments, fantasy_moments_packed, pack,
                                  read_masks, tile_plan)

F64 = torch.float64


def _cpu_model(n=12, d=3, m=1, seed=0):
    from botorch_amd.models import SingleTaskGP
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = torch.randn(n, m, generator=g, dtype=F64)
    return SingleTaskGP(X, Y)


def _sampler(N_f=5):
    from botorch_amd.sampling import SobolQMCNormalSampler
    return SobolQMCNormalSampler(sample_shape=torch.Size([N_f]))


@pytest.mark.parametrize("per_row_noise", [False, True])
def test_restatement_equals_refit(per_row_noise):
    """n = 40, d = 3, b = 2, q_a = 3, q = 2, N_f = 5: mean and covariance of
    every fantasy model by an explicit exact GP on the n + q_a points against
    the four formulas in the current model's joint posterior.  Bound 1e-9
    max|ref| + 1e-10; measured 1.4e-14 (mean, scale 4.1) and 2.1e-15
    (covariance, scale 0.21) with the model's noise, 7.1e-15 and 2.2e-15 with a
    noise per row."""
    from oracle.gp import ExactGPOracle, GPHyper
    n, d, b, q_a, q, N_f = 40, 3, 2, 3, 2, 5
    g = torch.Generator().manual_seed(11)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = 3.0 + 2.0 * torch.sin(3 * X.sum(-1, keepdim=True)) + 0.1 * torch.randn(n, 1, generator=g, dtype=F64)
    orc = ExactGPOracle(X, Y, GPHyper(torch.full((d,), 0.4, dtype=F64), 1e-2, 0.1))
    assert abs(float(orc.ymean)) > 1 and abs(float(orc.ystd) - 1) > 0.1
    Xa = torch.rand(b, q_a, d, generator=g, dtype=F64)
    Xp = torch.rand(b, N_f, q, d, generator=g, dtype=F64)
    Z = torch.randn(N_f, q_a, generator=g, dtype=F64)
    noise_tf = torch.tensor([5e-3, 2e-2, 8e-2], dtype=F64) if per_row_noise else None
    s2 = float(orc.ystd) ** 2
    noise = (noise_tf if per_row_noise else torch.full((q_a,), orc.h.noise, dtype=F64)) * s2
    joint = torch.cat([Xa.unsqueeze(1).expand(b, N_f, q_a, d), Xp], dim=-2)
    mean, cov = orc.posterior(joint)
    got_m, got_c = fantasy_moments(mean, cov, Z, noise, q_a)
    ref_m, ref_c = fantasy_by_refit(orc, Xa, Xp, Z, noise_tf)
    for what, got, ref in (("mean", got_m, ref_m), ("cov", got_c, ref_c)):
        diff = (got - ref).abs().max().item()
        lim = 1e-9 * ref.abs().max().item() + 1e-10
        print(f"{what}: restatement vs refit max abs diff {diff:.3e} (limit {lim:.3e}, "
              f"scale {ref.abs().max().item():.3g})")
        assert diff <= lim, what
    assert (ref_m - mean[..., q_a:]).abs().max() > 1e-3   # the fantasies do move the mean
    assert (ref_c - cov[..., q_a:, q_a:]).abs().max() > 1e-4  # and shrink the covariance
    # the packed statement reads the same numbers out of the tiles
    T, slots = tile_plan(q_a, q, N_f)
    pm, pc = orc.posterior(pack(Xa, Xp, slots).reshape(b * T, q_a + slots * q, d))
    pk_m, pk_c, _, _ = fantasy_moments_packed(pm, pc, Z, noise, q_a, q, slots, False)
    torch.testing.assert_close(pk_m, got_m, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(pk_c, got_c, rtol=1e-12, atol=1e-13)


def test_tile_plan_invariants():
    from botorch_amd import kernels
    for q_a in range(1, 16):
        for q in range(1, 16 - q_a + 1):
            for F in (1, 5, 64):
                T, slots = kernels.fantasy_tile_plan(q_a, q, F)
                assert (T, slots) == tile_plan(q_a, q, F), (q_a, q, F)
                assert slots >= 1 and q_a + slots * q <= 16
                assert T * slots >= F and (T - 1) * slots < F  # no empty tile
                # every group exactly once, in disjoint rows below the fantasised points
                seen = set()
                for g in range(F):
                    t, r0 = g // slots, q_a + (g % slots) * q
                    assert t < T and r0 + q <= q_a + slots * q
                    rows = {(t, r) for r in range(r0, r0 + q)}
                    assert not rows & seen
                    seen |= rows
                assert len(seen) == F * q
                rm, rc = read_masks(1, q_a, q, F, slots)
                assert rm.sum().item() == F * q
                assert rc.sum().item() == q_a * q_a + F * q * (q_a + q)
    assert kernels.fantasy_tile_plan(4, 1, 64) == kernels.kg_tile_plan(4, 64)  # KG: q = 1
    assert kernels.fantasy_tile_plan(8, 4, 3) == (2, 2)
    assert kernels.fantasy_tile_plan(2, 3, 1) == (1, 1)
    for bad in ((0, 1, 4), (1, 0, 4), (8, 9, 4), (16, 1, 4), (2, 2, 0)):
        with pytest.raises(ValueError):
            kernels.fantasy_tile_plan(*bad)


def test_packing_restatement():
    Xa = torch.arange(2 * 2 * 1, dtype=F64).view(2, 2, 1)
    Xp = 100 + torch.arange(2 * 3 * 2 * 1, dtype=F64).view(2, 3, 2, 1)
    tiles = pack(Xa, Xp, 2)  # T = 2, one spare group
    assert tiles.shape == (2, 2, 6, 1)
    assert tiles[1, :, :, 0].tolist() == [[2, 3, 106, 107, 108, 109], [2, 3, 110, 111, 110, 111]]


def test_refusals():
    from botorch_amd.exceptions import BotorchError, DeprecationError, UnsupportedError
    from botorch_amd.models import (FantasizedGP, GenericDeterministicModel, ModelListGP,
                                    SaasFullyBayesianSingleTaskGP)
    model = _cpu_model()
    X = torch.rand(2, 3, 3, dtype=F64)
    assert issubclass(DeprecationError, BotorchError)
    for flag in (True, False):
        with pytest.raises(DeprecationError,
                           match="`fantasize` no longer accepts a boolean for `observation_noise`."):
            model.fantasize(X, _sampler(), observation_noise=flag)
    with pytest.raises(UnsupportedError, match="multi-output"):
        _cpu_model(m=2).fantasize(X, _sampler())
    with pytest.raises(UnsupportedError, match="ModelListGP"):
        ModelListGP(_cpu_model(), _cpu_model(seed=1)).fantasize(X, _sampler())
    tX, tY = model.train_inputs[0], model._raw_train_Y
    with pytest.raises(UnsupportedError, match="SaasFullyBayesianSingleTaskGP"):
        SaasFullyBayesianSingleTaskGP(tX, tY).fantasize(X, _sampler())
    with pytest.raises(UnsupportedError, match="GenericDeterministicModel"):
        GenericDeterministicModel(lambda x: x.sum(-1, keepdim=True)).fantasize(X, _sampler())
    with pytest.raises(UnsupportedError, match="q_a = 0"):
        model.fantasize(torch.rand(2, 0, 3, dtype=F64), _sampler())
    with pytest.raises(UnsupportedError, match="unsupported arguments"):
        model.fantasize(X, _sampler(), noise=torch.ones(3, 1, dtype=F64))
    fm = model.fantasize(X, _sampler(), propagate_grads=True)  # accepted, no further effect
    assert isinstance(fm, FantasizedGP)
    with pytest.raises(UnsupportedError, match="nested"):
        fm.fantasize(X, _sampler())
    with pytest.raises(UnsupportedError, match="nested"):
        fm.condition_on_observations(X[0], torch.rand(3, 1, dtype=F64))
    with pytest.raises(UnsupportedError, match="observation_noise is True or False"):
        fm.posterior(X, observation_noise=torch.ones(3, 1, dtype=F64))
    # the refusals pinned elsewhere stay
    with pytest.raises(UnsupportedError, match="batched fantasy models"):
        model.condition_on_observations(X, torch.rand(2, 3, 1, dtype=F64))


def test_value_errors():
    from botorch_amd.sampling import SobolQMCNormalSampler
    model = _cpu_model()
    X = torch.rand(2, 3, 3, dtype=F64)
    with pytest.raises(ValueError, match="X must be"):
        model.fantasize(torch.rand(2, 3, 4, dtype=F64), _sampler())
    with pytest.raises(ValueError, match="one-dimensional"):
        model.fantasize(X, SobolQMCNormalSampler(sample_shape=torch.Size([2, 3])))
    with pytest.raises(ValueError, match="observation_noise must be"):
        model.fantasize(X, _sampler(), observation_noise=torch.ones(2, 1, dtype=F64))
    fm = model.fantasize(X, _sampler(5))
    for bad in ((3, 2, 3), (4, 2, 2, 3), (5, 3, 2, 3), (1, 5, 2, 2, 3)):
        with pytest.raises(ValueError, match="does not broadcast"):
            fm.posterior(torch.rand(*bad, dtype=F64))
    with pytest.raises(ValueError, match="X must be"):
        fm.posterior(torch.rand(2, 2, 4, dtype=F64))


def test_fantasy_model_shapes():
    from botorch_amd.models import FantasizedGP, Model
    model = _cpu_model(n=12, d=3)
    X = torch.rand(2, 3, 3, dtype=F64, requires_grad=True)
    fm = model.fantasize(X, _sampler(5))
    assert isinstance(fm, FantasizedGP) and isinstance(fm, Model)
    import botorch_amd
    assert botorch_amd.FantasizedGP is FantasizedGP and "FantasizedGP" in botorch_amd.__all__
    assert fm.batch_shape == torch.Size([5, 2]) and fm.num_outputs == 1
    assert not hasattr(fm, "prediction_cache")
    assert fm.source is model and model not in list(fm.modules())
    (ti,) = fm.train_inputs
    assert ti.shape == (5, 2, 15, 3) and not ti.requires_grad
    assert torch.equal(ti[4, 1, :12], model.train_inputs[0]) and torch.equal(ti[2, 1, 12:], X[1].detach())
    fm1 = model.fantasize(X[0].float(), _sampler(4), observation_noise=torch.full((3, 1), 0.1))
    assert fm1.batch_shape == torch.Size([4]) and fm1.train_inputs[0].shape == (4, 15, 3)
    assert fm1.train_inputs[0].dtype == F64
    if torch.cuda.is_available():  # the targets are drawn from the posterior: device kernels
        from botorch_amd.models import SingleTaskGP
        dm = SingleTaskGP(model.train_inputs[0].to("cuda"), model._raw_train_Y.to("cuda"))
        dfm = dm.fantasize(X.detach().to("cuda"), _sampler(5))
        assert dfm.train_targets.shape == (5, 2, 15) and not dfm.train_targets.requires_grad


def _fantasy_args(**kw):
    from botorch_amd import _lib
    fake = 64  # never dereferenced: the checks return before any launch
    base = dict(B=1, T=2, q_a=2, q=2, slots=3, N_f=5, shared=0, max_tries=6, jitter0=1e-8,
                noise_stride=0, mean=fake, cov=fake, Z=fake, noise=fake, mean_out=fake,
                cov_out=fake, L=fake, V=fake, info=fake, jitter=fake, dmean_out=fake,
                dcov_out=fake, dmean=fake, dcov=fake, dZ=fake)
    base.update(kw)
    return _lib.FantasyArgs(**base)


@pytest.mark.parametrize("bad, text", [
    (dict(q_a=0), "q_a >= 1 and q >= 1"),
    (dict(q=0), "q_a >= 1 and q >= 1"),
    (dict(q_a=8, q=3, slots=3), "q_a + slots q <= 16"),
    (dict(slots=0), "slots >= 1"),
    (dict(T=1), "holds fewer than F = 5"),
    (dict(shared=2), "shared is 0 or 1"),
    (dict(noise_stride=1), "noise_stride is 0 or q_a"),
    (dict(noise=None), "mean, cov and noise are required"),
    (dict(mean_out=None), "mean_out and cov_out are required"),
    (dict(L=None), "Z, L and V are required"),
    (dict(V=None), "Z, L and V are required"),
])
def test_bo_fantasy_refuses_bad_arguments(bad, text):
    from botorch_amd import _lib
    lib = _lib.lib()
    assert _lib.PLAIN_ARG_RECORDS["BoFantasyArgs"] is _lib.FantasyArgs
    assert lib.bo_struct_size(b"BoFantasyArgs") == ctypes.sizeof(_lib.FantasyArgs)
    a = _fantasy_args(**bad)
    assert lib.bo_fantasy_posterior(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert text in lib.bo_last_error().decode()


def test_bo_fantasy_backward_refuses_bad_arguments():
    from botorch_amd import _lib
    lib = _lib.lib()
    for bad, text in ((dict(q_a=0), "q_a >= 1"), (dict(q_a=15, q=1, slots=2), "q_a + slots q <= 16"),
                      (dict(T=1), "holds fewer than F"), (dict(dmean=None), "dmean and dcov"),
                      (dict(dcov=None), "dmean and dcov"), (dict(dmean_out=None), "dmean_out"),
                      (dict(dcov_out=None), "dcov_out")):
        a = _fantasy_args(**bad)
        assert lib.bo_fantasy_posterior_backward(ctypes.byref(a), None) == _lib.BO_ERR_ARG, bad
        assert text in lib.bo_last_error().decode()
    assert lib.bo_fantasy_posterior(ctypes.byref(_fantasy_args(shared=1, T=1, B=0)), None) == _lib.BO_OK
    # the header discipline of every record entry point: another ABI version, a short
    # struct_size and a null record are refused before anything is read
    assert set(_lib.PLAIN_RECORD_ENTRIES) == {"bo_fantasy_posterior", "bo_fantasy_posterior_backward"}
    for sym, rec in _lib.PLAIN_RECORD_ENTRIES.items():
        assert sym in _lib.exported_symbols() and sym not in _lib.RECORD_ENTRIES
        fn = getattr(lib, sym)
        a = _fantasy_args()
        a.abi_version = _lib.ABI_VERSION + 1
        assert fn(ctypes.byref(a), None) == _lib.BO_ERR_ARG and sym.encode() in lib.bo_last_error()
        a = _fantasy_args()
        a.struct_size = ctypes.sizeof(rec) - 8
        assert fn(ctypes.byref(a), None) == _lib.BO_ERR_ARG and sym.encode() in lib.bo_last_error()
        assert fn(None, None) == _lib.BO_ERR_ARG
    assert lib.bo_version() == _lib.ABI_VERSION == 12  # an additive change


def test_fantasy_op_fake_shapes():
    from botorch_amd import ops
    assert "fantasy_posterior" in ops.OPS and "fantasy_posterior_backward" in ops.OPS
    meta = dict(device="meta", dtype=F64)
    B, q_a, q, N_f = 3, 4, 3, 13
    for shared in (False, True):
        F = 1 if shared else N_f
        T, slots = tile_plan(q_a, q, F)
        qp = q_a + slots * q
        mean, cov = torch.empty(B * T, qp, **meta), torch.empty(B * T, qp, qp, **meta)
        Z, noise = torch.empty(N_f, q_a, **meta), torch.empty(q_a, **meta)
        mo, co, L, V, jit, info = torch.ops.bo.fantasy_posterior(mean, cov, Z, noise, q_a, q, slots,
                                                                 shared)
        assert mo.shape == (B, N_f, q) and co.shape == (B, F, q, q) and L.shape == (B, q_a, q_a)
        assert V.shape == (B, F, q, q_a) and jit.shape == (B,)
        assert info.shape == (B,) and info.dtype == torch.int32
        dmean, dcov, dZ = torch.ops.bo.fantasy_posterior_backward(mo, co, Z, L, V, slots, shared)
        assert dmean.shape == mean.shape and dcov.shape == cov.shape and dZ.shape == Z.shape
