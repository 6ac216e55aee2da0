"""The ParEGO surface without a GPU: get_chebyshev_scalarization against values worked by
hand, sample_simplex, the BoQmcChebArgs record and its entries, and qLogNParEGO on the
generic route against qLogNoisyExpectedImprovement over the same objective."""
import ctypes

import pytest
import torch

F64 = torch.float64


def test_scalarization_by_hand():
    from botorch_amd import get_chebyshev_scalarization
    w = torch.tensor([0.75, -0.25], dtype=F64)
    Y = torch.tensor([[1.0, 2.0], [3.0, 0.0], [2.0, 1.0]], dtype=F64)
    s = get_chebyshev_scalarization(w, Y)
    # -Y has bounds [-3, -1] x [-2, 0]; row (1, 2): y~ = (1, 0 - 1), w y~ = (0.75, 0.25),
    # -(0.75 + 0.05 * 1.0); row (3, 0): y~ = (0, 1 - 1) -> 0; row (2, 1): (0.375, 0.125)
    torch.testing.assert_close(s(Y), torch.tensor([-0.8, 0.0, -0.4], dtype=F64), rtol=0, atol=1e-15)
    torch.testing.assert_close(s.Y_bounds, torch.tensor([[-3.0, -2.0], [-1.0, 0.0]], dtype=F64))
    assert s.alpha == 0.05 and s.weights is w
    torch.testing.assert_close(s.a * Y + s.b, torch.tensor([[0.75, 0.25], [0.0, 0.0],
                                                            [0.375, 0.125]], dtype=F64))
    # n = 0: p = w (-y); y = (1, -2), w = (0.5, 0.5): -(max(-0.5, 1) + 0.1 * 0.5)
    s0 = get_chebyshev_scalarization(torch.tensor([0.5, 0.5], dtype=F64), Y[:0], alpha=0.1)
    torch.testing.assert_close(s0(torch.tensor([1.0, -2.0], dtype=F64)),
                               torch.tensor(-1.05, dtype=F64), rtol=0, atol=1e-15)
    assert s0.Y_bounds is None


def test_scalarization_errors():
    from botorch_amd import get_chebyshev_scalarization
    from botorch_amd.exceptions import BotorchTensorDimensionError, UnsupportedError
    w = torch.tensor([0.75, -0.25], dtype=F64)
    with pytest.raises(BotorchTensorDimensionError):
        get_chebyshev_scalarization(w, torch.zeros(4, 3, dtype=F64))
    with pytest.raises(NotImplementedError):
        get_chebyshev_scalarization(w, torch.zeros(2, 4, 2, dtype=F64))
    with pytest.raises(UnsupportedError):
        get_chebyshev_scalarization(w, torch.zeros(0, 2, dtype=F64))


@pytest.mark.parametrize("qmc", [False, True])
def test_sample_simplex(qmc):
    from botorch_amd import sample_simplex
    x = sample_simplex(5, n=7, qmc=qmc, seed=3, dtype=F64)
    assert x.shape == (7, 5) and (x >= 0).all()
    torch.testing.assert_close(x.sum(-1), torch.ones(7, dtype=F64))
    assert torch.equal(sample_simplex(1, n=2), torch.ones(2, 1))


def test_record_and_entries():
    import botorch_amd
    from botorch_amd import _lib
    assert _lib.lib().bo_struct_size(b"BoQmcChebArgs") == ctypes.sizeof(_lib.QmcChebArgs)
    for name in ("bo_qmc_cheb", "bo_qmc_cheb_backward"):
        assert name in _lib.exported_symbols() and name not in _lib.RECORD_ENTRIES
        assert _lib.CHEB_RECORD_ENTRIES[name] is _lib.QmcChebArgs
    a = _lib.QmcChebArgs(B=1, q=1, Mt=2, S=1, G=1, omask=3)
    a.abi_version += 1
    assert _lib.lib().bo_qmc_cheb(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert {"qLogNParEGO", "get_chebyshev_scalarization", "sample_simplex"} <= set(
        botorch_amd.__all__)


class _Posterior:
    def __init__(self, X):
        self.mean = torch.stack([X.sum(-1).sin(), (X * X).sum(-1), X[..., 0] - X[..., 1]], dim=-1)


class _Model:
    num_outputs = 3

    def posterior(self, X, posterior_transform=None, **kw):
        return _Posterior(X)


class _Sampler:
    sample_shape = torch.Size([4])

    def __call__(self, posterior):
        m = posterior.mean
        noise = torch.sin(torch.arange(4 * m.numel(), dtype=F64)).reshape(4, *m.shape)
        return m + 0.3 * noise


def test_parego_generic_route_is_qlognei_of_the_scalarization():
    from botorch_amd.acquisition import (IdentityMCMultiOutputObjective, qLogNParEGO,
                                         qLogNoisyExpectedImprovement)
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.objective import GenericMCObjective
    g = torch.Generator().manual_seed(0)
    Xb = torch.rand(6, 2, dtype=F64, generator=g)
    X = torch.rand(3, 2, 2, dtype=F64, generator=g)
    w = torch.tensor([0.6, -0.4], dtype=F64)
    cons = [lambda Z: Z[..., 1] - 1.0]
    pe = qLogNParEGO(_Model(), Xb, scalarization_weights=w, sampler=_Sampler(), cache_root=False,
                     objective=IdentityMCMultiOutputObjective(outcomes=[0, 2]), constraints=cons)
    assert pe.Y_baseline.shape == (6, 2) and pe.scalarization_weights is w
    torch.testing.assert_close(pe.Y_baseline, _Posterior(Xb).mean[:, [0, 2]])
    nei = qLogNoisyExpectedImprovement(
        _Model(), Xb, sampler=_Sampler(), cache_root=False, constraints=cons,
        objective=GenericMCObjective(lambda Y, X=None: pe.chebyshev_scalarization(Y[..., [0, 2]])))
    torch.testing.assert_close(pe(X), nei(X), rtol=0, atol=0)
    drawn = qLogNParEGO(_Model(), Xb, sampler=_Sampler(), cache_root=False)
    assert drawn.scalarization_weights.shape == (3,) and (drawn.scalarization_weights >= 0).all()
    pe.cheb_route = "fused"  # CPU tensors are not on the fused route
    with pytest.raises(UnsupportedError, match="cheb_route"):
        pe(X)
    bayes = _Model()
    bayes._is_fully_bayesian = True
    with pytest.raises(UnsupportedError, match="fully Bayesian"):
        qLogNParEGO(bayes, Xb, sampler=_Sampler(), cache_root=False)
