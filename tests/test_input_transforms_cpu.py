"""Input transforms without a device: semantics, the layout of the fit, the refusals."""
import pytest
import torch

from tests import warp_restatement as ref


def _tf():
    from botorch_amd.transforms import ChainedInputTransform, Normalize, Warp
    return Normalize, Warp, ChainedInputTransform


def test_normalize_learned_given_and_min_range():
    Normalize, _, _ = _tf()
    X = torch.tensor([[1.0, 5.0, 2.0], [3.0, 5.0, 4.0], [2.0, 5.0, 10.0]], dtype=torch.float64)
    t = Normalize(3)
    Z = t(X)  # train mode: the bounds are learned; the constant column keeps offset 0, range 1
    torch.testing.assert_close(t.bounds, torch.tensor([[1.0, 0.0, 2.0], [3.0, 1.0, 10.0]],
                                                      dtype=torch.float64))
    torch.testing.assert_close(Z, torch.tensor([[0.0, 5.0, 0.0], [1.0, 5.0, 0.25], [0.5, 5.0, 1.0]],
                                               dtype=torch.float64))
    t.eval()
    t(10.0 * X)
    assert float(t.bounds[1, 0]) == 3.0  # eval mode learns nothing
    given = Normalize(3, indices=[0, 2], bounds=torch.tensor([[0.0, 0.0], [4.0, 20.0]]))
    assert not given.learn_bounds
    torch.testing.assert_close(given(X)[0], torch.tensor([0.25, 5.0, 0.1], dtype=torch.float64))
    torch.testing.assert_close(given.untransform(given(X)), X)


@pytest.mark.parametrize("a,b", [(1e-4, 8.0), (0.3, 2.5), (1.0, 1.0), (2.5, 0.3), (8.0, 1e-4)])
def test_warp_matches_reference_formula_and_inverts(a, b):
    _, Warp, _ = _tf()
    w = Warp([0, 2]).eval()
    w.concentration1, w.concentration0 = a, b
    X = torch.rand(50, 3, dtype=torch.float64)
    flag = torch.tensor([True, False, True])
    want = ref.warp_reference(X, torch.zeros(3, dtype=torch.float64),
                              torch.ones(3, dtype=torch.float64), torch.tensor(a, dtype=torch.float64),
                              torch.tensor(b, dtype=torch.float64), flag)
    Z = w(X)
    torch.testing.assert_close(Z, want, rtol=0, atol=1e-11)  # the reference's own form loses 4.8e-12
    assert torch.equal(Z[:, 1], X[:, 1])
    inside = (Z > 1e-9) & (Z < 1 - 1e-9)  # where the inverse CDF is conditioned
    torch.testing.assert_close(w.untransform(Z)[inside], X[inside], rtol=1e-6, atol=1e-9)


def test_chain_order_and_layout():
    Normalize, Warp, Chained = _tf()
    from botorch_amd import fit
    from botorch_amd.models import SingleTaskGP
    X = 4.0 * torch.rand(12, 3, dtype=torch.float64) - 1.0
    Y = X.sum(-1, keepdim=True).sin()
    tf = Chained(n=Normalize(3), w=Warp([2, 0]))
    model = SingleTaskGP(X, Y, input_transform=tf)
    assert tf.keys() == ["n", "w"] and torch.equal(model.train_inputs[0], X)
    tf["w"].concentration1 = torch.tensor([2.0, 0.5])
    tf.eval()
    torch.testing.assert_close(tf(X), tf["w"](tf["n"](X)), rtol=0, atol=1e-15)
    layout = fit._layout(model)
    assert layout.segments[-2:] == [("concentration0", 5, 2), ("concentration1", 7, 2)]
    assert layout.bounds[-4:] == [(1e-4, None)] * 4 and layout.size == 9
    buffers = [(b.data_ptr(), b._version) for b in tf["n"].buffers()]
    tf.train()
    tf(X)  # the same bounds learned again: the buffers, part of the cache key, are untouched
    assert buffers == [(b.data_ptr(), b._version) for b in tf["n"].buffers()]
    tf.eval()
    x = layout.get()
    assert x[-2:].tolist() == [2.0, 0.5] and x[-4:-2].tolist() == [1.0, 1.0]
    x[-4:] = [0.7, 0.8, 1.5, 1.6]
    key = model._key()
    layout.set(x)
    assert tf["w"].concentration0.tolist() == [0.7, 0.8] and model._key() != key
    loss, grad = fit.mll_value_and_grad(model, x, layout, sync_model=False)  # the torch route
    h = 1e-6
    for i in (2, 5, 8):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        fd = (fit.mll_value_and_grad(model, xp, layout, sync_model=False)[0]
              - fit.mll_value_and_grad(model, xm, layout, sync_model=False)[0]) / (2 * h)
        assert abs(fd - grad[i]) < 1e-6 * max(1.0, abs(fd))


def test_refusals():
    Normalize, Warp, Chained = _tf()
    import botorch_amd
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.models import MultiTaskGP, SingleTaskGP
    assert botorch_amd.Warp is Warp and "Normalize" in botorch_amd.__all__
    with pytest.raises(UnsupportedError, match="batch_shape"):
        Normalize(2, batch_shape=torch.Size([3]))
    with pytest.raises(UnsupportedError, match="batch_shape"):
        Warp([0], batch_shape=torch.Size([3]))
    with pytest.raises(UnsupportedError, match="reverse"):
        Warp([0], reverse=True)
    X, Y = torch.rand(8, 2, dtype=torch.float64), torch.rand(8, 2, dtype=torch.float64)
    with pytest.raises(UnsupportedError, match="ModelListGP"):
        SingleTaskGP(X, Y, input_transform=Warp([0]))
    with pytest.raises(UnsupportedError, match="Normalize -> Warp|in that order"):
        SingleTaskGP(X, Y[:, :1], input_transform=Chained(w=Warp([0]), n=Normalize(2)))
    norm = Normalize(2)
    multi = SingleTaskGP(X, Y, input_transform=norm)  # multi-output takes Normalize
    assert multi.input_transform is norm and multi.models[0].input_transform is norm
    with pytest.raises(UnsupportedError):
        MultiTaskGP(torch.cat([X, torch.zeros(8, 1, dtype=torch.float64)], -1), Y[:, :1],
                    task_feature=-1, input_transform=Normalize(3))
