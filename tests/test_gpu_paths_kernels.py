"""kernels.paths_eval / kernels.paths_eval_backward (bo_paths_eval_v,
bo_paths_eval_backward_v) alone, against the torch restatement of the
definition (tests/pathwise_restatement.py) and CPU autograd through it for dX.

Omega, W, V and ``dout`` are random with mixed signs.  The kernel takes compact
arrays (it has no padded storage of its own), so every input is a window of a
larger buffer filled with NaN: a read outside an array, which is how a tiling
error shows, reaches the outputs, and these must be finite.  A second call is
bit-identical to the first (no atomics).  Bound (the project's
kernel-against-torch bound): max|got - ref| <= 1e-9 max|ref| + 1e-10.

Shapes: the smallest at which the tiling can go wrong -- d on both sides of the
16-column tiles of dX (1, 6, 9, 16, 17, 20, 33) and of the two-wave workgroup
(d > 64: 70, 128); n and M / 2 below, at and above the 16-feature step (0, 1,
17, 128, 130; M = 2, 64, 130); S around the 16-path tile and the 64-path
workgroup (1, 3, 16, 17, 70); R around the 16-row wave tile and past one
workgroup (1, 15, 16, 257)."""
import pytest
import torch

from tests import pathwise_restatement as pr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
RBF, M52 = pr.RBF, pr.MATERN52
#         kind, d,   n,   M,   S,  R
ALL = [(RBF, 1, 0, 2, 1, 1), (RBF, 6, 17, 64, 3, 15), (M52, 6, 130, 130, 16, 257),
       (RBF, 9, 128, 64, 17, 16), (M52, 20, 1, 130, 17, 257), (RBF, 20, 130, 2, 16, 16),
       (RBF, 6, 17, 64, 70, 33), (M52, 16, 17, 64, 3, 40), (RBF, 17, 17, 64, 3, 40),
       (RBF, 33, 17, 64, 3, 40), (M52, 70, 17, 64, 3, 40), (RBF, 128, 130, 130, 17, 70)]
#         kind, d,   n,   M,   S,  R, inner
MAPPED = [(RBF, 1, 0, 2, 1, 1, 1), (RBF, 6, 17, 64, 3, 15, 1), (RBF, 6, 17, 64, 3, 15, 5),
          (M52, 9, 130, 130, 16, 256, 1), (M52, 9, 130, 130, 16, 256, 16),
          (M52, 20, 128, 64, 17, 255, 15), (RBF, 20, 1, 130, 17, 257, 1),
          (RBF, 70, 17, 2, 3, 16, 1), (M52, 128, 17, 64, 1, 33, 33)]


def _bound(got, ref, what):
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got - ref).abs().max().item()
    lim = 1e-9 * ref.abs().max().item() + 1e-10
    print(f"{what}: max err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def _window(t):
    """t on the device as a window of a NaN buffer (64 doubles before and after)."""
    buf = torch.full((t.numel() + 128,), float("nan"), dtype=F64, device=DEV)
    buf[64:64 + t.numel()] = t.reshape(-1).to(DEV)
    return buf[64:64 + t.numel()].view(t.shape)


def _inputs(kind, d, n, M, S, R, inner, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    a = dict(X=torch.rand(R, d, generator=g, dtype=F64),
             Xt=torch.rand(n, d, generator=g, dtype=F64),
             ls=0.3 + 0.7 * torch.rand(d, generator=g, dtype=F64),
             Omega=rnd(M // 2, d), W=rnd(S, M), V=rnd(S, n),
             dout=rnd(R) if inner else rnd(S, R))
    a.update(o=1.7, c=0.3, ymean=-0.4, ystd=2.5)
    return a


def _reference(kind, a, inner):
    X = a["X"].clone().requires_grad_(True)
    args = (a["Xt"], a["ls"], a["o"], a["c"], a["ymean"], a["ystd"], a["Omega"], a["W"], a["V"])
    f = pr.mapped_values(kind, X, inner, *args) if inner else pr.path_values(kind, X, *args)
    (f * a["dout"]).sum().backward()
    return f.detach(), X.grad


def _check(kind, d, n, M, S, R, inner):
    from botorch_amd import kernels, ops  # noqa: F401
    a = _inputs(kind, d, n, M, S, R, inner, seed=d + 7 * n + M + 3 * S + R)
    ref, dref = _reference(kind, a, inner)
    X = _window(a["X"]).requires_grad_(True)
    dev = {k: _window(a[k]) for k in ("ls", "Omega", "W", "dout")}
    Xts = _window(a["Xt"] / a["ls"]) if n else None
    V = _window(a["V"]) if n else None
    consts = (kind, a["o"], a["c"], a["ymean"], a["ystd"], inner)
    out = torch.ops.bo.paths_eval(X, dev["ls"], dev["Omega"], dev["W"], Xts, V, *consts)
    assert tuple(out.shape) == ((R,) if inner else (S, R))
    (out * dev["dout"]).sum().backward()
    tag = f"kind={kind} d={d} n={n} M={M} S={S} R={R} inner={inner}"
    _bound(out.detach().cpu(), ref, f"out  {tag}")
    _bound(X.grad.cpu(), dref, f"dX   {tag}")
    # the kernel-level wrappers, twice: bit-identical
    Xd = X.detach()
    for _ in range(2):
        o2 = kernels.paths_eval(Xd, dev["ls"], dev["Omega"], dev["W"], Xts, V, *consts)
        g2 = kernels.paths_eval_backward(dev["dout"], Xd, dev["ls"], dev["Omega"], dev["W"], Xts,
                                         V, kind, a["o"], a["ystd"], inner)
        assert torch.equal(o2, out.detach()) and torch.equal(g2, X.grad)


@pytest.mark.parametrize("kind,d,n,M,S,R", ALL)
def test_paths_eval_all(kind, d, n, M, S, R):
    _check(kind, d, n, M, S, R, 0)


@pytest.mark.parametrize("kind,d,n,M,S,R,inner", MAPPED)
def test_paths_eval_mapped(kind, d, n, M, S, R, inner):
    _check(kind, d, n, M, S, R, inner)


def test_paths_eval_refuses_bad_arguments():
    from botorch_amd import kernels
    z = lambda *s: torch.zeros(*s, dtype=F64, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="even"):
        kernels.paths_eval(z(4, 3), z(3), z(1, 3), z(2, 3), None, None)
    with pytest.raises(ValueError, match="d <= 128"):
        kernels.paths_eval(z(4, 129), z(129), z(1, 129), z(2, 2), None, None)
    with pytest.raises(ValueError, match="go together"):
        kernels.paths_eval(z(4, 3), z(3), z(1, 3), z(2, 2), z(5, 3), None)
    with pytest.raises(ValueError, match="dout must be"):
        kernels.paths_eval_backward(z(4), z(4, 3), z(3), z(1, 3), z(2, 2), None, None)
