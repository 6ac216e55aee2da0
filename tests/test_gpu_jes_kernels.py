"""kernels.jes / kernels.jes_backward (bo_jes_v, bo_jes_backward_v) alone,
against the torch restatement of the definition (tests/jes_restatement.py) and
CPU autograd through it for dX, dmu and dvar.

The inputs come from a real GP (random data with noise 0.25, optima a little
above -- for w = -1 below -- every current posterior mean, which keeps z
between -3.2 and 22 and every pair off the clamps) and ``dout`` is random with
mixed signs.  The kernel takes compact arrays, so every
input is a window of a larger buffer filled with NaN: a read outside an array,
which is how a tiling error shows, reaches the outputs, and these must be
finite.  A second call is bit-identical to the first (no atomics).  Bound (the
project's kernel-against-torch bound): max|got - ref| <= 1e-9 max|ref| + 1e-10.

Shapes: the smallest at which the tiling can go wrong -- d on both sides of the
16-column tiles of dX and of the workgroup geometries (1, 6, 17, 40, 128: one,
two, four and eight tiles; two-wave workgroups past 32 backward and past 64
forward); n below, at and above the 16-point step (0, 1, 17, 130); P around the
16-optimum tile and the 64-optimum pass (1, 3, 16, 17, 70); R around the 16-row
wave tile and past one workgroup (1, 15, 16, 17, 33, 257).

The gradient cases assert on the restatement that no (i, j) pair sits on a
clamp.  The clamp case (values only) puts pairs on the floors of Phi and of
s2.  The floor of the inner term cannot be reached by any input: with Phi
through erfc, 1 - (z + r) r is the variance of a unit normal truncated at z,
which stays above 0.026 down to the z where Phi meets its floor (-5.61) and
exceeds 1 below it (there r < -z); the test asserts that on a grid of z."""
import math

import pytest
import torch

from tests import jes_restatement as jr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
RBF, M52 = jr.RBF, jr.MATERN52
#        kind, w,   d,   n,   P,   R
CASES = [(RBF, 1.0, 1, 0, 1, 1), (M52, -1.0, 6, 17, 3, 15), (RBF, -1.0, 6, 130, 16, 16),
         (M52, 1.0, 17, 1, 17, 17), (RBF, 1.0, 6, 130, 70, 257), (M52, -1.0, 128, 17, 17, 33),
         (RBF, 1.0, 128, 130, 70, 17), (M52, 1.0, 17, 130, 70, 33), (RBF, -1.0, 40, 17, 3, 33)]


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


def _inputs(kind, w, d, n, P, R, seed, noise=0.25):
    g = torch.Generator().manual_seed(seed)
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    y = torch.randn(n, generator=g, dtype=F64)
    ls = (0.3 + 0.7 * torch.rand(d, generator=g, dtype=F64)) * math.sqrt(d)
    gp = jr.make_gp(Xt, y, ls, noise, const=0.3, kind=kind, o=1.7)
    Xo = torch.rand(P, d, generator=g, dtype=F64)
    X = torch.rand(R, d, generator=g, dtype=F64)
    with torch.no_grad():
        mu = gp.const + jr.kernel(X, Xt, ls, kind, gp.o) @ gp.alpha
        Kx = jr.kernel(X, Xt, ls, kind, gp.o)
        var = gp.o - ((Kx * jr.solve(gp, Kx.mT).mT).sum(-1) if n else 0.0) + torch.zeros(R, dtype=F64)
        m_o = gp.const + jr.kernel(Xo, Xt, ls, kind, gp.o) @ gp.alpha
        top = w * torch.cat([w * mu, w * m_o]).max()
        f = top + w * (0.5 + torch.rand(P, generator=g, dtype=F64))
    opt = jr.make_optima(gp, Xo, f)
    dout = torch.randn(R, generator=g, dtype=F64)
    return gp, opt, X, mu, var, dout


def _device_args(gp, opt, X, mu, var, w):
    n = gp.Xt.shape[0]
    return dict(X=_window(X), mu=_window(mu), var=_window(var), ls=_window(gp.ls),
                Xts=_window(gp.Xt / gp.ls) if n else None, Xos=_window(opt.Xo / gp.ls),
                V=_window(opt.V) if n else None, g=_window(opt.g), sinv=_window(1.0 / opt.s),
                wf=_window(w * opt.f), tau2=_window(opt.tau2))


def _op(a, kind, o, w):
    return torch.ops.bo.jes(a["X"], a["mu"], a["var"], a["ls"], a["Xts"], a["Xos"], a["V"],
                            a["g"], a["sinv"], a["wf"], a["tau2"], kind, o, w)


def _kernels_twice(a, kind, o, w, dout, out, grads):
    from botorch_amd import kernels
    rest = (a["ls"], a["Xts"], a["Xos"], a["V"], a["g"], a["sinv"], a["wf"], a["tau2"],
            a["mu"].detach(), a["var"].detach(), kind, o, w)
    for _ in range(2):
        o2 = kernels.jes(a["X"].detach(), *rest)
        assert torch.equal(o2, out)
        if grads is not None:
            g2 = kernels.jes_backward(dout, a["X"].detach(), *rest)
            assert all(torch.equal(x, y) for x, y in zip(g2, grads))


@pytest.mark.parametrize("kind,w,d,n,P,R", CASES)
def test_jes_forward_and_backward(kind, w, d, n, P, R):
    from botorch_amd import ops  # noqa: F401
    gp, opt, X, mu, var, dout = _inputs(kind, w, d, n, P, R, seed=d + 7 * n + 3 * P + R)
    Xr, mur, varr = (t.clone().requires_grad_(True) for t in (X, mu, var))
    ch = jr.conditional_entropy(gp, opt, Xr, mur, varr, w)
    assert not (ch.on_s2 | ch.on_phi | ch.on_inner).any(), "a reference pair sits on a clamp"
    print(f"z in [{ch.z.min().item():.2f}, {ch.z.max().item():.2f}]")
    dXr, dmur, dvarr = torch.autograd.grad((ch.H * dout).sum(), (Xr, mur, varr))
    assert dXr.abs().max() > 0 or P * R == 1

    a = _device_args(gp, opt, X, mu, var, w)
    for k in ("X", "mu", "var"):
        a[k].requires_grad_(True)
    dd = _window(dout)
    out = _op(a, kind, gp.o, w)
    assert tuple(out.shape) == (R,)
    dX, dmu, dvar = torch.autograd.grad((out * dd).sum(), (a["X"], a["mu"], a["var"]))
    tag = f"kind={kind} w={w} d={d} n={n} P={P} R={R}"
    _bound(out.detach().cpu(), ch.H.detach(), f"H    {tag}")
    _bound(dX.cpu(), dXr, f"dX   {tag}")
    _bound(dmu.cpu(), dmur, f"dmu  {tag}")
    _bound(dvar.cpu(), dvarr, f"dvar {tag}")
    _kernels_twice(a, kind, gp.o, w, dd, out.detach(), (dX, dmu, dvar))


def test_jes_values_on_the_clamps():
    """Values only.  Optimum 0 sits on a training point of a GP with noise
    1e-11 and row 0 of X on it too (s2 = v nu / (v + nu) < 1e-10 under
    condition_noiseless); optimum 1 lies 50 below every posterior mean (Phi <
    1e-8)."""
    from botorch_amd import ops  # noqa: F401
    kind, w, d, n, P, R = RBF, 1.0, 6, 17, 5, 20
    gp, opt, X, mu, var, _ = _inputs(kind, w, d, n, P, R, seed=5, noise=1e-11)
    Xo = opt.Xo.clone()
    Xo[0] = gp.Xt[0]
    X = X.clone()
    X[0] = gp.Xt[0]
    f = opt.f.clone()
    f[1] = mu.min() - 50.0
    opt = jr.make_optima(gp, Xo, f)
    mu_all, Sigma = jr.posterior(gp, X)
    mu, var = mu_all, Sigma.diagonal().clone()
    ch = jr.conditional_entropy(gp, opt, X, mu, var, w)
    assert ch.on_s2[0, 0] and ch.on_phi[:, 1].all()
    assert not (ch.on_s2 | ch.on_phi)[1:, 2:].all()  # and pairs off every clamp
    # the floor of the inner term is out of reach of any z
    z = torch.linspace(-40.0, 40.0, 160001, dtype=F64)
    zc = jr.chain(torch.zeros(z.numel(), 1, dtype=F64), -z, torch.ones_like(z),
                  torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64), torch.zeros(1, dtype=F64),
                  torch.zeros(1, dtype=F64))
    assert torch.equal(zc.z.squeeze(-1), z) and not zc.on_inner.any() and zc.on_phi.any()
    assert zc.vt.min() > 0.026
    a = _device_args(gp, opt, X, mu, var, w)
    out = _op(a, kind, gp.o, w)
    _bound(out.cpu(), ch.H, "H on the clamps")
    _kernels_twice(a, kind, gp.o, w, None, out, None)


def test_jes_refuses_bad_arguments():
    from botorch_amd import kernels
    z = lambda *s: torch.zeros(*s, dtype=F64, device=DEV)  # noqa: E731
    ok = lambda d, P, R: (z(R, d), z(d), None, z(P, d), None, z(P), z(P), z(P), z(P), z(R), z(R))  # noqa: E731
    with pytest.raises(ValueError, match="d <= 128"):
        kernels.jes(*ok(129, 2, 4))
    with pytest.raises(ValueError, match="P >= 1"):
        kernels.jes(*ok(3, 0, 4))
    with pytest.raises(ValueError, match="R >= 1"):
        kernels.jes(*ok(3, 2, 0))
    with pytest.raises(ValueError, match="go together"):
        args = list(ok(3, 2, 4))
        args[2] = z(5, 3)
        kernels.jes(*args)
    with pytest.raises(ValueError, match="dout must be"):
        kernels.jes_backward(z(3), *ok(3, 2, 4))
