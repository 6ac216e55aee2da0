"""kernels.bald / kernels.bald_backward (bo_bald_v, bo_bald_backward_v) alone,
against the torch restatement of the definition (tests/bald_restatement.py) and
CPU autograd through it for dmean and dL with a random dout (not all ones, so
the mixture-entropy and the component-entropy parts are both weighted).

Means are N(0, 1) and the roots are the Cholesky factors of A A^T + I.  The
kernel takes compact arrays, so every input is a window of a larger buffer
filled with NaN: a read outside an array reaches the outputs, and these must be
finite.  A second call is bit-identical to the first (no atomics).  Bound (the
project's kernel-against-torch bound): max|got - ref| <= 1e-9 max|ref| + 1e-10.

Shapes: M on both sides of nothing-to-mix (1), small (2, 3), the bench's 16, a
ragged 17 and the limit 64; q at every padded width and just past each (1, 2,
3, 8, 9, 16); S around the wave (63, 64, 65), tiny (1, 2), ragged (130) and, as
a workgroup takes 256 samples per pass, on both sides of one and two passes
(257, 513); B with one and several workgroups per component (1, 3, 5, 17).  The
largest LDS image (M = 64, q = 16) is among them.  One case has components 40
apart: every log-density under another component is below -700, where exp
underflows and only the log-sum-exp keeps the gradient of the mixture term."""
import pytest
import torch

from tests import bald_restatement as br

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
#        M,  q,  S,   B, separation of the means
CASES = [(1, 1, 1, 1, 0.0), (2, 3, 63, 3, 0.0), (3, 16, 65, 5, 0.0), (16, 8, 64, 3, 0.0),
         (17, 9, 130, 1, 0.0), (64, 2, 65, 5, 0.0), (64, 16, 2, 1, 0.0), (2, 1, 130, 17, 0.0),
         (16, 2, 257, 3, 0.0), (3, 8, 513, 2, 0.0), (1, 9, 64, 17, 0.0), (17, 3, 63, 5, 0.0),
         (16, 4, 2, 17, 0.0), (3, 2, 64, 2, 40.0)]


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


_CACHE = {}


def _inputs(M, q, S, B, sep):
    """(mean, L, Z, dout, out_ref, dmean_ref, dL_ref) on the host, once per shape;
    mean B x M x q and L B x M x q x q as the restatement takes them."""
    key = (M, q, S, B, sep)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(M + 7 * q + 3 * S + 11 * B)
        mean = torch.randn(B, M, q, generator=g, dtype=F64)
        mean = mean + sep * torch.arange(M, dtype=F64).view(1, M, 1)
        A = torch.randn(B, M, q, q, generator=g, dtype=F64) * (0.3 if sep else 1.0)
        L = torch.linalg.cholesky(A @ A.mT + torch.eye(q, dtype=F64))
        Z = torch.randn(S, q, generator=g, dtype=F64)
        dout = torch.randn(B, M, generator=g, dtype=F64)
        mr, Lr = mean.clone().requires_grad_(True), L.clone().requires_grad_(True)
        out = br.bald_roots(mr, Lr.tril(), Z)
        dmean, dL = torch.autograd.grad((out * dout).sum(), (mr, Lr))
        _CACHE[key] = (mean, L, Z, dout, out.detach(), dmean, dL)
    return _CACHE[key]


def _rows(t):
    """B x M x ... -> the kernel's M B x ... (row m B + b)."""
    return t.transpose(0, 1).reshape(-1, *t.shape[2:]).contiguous()


def _unrows(t, M, B):
    return t.view(M, B, *t.shape[1:]).transpose(0, 1)


@pytest.mark.parametrize("M,q,S,B,sep", CASES)
def test_bald_forward(M, q, S, B, sep):
    from botorch_amd import kernels
    mean, L, Z, _, ref, _, _ = _inputs(M, q, S, B, sep)
    if sep:
        lp = br.log_densities(mean, L, Z)
        off = lp[:, :, ~torch.eye(M, dtype=torch.bool)]
        assert off.max() < -700.0, off.max()
    args = (_window(_rows(mean)), _window(_rows(L)), _window(Z), M)
    out = kernels.bald(*args)
    assert out.shape == (B, M)
    assert torch.equal(out, kernels.bald(*args))
    if M == 1:
        assert out.abs().max().item() <= 1e-10
    _bound(out.cpu(), ref, f"bald M={M} q={q} S={S} B={B} sep={sep}")


@pytest.mark.parametrize("M,q,S,B,sep", CASES)
def test_bald_backward(M, q, S, B, sep):
    from botorch_amd import kernels
    mean, L, Z, dout, _, dmean_ref, dL_ref = _inputs(M, q, S, B, sep)
    if M > 1:  # (M = 1: the gradient is exactly zero)
        assert dL_ref.abs().max() > 1e-6
        # components that do not overlap have H = log M + mean_m C_m, which no mean enters
        assert sep or dmean_ref.abs().max() > 1e-6
    assert dL_ref.triu(1).abs().max() == 0.0
    args = (_window(dout), _window(_rows(mean)), _window(_rows(L)), _window(Z), M)
    dmean, dL = kernels.bald_backward(*args)
    assert dmean.shape == (M * B, q) and dL.shape == (M * B, q, q)
    again = kernels.bald_backward(*args)
    assert torch.equal(dmean, again[0]) and torch.equal(dL, again[1])
    assert dL.triu(1).abs().max().item() == 0.0
    what = f"M={M} q={q} S={S} B={B} sep={sep}"
    _bound(_unrows(dmean.cpu(), M, B), dmean_ref, "bald_backward dmean " + what)
    _bound(_unrows(dL.cpu(), M, B), dL_ref, "bald_backward dL " + what)


def test_bald_op_autograd_and_empty():
    """torch.ops.bo.bald under autograd gives the backward kernel's gradients;
    B = 0 returns empty results without a launch."""
    from botorch_amd import kernels, ops  # noqa: F401
    M, q, S, B, sep = CASES[1]
    mean, L, Z, dout, ref, dmean_ref, dL_ref = _inputs(M, q, S, B, sep)
    md = _rows(mean).to(DEV).requires_grad_(True)
    Ld = _rows(L).to(DEV).requires_grad_(True)
    out = torch.ops.bo.bald(md, Ld, Z.to(DEV), M)
    _bound(out.detach().cpu(), ref, "bo::bald")
    gm, gL = torch.autograd.grad((out * dout.to(DEV)).sum(), (md, Ld))
    _bound(_unrows(gm.cpu(), M, B), dmean_ref, "bo::bald dmean")
    _bound(_unrows(gL.cpu(), M, B), dL_ref, "bo::bald dL")
    e = lambda *s: torch.empty(*s, dtype=F64, device=DEV)  # noqa: E731
    assert kernels.bald(e(0, q), e(0, q, q), Z.to(DEV), M).shape == (0, M)
    dm, dl = kernels.bald_backward(e(0, M), e(0, q), e(0, q, q), Z.to(DEV), M)
    assert dm.shape == (0, q) and dl.shape == (0, q, q)
