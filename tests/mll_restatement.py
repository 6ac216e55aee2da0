"""The exact marginal log likelihood restated in torch fp64 on the host: the
oracle of the MLL kernel tests (bo_mll_terms, fit.mll_terms,
fit.mll_value_and_grad).

Data term, for a constant mean c, a stationary kernel k with per-dimension
lengthscales, outputscale o and noise s2 (a scalar, or an n-vector of observed
variances for a fixed-noise likelihood):
  A  = o k(X, X) + diag(s2)
  ll = log N(y | c, A) = -1/2 (y-c)^T A^{-1} (y-c) - 1/2 log|A| - n/2 log 2 pi
  k  = exp(-r^2/2)                                   (RBF)
  k  = (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)         (Matern-5/2)
  r^2_ik = sum_j ((x_ij - x_kj) / ls_j)^2.

Two formulations that share nothing but the pairwise differences:
  ll_autograd  Cholesky, triangular solve, sum of the log diagonal; the
               gradient from torch.autograd.grad.
  ll_closed    A^{-1} from torch.linalg.inv, the value through slogdet, the
               gradient in closed form with alpha = A^{-1}(y-c) and
               W = alpha alpha^T - A^{-1}:
                 d/ds2   = 1/2 tr W            d/dc = sum alpha
                 d/dls_j = 1/2 o sum_ik W_ik g_ik Delta_ikj^2 / ls_j^3
                 d/do    = 1/2 sum_ik W_ik k_ik
               with g = k (RBF), g = 5/3 (1 + sqrt5 r) exp(-sqrt5 r) (Matern).
Both return (ll, grad) with grad in the order [noise, constant, ls_1..d,
outputscale].  For an n-vector of noises the first entry is the derivative
with respect to a common shift of all of them (1/2 tr W).

neg_mll_general is the loss of the fit's closure, -(ll + log priors) / n, with
a LogNormal prior on the lengthscales and on the noise only where one is given
(the noise prior never with fixed noise; no outputscale prior).

Nothing here is shared with the package or with oracle/."""
import math

import numpy as np
import torch

F64 = torch.float64
RBF, MATERN52 = 0, 1
SQRT5 = math.sqrt(5.0)


def _scaled_diffs(X, ls):
    """(x_i - x_k) / ls, n x n x d, from the differences themselves (no
    quadratic expansion: coincident rows give exactly 0)."""
    return (X.unsqueeze(1) - X.unsqueeze(0)) / ls


def _unit_kernel(X, ls, kind):
    r2 = _scaled_diffs(X, ls).pow(2).sum(-1)
    if kind == RBF:
        return torch.exp(-0.5 * r2)
    # sqrt behind a guard: d sqrt(r2) at r2 = 0 is infinite and autograd would
    # turn the coincident pairs' zero contribution into NaN
    pos = r2 > 0
    r = torch.where(pos, torch.where(pos, r2, torch.ones_like(r2)).sqrt(), torch.zeros_like(r2))
    return (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * torch.exp(-SQRT5 * r)


def _as_f64(v):
    return v.detach().to(F64).clone() if torch.is_tensor(v) else torch.tensor(float(v), dtype=F64)


def data_term(X, y, ls, noise, c, o, kind):
    """ll as a differentiable torch scalar (Cholesky formulation).  ``noise``:
    a 0-d tensor / float, or an n-vector."""
    n = X.shape[0]
    noise = torch.as_tensor(noise, dtype=F64)
    A = o * _unit_kernel(X, ls, kind) + torch.diag(noise.expand(n) if noise.dim() == 0 else noise)
    L = torch.linalg.cholesky(A)
    v = torch.linalg.solve_triangular(L, (y - c).unsqueeze(-1), upper=False)
    return -0.5 * (v * v).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)


def ll_autograd(X, y, ls, noise, c, o, kind):
    X, y = X.to(F64), y.to(F64)
    ls_t = _as_f64(ls).reshape(-1).requires_grad_(True)
    c_t = _as_f64(c).requires_grad_(True)
    o_t = _as_f64(o).requires_grad_(True)
    nz = _as_f64(noise)
    if nz.dim() == 0:
        nz.requires_grad_(True)
        ll = data_term(X, y, ls_t, nz, c_t, o_t, kind)
        wrt = nz
    else:  # fixed noise: the derivative with respect to a common shift
        wrt = torch.zeros((), dtype=F64, requires_grad=True)
        ll = data_term(X, y, ls_t, nz + wrt, c_t, o_t, kind)
    gn, gc, gl, go = torch.autograd.grad(ll, [wrt, c_t, ls_t, o_t])
    grad = np.concatenate([[gn.item(), gc.item()], gl.numpy(), [go.item()]])
    return ll.item(), grad


def ll_closed(X, y, ls, noise, c, o, kind):
    with torch.no_grad():
        X, y = X.to(F64), y.to(F64)
        ls, nz = _as_f64(ls).reshape(-1), _as_f64(noise)
        c, o = float(c), float(o)
        n = X.shape[0]
        D2 = (X.unsqueeze(1) - X.unsqueeze(0)).pow(2)        # Delta^2, n x n x d
        r2 = (D2 / ls.pow(2)).sum(-1)
        if kind == RBF:
            kbar = torch.exp(-0.5 * r2)
            g = kbar
        else:
            r = r2.sqrt()
            e = torch.exp(-SQRT5 * r)
            kbar = (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * e
            g = (5.0 / 3.0) * (1.0 + SQRT5 * r) * e
        A = o * kbar + torch.diag(nz.expand(n) if nz.dim() == 0 else nz)
        Ainv = torch.linalg.inv(A)
        Ainv = 0.5 * (Ainv + Ainv.T)
        res = y - c
        alpha = Ainv @ res
        sign, logabsdet = torch.linalg.slogdet(A)
        assert sign.item() > 0
        ll = -0.5 * (res @ alpha) - 0.5 * logabsdet - 0.5 * n * math.log(2 * math.pi)
        W = torch.outer(alpha, alpha) - Ainv
        g_ls = 0.5 * o * torch.einsum("ik,ikj->j", W * g, D2) / ls.pow(3)
        grad = np.concatenate([[0.5 * torch.trace(W).item(), alpha.sum().item()], g_ls.numpy(),
                               [0.5 * (W * kbar).sum().item()]])
        return ll.item(), grad


def lognormal_log_prob(x, loc, scale):
    lx = torch.log(x)
    return -((lx - loc) ** 2) / (2 * scale ** 2) - math.log(scale) - 0.5 * math.log(2 * math.pi) - lx


def neg_mll_general(X, y, ls, noise, c, o, kind, ls_prior=None, noise_prior=None):
    """-(ll + log priors) / n as a differentiable torch scalar.  ``ls_prior`` /
    ``noise_prior``: (loc, scale) of a LogNormal, or None; the noise prior is
    applied only to a scalar (learned) noise."""
    n = X.shape[0]
    noise = torch.as_tensor(noise, dtype=F64)
    total = data_term(X.to(F64), y.to(F64), ls, noise, c, o, kind)
    if ls_prior is not None:
        total = total + lognormal_log_prob(ls, *ls_prior).sum()
    if noise_prior is not None and noise.dim() == 0:
        total = total + lognormal_log_prob(noise, *noise_prior)
    return -total / n


def neg_mll_flat(x, X, y, kind, noise_vec=None, has_os=True, ls_prior=None, noise_prior=None):
    """neg_mll_general and its gradient over the fit's flat vector: [noise,]
    constant, ls_1..d [, outputscale] (no noise entry with ``noise_vec``, no
    outputscale entry without ``has_os``: outputscale 1)."""
    d = X.shape[1]
    t = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    off = 0 if noise_vec is not None else 1
    noise = noise_vec if noise_vec is not None else t[0]
    o = t[off + 1 + d] if has_os else torch.tensor(1.0, dtype=F64)
    loss = neg_mll_general(X, y, t[off + 1:off + 1 + d], noise, t[off], o, kind, ls_prior,
                           noise_prior)
    (g,) = torch.autograd.grad(loss, t)
    return loss.item(), g.numpy()


# ---- the case grid shared by the host and device tests ----------------------------------------
KINDS = (RBF, MATERN52)
DIMS = (1, 6, 7, 8, 9, 50, 64)
SIZES = (1, 2, 65, 257, 300)
OUTPUTSCALES = (1.0, 1.7)
CONSTANT = 0.3


def make_case(d, n, vector_noise, seed=0):
    """(X, y, ls, noise): X ~ U[0,1]^d with the last row equal to the first
    when n >= 65 (one coincident pair), distinct lengthscales
    (0.3 + 0.7 u) sqrt(d), a standardised smooth-plus-noise y, and a scalar
    noise 2e-2 or per-point noises in [1e-2, 3e-2]."""
    g = torch.Generator().manual_seed(1000 * d + n + 7919 * seed)
    X = torch.rand(n, d, generator=g, dtype=F64)
    if n >= 65:
        X[-1] = X[0]
    ls = (0.3 + 0.7 * torch.rand(d, generator=g, dtype=F64)) * math.sqrt(d)
    w = torch.rand(d, generator=g, dtype=F64)
    y = torch.sin(3.0 * X[:, 0]) + (X * w).sum(-1) / math.sqrt(d) \
        + 0.1 * torch.randn(n, generator=g, dtype=F64)
    if n > 1:
        y = (y - y.mean()) / y.std()
    nv = 1e-2 + 2e-2 * torch.rand(n, generator=g, dtype=F64)
    return X, y, ls, (nv if vector_noise else 2e-2)
