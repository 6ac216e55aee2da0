"""The multi-task GP with the intrinsic coregionalisation kernel restated in torch
fp64 on the host: the oracle of the MultiTaskGP tests (bo_icm_covar,
bo_icm_mll_terms, bo_icm_task_view, MultiTaskGP.posterior, the fit).

Model, for training points (x_i, tau_i), tau_i in 0..T-1:
  A  = o kbar(X, X) * B[tau, tau] + diag(s2),   B = F F^T + diag(v)
  ll = log N(y | c, A)
with kbar the unit-outputscale RBF / Matern-5/2 kernel of tests/mll_restatement.py.

  ll_autograd        Cholesky, triangular solve, log diagonal; torch.autograd.
  ll_closed          A^{-1} from torch.linalg.inv, slogdet, and the closed form
                     with W = alpha alpha^T - A^{-1}:
                       G[a,b]  = sum_{i,k: tau_i = a, tau_k = b} W_ik o kbar_ik
                       d/dF    = 1/2 (G + G^T) F        d/dv = 1/2 diag(G)
                       d/ds2   = 1/2 tr W               d/dc = sum alpha
                       d/dls_j = 1/2 o sum W_ik B_ik g_ik Delta_ikj^2 / ls_j^3
                       d/do    = 1/2 sum W_ik kbar_ik B_ik
  posterior_explicit an ordinary exact GP over (x, task) pairs with the product
                     kernel (no task view, no scaling identity).
Gradients are ordered [noise, constant, ls_1..d, outputscale, F (row-major), v].
neg_mll_flat is the fit's loss -(ll + log priors) / n over its flat vector.

Nothing here is shared with the package or with oracle/."""
import math

import numpy as np
import torch

F64 = torch.float64
RBF, MATERN52 = 0, 1
SQRT5 = math.sqrt(5.0)
CONSTANT = 0.3
OUTPUTSCALE = 1.7


def unit_kernel(X1, X2, ls, kind):
    """kbar(X1, X2) from the differences themselves (coincident rows give exactly 1)."""
    r2 = ((X1.unsqueeze(-2) - X2.unsqueeze(-3)) / ls).pow(2).sum(-1)
    if kind == RBF:
        return torch.exp(-0.5 * r2)
    pos = r2 > 0  # sqrt behind a guard: its derivative at 0 is infinite
    r = torch.where(pos, torch.where(pos, r2, torch.ones_like(r2)).sqrt(), torch.zeros_like(r2))
    return (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * torch.exp(-SQRT5 * r)


def task_covar(F, v):
    return F @ F.T + torch.diag(v)


def train_covar(X, task, ls, noise, o, B, kind):
    n = X.shape[0]
    noise = torch.as_tensor(noise, dtype=F64)
    return o * unit_kernel(X, X, ls, kind) * B[task][:, task] \
        + torch.diag(noise.expand(n) if noise.dim() == 0 else noise)


def data_term(X, task, y, ls, noise, c, o, F, v, kind):
    n = X.shape[0]
    A = train_covar(X, task, ls, noise, o, task_covar(F, v), kind)
    L = torch.linalg.cholesky(A)
    w = torch.linalg.solve_triangular(L, (y - c).unsqueeze(-1), upper=False)
    return -0.5 * (w * w).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)


def _t(v):
    return v.detach().to(F64).clone() if torch.is_tensor(v) else torch.tensor(float(v), dtype=F64)


def ll_autograd(X, task, y, ls, noise, c, o, F, v, kind):
    X, y = X.to(F64), y.to(F64)
    ls_t, c_t, o_t = (_t(ls).reshape(-1).requires_grad_(True), _t(c).requires_grad_(True),
                      _t(o).requires_grad_(True))
    F_t, v_t = _t(F).requires_grad_(True), _t(v).requires_grad_(True)
    nz = _t(noise)
    if nz.dim() == 0:
        wrt = nz.requires_grad_(True)
        ll = data_term(X, task, y, ls_t, wrt, c_t, o_t, F_t, v_t, kind)
    else:  # fixed noise: the derivative with respect to a common shift
        wrt = torch.zeros((), dtype=F64, requires_grad=True)
        ll = data_term(X, task, y, ls_t, nz + wrt, c_t, o_t, F_t, v_t, kind)
    gn, gc, gl, go, gF, gv = torch.autograd.grad(ll, [wrt, c_t, ls_t, o_t, F_t, v_t])
    grad = np.concatenate([[gn.item(), gc.item()], gl.numpy(), [go.item()], gF.reshape(-1).numpy(),
                           gv.numpy()])
    return ll.item(), grad


def task_sums(X, task, y, ls, noise, c, o, F, v, kind):
    """G (T x T) of the closed form."""
    with torch.no_grad():
        T = F.shape[0]
        A = train_covar(X, task, _t(ls).reshape(-1), _t(noise), float(o), task_covar(F, v), kind)
        Ainv = torch.linalg.inv(A)
        Ainv = 0.5 * (Ainv + Ainv.T)
        alpha = Ainv @ (y - c)
        W = torch.outer(alpha, alpha) - Ainv
        E = torch.nn.functional.one_hot(task, T).to(F64)
        return float(o) * (E.T @ (W * unit_kernel(X, X, _t(ls).reshape(-1), kind)) @ E)


def ll_closed(X, task, y, ls, noise, c, o, F, v, kind):
    with torch.no_grad():
        X, y = X.to(F64), y.to(F64)
        ls, nz, F, v = _t(ls).reshape(-1), _t(noise), _t(F), _t(v)
        c, o = float(c), float(o)
        n, T = X.shape[0], F.shape[0]
        D2 = (X.unsqueeze(1) - X.unsqueeze(0)).pow(2)
        r2 = (D2 / ls.pow(2)).sum(-1)
        if kind == RBF:
            kbar = torch.exp(-0.5 * r2)
            g = kbar
        else:
            r = r2.sqrt()
            e = torch.exp(-SQRT5 * r)
            kbar = (1.0 + SQRT5 * r + (5.0 / 3.0) * r2) * e
            g = (5.0 / 3.0) * (1.0 + SQRT5 * r) * e
        Bik = task_covar(F, v)[task][:, task]
        A = o * kbar * Bik + torch.diag(nz.expand(n) if nz.dim() == 0 else nz)
        Ainv = torch.linalg.inv(A)
        Ainv = 0.5 * (Ainv + Ainv.T)
        res = y - c
        alpha = Ainv @ res
        sign, logabsdet = torch.linalg.slogdet(A)
        assert sign.item() > 0
        ll = -0.5 * (res @ alpha) - 0.5 * logabsdet - 0.5 * n * math.log(2 * math.pi)
        W = torch.outer(alpha, alpha) - Ainv
        E = torch.nn.functional.one_hot(task, T).to(F64)
        G = o * (E.T @ (W * kbar) @ E)
        g_ls = 0.5 * o * torch.einsum("ik,ikj->j", W * g * Bik, D2) / ls.pow(3)
        grad = np.concatenate([[0.5 * torch.trace(W).item(), alpha.sum().item()], g_ls.numpy(),
                               [0.5 * (W * kbar * Bik).sum().item()],
                               (0.5 * (G + G.T) @ F).reshape(-1).numpy(),
                               0.5 * torch.diagonal(G).numpy()])
        return ll.item(), grad, G


def posterior_explicit(X, task, y, ls, noise, c, o, B, kind, Xq, tq):
    """Mean (.. x q) and covariance (.. x q x q) of the latent function at the
    points (Xq, tq): an exact GP over (x, task) pairs, k = o kbar(x, x') B[t, t'].
    Differentiable in Xq."""
    A = train_covar(X, task, ls, noise, o, B, kind)
    Ks = o * unit_kernel(Xq, X, ls, kind) * B[tq][..., task]              # .. x q x n
    Kss = o * unit_kernel(Xq, Xq, ls, kind) * B[tq.unsqueeze(-1), tq.unsqueeze(-2)]
    L = torch.linalg.cholesky(A)
    alpha = torch.cholesky_solve((y - c).unsqueeze(-1), L).squeeze(-1)
    V = torch.linalg.solve_triangular(L, Ks.mT, upper=False)              # .. x n x q
    return c + Ks @ alpha, Kss - V.mT @ V


def gamma_log_prob(x, concentration, rate):
    return (concentration * math.log(rate) + (concentration - 1.0) * torch.log(x) - rate * x
            - math.lgamma(concentration))


LS_PRIOR, OS_PRIOR, NOISE_PRIOR = (3.0, 6.0), (2.0, 0.15), (1.1, 0.05)


def neg_mll_flat(x, X, task, y, kind, T, rank, noise_vec=None, ls_prior=LS_PRIOR,
                 os_prior=OS_PRIOR, noise_prior=NOISE_PRIOR):
    """-(ll + log priors) / n and its gradient over the fit's flat vector: [noise,]
    constant, ls_1..d, outputscale, F (row-major), v, with Gamma priors on the
    lengthscales, the outputscale and a learned noise (None: no such prior)."""
    n, d = X.shape
    t = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    off = 0 if noise_vec is not None else 1
    noise = noise_vec if noise_vec is not None else t[0]
    ls, o = t[off + 1:off + 1 + d], t[off + 1 + d]
    f0 = off + 2 + d
    F, v = t[f0:f0 + T * rank].reshape(T, rank), t[f0 + T * rank:]
    total = data_term(X.to(F64), task, y.to(F64), ls, noise, t[off], o, F, v, kind)
    if ls_prior is not None:
        total = total + gamma_log_prob(ls, *ls_prior).sum()
    if os_prior is not None:
        total = total + gamma_log_prob(o, *os_prior)
    if noise_prior is not None and noise_vec is None:
        total = total + gamma_log_prob(noise, *noise_prior)
    loss = -total / n
    (g,) = torch.autograd.grad(loss, t)
    return loss.item(), g.numpy()


KINDS = (RBF, MATERN52)


def make_case(d, n, T, rank, vector_noise, seed=0, empty_tasks=()):
    """(X, task, y, ls, noise, F, v): X ~ U[0,1]^d with the last row equal to the
    first when n >= 65 (a coincident pair, in different tasks where T > 1), tasks
    dealt round-robin over the tasks that have data (``empty_tasks`` get none),
    distinct lengthscales (0.3 + 0.7 u) sqrt(d), y a smooth function plus a task
    offset plus noise, standardised; noise 0.3 or per-point in [0.2, 0.4]
    (>= 1e-2, so that cond(A) stays below 1e4 for n <= 300), F ~ 0.7 randn /
    sqrt(rank) with mixed signs and v in [0.3, 0.6]."""
    g = torch.Generator().manual_seed(100003 * d + 101 * n + 7 * T + rank + 7919 * seed)
    X = torch.rand(n, d, generator=g, dtype=F64)
    if n >= 65:
        X[-1] = X[0]
    live = [t for t in range(T) if t not in empty_tasks]
    task = torch.tensor([live[i % len(live)] for i in range(n)], dtype=torch.long)
    ls = (0.3 + 0.7 * torch.rand(d, generator=g, dtype=F64)) * math.sqrt(d)
    w = torch.rand(d, generator=g, dtype=F64)
    y = torch.sin(3.0 * X[:, 0]) + (X * w).sum(-1) / math.sqrt(d) + 0.3 * torch.cos(1.0 * task) \
        + 0.1 * torch.randn(n, generator=g, dtype=F64)
    if n > 1:
        y = (y - y.mean()) / y.std()
    nv = 0.2 + 0.2 * torch.rand(n, generator=g, dtype=F64)
    F = 0.7 * torch.randn(T, rank, generator=g, dtype=F64) / math.sqrt(rank)
    v = 0.3 + 0.3 * torch.rand(T, generator=g, dtype=F64)
    return X, task, y, ls, (nv if vector_noise else 0.3), F, v
