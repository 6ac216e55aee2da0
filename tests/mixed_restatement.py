"""The mixed continuous / categorical exact GP restated in torch fp64 on the host,
from botorch/models/gp_regression_mixed.py:133-173 and models/kernels/categorical.py;
shares nothing with the package or oracle/.

  K = os (kbar(l1) + oc kap(lam1)) + op kbar(l2) kap(lam2),  kap = exp(-mean_j [c_j != c'_j] / lam_j)

A parameter set ``p`` is a dict: kind (0 RBF, 1 Matern-5/2), cont, cat (column
lists), l1, lam1, l2, lam2 (tensors), os, oc, op (0-dim tensors)."""
import math

import numpy as np
import torch

NAMES = ("l1", "lam1", "l2", "lam2", "os", "oc", "op")


def _parts(Z1, Z2, p):
    diff = Z1[..., p["cont"]].unsqueeze(-2) - Z2[..., p["cont"]].unsqueeze(-3)
    ne = (Z1[..., p["cat"]].unsqueeze(-2) != Z2[..., p["cat"]].unsqueeze(-3)).to(torch.float64)
    return diff, ne


def _kbar_g(diff, ls, kind):
    r2 = (diff / ls).pow(2).sum(-1)
    if kind == 0:
        k = torch.exp(-0.5 * r2)
        return k, k
    s5r = math.sqrt(5.0) * (r2 + 1e-300).sqrt()
    e = torch.exp(-s5r)
    return (1.0 + s5r + (5.0 / 3.0) * r2) * e, (5.0 / 3.0) * (1.0 + s5r) * e


def kernel(Z1, Z2, p):
    diff, ne = _parts(Z1, Z2, p)
    k1, _ = _kbar_g(diff, p["l1"], p["kind"])
    k2, _ = _kbar_g(diff, p["l2"], p["kind"])
    kp1 = torch.exp(-(ne / p["lam1"]).mean(-1))
    kp2 = torch.exp(-(ne / p["lam2"]).mean(-1))
    return p["os"] * (k1 + p["oc"] * kp1) + p["op"] * k2 * kp2


def _noise_matrix(noise, n):
    return torch.diag(noise) if noise.ndim else noise * torch.eye(n, dtype=torch.float64)


def ll_autograd(Z, y, p, noise, const):
    """log N(y | const, K + noise) by Cholesky and its gradient by autograd:
    (ll, {name: grad}) over NAMES, "noise" and "const"."""
    leaves = {k: p[k].clone().requires_grad_(True) for k in NAMES}
    leaves["noise"] = noise.clone().requires_grad_(True)
    leaves["const"] = torch.tensor(float(const), dtype=torch.float64, requires_grad=True)
    pp = dict(p, **{k: leaves[k] for k in NAMES})
    n = Z.shape[0]
    L = torch.linalg.cholesky(kernel(Z, Z, pp) + _noise_matrix(leaves["noise"], n))
    b = torch.linalg.solve_triangular(L, (y - leaves["const"]).unsqueeze(-1), upper=False)
    ll = -0.5 * (b * b).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)
    grads = torch.autograd.grad(ll, list(leaves.values()))
    return ll.detach(), {k: g for k, g in zip(leaves, grads)}


def ll_closed(Z, y, p, noise, const):
    """The same by linalg.inv, slogdet and the closed-form sums 1/2 sum_ik W_ik dK_ik/dtheta,
    W = alpha alpha^T - A^{-1}.  Returns (ll, grads, S, W): S[name] holds the summands
    (n x n, or n x n x dim for the lengthscales) whose total is the gradient."""
    n = Z.shape[0]
    diff, ne = _parts(Z, Z, p)
    k1, g1 = _kbar_g(diff, p["l1"], p["kind"])
    k2, g2 = _kbar_g(diff, p["l2"], p["kind"])
    dk = len(p["cat"])
    kp1 = torch.exp(-(ne / p["lam1"]).mean(-1))
    kp2 = torch.exp(-(ne / p["lam2"]).mean(-1))
    A = p["os"] * (k1 + p["oc"] * kp1) + p["op"] * k2 * kp2 + _noise_matrix(noise, n)
    Ainv = torch.linalg.inv(A)
    alpha = Ainv @ (y - const)
    W = torch.outer(alpha, alpha) - Ainv
    ll = -0.5 * (y - const) @ alpha - 0.5 * torch.linalg.slogdet(A)[1] - 0.5 * n * math.log(2 * math.pi)
    h = (0.5 * W).unsqueeze(-1)
    d2 = diff.pow(2)
    S = {"l1": h * (p["os"] * g1).unsqueeze(-1) * d2 / p["l1"] ** 3,
         "l2": h * (p["op"] * kp2 * g2).unsqueeze(-1) * d2 / p["l2"] ** 3,
         "lam1": h * (p["os"] * p["oc"] * kp1).unsqueeze(-1) * ne / (dk * p["lam1"] ** 2),
         "lam2": h * (p["op"] * k2 * kp2).unsqueeze(-1) * ne / (dk * p["lam2"] ** 2),
         "os": 0.5 * W * (k1 + p["oc"] * kp1), "oc": 0.5 * W * p["os"] * kp1,
         "op": 0.5 * W * k2 * kp2}
    grads = {k: v.sum(dim=(0, 1)) for k, v in S.items()}
    grads["noise"] = 0.5 * torch.diagonal(W) if noise.ndim else 0.5 * torch.trace(W)
    grads["const"] = alpha.sum()
    return ll, grads, S, W


def posterior_explicit(Z, y, p, noise, const, Xq):
    """An ordinary exact GP over the (x, c) rows: (mean, cov) at Xq (... x q x d)."""
    n = Z.shape[0]
    L = torch.linalg.cholesky(kernel(Z, Z, p) + _noise_matrix(noise, n))
    Kx = kernel(Xq, Z, p)
    mean = const + Kx @ torch.cholesky_solve((y - const).unsqueeze(-1), L).squeeze(-1)
    V = torch.linalg.solve_triangular(L, Kx.mT, upper=False)
    return mean, kernel(Xq, Xq, p) - V.mT @ V


def posterior_inverse(Z, y, p, noise, const, Xq):
    """The same through linalg.inv (a second reference), with sum |summand| of the mean
    and of every covariance entry: (mean, cov, mass_mean, mass_cov)."""
    Ainv = torch.linalg.inv(kernel(Z, Z, p) + _noise_matrix(noise, Z.shape[0]))
    Kx, Kxx, alpha = kernel(Xq, Z, p), kernel(Xq, Xq, p), Ainv @ (y - const)
    return (const + Kx @ alpha, Kxx - Kx @ Ainv @ Kx.mT, abs(const) + Kx.abs() @ alpha.abs(),
            Kxx.abs() + Kx.abs() @ Ainv.abs() @ Kx.abs().mT)


def neg_mll_flat(x, Z, y, kind, cont, cat, prior=(0.9, 10.0)):
    """The fit's loss over its flat vector [noise, const, l1, lam1, l2, lam2, os, oc, op]:
    -(ll + log Gamma(noise; 0.9, 10)) / n, and its gradient (numpy)."""
    t = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    dc, dk = len(cont), len(cat)
    h = t[2:]
    p = dict(kind=kind, cont=cont, cat=cat, l1=h[:dc], lam1=h[dc:dc + dk],
             l2=h[dc + dk:2 * dc + dk], lam2=h[2 * dc + dk:2 * dc + 2 * dk],
             os=h[-3], oc=h[-2], op=h[-1])
    n = Z.shape[0]
    L = torch.linalg.cholesky(kernel(Z, Z, p) + t[0] * torch.eye(n, dtype=torch.float64))
    b = torch.linalg.solve_triangular(L, (y - t[1]).unsqueeze(-1), upper=False)
    ll = -0.5 * (b * b).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)
    a, r = prior
    ll = ll + a * math.log(r) + (a - 1.0) * torch.log(t[0]) - r * t[0] - math.lgamma(a)
    loss = -ll / n
    (g,) = torch.autograd.grad(loss, t)
    return float(loss.detach()), g.numpy()


def make_case(kind, dc, dk, n, seed=0, fixed_noise=False):
    """Rows with interleaved columns (categorical first and every other), non-integer
    category values, a duplicated training row, and a parameter set with distinct
    values everywhere.  Returns (Z, y, p, noise, const)."""
    g = torch.Generator().manual_seed(1000 * seed + 37 * dc + 5 * dk + n + kind)
    d = dc + dk
    cat = [j for j in range(d) if j % 2 == 0][:dk]
    cat += [j for j in range(d) if j not in cat][:dk - len(cat)]
    cat = sorted(cat)
    cont = [j for j in range(d) if j not in cat]
    Z = torch.rand(n, d, dtype=torch.float64, generator=g)
    Z[:, cat] = torch.randint(0, 3, (n, dk), generator=g).to(torch.float64) * 0.5 + 0.25
    if n > 2:
        Z[n - 1] = Z[0]
    y = torch.sin(3.0 * Z.sum(-1)) + 0.1 * torch.randn(n, dtype=torch.float64, generator=g)
    u = lambda k, lo, hi: lo + (hi - lo) * torch.rand(k, dtype=torch.float64, generator=g)  # noqa: E731
    p = dict(kind=kind, cont=cont, cat=cat, l1=u(dc, 0.3, 1.2), lam1=u(dk, 0.4, 2.0),
             l2=u(dc, 0.5, 1.5), lam2=u(dk, 0.3, 1.0), os=u(1, 0.5, 1.5)[0], oc=u(1, 0.3, 1.0)[0],
             op=u(1, 0.4, 1.2)[0])
    noise = u(n, 0.02, 0.1) if fixed_noise else torch.tensor(0.05, dtype=torch.float64)
    return Z, y, p, noise, 0.3


def make_queries(Z, p, B, q, seed=0):
    """B x q x d queries: a row equal to a training row, two equal rows inside a
    t-batch (q > 1), an unseen category value."""
    g = torch.Generator().manual_seed(77 + seed + 13 * B + q)
    d = Z.shape[1]
    X = torch.rand(B, q, d, dtype=torch.float64, generator=g)
    X[..., p["cat"]] = torch.randint(0, 3, (B, q, len(p["cat"])), generator=g).to(torch.float64) * 0.5 + 0.25
    X[0, 0] = Z[min(3, Z.shape[0] - 1)]
    if q > 1:
        X[-1, q - 1] = X[-1, 0]
    if B * q > 1:
        X[B // 2, max(q // 2, 1 if B == 1 else 0), p["cat"][0]] = 7.125
    return X
