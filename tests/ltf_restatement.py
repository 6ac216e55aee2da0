"""The multi-fidelity exact GP with the linear truncated fidelity kernel restated in
torch fp64 on the host, from botorch/models/kernels/linear_truncated_fidelity.py:183-238
and models/gp_regression_fidelity.py:218-308; shares nothing with the package or oracle/.

  K = o [k0(x; l0) + c k1(x; l1)],  s = clamp(., 0, 1), u = 1 - s
  c = u1 u1' (1 + s1 s1')^p [+ u2 u2' (1 + s2 s2')^p + u1 u1' u2 u2' (1 + s1 s1' + s2 s2')^p]

k0, k1 Matern-5/2 ARD.  A parameter set ``p`` is a dict: xc, fc (column lists), l0, l1
(tensors), pw, o (0-dim tensors).  The powers are written with ``pow``, as the
reference writes them."""
import math

import torch

NAMES = ("l0", "l1", "pw", "o")


def _matern_g(diff, ls):
    r2 = (diff / ls).pow(2).sum(-1)
    s5r = math.sqrt(5.0) * (r2 + 1e-300).sqrt()
    e = torch.exp(-s5r)
    return (1.0 + s5r + (5.0 / 3.0) * r2) * e, (5.0 / 3.0) * (1.0 + s5r) * e


def _diff(Z1, Z2, p):
    return Z1[..., p["xc"]].unsqueeze(-2) - Z2[..., p["xc"]].unsqueeze(-3)


def bias(Z1, Z2, p, dpw=False, log1p=False):
    """c(s, s') (... x a x b); with ``dpw`` its closed-form derivative in the power; with
    ``log1p`` the powers as exp(p log1p(t)) (the second form of the values)."""
    s = [Z1[..., j].clamp(0, 1).unsqueeze(-1) for j in p["fc"]]
    t = [Z2[..., j].clamp(0, 1).unsqueeze(-2) for j in p["fc"]]
    w = [(1 - a) * (1 - b) for a, b in zip(s, t)]
    bases = [(w[0], 1 + s[0] * t[0])]
    if len(p["fc"]) == 2:
        bases += [(w[1], 1 + s[1] * t[1]), (w[1] * w[0], 1 + s[0] * t[0] + s[1] * t[1])]
    if dpw:
        return sum(wt * b.pow(p["pw"]) * torch.log(b) for wt, b in bases)
    if log1p:
        return sum(wt * torch.exp(p["pw"] * torch.log1p(b - 1)) for wt, b in bases)
    return sum(wt * b.pow(p["pw"]) for wt, b in bases)


def kernel(Z1, Z2, p, log1p=False):
    diff = _diff(Z1, Z2, p)
    return p["o"] * (_matern_g(diff, p["l0"])[0]
                     + bias(Z1, Z2, p, log1p=log1p) * _matern_g(diff, p["l1"])[0])


def kernel_product(Z1, Z2, q):
    """The ``linear_truncated=False`` kernel (models/gp_regression_fidelity.py:270-308,
    kernels/exponential_decay.py:115-125, kernels/downsampling.py:117-130): o RBF(x; ls)
    [off + (|s + s'| / l + 1)^(-pw)] prod_j [off_j + (1 - s_j)^(1 + pw_j) (1 - s_j')^(1 + pw_j)].
    ``q``: xc (columns), ls, o, it (column or None), ed (l, pw, off), dfs (columns), ds
    (a list of (pw, off))."""
    diff = Z1[..., q["xc"]].unsqueeze(-2) - Z2[..., q["xc"]].unsqueeze(-3)
    K = torch.exp(-0.5 * (diff / q["ls"]).pow(2).sum(-1))
    if q["it"] is not None:
        l, pw, off = q["ed"]
        dist = (Z1[..., q["it"]].unsqueeze(-1) / l + Z2[..., q["it"]].unsqueeze(-2) / l).abs()
        K = K * (off + (dist + 1).pow(-pw))
    for j, (pw, off) in zip(q["dfs"], q["ds"]):
        K = K * (off + (1 - Z1[..., j]).pow(1 + pw).unsqueeze(-1) * (1 - Z2[..., j]).pow(1 + pw).unsqueeze(-2))
    return q["o"] * K


def bound(Z1, Z2, p):
    """o (1 + |c|): what an entry of K is held relative to."""
    return p["o"] * (1.0 + bias(Z1, Z2, p).abs())


def _noise_matrix(noise, n):
    return torch.diag(noise) if noise.ndim else noise * torch.eye(n, dtype=torch.float64)


def ll_autograd(Z, y, p, noise, const):
    """log N(y | const, K + noise) by Cholesky and its gradient by autograd:
    (ll, {name: grad}) over NAMES, "noise" and "const"."""
    leaves = {k: p[k].clone().requires_grad_(True) for k in NAMES}
    leaves["noise"] = noise.clone().requires_grad_(True)
    leaves["const"] = torch.tensor(float(const), dtype=torch.float64, requires_grad=True)
    n = Z.shape[0]
    L = torch.linalg.cholesky(kernel(Z, Z, dict(p, **{k: leaves[k] for k in NAMES}))
                              + _noise_matrix(leaves["noise"], n))
    b = torch.linalg.solve_triangular(L, (y - leaves["const"]).unsqueeze(-1), upper=False)
    ll = -0.5 * (b * b).sum() - torch.log(torch.diagonal(L)).sum() - 0.5 * n * math.log(2 * math.pi)
    grads = torch.autograd.grad(ll, list(leaves.values()))
    return ll.detach(), {k: g for k, g in zip(leaves, grads)}


def ll_closed(Z, y, p, noise, const):
    """The same by linalg.inv, slogdet and the closed-form sums 1/2 sum_ik W_ik dK_ik/dtheta,
    W = alpha alpha^T - A^{-1}.  Returns (ll, grads, S, W): S[name] holds the summands
    (n x n, or n x n x d_x for the lengthscales) whose total is the gradient."""
    n = Z.shape[0]
    diff = _diff(Z, Z, p)
    k0, g0 = _matern_g(diff, p["l0"])
    k1, g1 = _matern_g(diff, p["l1"])
    c = bias(Z, Z, p)
    A = p["o"] * (k0 + c * k1) + _noise_matrix(noise, n)
    Ainv = torch.linalg.inv(A)
    alpha = Ainv @ (y - const)
    W = torch.outer(alpha, alpha) - Ainv
    ll = -0.5 * (y - const) @ alpha - 0.5 * torch.linalg.slogdet(A)[1] - 0.5 * n * math.log(2 * math.pi)
    h, d2 = (0.5 * W).unsqueeze(-1), diff.pow(2)
    S = {"l0": h * (p["o"] * g0).unsqueeze(-1) * d2 / p["l0"] ** 3,
         "l1": h * (p["o"] * c * g1).unsqueeze(-1) * d2 / p["l1"] ** 3,
         "pw": 0.5 * W * p["o"] * k1 * bias(Z, Z, p, dpw=True), "o": 0.5 * W * (k0 + c * k1)}
    grads = {k: v.sum(dim=(0, 1)) for k, v in S.items()}
    grads["noise"] = 0.5 * torch.diagonal(W) if noise.ndim else 0.5 * torch.trace(W)
    grads["const"] = alpha.sum()
    return ll, grads, S, W


def posterior(Z, y, p, noise, const, Xq):
    """An ordinary exact GP over the (x, s) rows: (mean, cov) at Xq (... x q x d)."""
    L = torch.linalg.cholesky(kernel(Z, Z, p) + _noise_matrix(noise, Z.shape[0]))
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


def mfkg(mean, cov, Zb, noise, q_a, current_value, cost):
    """The multi-fidelity knowledge gradient from the joint moments of (X_actual,
    project(X_fantasies)) (B x (q_a + N_f)): v_i = mu(x'_i) + Sigma(x'_i, X) L^{-T} z_i with
    L L^T = Sigma(X, X) + noise I and Zb the N_f x q_a base samples; then the reference's
    order: minus current_value, the inverse-cost weighting per fantasy (cost: B), the
    mean.  Returns (acq, the mean taken before the weighting instead)."""
    L = torch.linalg.cholesky(cov[:, :q_a, :q_a] + noise * torch.eye(q_a, dtype=torch.float64))
    Wt = torch.linalg.solve_triangular(L.mT, Zb.T.expand(mean.shape[0], q_a, Zb.shape[0]), upper=True)
    v = mean[:, q_a:] + (cov[:, q_a:, :q_a] * Wt.mT).sum(-1) - current_value
    c = cost.unsqueeze(-1)
    early = v.mean(-1, keepdim=True)
    return (torch.where(v > 0, v / c, v * c).mean(-1),
            torch.where(early > 0, early / c, early * c).squeeze(-1))


def cross_grad(X, Z, p, dK, G):
    """The first argument's gradient of every pair, weighted: (sum, sum |summand|) over
    the n training partners (dK: B x q x n) and the q partners of the row's own
    t-batch (G: B x q x q), each B x q x d, by autograd one pair at a time."""
    B, q, d = X.shape
    P = torch.cat([Z.expand(B, q, *Z.shape), X.unsqueeze(1).expand(B, q, q, d)], dim=2)  # B q (n+q) d
    w = torch.cat([dK, G], dim=-1)
    A = X.unsqueeze(2).expand_as(P).clone().requires_grad_(True)
    k = kernel(A.reshape(-1, 1, d), P.reshape(-1, 1, d), p).reshape(w.shape)
    (g,) = torch.autograd.grad(k.sum(), A)
    terms = w.unsqueeze(-1) * g
    return terms.sum(2), terms.abs().sum(2)


def make_case(nf, dx, n, seed=0, fixed_noise=False, pw=None):
    """Rows with the fidelity columns first and in the middle, fidelities outside [0, 1],
    exactly 0 and 1, target-fidelity rows (every fidelity >= 1) among others, a
    duplicated row; ``pw`` replaces the drawn power.  Returns (Z, y, p, noise, const)."""
    g = torch.Generator().manual_seed(1000 * seed + 37 * dx + 5 * nf + n)
    d = dx + nf
    fc = [0, d // 2][:nf]  # (d >= n_f + 1, so the two differ)
    xc = [j for j in range(d) if j not in fc]
    Z = torch.rand(n, d, dtype=torch.float64, generator=g)
    vals = torch.tensor([-0.25, 0.0, 0.3, 0.75, 1.0, 1.0, 1.4], dtype=torch.float64)
    Z[:, fc] = vals[torch.randint(0, 7, (n, nf), generator=g)]
    if n > 2:
        Z[n - 1] = Z[0]
    y = torch.sin(3.0 * Z.sum(-1)) + 0.1 * torch.randn(n, dtype=torch.float64, generator=g)
    u = lambda k, lo, hi: lo + (hi - lo) * torch.rand(k, dtype=torch.float64, generator=g)  # noqa: E731
    p = dict(xc=xc, fc=fc, l0=u(dx, 0.3, 1.2), l1=u(dx, 0.5, 1.5), pw=u(1, 0.4, 2.0)[0],
             o=u(1, 0.5, 1.5)[0])
    if pw is not None:
        p["pw"] = torch.tensor(pw, dtype=torch.float64)
    noise = u(n, 0.02, 0.1) if fixed_noise else torch.tensor(0.05, dtype=torch.float64)
    return Z, y, p, noise, 0.3


def make_queries(Z, p, B, q, seed=0):
    """B x q x d queries: a row equal to a training row, two equal rows inside a t-batch
    (q > 1), fidelities from the same set of values; the last t-batch wholly at target
    fidelity (1.0 and beyond)."""
    g = torch.Generator().manual_seed(77 + seed + 13 * B + q)
    X = torch.rand(B, q, Z.shape[1], dtype=torch.float64, generator=g)
    vals = torch.tensor([-0.25, 0.0, 0.3, 0.75, 1.0, 1.0, 1.4], dtype=torch.float64)
    X[..., p["fc"]] = vals[torch.randint(0, 7, (B, q, len(p["fc"])), generator=g)]
    X[-1][:, p["fc"]] = vals[torch.randint(4, 7, (q, len(p["fc"])), generator=g)]
    if B > 1:
        X[0, 0] = Z[min(3, Z.shape[0] - 1)]
    if q > 1:
        X[-1, q - 1] = X[-1, 0]
    return X
