"""Plain torch fp64 restatement of the preference GP's Laplace approximation, written from
the reference's formulas (models/pairwise_gp.py, likelihoods/pairwise.py) in the
unwhitened variables: K^{-1} explicitly, the root of K^{-1} f + b(f) by Newton until the
residual stops falling, the evidence as PairwiseLaplaceMarginalLogLikelihood.forward
states it, its gradient by autograd through ONE Newton step from the converged root with
the Jacobian K^{-1} + C_iota (the exact implicit derivative), the posterior by the
hlcov_eye solve.  ``perm`` runs the same on permuted datapoints (results permuted back):
the second, independent form the tests' bounds are measured with.  A helper, not a test.
"""
import math

import torch

F64 = torch.float64


def make_case(n, m, d, scale, seed=0):
    """X in [0, 1]^d, utility scale * sin(3 sum x), m comparisons of distinct random
    pairs (the better one first; with m = 1 datapoints stay without a comparison)."""
    g = torch.Generator().manual_seed(1000 * n + 10 * d + m + seed)
    X = torch.rand(n, d, dtype=F64, generator=g)
    util = scale * torch.sin(3.0 * X.sum(-1))
    i = torch.randint(0, n, (m,), generator=g)
    j = (i + 1 + torch.randint(0, n - 1, (m,), generator=g)) % n
    swap = util[i] < util[j]
    comp = torch.stack([torch.where(swap, j, i), torch.where(swap, i, j)], dim=-1)
    hyper = torch.cat([torch.tensor([1.3], dtype=F64),
                       0.4 * math.sqrt(d) * (1.0 + 0.25 * torch.rand(d, dtype=F64, generator=g))])
    return X, comp, hyper


def kernel(X1, X2, hyper, kind):
    os_, ls = hyper[0], hyper[1:]
    r2 = ((X1.unsqueeze(-2) / ls - X2.unsqueeze(-3) / ls) ** 2).sum(-1)
    if kind == 0:
        return os_ * torch.exp(-0.5 * r2)
    r = torch.sqrt(r2.clamp_min(1e-30))
    return os_ * (1.0 + math.sqrt(5.0) * r + (5.0 / 3.0) * r2) * torch.exp(-math.sqrt(5.0) * r)


def _likelihood(f, D, only_unclamped=False):
    zr = D @ f / math.sqrt(2.0)
    z = zr.clamp(-3.0, 3.0)
    logcdf = torch.special.log_ndtr(z)
    h = torch.exp(-0.5 * z * z - 0.5 * math.log(2.0 * math.pi) - logcdf)
    c = h * (h + z) / 2.0
    if only_unclamped:
        c = c * (zr.abs() <= 3.0)
    return logcdf.sum(), -(D.mT @ h) / math.sqrt(2.0), D.mT @ (c.unsqueeze(-1) * D)


def restate(X, comp, hyper, kind, jitter=0.0, perm=None, Xq=None):
    """dict(psi, f, grad (d + 1: outputscale first), mean, cov at Xq (q x d))."""
    n = X.shape[0]
    if perm is not None:
        inv = torch.argsort(perm)
        X, comp = X[perm], inv[comp]
    D = torch.zeros(comp.shape[0], n, dtype=F64)
    D[torch.arange(comp.shape[0]), comp[:, 0]] = 1.0
    D[torch.arange(comp.shape[0]), comp[:, 1]] -= 1.0
    eye = torch.eye(n, dtype=F64)
    theta = hyper.clone().requires_grad_(True)
    K = kernel(X, X, theta, kind) + jitter * theta[0] * eye
    Kinv = torch.linalg.inv(K)
    with torch.no_grad():
        f, best = torch.zeros(n, dtype=F64), math.inf
        for _ in range(200):
            _, b, C = _likelihood(f, D)
            g = Kinv @ f + b
            res = float(g.norm())
            if not res < best:
                break
            best, keep = res, f
            f = f - torch.linalg.solve(Kinv + C, g)
        f0 = keep
    _, b, _ = _likelihood(f0, D)
    _, _, C_iota = _likelihood(f0, D, only_unclamped=True)
    f1 = f0 - torch.linalg.solve(Kinv + C_iota.detach(), Kinv @ f0 + b.detach())
    loglik, _, C = _likelihood(f1, D)
    psi = loglik - 0.5 * f1 @ Kinv @ f1 - 0.5 * torch.logdet(eye + K @ C)
    (grad,) = torch.autograd.grad(psi, theta)
    out = dict(psi=psi.detach(), f=f0, grad=grad,
               state=(X, hyper, kind, K.detach(), _likelihood(f0, D)[2], f0))
    if Xq is not None:
        with torch.no_grad():
            out["mean"], out["cov"] = posterior_at(out["state"], Xq)
    if perm is not None:
        out["f"] = out["f"][inv]
    return out


def posterior_at(state, Xq):
    """(mean, cov) at Xq (... x q x d) from restate()'s ``state``; differentiable in Xq."""
    X, hyper, kind, K, C, f = state
    kx = kernel(Xq, X, hyper, kind)
    return kx @ torch.linalg.inv(K) @ f, kernel(Xq, Xq, hyper, kind) - kx @ torch.linalg.solve(
        C @ K + torch.eye(X.shape[0], dtype=F64), C @ kx.mT)
