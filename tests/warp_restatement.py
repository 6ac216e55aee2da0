"""Plain fp64 torch restatement of the input transforms and of the exact MLL (Cholesky +
autograd), and a 50-digit mpmath evaluation of the Kumaraswamy step.  CPU only."""
import math

import mpmath
import torch

EPS = 1e-7


def warp_reference(X, offset, rscale, a, b, flag, eps=EPS):
    """The reference's formulas: (X - offset) / range, then 1 - (1 - u^a)^b on flagged columns."""
    v = (X - offset) * rscale
    u = (v * (1.0 - 2.0 * eps) + eps).clamp(eps, 1.0 - eps)
    return torch.where(flag, 1.0 - (1.0 - u.pow(a)).pow(b), v)


def warp_logspace(X, offset, rscale, a, b, flag, eps=EPS):
    """The same map with the Kumaraswamy step in log space (what the kernels evaluate)."""
    v = (X - offset) * rscale
    u = (v * (1.0 - 2.0 * eps) + eps).clamp(eps, 1.0 - eps)
    return torch.where(flag, -torch.expm1(b * torch.log(-torch.expm1(a * torch.log(u)))), v)


def kumaraswamy_mp(x: float, a: float, b: float, eps=EPS):
    """(z, dz/du) to 50 digits at the fp64 u = clamp(fma(x, 1 - 2 eps, eps), eps, 1 - eps) that
    the formula is evaluated at (the fma rounds once: the 50-digit sum rounded to fp64), as
    floats rounded once at the end."""
    with mpmath.workdps(50):
        u = float(mpmath.mpf(x) * mpmath.mpf(1.0 - 2.0 * eps) + mpmath.mpf(eps))
        u = mpmath.mpf(min(max(u, eps), 1.0 - eps))
        a, b = mpmath.mpf(a), mpmath.mpf(b)
        w = 1 - u ** a
        return float(1 - w ** b), float(a * b * u ** (a - 1) * w ** (b - 1))


def covariance(Xt, ls, os_, kind):
    D = (Xt.unsqueeze(1) - Xt.unsqueeze(0)) / ls
    r2 = (D * D).sum(-1)
    if kind == 0:
        return os_ * torch.exp(-0.5 * r2)
    s5r = math.sqrt(5.0) * torch.sqrt(r2.clamp_min(1e-300))
    return os_ * (1.0 + s5r + (5.0 / 3.0) * r2) * torch.exp(-s5r)


def mll(Xt, y, ls, noise, const, os_, kind):
    """log N(y | const, K + diag(noise)); noise a scalar or an n-vector."""
    n = Xt.shape[0]
    noise = torch.as_tensor(noise, dtype=torch.float64)
    A = covariance(Xt, ls, os_, kind) + torch.diag_embed(noise.expand(n))
    L = torch.linalg.cholesky(A)
    r = (y - const).unsqueeze(-1)
    return (-0.5 * (r * torch.cholesky_solve(r, L)).sum() - torch.log(torch.diagonal(L)).sum()
            - 0.5 * n * math.log(2 * math.pi))


def lognormal_logpdf(x, loc, scale):
    lx = torch.log(x)
    return (-((lx - loc) ** 2) / (2 * scale ** 2) - math.log(scale) - 0.5 * math.log(2 * math.pi)
            - lx).sum()
