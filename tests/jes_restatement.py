"""qJointEntropySearch, lower bound, restated in torch fp64 on the CPU
(botorch/acquisition/joint_entropy_search.py:195-265) without any fantasy
model: conditioning an exact GP on one pair (x*_j, f*_j) with noise nu_j is a
rank-one correction of the current posterior.  Everything is in the model's
transformed outcome space.

    c_ij  = cov(f(x_i), f(x*_j) | data) = k(x_i, x*_j) - k(x_i, Xt) A^{-1} k(Xt, x*_j)
    mu_ji = mu_i + c_ij g_j,  g_j = (f*_j - m_j) / s_j,  s_j = v_j + nu_j
    s2_ji = max(var_i - c_ij^2 / s_j, 1e-10)
    z     = (w f*_j - w mu_ji) / sqrt(s2_ji)
    r     = phi(z) / max(Phi(z), 1e-8),  Phi(z) = erfc(-z / sqrt 2) / 2
    vt_ji = s2_ji max(1 - (z + r) r, 1e-8) + tau2_j
    H_i   = mean_j log(vt_ji) / 2
    acq   = logdet(Sigma + tau2 I) / 2 - sum_i H_i

``explicit_conditioned`` is the same model j by a dense solve of the
(n + 1) x (n + 1) system, for the tests of the rank-one identities."""
import math
from typing import NamedTuple, Optional

import torch

F64 = torch.float64
RBF, MATERN52 = 0, 1
S2_FLOOR, PHI_FLOOR, INNER_FLOOR = 1e-10, 1e-8, 1e-8
MIN_INFERRED_NOISE_LEVEL = 1e-4


def kernel(X1, X2, ls, kind=RBF, o=1.0):
    """o k(X1, X2) for ARD lengthscales ls; X1 (... x a x d), X2 (... x b x d)."""
    diff = (X1 / ls).unsqueeze(-2) - (X2 / ls).unsqueeze(-3)
    d2 = (diff * diff).sum(-1)
    if kind == RBF:
        return o * torch.exp(-0.5 * d2)
    r = d2.clamp_min(1e-30).sqrt()
    s5r = math.sqrt(5.0) * r
    return o * (1.0 + s5r + (5.0 / 3.0) * d2) * torch.exp(-s5r)


class GP(NamedTuple):
    Xt: torch.Tensor      # n x d
    y: torch.Tensor       # n, transformed targets
    ls: torch.Tensor      # d
    kind: int
    o: float
    noise: torch.Tensor   # n (a homoskedastic level repeated)
    const: float
    fixed: bool
    L: torch.Tensor       # chol(K + diag(noise))
    alpha: torch.Tensor   # A^{-1} (y - const)

    @property
    def tau2(self):
        """The observation noise of a posterior: the level, or the mean of the
        fixed variances."""
        return self.noise.mean() if self.noise.numel() else torch.zeros((), dtype=F64)


def make_gp(Xt, y, ls, noise, const=0.0, kind=RBF, o=1.0) -> GP:
    """noise: a float (homoskedastic) or n variances (fixed noise)."""
    n = Xt.shape[0]
    fixed = torch.is_tensor(noise) and noise.numel() == n and noise.dim() == 1
    nv = noise.to(F64) if fixed else torch.full((n,), float(noise), dtype=F64)
    ls = torch.as_tensor(ls, dtype=F64).reshape(-1)
    A = kernel(Xt, Xt, ls, kind, o) + torch.diag(nv)
    L = torch.linalg.cholesky(A) if n else A
    alpha = torch.cholesky_solve((y - const).unsqueeze(-1), L).squeeze(-1) if n else y
    return GP(Xt, y, ls, kind, float(o), nv, float(const), bool(fixed), L, alpha)


def solve(gp: GP, Kt):
    """A^{-1} Kt for Kt n x m."""
    return torch.cholesky_solve(Kt, gp.L) if gp.Xt.shape[0] else Kt


def posterior(gp: GP, X):
    """(mu ... x q, Sigma ... x q x q), noiseless."""
    Kx = kernel(X, gp.Xt, gp.ls, gp.kind, gp.o)                     # ... x q x n
    mu = gp.const + Kx @ gp.alpha
    Sigma = kernel(X, X, gp.ls, gp.kind, gp.o)
    if gp.Xt.shape[0]:
        Sigma = Sigma - Kx @ solve(gp, Kx.mT)
    return mu, Sigma


class Optima(NamedTuple):
    Xo: torch.Tensor     # P x d
    f: torch.Tensor      # P, transformed
    m: torch.Tensor      # P posterior mean at x*_j
    v: torch.Tensor      # P posterior variance at x*_j
    V: torch.Tensor      # P x n, A^{-1} k(Xt, x*_j)
    nu: torch.Tensor     # P noise on the optimum
    s: torch.Tensor      # v + nu
    g: torch.Tensor      # (f - m) / s
    tau2: torch.Tensor   # P observation noise of the conditioned model


def make_optima(gp: GP, Xo, f, condition_noiseless=True) -> Optima:
    P, n = Xo.shape[0], gp.Xt.shape[0]
    if condition_noiseless:
        nu = torch.full((P,), MIN_INFERRED_NOISE_LEVEL, dtype=F64)
    elif gp.fixed:
        raise RuntimeError("FixedNoiseGaussianLikelihood.fantasize requires a `noise` kwarg")
    else:
        nu = gp.tau2.expand(P).clone()
    Ko = kernel(Xo, gp.Xt, gp.ls, gp.kind, gp.o)                    # P x n
    V = solve(gp, Ko.mT).mT if n else Ko
    m = gp.const + Ko @ gp.alpha
    v = gp.o - (Ko * V).sum(-1)
    s = v + nu
    tau2 = (n * gp.tau2 + nu) / (n + 1) if gp.fixed else gp.tau2.expand(P).clone()
    return Optima(Xo, f, m, v, V, nu, s, (f - m) / s, tau2)


def cross_cov(gp: GP, opt: Optima, X):
    """c (... x P): the posterior covariance of the rows of X with the optima."""
    return kernel(X, opt.Xo, gp.ls, gp.kind, gp.o) - kernel(X, gp.Xt, gp.ls, gp.kind, gp.o) @ opt.V.mT


def rank_one_moments(c, mu, var, opt: Optima):
    """(mu_ji, s2_ji unclamped), both ... x P, of the models conditioned on one optimum."""
    return mu.unsqueeze(-1) + c * opt.g, var.unsqueeze(-1) - c * c / opt.s


class Chain(NamedTuple):
    H: torch.Tensor        # ... : mean_j log(vt) / 2
    z: torch.Tensor        # ... x P
    on_s2: torch.Tensor    # clamp masks, ... x P
    on_phi: torch.Tensor
    on_inner: torch.Tensor
    vt: torch.Tensor


def chain(c, mu, var, g, sinv, wf, tau2, w=1.0) -> Chain:
    """The elementwise chain from c (... x P) and the rows' mu, var (...)."""
    mu_j = mu.unsqueeze(-1) + c * g
    s2u = var.unsqueeze(-1) - c * c * sinv
    s2 = s2u.clamp_min(S2_FLOOR)
    z = (wf - w * mu_j) / s2.sqrt()
    Phi = 0.5 * torch.erfc(-z / math.sqrt(2.0))
    r = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) / Phi.clamp_min(PHI_FLOOR)
    inu = 1.0 - (z + r) * r
    vt = s2 * inu.clamp_min(INNER_FLOOR) + tau2
    return Chain(0.5 * torch.log(vt).mean(-1), z, s2u <= S2_FLOOR, Phi <= PHI_FLOOR,
                 inu <= INNER_FLOOR, vt)


def conditional_entropy(gp: GP, opt: Optima, X, mu, var, w=1.0) -> Chain:
    return chain(cross_cov(gp, opt, X), mu, var, opt.g, 1.0 / opt.s, w * opt.f, opt.tau2, w)


def jes_lower_bound(gp: GP, opt: Optima, X, maximize=True):
    """acq (...) of X (... x q x d)."""
    w = 1.0 if maximize else -1.0
    mu, Sigma = posterior(gp, X)
    q = X.shape[-2]
    A = Sigma + gp.tau2 * torch.eye(q, dtype=F64)
    H0 = 0.5 * torch.logdet(A)
    H = conditional_entropy(gp, opt, X, mu, Sigma.diagonal(dim1=-2, dim2=-1), w).H
    return H0 - H.sum(-1)


def explicit_conditioned(gp: GP, opt: Optima, j: int, X):
    """(mean, variance) at the rows of X (R x d) of the GP refitted on the n + 1
    points (Xt, x*_j) with noise diag(noise, nu_j): a dense solve, no rank-one
    identity."""
    Xa = torch.cat([gp.Xt, opt.Xo[j:j + 1]])
    ya = torch.cat([gp.y, opt.f[j:j + 1]])
    A = kernel(Xa, Xa, gp.ls, gp.kind, gp.o) + torch.diag(torch.cat([gp.noise, opt.nu[j:j + 1]]))
    Kx = kernel(X, Xa, gp.ls, gp.kind, gp.o)
    sol = torch.linalg.solve(A, torch.cat([(ya - gp.const).unsqueeze(-1), Kx.mT], dim=-1))
    return gp.const + Kx @ sol[:, 0], gp.o - (Kx * sol[:, 1:].mT).sum(-1)
