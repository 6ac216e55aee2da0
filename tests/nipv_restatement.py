"""qNegIntegratedPosteriorVariance restated in torch fp64 on the CPU
(botorch/acquisition/active_learning.py:40-126) without any fantasy model:
conditioning an exact GP on observations at the q points X_b with noise tau2 is
a rank-q correction of the current posterior.  Everything is in the model's
transformed outcome space.

    c(x_i, z) = o k(x_i, z) - o k(x_i, Xt) V[z],   V[z] = A^{-1} o k(Xt, z)
    C_b       = [c(x_i, z)]  (q x N),   G_b = C_b C_b^T
    M_b       = Sigma(X_b, X_b) + tau2 I
    vbar      = mean_z Sigma(z, z)
    nipv_b    = -(vbar - tr(M_b^{-1} G_b) / N)

``explicit_refit`` is the same quantity from the dense (n + q)-point model with
noise diag(noise, tau2 1_q): no rank-q identity."""
import torch

from tests.jes_restatement import F64, GP, kernel, make_gp, posterior, solve  # noqa: F401


def make_V(gp: GP, Z):
    """V (N x n) = (A^{-1} o k(Xt, Z))^T."""
    Kz = kernel(Z, gp.Xt, gp.ls, gp.kind, gp.o)
    return solve(gp, Kz.mT).mT if gp.Xt.shape[0] else Kz


def cross_cov(gp: GP, Z, V, X):
    """C (... x q x N): the posterior covariance of the rows of X with the
    integration points."""
    return kernel(X, Z, gp.ls, gp.kind, gp.o) - kernel(X, gp.Xt, gp.ls, gp.kind, gp.o) @ V.mT


def gram(gp: GP, Z, V, X):
    """G (... x q x q) = C C^T for X (... x q x d)."""
    C = cross_cov(gp, Z, V, X)
    return C @ C.mT


def nipv(gp: GP, Z, X):
    """-(integrated posterior variance) (...) after observing X (... x q x d)
    with noise gp.tau2."""
    N, q = Z.shape[0], X.shape[-2]
    G = gram(gp, Z, make_V(gp, Z), X)
    _, Sigma = posterior(gp, X)
    M = Sigma + gp.tau2 * torch.eye(q, dtype=F64)
    vbar = posterior(gp, Z.unsqueeze(-2))[1].reshape(-1).mean()
    tr = (torch.linalg.solve(M, G)).diagonal(dim1=-2, dim2=-1).sum(-1)
    return -(vbar - tr / N)


def explicit_refit(gp: GP, Z, Xb):
    """-(mean posterior variance at Z) of the GP refitted on the n + q points
    (Xt, Xb) with noise diag(noise, tau2 1_q): a dense solve."""
    q = Xb.shape[0]
    Xa = torch.cat([gp.Xt, Xb])
    nz = torch.cat([gp.noise, gp.tau2.expand(q).to(F64)])
    A = kernel(Xa, Xa, gp.ls, gp.kind, gp.o) + torch.diag(nz)
    Kz = kernel(Z, Xa, gp.ls, gp.kind, gp.o)
    var = gp.o - (Kz * torch.linalg.solve(A, Kz.mT).mT).sum(-1)
    return -var.mean()
