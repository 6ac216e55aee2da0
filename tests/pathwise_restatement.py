"""Pathwise posterior samples (Matheron paths) of a single-output exact GP,
restated in torch fp64 on the CPU (a helper, not a test).

The reference builds a MatheronPath of an ExactGP from

* random Fourier features (sampling/pathwise/features/generators.py:66-193):
  the input divided by the lengthscale, the H = M / 2 frequencies Omega, the
  sine features first and the cosine features after them, scaled by
  (2 / M)^0.5 and, under a ScaleKernel, by outputscale^0.5
  (OutputscaleTransform, :171-193);
* the prior path (prior_samplers.py:52-106): a linear model on those features
  with weights W and the mean module as its bias;
* the update path (update_strategies.py:72-135): the kernel row against
  V = (K + noise)^{-1} (y - prior(Xt) - eps), eps ~ N(0, noise);
* the outcome transform, removed while drawing and applied to the sum
  (posterior_samplers.py:198-224).

With theta_j(x) = sum_t Omega[j, t] x_t / l_t:

    g_s(x) = c + sqrt(2 o / M) sum_{j<H} (W[s, j] sin theta_j + W[s, H + j] cos theta_j)
               + sum_i V[s, i] o k(x, Xt_i)
    f_s(x) = ymean + ystd g_s(x)
"""
import math

import torch

F64 = torch.float64
RBF, MATERN52 = 0, 1


def kernel_matrix(kind, X1, X2, lengthscale, outputscale):
    """o k(X1, X2): RBF or Matern-5/2 on the lengthscale-scaled inputs, from the
    differences themselves (no |a|^2 + |b|^2 - 2 a.b cancellation)."""
    diff = (X1 / lengthscale).unsqueeze(-2) - (X2 / lengthscale).unsqueeze(-3)
    d2 = (diff * diff).sum(-1)
    if kind == RBF:
        return outputscale * torch.exp(-0.5 * d2)
    r = d2.clamp_min(1e-30).sqrt()
    s5r = math.sqrt(5.0) * r
    return outputscale * (1.0 + s5r + (5.0 / 3.0) * d2) * torch.exp(-s5r)


def features(X, Omega, lengthscale, outputscale):
    """R x M: sqrt(2 o / M) [sin theta, cos theta] (generators.py:66-109, 171-193)."""
    theta = (X / lengthscale) @ Omega.T
    M = 2 * Omega.shape[0]
    return math.sqrt(2.0 * outputscale / M) * torch.cat([theta.sin(), theta.cos()], dim=-1)


def prior_values(X, Omega, W, lengthscale, outputscale, constant):
    """S x R values of the prior paths (prior_samplers.py:52-106)."""
    return constant + W @ features(X, Omega, lengthscale, outputscale).T


def noisy_covariance(kind, Xt, lengthscale, outputscale, noise, jitter=0.0):
    """A = o k(Xt, Xt) + diag(noise) (+ jitter I); noise a float or n values."""
    n = Xt.shape[0]
    nz = torch.as_tensor(noise, dtype=F64).expand(n) + jitter
    return kernel_matrix(kind, Xt, Xt, lengthscale, outputscale) + torch.diag(nz)


def update_weights(kind, Xt, lengthscale, outputscale, noise, y_tf, prior_at_Xt, eps, jitter=0.0):
    """V (S x n) = A^{-1} (y_tf - prior(Xt) - eps) by cholesky_solve
    (update_strategies.py:81-104)."""
    L = torch.linalg.cholesky(noisy_covariance(kind, Xt, lengthscale, outputscale, noise, jitter))
    E = y_tf.unsqueeze(0) - prior_at_Xt - eps
    return torch.cholesky_solve(E.T, L).T


def path_values(kind, X, Xt, lengthscale, outputscale, constant, ymean, ystd, Omega, W, V):
    """S x R values f_s(X_r) of the definition above (V None: the prior alone)."""
    g = prior_values(X, Omega, W, lengthscale, outputscale, constant)
    if V is not None and V.shape[1] > 0:
        g = g + V @ kernel_matrix(kind, Xt, X, lengthscale, outputscale)
    return ymean + ystd * g


def mapped_values(kind, X, inner, *args):
    """The mapped form: row r on path (r // inner) % S -> R values."""
    f = path_values(kind, X, *args)
    S, R = f.shape
    p = (torch.arange(R) // inner) % S
    return f[p, torch.arange(R)]
