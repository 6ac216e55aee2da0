"""qBayesianActiveLearningByDisagreement restated in torch fp64 on the host,
from the mixture's means, covariances (observation noise included) and the
shared base samples: the oracle of the BALD tests.

For one t-batch with components m = 1..M, y_ms = mu_m + L_m z_s and
l_msm' = log N(y_ms; mu_m', Sigma_m'):
  H   = -mean_{m,s} log mean_m' exp l_msm'      (mixture entropy)
  C_m = -mean_s l_msm                           (component entropy)
  out[m] = H - C_m,   acquisition = mean_m out[m].
``form="exp"`` writes the mixture density as the reference does
(exp().mean().log()); ``form="lse"`` as a log-sum-exp.  They are the same number
wherever the first is finite.  Nothing here is shared with the package."""
import math

import torch

F64 = torch.float64


def log_densities(mean, L, Z):
    """lp (S x B x M x M): sample s of component m (dim 2) of t-batch b under
    component m' (dim 3).  mean B x M x q, L B x M x q x q, Z S x q."""
    B, M, q = mean.shape
    S = Z.shape[0]
    y = mean.unsqueeze(0) + torch.einsum("bmij,sj->sbmi", L, Z)          # S x B x M x q
    r = (y.unsqueeze(3) - mean.view(1, B, 1, M, q)).unsqueeze(-1)         # S x B x M x M x q x 1
    Lb = L.view(1, B, 1, M, q, q).expand(S, B, M, M, q, q)
    w = torch.linalg.solve_triangular(Lb, r, upper=False).squeeze(-1)
    half_log_det = L.diagonal(dim1=-2, dim2=-1).log().sum(-1)            # B x M
    return (-0.5 * (w * w).sum(-1) - half_log_det.view(1, B, 1, M)
            - 0.5 * q * math.log(2.0 * math.pi))


def bald_roots(mean, L, Z, form="lse"):
    """out (B x M) from the components' Cholesky roots."""
    lp = log_densities(mean, L, Z)
    M = mean.shape[1]
    if form == "exp":
        mix = lp.exp().mean(-1).log()
    else:
        mix = torch.logsumexp(lp, dim=-1) - math.log(M)
    H = -mix.mean(dim=(0, 2))
    C = -torch.diagonal(lp, dim1=2, dim2=3).mean(0)
    return H.unsqueeze(-1) - C


def bald(mean, cov, Z, form="lse"):
    """The acquisition value (B) from means and covariances."""
    return bald_roots(mean, torch.linalg.cholesky(cov), Z, form).mean(-1)


def member_moments(members, X):
    """mean (B x M x q), cov (B x M x q x q) of oracle.acquisition.saas_members at
    X (B x q x d), outcome space, each member's noise added in its model space
    (before the outcome untransform)."""
    means, covs = [], []
    for mm in members:
        mu, cov, _ = mm.latent(X)
        cov = cov + mm.h.noise * torch.eye(X.shape[-2], dtype=F64)
        s = mm.ystd.squeeze()
        means.append(mm.ymean.squeeze() + s * mu)
        covs.append(cov * (s * s))
    return torch.stack(means, dim=1), torch.stack(covs, dim=1)


def bald_members(members, X, Z, form="lse"):
    mean, cov = member_moments(members, X)
    return bald(mean, cov, Z, form)


# the three end-to-end problems (d, M, q, n, S, B) of the BALD tests
CASES = [(10, 3, 2, 32, 64, 4), (50, 16, 8, 64, 128, 3), (6, 4, 16, 24, 32, 2)]


def problem(d, M, q, n, S, B, standardize=False, seed=1):
    """Training data (Hartmann on the first six inputs for d >= 10, else a sine),
    SAAS-prior hyperparameters, candidates and base samples, all on the host."""
    from botorch_amd.models import sample_saas_prior
    from botorch_amd.test_functions import Hartmann
    from oracle.sampling import base_samples_single_output, draw_sobol_samples
    lo = torch.zeros(d, dtype=F64)
    X = draw_sobol_samples(lo, lo + 1, n, 1, 0).squeeze(1)
    if d >= 10:
        Y = Hartmann(negate=True)(X[:, :6]).unsqueeze(-1)
    else:
        Y = torch.sin(3.0 * X.sum(-1, keepdim=True))
    if standardize:
        Y = 3.0 + 5.0 * Y
    else:
        Y = (Y - Y.mean()) / Y.std()
    smp = sample_saas_prior(d, M, seed=seed)
    Xc = draw_sobol_samples(lo, lo + 1, B, q, 3)
    Z = base_samples_single_output(S, q, 2)
    return X, Y, smp, Xc, Z
