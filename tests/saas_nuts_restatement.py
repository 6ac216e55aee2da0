"""The SAAS log-density restated from SaasPyroModel.sample (botorch/models/
fully_bayesian.py:168-247), independently of the package: torch.distributions
for every term, the reference's Matern-5/2 formula with clamp_min(1e-30).sqrt(),
the Jacobians of the exp transforms, and the gradient by autograd.  One row at
a time, on the host, in fp64.  The oracle of tests/test_nuts_cpu.py,
tests/test_gpu_saas_potential.py and tests/test_gpu_nuts.py.

z = [log outputscale, mean, log g, log tau, log iota_1 .. log iota_d]; g is the
raw Gamma noise draw (noise = 1e-4 + g), tau kernel_tausq and iota
_kernel_inv_length_sq."""
import math

import torch
from torch.distributions import Gamma, HalfCauchy, MultivariateNormal, Normal

F64 = torch.float64
SQRT5 = math.sqrt(5)

# (n, d) of the regular cases, z ~ U(-2, 2)
REGULAR = [(0, 3), (1, 1), (2, 3), (17, 3), (64, 50), (65, 4), (130, 50)]
# ill-conditioned: sigma^2 ~ 1e-4, long lengthscales, cond(A) ~ 1e7
ILL = [(130, 3), (64, 2)]


def t(v):
    return torch.tensor(v, dtype=F64)


def log_density(z, X, y):
    """log p(z, Y) of one unconstrained vector z (D)."""
    n = X.shape[0]
    os, c, g, tau, iota = z[0].exp(), z[1], z[2].exp(), z[3].exp(), z[4:].exp()
    lp = Gamma(t(2.0), t(0.15)).log_prob(os) + Normal(t(0.0), t(1.0)).log_prob(c)
    lp = lp + Gamma(t(0.9), t(10.0)).log_prob(g) + HalfCauchy(t(0.1)).log_prob(tau)
    lp = lp + HalfCauchy(torch.ones_like(iota)).log_prob(iota).sum()
    lp = lp + z[0] + z[2] + z[3] + z[4:].sum()
    if n > 0:
        lengthscale = (tau * iota).rsqrt()
        Xs = X / lengthscale
        dist = ((Xs[:, None, :] - Xs[None, :, :]) ** 2).sum(-1).clamp_min(1e-30).sqrt()
        s5 = SQRT5 * dist
        K = s5.add(1 + 5 / 3 * (dist ** 2)) * torch.exp(-s5)
        K = os * K + (1e-4 + g) * torch.eye(n, dtype=F64)
        lp = lp + MultivariateNormal(loc=c.view(-1).expand(n), covariance_matrix=K).log_prob(y)
    return lp


def potential(z, X, y):
    """(U (C), grad (C x D), status (C) = 0) at the rows of z: the batched
    potential in the sampler's form."""
    U, G = [], []
    for row in z.detach().to(F64):
        zr = row.clone().requires_grad_(True)
        u = -log_density(zr, X, y)
        (g,) = torch.autograd.grad(u, zr)
        U.append(u.detach())
        G.append(g)
    return torch.stack(U), torch.stack(G), torch.zeros(len(U), dtype=torch.int32)


def data(n, d, seed=0):
    """X ~ U(0, 1)^(n x d), y a standardised smooth function of the first
    coordinates plus a little noise."""
    g = torch.Generator().manual_seed(1000 * n + d + seed)
    X = torch.rand(n, d, generator=g, dtype=F64)
    y = torch.sin(6.0 * X[:, 0]) + 0.1 * torch.randn(n, generator=g, dtype=F64)
    if d > 1:
        y = y + X[:, 1] ** 2
    if n > 1:
        y = (y - y.mean()) / y.std()
    return X, y


def regular_z(d, C=1, seed=0):
    g = torch.Generator().manual_seed(77 + 13 * d + seed)
    return 4.0 * torch.rand(C, d + 4, generator=g, dtype=F64) - 2.0


def ill_z(d):
    return torch.tensor([[3.0, 0.3, -12.0, -6.0] + [-2.0] * d], dtype=F64)


def permuted(X, y, seed=5):
    p = torch.randperm(X.shape[0], generator=torch.Generator().manual_seed(seed))
    return X[p], y[p]


def project_bound(ref):
    """The project's kernel-against-torch bound."""
    return 1e-9 * float(ref.abs().max()) + 1e-10


def ill_limits(X, y, z):
    """(limit for U, limit for the gradient, U, grad) of an ill-conditioned case:
    the larger of the project bound and 20 x the restatement's own discrepancy
    under a permutation of the training data."""
    U, G, _ = potential(z, X, y)
    Up, Gp, _ = potential(z, *permuted(X, y))
    return (max(project_bound(U), 20.0 * float((U - Up).abs().max())),
            max(project_bound(G), 20.0 * float((G - Gp).abs().max())), U, G)


def nuts_problem():
    """n = 20, d = 3: X ~ U(0, 1) seeded, y = standardised sin(6 x_0)."""
    g = torch.Generator().manual_seed(0)
    X = torch.rand(20, 3, generator=g, dtype=F64)
    y = torch.sin(6.0 * X[:, 0])
    return X, (y - y.mean()) / y.std()
