"""Batched fantasy models restated in torch fp64 on the CPU (a helper, not a
test).

The reference (models/model.py:328-407, models/gpytorch.py:468-531) samples
Y_f = mu(X) + L z_f under observation noise, conditions the model on (X, Y_f)
with the same noise and evaluates the new model's posterior at X'_f.  In the
current model's joint posterior at [X; X'_f], all moments in outcome space,

    A     = Sigma(X, X) + diag(s'^2)         L = psd_safe_cholesky(A)
    V_f   = Sigma(X'_f, X) L^{-T}
    mu'_f = mu(X'_f) + V_f z_f               (Y_f - mu(X) = L z_f)
    S'_f  = Sigma(X'_f, X'_f) - V_f V_f^T

``fantasy_moments`` states this on un-packed joint moments,
``fantasy_moments_packed`` on the packed tiles the device kernel reads (with its
own statement of the packing), and ``fantasy_by_refit`` does what the reference
does: an explicit exact GP on the n + q_a points per fantasy."""
import math

import torch

from oracle.gp import ExactGPOracle, GPHyper, psd_safe_cholesky

F64 = torch.float64
TILE_ROWS = 16


def tile_plan(q_a: int, q: int, F: int):
    """(T, slots): the fewest tiles of at most 16 rows that hold the q_a
    fantasised points plus a share of the F groups of q points each, the
    shares even."""
    T = math.ceil(F / ((TILE_ROWS - q_a) // q))
    return T, math.ceil(F / T)


def group_rows(g: int, q_a: int, q: int, slots: int):
    """(tile, first row in the tile) of group g."""
    return g // slots, q_a + (g % slots) * q


def pack(Xa: torch.Tensor, Xp: torch.Tensor, slots: int) -> torch.Tensor:
    """Xa B x q_a x d, Xp B x F x q x d -> B x T x (q_a + slots q) x d; the spare
    groups of the last tile repeat the last group."""
    F = Xp.shape[1]
    T = math.ceil(F / slots)
    tiles = []
    for t in range(T):
        groups = [Xp[:, min(t * slots + s, F - 1)] for s in range(slots)]
        tiles.append(torch.cat([Xa] + groups, dim=1))
    return torch.stack(tiles, dim=1)


def _moments(A, mu_p, C, D, Z):
    """A B x q_a x q_a (noise included), mu_p B x F x q, C B x F x q x q_a,
    D B x F x q x q, Z N_f x q_a (F = N_f or 1) -> (mean B x N_f x q, cov B x F x
    q x q, L, jitter B)."""
    L, jitter = psd_safe_cholesky(A)
    V = torch.linalg.solve_triangular(L.unsqueeze(1), C.mT, upper=False).mT   # C L^{-T}
    if C.shape[1] == 1:  # one group serves every fantasy
        mean = mu_p + torch.einsum("brj,fj->bfr", V[:, 0], Z)
    else:
        mean = mu_p + torch.einsum("bfrj,fj->bfr", V, Z)
    return mean, D - V @ V.mT, L, jitter


def fantasy_moments(mean, cov, Z, noise, q_a: int):
    """Joint moments mean B x F x (q_a + q), cov B x F x (q_a + q) x (q_a + q) of
    [X; X'_g] in outcome space, noise (q_a) or a float -> (mean B x N_f x q, cov
    B x F x q x q); differentiable."""
    nv = torch.as_tensor(noise, dtype=F64).expand(q_a)
    A = cov[:, 0, :q_a, :q_a] + torch.diag(nv)
    return _moments(A, mean[..., q_a:], cov[..., q_a:, :q_a], cov[..., q_a:, q_a:], Z)[:2]


def read_masks(B: int, q_a: int, q: int, F: int, slots: int):
    """Boolean masks (mean (B T) x q', cov (B T) x q' x q') of what the
    definition reads of the packed moments: tile 0's X x X block, each group's
    cross block, own diagonal block and mean."""
    T = math.ceil(F / slots)
    qp = q_a + slots * q
    rm = torch.zeros(B * T, qp, dtype=torch.bool)
    rc = torch.zeros(B * T, qp, qp, dtype=torch.bool)
    rc[::T, :q_a, :q_a] = True
    for b in range(B):
        for g in range(F):
            t, r0 = group_rows(g, q_a, q, slots)
            rm[b * T + t, r0:r0 + q] = True
            rc[b * T + t, r0:r0 + q, :q_a] = True
            rc[b * T + t, r0:r0 + q, r0:r0 + q] = True
    return rm, rc


def fantasy_moments_packed(mean, cov, Z, noise, q_a: int, q: int, slots: int, shared: bool):
    """Packed moments mean (B T) x q', cov (B T) x q' x q', noise (q_a) ->
    (mean_out B x N_f x q, cov_out B x F x q x q, L B x q_a x q_a, jitter B),
    reading what ``read_masks`` marks and nothing else."""
    N_f = Z.shape[0]
    F = 1 if shared else N_f
    T = math.ceil(F / slots)
    B = mean.shape[0] // T
    mu_p, C, D = [], [], []
    for g in range(F):
        t, r0 = group_rows(g, q_a, q, slots)
        mu_p.append(mean[t::T, r0:r0 + q])
        C.append(cov[t::T, r0:r0 + q, :q_a])
        D.append(cov[t::T, r0:r0 + q, r0:r0 + q])
    A = cov[::T, :q_a, :q_a] + torch.diag_embed(noise.expand(B, q_a))
    return _moments(A, torch.stack(mu_p, 1), torch.stack(C, 1), torch.stack(D, 1), Z)


def fantasy_by_refit(orc: ExactGPOracle, Xa, Xp, Z, noise_tf=None):
    """(mean B x N_f x q, cov B x N_f x q x q) by refitting: per (b, f) the
    observations Y_f = mu(X_b) + L z_f join the training data (standardised with
    the old statistics, the hyperparameters kept) and the new model's posterior
    is taken at Xp[b, f] (Xp B x N_f x q x d).  noise_tf: the fantasy noise per
    row in the standardised space (q_a), default the model's noise."""
    B, q_a, _ = Xa.shape
    N_f, q = Xp.shape[1], Xp.shape[2]
    n = orc.train_X.shape[0]
    s, m = orc.ystd.squeeze(), orc.ymean.squeeze()
    nv = torch.full((q_a,), float(orc.h.noise), dtype=F64) if noise_tf is None else noise_tf
    hyper = GPHyper(orc.h.lengthscale, torch.cat([torch.full((n,), float(orc.h.noise), dtype=F64), nv]),
                    orc.h.constant, orc.h.outputscale, orc.h.kind)
    mean = torch.empty(B, N_f, q, dtype=F64)
    cov = torch.empty(B, N_f, q, q, dtype=F64)
    for b in range(B):
        mu, Sigma = orc.posterior(Xa[b])
        L = torch.linalg.cholesky(Sigma + torch.diag(nv) * s * s)
        for f in range(N_f):
            Y = mu + L @ Z[f]
            new = ExactGPOracle(torch.cat([orc.train_X, Xa[b]]),
                                torch.cat([orc.train_y, (Y - m) / s]), hyper, standardize=False)
            lm, lc, _ = new.latent(Xp[b, f])
            mean[b, f], cov[b, f] = m + s * lm, lc * s * s
    return mean, cov
