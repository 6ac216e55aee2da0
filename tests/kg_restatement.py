"""One-shot knowledge gradient with the posterior mean as inner value, restated
in torch fp64 on the CPU (a helper, not a test).

The reference (acquisition/knowledge_gradient.py:151-207, models/model.py:
328-407) samples Y_i = mu(X) + L z_i under observation noise, conditions the
model on (X, Y_i) with the same noise and takes the fantasy model's posterior
mean at x'_i.  In the current model's joint posterior that mean is

    v_i = mu(x'_i) + Sigma(x'_i, X) L^{-T} z_i,    L L^T = Sigma(X, X) + s2 I

``kg_values`` states this on un-packed joint moments, ``kg_values_packed`` on
the packed tiles the device kernel reads (with its own statement of the
packing), and ``kg_by_refit`` does what the reference does: an explicit exact
GP on the n + q points per fantasy."""
import math

import torch

from oracle.gp import ExactGPOracle, psd_safe_cholesky

F64 = torch.float64
TILE_ROWS = 16


def tile_plan(q_a: int, N_f: int):
    """(T, slots): the fewest tiles of at most 16 rows that hold the q_a actual
    points plus a share of the N_f fantasy solutions each, the shares even."""
    T = math.ceil(N_f / (TILE_ROWS - q_a))
    return T, math.ceil(N_f / T)


def fantasy_row(i: int, q_a: int, slots: int):
    """(tile, row in the tile) of fantasy solution i."""
    return i // slots, q_a + i % slots


def pack(Xa: torch.Tensor, Xf: torch.Tensor, slots: int) -> torch.Tensor:
    """Xa B x q_a x d, Xf B x N_f x d -> B x T x (q_a + slots) x d; the spare
    slots of the last tile repeat the last fantasy solution."""
    B, q_a, d = Xa.shape
    N_f = Xf.shape[1]
    T = math.ceil(N_f / slots)
    rows = []
    for t in range(T):
        fant = [Xf[:, min(t * slots + s, N_f - 1)] for s in range(slots)]
        rows.append(torch.cat([Xa, torch.stack(fant, dim=1)], dim=1))
    return torch.stack(rows, dim=1)


def _values(A, mu_f, cross, Z):
    """A B x q x q (noise included), mu_f B x N_f, cross B x N_f x q, Z N_f x q
    -> (values B x N_f, jitter B)."""
    L, jitter = psd_safe_cholesky(A)
    B, q = A.shape[0], A.shape[-1]
    Wt = torch.linalg.solve_triangular(L.mT, Z.T.expand(B, q, Z.shape[0]), upper=True)
    return mu_f + (cross * Wt.mT).sum(dim=-1), jitter


def kg_values(mean: torch.Tensor, cov: torch.Tensor, Z: torch.Tensor, noise: float, q_a: int):
    """Joint moments mean B x (q_a + N_f), cov B x (q_a + N_f) x (q_a + N_f) of
    [X; X'] in outcome space -> values B x N_f (differentiable)."""
    eye = torch.eye(q_a, dtype=cov.dtype)
    return _values(cov[:, :q_a, :q_a] + noise * eye, mean[:, q_a:], cov[:, q_a:, :q_a], Z)[0]


def read_entries(B: int, q_a: int, N_f: int, slots: int):
    """Index tensors of what the definition reads of the packed moments:
    (tile index B x N_f, row B x N_f) of the fantasy rows."""
    T = math.ceil(N_f / slots)
    tr = [fantasy_row(i, q_a, slots) for i in range(N_f)]
    tile = torch.tensor([[b * T + t for t, _ in tr] for b in range(B)])
    row = torch.tensor([[r for _, r in tr] for _ in range(B)])
    return tile, row


def kg_values_packed(mean: torch.Tensor, cov: torch.Tensor, Z: torch.Tensor, noise: float,
                     q_a: int, slots: int):
    """Packed moments mean (B T) x q', cov (B T) x q' x q' -> (values B x N_f,
    jitter B), reading Sigma(X, X) from tile 0 of each restart and the cross
    block from the fantasy rows, columns 0..q_a-1, and nothing else."""
    N_f = Z.shape[0]
    T = math.ceil(N_f / slots)
    B = mean.shape[0] // T
    tile, row = read_entries(B, q_a, N_f, slots)
    A = cov[::T, :q_a, :q_a] + noise * torch.eye(q_a, dtype=cov.dtype)
    return _values(A, mean[tile, row], cov[tile, row, :q_a], Z)


def kg_by_refit(orc: ExactGPOracle, Xa: torch.Tensor, Xf: torch.Tensor, Z: torch.Tensor):
    """values B x N_f by refitting: per (b, i) the observations Y_i = mu(X_b) +
    L z_i join the training data (standardised with the old statistics, the
    hyperparameters kept) and the new model's mean is taken at x'_{b,i}."""
    B, q_a, _ = Xa.shape
    N_f = Xf.shape[1]
    s, m = orc.ystd.squeeze(), orc.ymean.squeeze()
    out = torch.empty(B, N_f, dtype=F64)
    for b in range(B):
        mu, Sigma = orc.posterior(Xa[b])
        L = torch.linalg.cholesky(Sigma + orc.h.noise * s * s * torch.eye(q_a, dtype=F64))
        for i in range(N_f):
            Y = mu + L @ Z[i]
            new = ExactGPOracle(torch.cat([orc.train_X, Xa[b]]),
                                torch.cat([orc.train_y, (Y - m) / s]), orc.h, standardize=False)
            out[b, i] = m + s * new.latent(Xf[b, i:i + 1])[0][0]
    return out
