"""Max-value entropy search restated in torch fp64 on the CPU, from the
formulas of DESIGN.md section 18 (botorch/acquisition/max_value_entropy_search.py:
qMaxValueEntropy 399-515 without fantasies or trace observations, GIBBON
537-664, the Gumbel fit's quantiles 983-1010).  Everything is in outcome space;
one row is one t-batch of q = 1.

    mu, var   noiseless posterior mean and variance of the row
    tau2      what observation_noise=True adds (noise level x ystd^2)
    w         +1 maximize, -1 minimize;  fstar (S_M) max values, w-signed
    z (S_m)   base samples, shared by all rows

MES:
    m = w mu   vM = max(var, 1e-8)   vm = var + tau2   t = vM / vm
    mean_new_k = m + t sqrt(vm) w z_k
        (the reference draws samples_m = w (mu + sqrt(vm) z) and mean_m = w mu,
         lines 434-448, so samples_m - mean_m = w sqrt(vm) z: the sign of z
         flips with w; only log_prob(w samples_m), whose w w cancels, is
         even in z)
    s2n = max(vM - vM^2 / vm, 1e-8)
    Phin_jk = max(Phi((fstar_j - mean_new_k) / sqrt s2n), 1e-8)
    Phi0_j = max(Phi((fstar_j - m) / sqrt vM), 1e-8)      Z = Phin / Phi0
    lp_k = -z_k^2 / 2 - log(2 pi vm) / 2     h1 = -Z log Z - Z lp_k     h0_k = -lp_k
    H1bar = mean_jk h1    cov = mean_jk (h1 - H1bar)(h0_k - mean h0)
    beta = cov / sqrt(var_k(h0) var_jk(h1))   (unbiased variances)
    ig = H0 - H1bar + beta (mean_k h0 - H0),   H0 = log(2 pi e vm) / 2

GIBBON:
    vm = max(var + tau2, 1e-8)   gamma_j = (fstar_j - w mu) / sqrt vM
    r_j = phi(gamma_j) / max(Phi(gamma_j), 1e-8)    rho2 = vM / vm
    acq = -mean_j log max(1 - rho2 r_j (gamma_j + r_j), 1e-8) / 2
    with pending points: qf = A Binv A^T,
    acq += (log(max(vm, qf (1 + 1e-12)) - qf) - log vm) / 2

Phi goes through erfc.  ``Mes`` / ``Gibbon`` also return the unclamped
quantities next to their floors, for the tests' distance-to-clamp assertions."""
import math
from typing import NamedTuple, Optional

import torch

F64 = torch.float64
CLAMP_LB = 1e-8
VDET_EPS = (1.0 + 1e-12) - 1.0
QUANTILE_P = (0.25, 0.5, 0.75)


def Phi(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def host_constants(z):
    """(kappa, var_h0, zsq_mean): mean_k h0 - H0, var_k(h0) and mean z^2."""
    zz = z.to(F64) ** 2
    return 0.5 * (zz.mean().item() - 1.0), (0.5 * zz).var().item(), zz.mean().item()


class Mes(NamedTuple):
    ig: torch.Tensor        # R
    beta: torch.Tensor      # R
    H1bar: torch.Tensor     # R
    clamped: dict           # name -> (unclamped quantity, floor)


def mes(mu, var, fstar, z, tau2, w=1.0) -> Mes:
    """mu, var (R); fstar (S_M); z (S_m)."""
    m = (w * mu)[:, None, None]
    vMu = var
    vM = vMu.clamp_min(CLAMP_LB)[:, None, None]
    vm = (var + tau2)[:, None, None]
    zk = z[None, None, :]
    f = fstar[None, :, None]
    mean_new = m + (vM / vm) * vm.sqrt() * (w * zk)
    s2u = vM - vM * vM / vm
    s2n = s2u.clamp_min(CLAMP_LB)
    Pn = Phi((f - mean_new) / s2n.sqrt())
    P0 = Phi((f - m) / vM.sqrt())
    Z = Pn.clamp_min(CLAMP_LB) / P0.clamp_min(CLAMP_LB)
    lp = -0.5 * zk * zk - 0.5 * torch.log(2.0 * math.pi * vm)      # R x 1 x S_m
    h1 = -Z * Z.log() - Z * lp                                       # R x S_M x S_m
    h0 = -lp
    H1bar = h1.mean(dim=(1, 2))
    H0bar = h0.mean(dim=(1, 2))
    cov = ((h1 - H1bar[:, None, None]) * (h0 - H0bar[:, None, None])).mean(dim=(1, 2))
    beta = cov / (h0.var(dim=(1, 2)) * h1.var(dim=(1, 2))).sqrt()
    H0 = 0.5 * torch.log(2.0 * math.pi * math.e * vm.reshape(-1))
    ig = H0 - H1bar + beta * (H0bar - H0)
    return Mes(ig, beta, H1bar, {"vM": (vMu, CLAMP_LB), "s2n": (s2u.reshape(-1), CLAMP_LB),
                                 "Phin": (Pn, CLAMP_LB), "Phi0": (P0, CLAMP_LB)})


class Gibbon(NamedTuple):
    acq: torch.Tensor
    qf: Optional[torch.Tensor]
    clamped: dict


def gibbon(mu, var, fstar, tau2, w=1.0, A=None, Binv=None) -> Gibbon:
    """mu, var (R); fstar (S_M); A (R x m) and Binv (m x m), or neither."""
    vM = var.clamp_min(CLAMP_LB)
    vmu = var + tau2
    vm = vmu.clamp_min(CLAMP_LB)
    g = (fstar[None, :] - (w * mu)[:, None]) / vM.sqrt()[:, None]
    P = Phi(g)
    r = phi(g) / P.clamp_min(CLAMP_LB)
    inner = 1.0 - (vM / vm)[:, None] * r * (g + r)
    acq = -0.5 * inner.clamp_min(CLAMP_LB).log().mean(dim=1)
    cl = {"vM": (var, CLAMP_LB), "vm": (vmu, CLAMP_LB), "Phi": (P, CLAMP_LB),
          "inner": (inner, CLAMP_LB)}
    qf = None
    if A is not None and A.shape[-1] > 0:
        qf = ((A @ Binv) * A).sum(-1)
        lim = qf * (1.0 + 1e-12)
        cl["vdet"] = (vm, lim)
        # on the clamped branch lim - qf = qf ((1 + 1e-12) - 1): written so, the
        # value and autograd's gradient keep their digits (the subtraction
        # cancels twelve of sixteen)
        vdet = torch.where(vm >= lim, vm - qf, qf * VDET_EPS)
        acq = acq + 0.5 * (torch.log(vdet) - torch.log(vm))
    return Gibbon(acq, qf, cl)


def near_clamp(clamped: dict, frac: float = 0.01):
    """Rows (first axis) with a quantity within ``frac`` (relative) of its floor."""
    bad = None
    for q, lim in clamped.values():
        lim = torch.as_tensor(lim, dtype=F64)
        near = (q - lim).abs() <= frac * lim.abs()
        near = near.reshape(near.shape[0], -1).any(dim=1)
        bad = near if bad is None else bad | near
    return bad


def log_Phi(x):
    """log Phi(x), tail-safe on both sides (-inf once erfc underflows)."""
    pos = torch.log1p(-0.5 * torch.erfc(x.clamp_min(0.0) / math.sqrt(2.0)))
    neg = torch.log(0.5 * torch.erfc(-x.clamp_max(0.0) / math.sqrt(2.0)))
    return torch.where(x > 0, pos, neg)


def quantile_objective(y: float, mu, sigma) -> float:
    """sum_i log Phi((y - mu_i) / sigma_i)."""
    return log_Phi((y - mu) / sigma).sum().item()


def quantiles(mu, sigma, bounds=None, iters: int = 200):
    """The three roots of ``quantile_objective = log p`` by bisection on
    [min(mu - 3 sigma), max(mu + 5 sigma)]; (y (3), status (3))."""
    lo0 = (mu - 3.0 * sigma).min().item() if bounds is None else bounds[0]
    hi0 = (mu + 5.0 * sigma).max().item() if bounds is None else bounds[1]
    out, status = [], []
    for p in QUANTILE_P:
        lp, lo, hi = math.log(p), lo0, hi0
        ok = quantile_objective(lo, mu, sigma) < lp and not quantile_objective(hi, mu, sigma) < lp
        y = 0.5 * (lo + hi)
        for _ in range(iters if ok else 0):
            y = 0.5 * (lo + hi)
            if not lo < y < hi or hi - lo <= 4 * 2.220446049250313e-16 * max(abs(lo), abs(hi)):
                break
            if quantile_objective(y, mu, sigma) < lp:
                lo = y
            else:
                hi = y
        out.append(y)
        status.append(0 if ok else 1)
    return torch.tensor(out, dtype=F64), status


def gumbel_fit(q25, q50, q75):
    """(a, b) of the Gumbel matched at the three quantiles (lines 1013-1015)."""
    b = (q25 - q75) / (math.log(math.log(4.0 / 3.0)) - math.log(math.log(4.0)))
    return q50 + b * math.log(math.log(2.0)), b
