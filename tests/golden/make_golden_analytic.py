"""Fixtures of the analytic acquisition family: tests/golden/golden_analytic.npz.

For a grid of u (log_ei), of x (log_ndtr) and a dozen pairs (a, b)
(log_prob_normal_in) it records
  (a) the reference's value and autograd gradient -- botorch.utils.probability.
      utils and botorch.utils.safe_math loaded through _refload and composed as
      acquisition/analytic.py:975-1053 and 1182-1220 compose them (analytic.py
      itself imports gpytorch and does not load without it),
  (b) the truth from mpmath at 80 digits, and
  (c) the reference's own relative error against the truth (values relative to
      max(1, |truth|), gradients relative to |truth|).
Data only.  Run from the repository root:  python -m tests.golden.make_golden_analytic
"""
import math
import os

import mpmath as mp
import numpy as np
import torch

from tests.golden import _refload

mp.mp.dps = 80
F64 = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))

PAIRS = [(-1.0, 1.0), (5.0, 6.0), (-40.0, -39.0), (-1e-9, 1e-9), (-1e3, -999.0),
         (-1e6, -999999.0), (-2.0, 0.5), (-0.5, 2.0), (0.1, 0.2), (-8.0, -1.0), (-3.0, 3.0),
         (-100.0, -99.5)]
X_NDTR = [8.0, 0.0, -5.0, -38.0, -40.0, -1e3, -1e8, -1e100]


def u_grid():
    special = [-1.0, -1.0 - 1e-7, -1.0 + 1e-7, -1e6, -1e6 * (1 + 1e-7), -1e6 * (1 - 1e-7), -1e8,
               -1e20, -1e100]
    return np.concatenate([np.linspace(-1.5, 6.0, 31), -np.logspace(0.0, 6.3, 64),
                           np.array(special)])


# ---- the reference, composed as analytic.py composes its leaf functions -------------------
def reference():
    pu = _refload.load("botorch.utils.probability.utils")
    sm = _refload.load("botorch.utils.safe_math")

    def ei_helper(u):  # analytic.py:968-972
        return pu.phi(u) + u * pu.ndtr(u)

    def log_abs_u_Phi_div_phi(u):  # analytic.py:1026-1053
        a, b = -(1 / math.sqrt(2)), math.log(math.pi / 2) / 2
        return torch.log(torch.special.erfcx(a * u) * u.abs()) + b

    def log_ei_helper(u):  # analytic.py:975-1023
        bound = -1
        u_upper = u.masked_fill(u < bound, bound)
        log_ei_upper = ei_helper(u_upper).log()
        neg_inv_sqrt_eps = -1e6
        u_lower = u.masked_fill(u > bound, bound)
        u_eps = u_lower.masked_fill(u < neg_inv_sqrt_eps, neg_inv_sqrt_eps)
        w = log_abs_u_Phi_div_phi(u_eps)
        log_ei_lower = pu.log_phi(u) + torch.where(u > neg_inv_sqrt_eps, sm.log1mexp(w),
                                                   -2 * u_lower.abs().log())
        return torch.where(u > bound, log_ei_upper, log_ei_lower)

    return log_ei_helper, pu.log_ndtr, pu.log_prob_normal_in


def with_grad(f, *xs):
    xs = [torch.tensor(np.asarray(x), dtype=F64, requires_grad=True) for x in xs]
    y = f(*xs)
    gs = torch.autograd.grad(y.sum(), xs)
    return y.detach().numpy(), [g.numpy() for g in gs]


# ---- the truth ------------------------------------------------------------------------------
def _D_series(x, terms=30):
    """1 - x R(x), R the Mills ratio, by its asymptotic series (x >= 1e3: the
    30th term is below 1e-100 of the first)."""
    s, t = mp.mpf(0), mp.mpf(1)
    for k in range(1, terms + 1):
        t = t * (2 * k - 1) / (x * x)
        s += t if k % 2 else -t
    return s


def _mills(x):
    """(1 - Phi(x)) / phi(x), x > 0."""
    if x >= 1000:
        return (1 - _D_series(x)) / x
    return mp.sqrt(mp.pi / 2) * mp.erfc(x / mp.sqrt(2)) * mp.exp(x * x / 2)


def _log_phi(x):
    return -x * x / 2 - mp.log(2 * mp.pi) / 2


def true_log_ei(u):
    """(log(phi + u Phi), Phi / (phi + u Phi)); below -5 in the Mills-ratio form
    log phi(u) + log(1 - x R(x)), R / (1 - x R), x = -u."""
    u = mp.mpf(float(u))
    if u > -5:
        ph, Ph = mp.npdf(u), mp.ncdf(u)
        return mp.log(ph + u * Ph), Ph / (ph + u * Ph)
    x = -u
    R = _mills(x)
    D = _D_series(x) if x >= 1000 else 1 - x * R
    return _log_phi(u) + mp.log(D), R / D


def true_log_ndtr(x):
    """(log Phi(x), phi(x) / Phi(x))."""
    x = mp.mpf(float(x))
    if x > -5:
        return mp.log(mp.ncdf(x)), mp.npdf(x) / mp.ncdf(x)
    R = _mills(-x)
    return _log_phi(x) + mp.log(R), 1 / R


def true_log_prob_in(a, b):
    """(log(Phi(b) - Phi(a)), d / da, d / db), each difference taken where it does
    not cancel."""
    a, b = mp.mpf(float(a)), mp.mpf(float(b))
    s = mp.sqrt(2)
    if b <= 0:
        P = (mp.erfc(-b / s) - mp.erfc(-a / s)) / 2
    elif a >= 0:
        P = (mp.erfc(a / s) - mp.erfc(b / s)) / 2
    else:
        P = (mp.erf(b / s) + mp.erf(-a / s)) / 2
    lp = mp.log(P)
    return lp, -mp.exp(_log_phi(a) - lp), mp.exp(_log_phi(b) - lp)


def rel(got, true, value: bool):
    out = []
    for g, t in zip(got, true):
        # (a gradient below the doubles' range: the absolute error)
        den = max(mp.mpf(1), abs(t)) if value else abs(t) if abs(t) > mp.mpf("1e-300") else 1
        out.append(float(abs(mp.mpf(float(g)) - t) / den))
    return np.array(out)


def main():
    log_ei_helper, log_ndtr, log_prob_normal_in = reference()
    out = {}
    u = u_grid()
    v, (g,) = with_grad(log_ei_helper, u)
    tv, tg = zip(*[true_log_ei(x) for x in u])
    out.update(lei_u=u, lei_ref=v, lei_ref_grad=g, lei_true=np.array([float(t) for t in tv]),
               lei_true_grad=np.array([float(t) for t in tg]), lei_ref_err=rel(v, tv, True),
               lei_ref_grad_err=rel(g, tg, False))
    x = np.array(X_NDTR)
    v, (g,) = with_grad(log_ndtr, x)
    tv, tg = zip(*[true_log_ndtr(t) for t in x])
    out.update(lnd_x=x, lnd_ref=v, lnd_ref_grad=g, lnd_true=np.array([float(t) for t in tv]),
               lnd_true_grad=np.array([float(t) for t in tg]), lnd_ref_err=rel(v, tv, True),
               lnd_ref_grad_err=rel(g, tg, False))
    ab = np.array(PAIRS)
    v, (ga, gb) = with_grad(lambda a, b: log_prob_normal_in(a=a, b=b), ab[:, 0], ab[:, 1])
    tv, ta, tb = zip(*[true_log_prob_in(a, b) for a, b in PAIRS])
    out.update(lpn_ab=ab, lpn_ref=v, lpn_ref_da=ga, lpn_ref_db=gb,
               lpn_true=np.array([float(t) for t in tv]),
               lpn_true_da=np.array([float(t) for t in ta]),
               lpn_true_db=np.array([float(t) for t in tb]), lpn_ref_err=rel(v, tv, True),
               lpn_ref_da_err=rel(ga, ta, False), lpn_ref_db_err=rel(gb, tb, False))
    for k, a in out.items():
        assert np.all(np.isfinite(a)), k
    np.savez(os.path.join(HERE, "golden_analytic.npz"), **out)
    up = (u > -1) & (u <= 10)
    print(f"log_ei: value err max {out['lei_ref_err'].max():.2e}; gradient err max on (-1, 10] "
          f"{out['lei_ref_grad_err'][up].max():.2e}")
    for lo in range(0, 7):
        sel = (-u >= 10.0 ** lo) & (-u < 10.0 ** (lo + 1))
        if sel.any():
            print(f"  |u| in [1e{lo}, 1e{lo + 1}): gradient err max "
                  f"{out['lei_ref_grad_err'][sel].max():.2e}")
    print(f"log_ndtr: value {out['lnd_ref_err'].max():.2e} gradient "
          f"{out['lnd_ref_grad_err'].max():.2e}")
    for p, e, ea, eb in zip(PAIRS, out["lpn_ref_err"], out["lpn_ref_da_err"],
                            out["lpn_ref_db_err"]):
        print(f"  pair {p}: value {e:.2e} d/da {ea:.2e} d/db {eb:.2e}")


if __name__ == "__main__":
    main()
