"""The analytic q = 1 acquisition chain restated in plain torch fp64: the six
modes of bo_analytic and the feasibility terms, composed as
botorch/acquisition/analytic.py:960-1053 and 1182-1220 compose them (the same
masking, so autograd through it meets no NaN).  The reference of the GPU tests,
values and, through CPU autograd, gradients; tests/test_analytic_cpu.py pins it
to the reference's own outputs (tests/golden/golden_analytic.npz).

Nothing here imports the package."""
import math

import torch

LOG_EI, EI, LOG_PI, PI, UCB, STD = range(6)
LOWER, UPPER, BOTH = range(3)
MIN_VAR = 1e-12
_NEG_INV_SQRT2 = -(1 / math.sqrt(2))
_INV_SQRT_2PI = 1 / math.sqrt(2 * math.pi)
_LOG_2 = math.log(2)
_LOG_SQRT_2PI = math.log(2 * math.pi) / 2
_LOG_SQRT_PI_DIV_2 = math.log(math.pi / 2) / 2


def Phi(x):
    return 0.5 * torch.erfc(_NEG_INV_SQRT2 * x)


def phi(x):
    return _INV_SQRT_2PI * (-0.5 * x.square()).exp()


def log_phi(x):
    return -0.5 * x.square() - _LOG_SQRT_2PI


def log1mexp(x):
    return torch.where(-_LOG_2 < x, (-x.expm1()).log(), (-x.exp()).log1p())


def log_erfc(x):
    pos = x > 0
    xp, xn = x.masked_fill(~pos, 0), x.masked_fill(pos, 0)
    return torch.where(pos, torch.log(torch.special.erfcx(xp)) - xp.square(),
                       torch.log(torch.special.erfc(xn)))


def log_ndtr(x):
    return log_erfc(_NEG_INV_SQRT2 * x) - _LOG_2


def log_prob_normal_in(a, b):
    rev = b.abs() > a.abs()
    a, b = torch.where(rev, -b, a), torch.where(rev, -a, b)
    la, lb = log_ndtr(a), log_ndtr(b)
    return lb + log1mexp(la - lb.masked_fill(lb == -math.inf, 0.0))


def ei_helper(u):
    return phi(u) + u * Phi(u)


def log_ei(u):
    bound, eps = -1.0, -1e6
    upper = ei_helper(u.masked_fill(u < bound, bound)).log()
    u_lower = u.masked_fill(u > bound, bound)
    u_eps = u_lower.masked_fill(u < eps, eps)
    w = torch.log(torch.special.erfcx(_NEG_INV_SQRT2 * u_eps) * u_eps.abs()) + _LOG_SQRT_PI_DIV_2
    lower = log_phi(u) + torch.where(u > eps, log1mexp(w), -2 * u_lower.abs().log())
    return torch.where(u > bound, upper, lower)


def _sigma(var, min_var):
    """sqrt(max(var, min_var)); on the floor (var <= min_var) no gradient."""
    return torch.where(var > min_var, var, torch.full_like(var, min_var)).sqrt()


def log_prob_feas(mean, var, constraints, min_var=MIN_VAR):
    """The sum over ``constraints`` -- (member, lower, upper, kind) each -- of the
    log probability that the member lies within its bounds; mean, var Mt x R."""
    lp = torch.zeros_like(mean[0])
    for member, lower, upper, kind in constraints:
        mu, sg = mean[member], _sigma(var[member], min_var)
        if kind == LOWER:
            lp = lp + log_ndtr(-((lower - mu) / sg))
        elif kind == UPPER:
            lp = lp + log_ndtr((upper - mu) / sg)
        else:
            lp = lp + log_prob_normal_in((lower - mu) / sg, (upper - mu) / sg)
    return lp


def analytic(mean, var, best_f, mode, obj=0, w=1.0, beta=0.0, min_var=MIN_VAR, constraints=()):
    """acq (R) of bo_analytic from mean, var (Mt x R) and best_f (a scalar
    tensor or R entries)."""
    mu, sg = mean[obj], _sigma(var[obj], min_var)
    if mode == UCB:
        val = w * mu + math.sqrt(beta) * sg
    elif mode == STD:
        val = w * sg
    else:
        u = (mu - best_f) / sg
        u = u if w > 0 else -u
        val = {LOG_EI: lambda: log_ei(u) + sg.log(), EI: lambda: sg * ei_helper(u),
               LOG_PI: lambda: log_ndtr(u), PI: lambda: Phi(u)}[mode]()
    if not constraints:
        return val
    lp = log_prob_feas(mean, var, constraints, min_var)
    return val + lp if mode in (LOG_EI, LOG_PI) else val * lp.exp()


def analytic_with_grad(mean, var, best_f, mode, dacq, **kw):
    """(acq, dmean, dvar) by CPU autograd through :func:`analytic`."""
    mean = mean.detach().clone().requires_grad_(True)
    var = var.detach().clone().requires_grad_(True)
    acq = analytic(mean, var, best_f, mode, **kw)
    dmean, dvar = torch.autograd.grad(acq, (mean, var), dacq, allow_unused=True)
    zeros = torch.zeros_like(mean)
    return acq.detach(), zeros if dmean is None else dmean, zeros if dvar is None else dvar
