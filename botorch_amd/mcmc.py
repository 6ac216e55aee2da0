"""NUTS for the fully Bayesian SAAS GP.

Three parts:

* :func:`saas_potential_torch`: U = -log p(z, Y) of the SAAS model
  (models/fully_bayesian.py:168-247, SaasPyroModel.sample) and its closed-form
  gradient in batched torch fp64, on host or device tensors.  It is the route
  outside the fused kernel's limits and on a machine without the library, and
  the comparator of the benchmark.
* :func:`saas_potential_fn`: the batched potential of a data set for the
  sampler: the fused kernel (``torch.ops.bo.saas_potential``) for device data
  inside its limits, the torch route otherwise.
* :func:`run_nuts`: multinomial NUTS with dual-averaging step size and Stan's
  windowed mass adaptation, on the host in fp64, generic over a batched
  potential.  Every chain is a generator that yields the point at which it needs
  U and its gradient; a scheduler gathers the requests of all live chains into
  one batched call, so C chains cost the rounds of the longest tree.

The unconstrained vector is z = [log outputscale, mean, log g, log tau,
log iota_1 .. log iota_d] (g: the raw Gamma noise draw, noise = 1e-4 + g).
Draws are not comparable with pyro's: the density is the reference's, the
sampler is specified in DESIGN.md section 22 and checked by its invariants and
statistics.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

F64 = torch.float64
_SQRT5 = math.sqrt(5.0)
_LOG_2PI = math.log(2.0 * math.pi)
_PAIR_LIMIT = 1 << 24  # doubles of one block of squared differences (n_rows x n x d)


# ---- the density ---------------------------------------------------------------------------------
def _pair_blocks(X: Tensor):
    """Row blocks [(i0, i1, (X_i - X_k)^2 of shape (i1 - i0) n x d)] of the
    squared differences, each block of at most _PAIR_LIMIT values."""
    n, d = X.shape
    if n == 0:
        return []
    rows = max(1, min(n, _PAIR_LIMIT // max(1, n * d)))
    out = []
    for i0 in range(0, n, rows):
        i1 = min(n, i0 + rows)
        out.append((i0, i1, ((X[i0:i1, None, :] - X[None, :, :]) ** 2).reshape(-1, d)))
    return out


def _saas_potential_blocks(z: Tensor, X: Tensor, y: Tensor, blocks):
    C = z.shape[0]
    n, d = X.shape
    finite = torch.isfinite(z).all(dim=1)
    if not (bool(torch.isfinite(X).all()) and bool(torch.isfinite(y).all())):
        finite = torch.zeros_like(finite)
    zs = torch.where(finite[:, None], z, torch.zeros_like(z))
    os, c, g, tau, io = zs[:, 0].exp(), zs[:, 1], zs[:, 2].exp(), zs[:, 3].exp(), zs[:, 4:].exp()
    s2 = 1e-4 + g
    w = tau[:, None] * io
    finite = finite & torch.isfinite(os) & torch.isfinite(s2) & torch.isfinite(w).all(dim=1)
    # rows that are out already go on as z = 0 (their results are discarded)
    keep = finite[:, None]
    zs = torch.where(keep, zs, torch.zeros_like(zs))
    os, c, g, tau, io = zs[:, 0].exp(), zs[:, 1], zs[:, 2].exp(), zs[:, 3].exp(), zs[:, 4:].exp()
    s2 = 1e-4 + g
    w = tau[:, None] * io
    t = tau / 0.1
    lp = (2.0 * math.log(0.15) + 2.0 * zs[:, 0] - 0.15 * os
          - 0.5 * c * c - 0.5 * _LOG_2PI
          + 0.9 * math.log(10.0) - math.lgamma(0.9) + 0.9 * zs[:, 2] - 10.0 * g
          + math.log(2.0 / (math.pi * 0.1)) - torch.log1p(t * t) + zs[:, 3]
          + (math.log(2.0 / math.pi) - torch.log1p(io * io) + zs[:, 4:]).sum(dim=1))
    grad = torch.empty_like(zs)
    grad[:, 0] = 2.0 - 0.15 * os
    grad[:, 1] = -c
    grad[:, 2] = 0.9 - 10.0 * g
    grad[:, 3] = 1.0 - 2.0 / (1.0 + 1.0 / (t * t))
    grad[:, 4:] = 1.0 - 2.0 / (1.0 + 1.0 / (io * io))
    status = torch.where(finite, 0, 1).to(torch.int32)
    ll = torch.zeros_like(lp)
    if n > 0:
        r2 = torch.empty(C, n, n, dtype=z.dtype, device=z.device)
        for i0, i1, D2 in blocks:
            r2[:, i0:i1] = (D2 @ w.T).T.reshape(C, i1 - i0, n)
        s5r = _SQRT5 * r2.clamp_min(1e-30).sqrt()
        ex = torch.exp(-s5r)
        Kb = (1.0 + s5r + (5.0 / 3.0) * r2) * ex
        eye = torch.eye(n, dtype=z.dtype, device=z.device)
        A = os[:, None, None] * Kb + s2[:, None, None] * eye
        L, info = torch.linalg.cholesky_ex(A)
        ok = (info == 0) & torch.isfinite(L).all(dim=(1, 2))
        status = torch.where(finite & ~ok, 2, status.to(torch.int64)).to(torch.int32)
        L = torch.where(ok[:, None, None], L, eye)
        resid = (y[None, :] - c[:, None]).unsqueeze(-1)
        beta = torch.linalg.solve_triangular(L, resid, upper=False).squeeze(-1)
        Ainv = torch.cholesky_inverse(L)
        alpha = (Ainv @ resid).squeeze(-1)
        W = alpha[:, :, None] * alpha[:, None, :] - Ainv
        ll = (-0.5 * (beta * beta).sum(dim=1) - L.diagonal(dim1=1, dim2=2).log().sum(dim=1)
              - 0.5 * n * _LOG_2PI)
        grad[:, 0] += 0.5 * os * (W * Kb).sum(dim=(1, 2))
        grad[:, 1] += alpha.sum(dim=1)
        grad[:, 2] += 0.5 * g * W.diagonal(dim1=1, dim2=2).sum(dim=1)
        V = W * (-(5.0 / 6.0) * (1.0 + s5r) * ex)
        gw = torch.zeros(C, d, dtype=z.dtype, device=z.device)
        for i0, i1, D2 in blocks:
            gw += V[:, i0:i1].reshape(C, -1) @ D2
        gl = w * (0.5 * os[:, None] * gw)
        grad[:, 4:] += gl
        grad[:, 3] += gl.sum(dim=1)
    U = -(ll + lp)
    grad = -grad
    done = torch.isfinite(U) & torch.isfinite(grad).all(dim=1)
    status = torch.where((status == 0) & ~done, 1, status.to(torch.int64)).to(torch.int32)
    good = status == 0
    U = torch.where(good, U, torch.full_like(U, math.inf))
    grad = torch.where(good[:, None], grad, torch.zeros_like(grad))
    return U, grad, status


def saas_potential_torch(z: Tensor, X: Tensor, y: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(U (C), grad (C x (d + 4)), status (C, int32)): U = -log p(z, Y) of the
    SAAS model over X (n x d), y (n) at the rows of z, and dU/dz, in batched
    torch fp64 on the tensors' device.  status: 0 ok, 1 a non-finite input,
    hyperparameter or result, 2 a failed Cholesky; such a row has U = +inf and a
    zero gradient (the contract of ``kernels.saas_potential``)."""
    if z.dim() != 2 or X.dim() != 2 or y.dim() != 1 or z.shape[1] != X.shape[1] + 4 \
            or y.shape[0] != X.shape[0]:
        raise ValueError(f"saas_potential_torch: z must be C x (d + 4), X n x d and y n, got "
                         f"{tuple(z.shape)}, {tuple(X.shape)} and {tuple(y.shape)}")
    return _saas_potential_blocks(z, X, y, _pair_blocks(X))


def saas_potential_fn(X: Tensor, y: Tensor, route: Optional[str] = None) -> Callable:
    """The batched potential of the data (X, y) for :func:`run_nuts`: takes z
    (C x D, host fp64) and returns host (U, grad, status).  route "fused": the
    HIP kernel (device data inside ``kernels.saas_potential_check``'s limits);
    "torch": :func:`saas_potential_torch` on X's device; None: fused where it
    applies."""
    X = X.detach().to(F64).contiguous()
    y = y.detach().to(F64).reshape(-1).contiguous()
    n, d = X.shape
    if route is None:
        route = "fused" if X.is_cuda and n <= 1024 and d <= 256 else "torch"
    if route == "torch":
        blocks = _pair_blocks(X)

        def potential(z: Tensor):
            U, grad, status = _saas_potential_blocks(z.to(X.device), X, y, blocks)
            return U.cpu(), grad.cpu(), status.cpu()
        return potential
    if route != "fused":
        raise ValueError(f"saas_potential_fn: route must be 'fused', 'torch' or None, got {route!r}")
    from . import kernels, ops  # noqa: F401  (registers torch.ops.bo.saas_potential)
    kernels.saas_potential_check(n, d, 1)
    work = {}

    def potential(z: Tensor):
        C = z.shape[0]
        kernels.saas_potential_check(n, d, C)
        if C not in work:  # the workspace of a batch size is kept between the rounds
            work[C] = torch.empty(max(1, kernels.saas_potential_work(n, d, C)), dtype=F64,
                                  device=X.device)
        U, grad, status = torch.ops.bo.saas_potential(z.to(X.device), X, y, work[C])
        # one device-to-host copy per round
        out = torch.cat([U[:, None], grad, status[:, None].to(F64)], dim=1).cpu()
        return out[:, 0], out[:, 1:-1], out[:, -1].to(torch.int32)
    return potential


# ---- the sampler ---------------------------------------------------------------------------------
class _Mass:
    """The inverse mass matrix M^{-1} (the covariance estimate): identity,
    diagonal or dense."""

    def __init__(self, D: int):
        self.D = D
        self.var = np.ones(D)
        self.cov = None
        self.chol = None

    def set(self, cov: np.ndarray, dense: bool) -> None:
        if dense:
            self.cov = cov
            self.chol = np.linalg.cholesky(cov)
        else:
            self.var = np.diag(cov).copy() if cov.ndim == 2 else cov.copy()

    def velocity(self, r: np.ndarray) -> np.ndarray:  # M^{-1} r
        return self.cov @ r if self.cov is not None else self.var * r

    def momentum(self, eps: np.ndarray) -> np.ndarray:  # r ~ N(0, M) from eps ~ N(0, I)
        if self.chol is not None:
            return np.linalg.solve(self.chol.T, eps)
        return eps / np.sqrt(self.var)

    def kinetic(self, r: np.ndarray) -> float:
        return 0.5 * float(r @ self.velocity(r))


class _Welford:
    def __init__(self, D: int, dense: bool):
        self.k, self.mean, self.dense = 0, np.zeros(D), dense
        self.m2 = np.zeros((D, D)) if dense else np.zeros(D)

    def add(self, x: np.ndarray) -> None:
        self.k += 1
        delta = x - self.mean
        self.mean = self.mean + delta / self.k
        self.m2 += np.outer(delta, x - self.mean) if self.dense else delta * (x - self.mean)

    def regularised(self) -> np.ndarray:
        k = self.k
        c = self.m2 / (k - 1)
        shrink = 1e-3 * (5.0 / (k + 5.0))
        if self.dense:
            return (k / (k + 5.0)) * c + shrink * np.eye(len(self.mean))
        return (k / (k + 5.0)) * c + shrink


class _DualAveraging:
    """Dual averaging of log step size: t0 = 10, kappa = 0.75, gamma = 0.05,
    mu = log(10 eps0)."""

    def __init__(self, eps0: float):
        self.mu = math.log(10.0 * eps0)
        self.t, self.hbar, self.log_eps, self.log_eps_bar = 0, 0.0, math.log(eps0), 0.0

    def step(self, accept: float, target: float) -> float:
        self.t += 1
        t = self.t
        self.hbar = (1.0 - 1.0 / (t + 10.0)) * self.hbar + (target - accept) / (t + 10.0)
        self.log_eps = self.mu - math.sqrt(t) / 0.05 * self.hbar
        eta = t ** -0.75
        self.log_eps_bar = eta * self.log_eps + (1.0 - eta) * self.log_eps_bar
        return math.exp(self.log_eps)

    def final(self) -> float:
        return math.exp(self.log_eps_bar)


def adaptation_windows(warmup_steps: int):
    """(first slow step, [window ends], end of the slow phase) of Stan's warmup
    schedule: initial buffer 75, terminal buffer 50, base window 25 doubling; 15 %
    / 75 % / 10 % below 150 steps; no mass adaptation below 20."""
    W = warmup_steps
    if W < 20:
        return W, [], W
    if W < 150:
        init, term = int(0.15 * W), int(0.10 * W)
        size = W - init - term
    else:
        init, term, size = 75, 50, 25
    slow_end = W - term
    ends, start = [], init
    while start < slow_end:
        end = start + size
        if end + 2 * size > slow_end:
            end = slow_end
        ends.append(end)
        start, size = end, 2 * size
    return init, ends, slow_end


def _logaddexp(a: float, b: float) -> float:
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = max(a, b)
    return m + math.log(math.exp(a - m) + math.exp(b - m))


class _Tree:
    __slots__ = ("zl", "rl", "gl", "zr", "rr", "gr", "zp", "Up", "gp", "logw", "rho", "sum_acc",
                 "leaves", "turning", "divergent")


class _Chain:
    """One chain.  ``run()`` is a generator: it yields z (numpy, D) whenever it
    needs the potential there and is sent back (U, grad, status)."""

    def __init__(self, k, z0, D, cfg):
        self.cfg = cfg
        self.D = D
        self.gen = torch.Generator().manual_seed(cfg["seed"] + k)
        self.z0 = None if z0 is None else np.array(z0, dtype=np.float64)
        self.mass = _Mass(D)
        self.rounds = 0
        self.samples = np.zeros((cfg["num_samples"], D))
        self.info = {}

    # -- random draws of this chain's own generator
    def _normal(self):
        return torch.randn(self.D, generator=self.gen, dtype=F64).numpy()

    def _uniform(self) -> float:
        return float(torch.rand(1, generator=self.gen, dtype=F64))

    def _eval(self, z):
        self.rounds += 1
        U, grad, status = yield z
        return float(U), np.asarray(grad, dtype=np.float64), int(status)

    def _leapfrog(self, z, r, grad, eps):
        r_half = r - 0.5 * eps * grad
        z1 = z + eps * self.mass.velocity(r_half)
        U1, g1, st = yield from self._eval(z1)
        r1 = r_half - 0.5 * eps * g1
        return z1, r1, U1, g1, st

    def _turning(self, t) -> bool:
        vl, vr = self.mass.velocity(t.rl), self.mass.velocity(t.rr)
        return bool(vl @ (t.rho - t.rl) <= 0.0 or vr @ (t.rho - t.rr) <= 0.0)

    def _build(self, z, r, grad, direction, depth, eps, H0):
        if depth == 0:
            z1, r1, U1, g1, st = yield from self._leapfrog(z, r, grad, direction * eps)
            H = U1 + self.mass.kinetic(r1)
            dH = H - H0
            t = _Tree()
            t.divergent = bool(st != 0 or not math.isfinite(H) or dH > 1000.0)
            t.logw = -math.inf if t.divergent else -dH
            t.sum_acc = 0.0 if t.divergent else min(1.0, math.exp(min(0.0, -dH)))
            t.leaves = 1
            t.zl = t.zr = t.zp = z1
            t.rl = t.rr = t.rho = r1
            t.gl = t.gr = t.gp = g1
            t.Up = U1
            t.turning = False
            return t
        a = yield from self._build(z, r, grad, direction, depth - 1, eps, H0)
        if a.divergent or a.turning:
            return a
        if direction > 0:
            b = yield from self._build(a.zr, a.rr, a.gr, direction, depth - 1, eps, H0)
        else:
            b = yield from self._build(a.zl, a.rl, a.gl, direction, depth - 1, eps, H0)
        u = self._uniform()
        t = _Tree()
        t.logw = _logaddexp(a.logw, b.logw)
        take_b = b.logw > -math.inf and math.log(u) < b.logw - t.logw if u > 0.0 else False
        src = b if take_b else a
        t.zp, t.Up, t.gp = src.zp, src.Up, src.gp
        lo, hi = (a, b) if direction > 0 else (b, a)
        t.zl, t.rl, t.gl = lo.zl, lo.rl, lo.gl
        t.zr, t.rr, t.gr = hi.zr, hi.rr, hi.gr
        t.rho = a.rho + b.rho
        t.sum_acc = a.sum_acc + b.sum_acc
        t.leaves = a.leaves + b.leaves
        t.divergent = b.divergent
        t.turning = b.turning or (not b.divergent and self._turning(t))
        return t

    def _transition(self, z, U, grad, eps):
        """One multinomial NUTS transition from (z, U, grad)."""
        r0 = self.mass.momentum(self._normal())
        H0 = U + self.mass.kinetic(r0)
        t = _Tree()
        t.zl = t.zr = t.zp = z
        t.rl = t.rr = t.rho = r0
        t.gl = t.gr = t.gp = grad
        t.Up, t.logw = U, 0.0
        sum_acc, leaves, depth, divergent = 0.0, 0, 0, False
        for j in range(self.cfg["max_tree_depth"]):
            direction = 1 if self._uniform() < 0.5 else -1
            u = self._uniform()
            if direction > 0:
                new = yield from self._build(t.zr, t.rr, t.gr, 1, j, eps, H0)
            else:
                new = yield from self._build(t.zl, t.rl, t.gl, -1, j, eps, H0)
            depth = j + 1
            sum_acc += new.sum_acc
            leaves += new.leaves
            if new.divergent:
                divergent = True
                break
            if new.turning:
                break
            if u > 0.0 and math.log(u) < new.logw - t.logw:
                t.zp, t.Up, t.gp = new.zp, new.Up, new.gp
            if direction > 0:
                t.zr, t.rr, t.gr = new.zr, new.rr, new.gr
            else:
                t.zl, t.rl, t.gl = new.zl, new.rl, new.gl
            t.rho = t.rho + new.rho
            t.logw = _logaddexp(t.logw, new.logw)
            if self._turning(t):
                break
        return t.zp, t.Up, t.gp, sum_acc / max(leaves, 1), depth, divergent, leaves

    def _find_step_size(self, z, U, grad, eps):
        """The doubling / halving heuristic (Hoffman & Gelman 2014, algorithm 4)."""
        r = self.mass.momentum(self._normal())
        H0 = U + self.mass.kinetic(r)

        def log_accept(eps):
            _, r1, U1, _, st = yield from self._leapfrog(z, r, grad, eps)
            H = U1 + self.mass.kinetic(r1)
            return -math.inf if (st != 0 or not math.isfinite(H)) else H0 - H
        la = yield from log_accept(eps)
        direction = 1 if la > math.log(0.5) else -1
        for _ in range(100):
            if not direction * la > -direction * math.log(2.0):
                break
            eps = eps * 2.0 ** direction
            la = yield from log_accept(eps)
        return eps

    def run(self):
        cfg = self.cfg
        D = self.D
        # the start: z0 given, or U(-2, 2)^D redrawn while the potential is not finite
        if self.z0 is not None:
            z = self.z0
            U, grad, st = yield from self._eval(z)
            if st != 0 or not math.isfinite(U):
                raise RuntimeError("run_nuts: the potential is not finite at the given start")
        else:
            for _ in range(100):
                z = 4.0 * torch.rand(D, generator=self.gen, dtype=F64).numpy() - 2.0
                U, grad, st = yield from self._eval(z)
                if st == 0 and math.isfinite(U):
                    break
            else:
                raise RuntimeError("run_nuts: no start with a finite potential in 100 draws")
        W, N = cfg["warmup_steps"], cfg["num_samples"]
        adapt_eps = cfg["adapt_step_size"] and W > 0
        eps = cfg["step_size"]
        if eps is None:
            eps = yield from self._find_step_size(z, U, grad, 1.0)
        da = _DualAveraging(eps) if adapt_eps else None
        init, ends, slow_end = adaptation_windows(W) if cfg["adapt_mass_matrix"] else (W, [], W)
        welford = _Welford(D, cfg["full_mass"])
        warm_div = 0
        for it in range(W):
            z, U, grad, acc, _, div, _ = yield from self._transition(z, U, grad, eps)
            warm_div += int(div)
            if adapt_eps:
                eps = da.step(acc, cfg["target_accept_prob"])
            if init <= it < slow_end:
                welford.add(z)
                if it + 1 in ends:
                    self.mass.set(welford.regularised(), cfg["full_mass"])
                    welford = _Welford(D, cfg["full_mass"])
                    if adapt_eps:
                        eps = yield from self._find_step_size(z, U, grad, eps)
                        da = _DualAveraging(eps)
        if adapt_eps:
            eps = da.final()
        depths, accs, divs, leaves = [], [], 0, 0
        for it in range(N):
            z, U, grad, acc, depth, div, nl = yield from self._transition(z, U, grad, eps)
            self.samples[it] = z
            depths.append(depth)
            accs.append(acc)
            divs += int(div)
            leaves += nl
        self.info = {"step_size": eps, "mean_accept": float(np.mean(accs)) if accs else math.nan,
                     "tree_depths": depths, "accept": accs, "divergences": divs,
                     "warmup_divergences": warm_div, "leapfrogs": leaves, "rounds": self.rounds}


def run_nuts(potential_fn: Callable, z0, *, warmup_steps: int, num_samples: int,
             max_tree_depth: int, full_mass: bool = True, step_size: Optional[float] = None,
             adapt_step_size: bool = True, adapt_mass_matrix: bool = True,
             target_accept_prob: float = 0.8, seed: Optional[int] = None):
    """Multinomial NUTS (Hoffman & Gelman 2014; Betancourt 2017) over a batched
    potential.

    potential_fn(z: C' x D host fp64) -> (U (C'), grad (C' x D), status (C')), on
    any device; a row with status != 0 (or a non-finite U) is a divergent leaf.
    z0: the starts (C x D), or a pair (C, D) for starts drawn from U(-2, 2)^D,
    redrawn up to 100 times while the potential is not finite.  Chain k draws
    from its own generator seeded ``seed + k``, so its draws do not depend on the
    chains beside it.  Returns (samples C x num_samples x D, info); info is a
    list of one record per chain (step_size, mean_accept, tree_depths,
    divergences, leapfrogs, rounds, ...) with the scheduler's total in
    ``info[k]["total_rounds"]``.  The sampler is specified in DESIGN.md section 22."""
    if isinstance(z0, Tensor):
        if z0.dim() != 2:
            raise ValueError("run_nuts: z0 must be C x D, or a pair (C, D)")
        C, D = z0.shape
        starts = [z0[k].detach().to("cpu", F64).numpy() for k in range(C)]
    else:
        C, D = (int(v) for v in z0)
        starts = [None] * C
    if C < 1 or D < 1 or num_samples < 0 or warmup_steps < 0 or max_tree_depth < 1:
        raise ValueError("run_nuts: C, D, max_tree_depth >= 1 and warmup_steps, num_samples >= 0")
    if seed is None:
        seed = int(torch.randint(2 ** 31 - 1, (1,)))
    cfg = dict(warmup_steps=warmup_steps, num_samples=num_samples, max_tree_depth=max_tree_depth,
               full_mass=full_mass, step_size=step_size, adapt_step_size=adapt_step_size,
               adapt_mass_matrix=adapt_mass_matrix, target_accept_prob=target_accept_prob,
               seed=int(seed))
    chains = [_Chain(k, starts[k], D, cfg) for k in range(C)]
    total = _drive([c.run() for c in chains], potential_fn)
    samples = torch.from_numpy(np.stack([c.samples for c in chains]))
    info = [dict(c.info, total_rounds=total) for c in chains]
    return samples, info


def _drive(gens, potential_fn: Callable) -> int:
    """The scheduler: run the generators to their ends, answering the pending
    requests of all live ones with one batched ``potential_fn`` call per round.
    Returns the number of rounds."""
    pending = {}
    for k, gen in enumerate(gens):
        try:
            pending[k] = next(gen)
        except StopIteration:
            pass
    total = 0
    while pending:
        live = sorted(pending)
        zb = torch.from_numpy(np.stack([pending[k] for k in live]))
        U, grad, status = potential_fn(zb)
        total += 1
        U = U.detach().to("cpu", F64).numpy()
        grad = grad.detach().to("cpu", F64).numpy()
        status = status.detach().to("cpu").numpy()
        pending = {}
        for row, k in enumerate(live):
            try:
                pending[k] = gens[k].send((U[row], grad[row], status[row]))
            except StopIteration:
                pass
    return total


def leapfrog(potential_fn: Callable, z: Tensor, r: Tensor, step_size: float, steps: int):
    """``steps`` leapfrog steps of the sampler's integrator (identity mass) from
    position z and momentum r (D each): (z', r').  A negative step size
    integrates backwards."""
    chain = _Chain(0, None, z.numel(), dict(seed=0, num_samples=0))
    out = {}

    def run():
        zz = z.detach().to("cpu", F64).numpy().copy()
        rr = r.detach().to("cpu", F64).numpy().copy()
        _, grad, _ = yield from chain._eval(zz)
        for _ in range(steps):
            zz, rr, _, grad, _ = yield from chain._leapfrog(zz, rr, grad, step_size)
        out["z"], out["r"] = zz, rr
    _drive([run()], potential_fn)
    return torch.from_numpy(out["z"]), torch.from_numpy(out["r"])
