"""Generate ``golden_logehvi.npz``: the reference's log-space hypervolume
improvement (qLogEHVI / qLogNEHVI) on recorded samples, values and gradients.

Runs ONLY in the development container, where the reference tree exists (see
``_refload.py``).  ``acquisition/multi_objective/logei.py`` itself pulls in
gpytorch and cannot be imported, so ``ref_log_qehvi`` below composes the
reference's own ``botorch/utils/safe_math.py`` functions step by step as
``_compute_log_qehvi`` does (logei.py:147-310; the steps cite its lines), on
cells of the reference's FastNondominatedPartitioning
(utils/multi_objective/box_decompositions/non_dominated.py).

Usage:  python tests/golden/make_golden_logehvi.py

Recorded per case ``<tag>``: ``<tag>_acq`` (b), ``<tag>_dobj`` (S x b x q x m)
and, with feasibility weights, ``<tag>_dlogw`` (S x b x q), the gradients of
acq.sum(); ``fn_*``: the reference's smooth functions on their own (see
``function_fixtures``).  Inputs per input set ``<inp>``: ``<inp>_obj``, ``<inp>_logw``,
``<inp>_lo`` / ``<inp>_hi`` (shared cells, K x m), ``<inp>_lo_s`` / ``<inp>_hi_s``
(per-sample cells S x K' x m, zero-padded as BoxDecompositionList pads them,
box_decomposition_list.py:62-94).
"""
import os
import sys
from itertools import combinations

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

S, B = 8, 2
TAUS = {"d": (1e-6, 1e-2), "n": (1e-6, 1e-3), "w": (1e-3, 1e-1)}  # (tau_relu, tau_max)


def case_table():
    """(tag, input set, fat, tau key, per-sample cells, with logw).  Every
    (m, q) with the qLogEHVI defaults on shared cells and with the sharp
    qLogNEHVI temperatures, fat off, on per-sample cells with weights; every
    (fat, temperatures, cells / weights) combination at (m, q) = (2, 3) and
    (3, 2); the hopeless set with both fat values."""
    cases = []
    for m in (2, 3):
        for q in (1, 2, 3, 4):
            inp = f"m{m}q{q}"
            cases.append((inp, True, "d", False, False))
            cases.append((inp, False, "n", True, True))
    for inp in ("m2q3", "m3q2"):
        for fat in (True, False):
            for tk in TAUS:
                for per_sample, with_w in ((False, False), (True, True), (False, True)):
                    cases.append((inp, fat, tk, per_sample, with_w))
    for fat in (True, False):
        cases.append(("hopeless", fat, "d", False, False))
    out, seen = [], set()
    for inp, fat, tk, ps, ww in cases:
        tag = f"{inp}_{'fat' if fat else 'nofat'}_{tk}_{'ps' if ps else 'sh'}_{'w' if ww else 'u'}"
        if tag not in seen:
            seen.add(tag)
            out.append((tag, inp, fat, tk, ps, ww))
    return out


def ref_log_qehvi(sm, obj, lo, hi, logw, fat, tau_relu, tau_max):
    """The reference's log-space reduction (logei.py:147-267) on objective
    samples S x b x q x m, written here with the reference's ``sm`` functions;
    the comments cite the step of logei.py each line stands for."""
    relu = sm.log_fatplus if fat else sm.log_softplus                 # :300-302
    smin = sm.fatmin if fat else sm.smooth_amin                       # :304-306
    n_s, n_b, q, m = obj.shape
    K = lo.shape[-2]
    # cells against S x b x K x (subsets) x m: shared cells broadcast over the
    # samples, per-sample cells (S x K x m) carry them (:185-201)
    cshape = (n_s if lo.dim() == 3 else 1, 1, K, 1, m)
    lower = lo.reshape(cshape)
    side = (hi.clamp_max(1e10) - lo).log().reshape(cshape)            # :287-293
    parity = [torch.full((n_s, n_b, K), float("-inf"), dtype=obj.dtype) for _ in range(2)]  # :174-183
    for size in range(1, q + 1):                                      # :203
        members = torch.tensor(list(combinations(range(q), size)), dtype=torch.long)  # C x size
        pts = obj[:, :, members]                                      # S x b x C x size x m (:208-213)
        li = relu(pts.unsqueeze(2) - lower.unsqueeze(-2), tau=tau_relu)   # step 1, :221, 269-282
        li = smin(li, dim=-2, tau=tau_max)                            # step 2, :227-230
        pair = torch.stack((li, side.expand_as(li)), dim=-1)          # step 3, :234, 308-310
        area = smin(pair, dim=-1, tau=tau_max).sum(dim=-1)            # step 4, :238
        if logw is not None:                                          # step 5, :242-246
            area = area + logw[:, :, members].sum(dim=-1).unsqueeze(2)
        total = sm.logsumexp(area, dim=-1)                            # step 6, :250
        parity[size % 2] = sm.logplusexp(parity[size % 2], total)     # step 7, :256-259
    cell = sm.logdiffexp(log_a=parity[0], log_b=parity[1])            # step 8, :262-264
    return sm.logmeanexp(sm.logsumexp(cell, dim=-1), dim=0)           # step 9, :267


def function_fixtures(sm, out):
    """Outputs of the reference's own smooth functions (safe_math.py:72-121,
    276-283, 355-419) on recorded inputs, with the gradients of the two
    minima: ``fn_*``."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(6, 5, generator=g, dtype=torch.double)
    y = torch.randn(6, 5, generator=g, dtype=torch.double)
    x[0, 1] = x[0, 3]                       # a tie
    x[1, 2] = float("-inf")                 # an infinite entry
    z = -torch.logspace(-12, 2, 57, dtype=torch.double)
    out["fn_x"], out["fn_y"], out["fn_z"] = x.numpy(), y.numpy(), z.numpy()
    for tau in (1e-1, 1e-3):
        t = f"{tau:g}"
        out[f"fn_fatmin_{t}"] = sm.fatmin(x, dim=-1, tau=tau).numpy()
        out[f"fn_smooth_amin_{t}"] = sm.smooth_amin(x, dim=-1, tau=tau).numpy()
        out[f"fn_fatminimum_{t}"] = sm.fatminimum(x, y, tau=tau).numpy()
        for name in ("fatmin", "smooth_amin"):
            xf = x[2:].clone().requires_grad_(True)     # the finite rows
            (gx,) = torch.autograd.grad(getattr(sm, name)(xf, dim=-1, tau=tau).sum(), xf)
            out[f"fn_{name}_{t}_grad"] = gx.numpy()
    out["fn_logplusexp"] = sm.logplusexp(x, y).numpy()
    out["fn_log1mexp"] = sm.log1mexp(z).numpy()
    xf, yf = x[2:], y[2:]
    out["fn_logdiffexp"] = sm.logdiffexp(torch.minimum(xf, yf) - 0.5, torch.maximum(xf, yf)).numpy()
    ninf = torch.full((3,), float("-inf"), dtype=torch.double)
    out["fn_logdiffexp_inf"] = sm.logdiffexp(ninf, torch.cat([ninf[:1], x[3, :2]])).numpy()


def make_inputs(nd, out):
    g = torch.Generator().manual_seed(31)
    dd = dict(generator=g, dtype=torch.double)

    def front(m, n):
        Y = 0.7 + 0.15 * torch.randn(n, m, **dd)
        ref = torch.zeros(m, dtype=torch.double)
        cb = nd.FastNondominatedPartitioning(ref_point=ref, Y=Y).get_hypercell_bounds()
        return cb[0], cb[1]

    def one(inp, m, q, centre, spread):
        obj = centre + spread * torch.randn(S, B, q, m, **dd)
        w = torch.rand(S, B, q, **dd)
        w[torch.rand(S, B, q, **dd) < 0.25] = 1.0      # log weight exactly 0.0
        lo, hi = front(m, 5)
        # per-sample cells: samples have fronts of different sizes and are
        # padded with lo = hi = 0 cells to the common count + 2
        per = [front(m, 2 + s % 3) for s in range(S)]
        Kmax = max(p[0].shape[0] for p in per) + 2
        lo_s = torch.zeros(S, Kmax, m, dtype=torch.double)
        hi_s = torch.zeros(S, Kmax, m, dtype=torch.double)
        for s, (l_, h_) in enumerate(per):
            lo_s[s, : l_.shape[0]], hi_s[s, : h_.shape[0]] = l_, h_
        for k, v in (("obj", obj), ("logw", w.log()), ("lo", lo), ("hi", hi), ("lo_s", lo_s),
                     ("hi_s", hi_s)):
            out[f"{inp}_{k}"] = v.numpy()

    for m in (2, 3):
        for q in (1, 2, 3, 4):
            one(f"m{m}q{q}", m, q, 0.6, 0.25)
    one("hopeless", 2, 4, 0.2, 0.02)


def main():
    sm = _refload.load("botorch.utils.safe_math")
    nd = _refload.load("botorch.utils.multi_objective.box_decompositions.non_dominated")
    out = {}
    make_inputs(nd, out)
    for tag, inp, fat, tk, per_sample, with_w in case_table():
        tau_relu, tau_max = TAUS[tk]
        obj = torch.from_numpy(out[f"{inp}_obj"]).clone().requires_grad_(True)
        logw = torch.from_numpy(out[f"{inp}_logw"]).clone().requires_grad_(True) if with_w else None
        sfx = "_s" if per_sample else ""
        lo, hi = (torch.from_numpy(out[f"{inp}_{k}{sfx}"]) for k in ("lo", "hi"))
        acq = ref_log_qehvi(sm, obj, lo, hi, logw, fat, tau_relu, tau_max)
        grads = torch.autograd.grad(acq.sum(), [obj] + ([logw] if with_w else []))
        assert torch.isfinite(acq).all() and all(torch.isfinite(g_).all() for g_ in grads), tag
        out[f"{tag}_acq"] = acq.detach().numpy()
        out[f"{tag}_dobj"] = grads[0].numpy()
        if with_w:
            out[f"{tag}_dlogw"] = grads[1].numpy()
    function_fixtures(sm, out)
    path = os.path.join(HERE, "golden_logehvi.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
