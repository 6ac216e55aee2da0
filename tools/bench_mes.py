#!/usr/bin/env python3
"""Time the fused routes of qMaxValueEntropy (bo::mes) and
qLowerBoundMaxValueEntropy (bo::gibbon) against their generic routes (the
reference's formulation as broadcast torch tensors on the same
posterior_moments), on the GPU, in one process, and the construction with the
on-device quantile bisection (bo::mv_quantiles) against the same construction
with the quantiles found by scipy's brentq on host copies.

Shape (defaults): n = 1024 training points, d = 6, RBF, 1000 candidates,
S_M = 10 max values, S_m = 128 base samples; forward alone (no_grad) at
B = 16384 and B = 512 t-batches, forward + backward (dX) at B = 16, at points
scattered around the best training points; GIBBON without and with 4 pending
points.
--runs alternating runs of each route (fused, generic, fused, ...); a run is
the median of --reps calls after --warmup untimed ones, each call between two
HIP events on the current stream.  ``fused_wins`` says whether the fused
median beats the generic one by more than the larger run-to-run range of the
two.  The peak transient memory of one forward of each route is recorded at
the largest B, and the agreement of the two routes per shape.

Writes one JSON object to --out (default profiles/mes/bench.json) and prints it
on one line.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
F64 = torch.float64


def _timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times)


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def _peak_mb(fn):
    """Peak memory above the resident level during one call, in MB."""
    from botorch_amd import kernels
    fn()
    kernels.drop_keepalive()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    kernels.drop_keepalive()
    return round(peak / 2 ** 20, 1)


def _gumbel_brentq(model, candidate_set, num_samples, posterior_transform=None, maximize=True):
    """The reference's _sample_max_value_Gumbel: the quantiles by brentq on numpy
    copies of the candidate set's posterior (lines 994-1010), the rest alike."""
    import numpy as np
    from scipy.optimize import brentq
    from scipy.stats import norm
    from botorch_amd.acquisition import _mv_moments
    mu, sigma = _mv_moments(model, candidate_set, maximize)
    lo, hi = (mu - 3 * sigma).min().item(), (mu + 5 * sigma).max().item()
    dist = norm(mu.cpu().numpy(), sigma.cpu().numpy())
    q25, q50, q75 = (brentq(lambda y: np.exp(np.sum(dist.logcdf(y))) - p, lo, hi)
                     for p in (0.25, 0.5, 0.75))
    b = (q25 - q75) / (math.log(math.log(4.0 / 3.0)) - math.log(math.log(4.0)))
    a = q50 + b * math.log(math.log(2.0))
    eps = torch.rand(num_samples, 1, device=mu.device, dtype=mu.dtype)
    return a - b * eps.log().mul(-1.0).log()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--num-mv-samples", type=int, default=10)
    ap.add_argument("--num-y-samples", type=int, default=128)
    ap.add_argument("--B-forward", type=int, nargs="+", default=[16384, 512])
    ap.add_argument("--B-backward", type=int, default=16)
    ap.add_argument("--pending", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mes", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mes: needs the GPU (no CPU timing)")
    from botorch_amd import acquisition, kernels
    from botorch_amd.acquisition import qLowerBoundMaxValueEntropy, qMaxValueEntropy
    from botorch_amd.models import SingleTaskGP
    n, d = args.n, args.d
    g = torch.Generator().manual_seed(0)
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    Y = (torch.sin(4 * Xt).sum(-1, keepdim=True) + 0.1 * torch.randn(n, 1, generator=g, dtype=F64))
    model = SingleTaskGP(Xt.to(DEV), Y.to(DEV))
    model.covar_module.lengthscale = torch.full((1, d), 0.5, dtype=F64)
    model.likelihood.noise = torch.tensor([1e-2], dtype=F64)
    model.eval()
    cand = torch.rand(args.candidates, d, generator=g, dtype=F64).to(DEV)
    torch.manual_seed(0)
    kw = dict(num_mv_samples=args.num_mv_samples)
    mes = qMaxValueEntropy(model, cand, num_y_samples=args.num_y_samples, **kw)
    gib = qLowerBoundMaxValueEntropy(model, cand, **kw)
    gibp = qLowerBoundMaxValueEntropy(
        model, cand, X_pending=torch.rand(args.pending, d, generator=g, dtype=F64).to(DEV), **kw)

    def forward_fn(acqf, X, route):
        def fn():
            acqf._route = route
            with torch.no_grad():
                return acqf(X)
        return fn

    def backward_fn(acqf, X, route):
        def fn():
            acqf._route = route
            Xg = X.detach().requires_grad_(True)
            val = acqf(Xg)
            (gx,) = torch.autograd.grad(val.sum(), Xg)
            return val.detach(), gx
        return fn

    best = Xt[Y.reshape(-1).topk(min(n, 64)).indices]

    def points(B):
        """B x 1 x d points around the best training points (sigma 0.05, clipped
        to the unit cube): where an optimiser's iterates lie, and where both
        acquisition functions have a gradient above rounding."""
        X = best[torch.randint(best.shape[0], (B,), generator=g)]
        X = X + 0.05 * torch.randn(B, d, generator=g, dtype=F64)
        return X.clamp(0.0, 1.0).unsqueeze(1).to(DEV)

    rows = []
    shapes = [("forward", B, forward_fn) for B in args.B_forward]
    shapes.append(("forward_backward", args.B_backward, backward_fn))
    for name, acqf in (("qMaxValueEntropy", mes), ("qLowerBoundMaxValueEntropy", gib),
                       (f"qLowerBoundMaxValueEntropy, {args.pending} pending", gibp)):
        for what, B, make in shapes:
            X = points(B)
            fused, generic = make(acqf, X, "fused"), make(acqf, X, "generic")
            a, b = fused(), generic()
            if what == "forward":
                agree = dict(value=_rel(a, b))
            else:
                # (the acquisition is flat to rounding at most of these points, so
                # the absolute difference is recorded next to the relative one)
                agree = dict(value=_rel(a[0], b[0]), dX=_rel(a[1], b[1]),
                             dX_max_abs_difference=(a[1] - b[1]).abs().max().item(),
                             dX_max_abs=b[1].abs().max().item())
            del a, b
            kernels.drop_keepalive()
            t_f, t_g = [], []
            for _ in range(args.runs):
                t_f.append(round(_timed(fused, args.warmup, args.reps), 4))
                kernels.drop_keepalive()
                t_g.append(round(_timed(generic, args.warmup, args.reps), 4))
                kernels.drop_keepalive()
            med_f, med_g = statistics.median(t_f), statistics.median(t_g)
            spread = max(max(t_f) - min(t_f), max(t_g) - min(t_g))
            row = dict(acqf=name, what=what, B=B, fused_ms=t_f, generic_ms=t_g,
                       fused_median_ms=med_f, generic_median_ms=med_g,
                       speedup=round(med_g / med_f, 2), run_to_run_range_ms=round(spread, 4),
                       fused_wins=bool(med_g - med_f > spread), max_rel_difference=agree)
            if what == "forward" and B == max(args.B_forward):
                row["peak_transient_mb"] = dict(fused=_peak_mb(fused), generic=_peak_mb(generic))
            rows.append(row)
        acqf._route = None

    # construction: the on-device bisection against brentq on host copies
    def construct():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        qLowerBoundMaxValueEntropy(model, cand, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    device_sampler = acquisition._sample_max_value_Gumbel
    t_dev, t_host = [], []
    for _ in range(args.runs):
        acquisition._sample_max_value_Gumbel = device_sampler
        construct()
        t_dev.append(round(statistics.median(construct() for _ in range(args.reps)), 4))
        acquisition._sample_max_value_Gumbel = _gumbel_brentq
        construct()
        t_host.append(round(statistics.median(construct() for _ in range(args.reps)), 4))
    acquisition._sample_max_value_Gumbel = device_sampler
    construction = dict(what="construction, Gumbel max values (wall clock, ms)",
                        candidates=args.candidates + n, device_bisection_ms=t_dev,
                        host_brentq_ms=t_host,
                        device_median_ms=statistics.median(t_dev),
                        host_median_ms=statistics.median(t_host))
    res = dict(tool="bench_mes", device=torch.cuda.get_device_name(0), n=n, d=d, kind="rbf",
               candidates=args.candidates, num_mv_samples=args.num_mv_samples,
               num_y_samples=args.num_y_samples, runs=args.runs, warmup=args.warmup,
               reps=args.reps, results=rows, construction=construction)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
