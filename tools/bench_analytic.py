#!/usr/bin/env python3
"""Time the fused route of LogExpectedImprovement and
LogConstrainedExpectedImprovement (posterior moments -> bo::analytic, one
launch each way) against their generic route (the same moments, then the
reference's chain of small torch launches), on the GPU, in one process.

Shape (defaults): n = 1024 training points, d = 6, RBF; LogEI over one model,
LogCEI with 3 constraints (one lower, one upper, one two-sided) over a 4-member
ModelListGP; forward alone (no_grad) at B = 512 and B = 16384 t-batches, forward +
backward (dX) at B = 16, at points scattered around the best training points.
--runs alternating runs of each route (fused, generic, fused, ...); a run is
the median of --reps calls after --warmup untimed ones, each call between two
HIP events on the current stream.  ``fused_wins`` says whether the fused
median beats the generic one by more than the larger run-to-run range of the
two.  The peak transient memory of one forward of each route is recorded at
the largest B, and the agreement of the two routes per shape.

Writes one JSON object to --out (default profiles/analytic/bench.json) and
prints it on one line.
"""
import argparse
import json
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--B-forward", type=int, nargs="+", default=[512, 16384])
    ap.add_argument("--B-backward", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "analytic", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_analytic: needs the GPU (no CPU timing)")
    from botorch_amd import kernels
    from botorch_amd.acquisition import LogConstrainedExpectedImprovement, LogExpectedImprovement
    from botorch_amd.models import ModelListGP, SingleTaskGP
    n, d = args.n, args.d
    g = torch.Generator().manual_seed(0)
    Xt = torch.rand(n, d, generator=g, dtype=F64)

    def member(t):
        Y = torch.sin(4 * Xt + t).sum(-1, keepdim=True) + 0.1 * torch.randn(n, 1, generator=g,
                                                                             dtype=F64)
        mm = SingleTaskGP(Xt.to(DEV), Y.to(DEV))
        mm.covar_module.lengthscale = torch.full((1, d), 0.5, dtype=F64)
        mm.likelihood.noise = torch.tensor([1e-2], dtype=F64)
        return mm, Y

    members = [member(t) for t in range(4)]
    single, Y0 = members[0]
    single.eval()
    mlist = ModelListGP(*[mm for mm, _ in members]).eval()
    best_f = Y0.max().item()
    acqfs = [("LogExpectedImprovement", LogExpectedImprovement(single, best_f)),
             ("LogConstrainedExpectedImprovement, 3 constraints, 4 members",
              LogConstrainedExpectedImprovement(mlist, best_f, 0, {1: (-1.0, None), 2: (None, 1.5),
                                                                    3: (-2.0, 2.0)}))]

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

    best = Xt[Y0.reshape(-1).topk(min(n, 64)).indices]

    def points(B):
        """B x 1 x d points around the best training points (sigma 0.05, clipped
        to the unit cube): where an optimiser's iterates lie."""
        X = best[torch.randint(best.shape[0], (B,), generator=g)]
        X = X + 0.05 * torch.randn(B, d, generator=g, dtype=F64)
        return X.clamp(0.0, 1.0).unsqueeze(1).to(DEV)

    rows = []
    shapes = [("forward", B, forward_fn) for B in args.B_forward]
    shapes.append(("forward_backward", args.B_backward, backward_fn))
    for name, acqf in acqfs:
        for what, B, make in shapes:
            X = points(B)
            fused, generic = make(acqf, X, "fused"), make(acqf, X, "generic")
            a, b = fused(), generic()
            if what == "forward":
                agree = dict(value=_rel(a, b))
            else:
                agree = dict(value=_rel(a[0], b[0]), dX=_rel(a[1], b[1]))
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
    res = dict(tool="bench_analytic", device=torch.cuda.get_device_name(0), n=n, d=d, kind="rbf",
               runs=args.runs, warmup=args.warmup, reps=args.reps, results=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
