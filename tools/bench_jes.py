#!/usr/bin/env python3
"""Time qJointEntropySearch's fused route (bo::jes: the covariance with the
optima formed on the matrix cores, the entropy chain on the accumulator)
against its generic route (posterior_moments on the q + P points, the chain in
torch), on the GPU, in one process.

Shape (defaults): n = 1024 training points, d = 6, P = 64 optima, RBF;
forward alone (no_grad) at B = 512 t-batches and forward + backward (dX) at
B = 16, each for q in {1, 4, 8}.
--runs alternating runs of each route (fused, generic, fused, ...); a run is
the median of --reps calls after --warmup untimed ones, each call between two
HIP events on the current stream.  The agreement of the two routes (values and
dX, max relative difference) is recorded per shape.

Writes one JSON object to --out (default profiles/jes/bench.json) and prints it
on one line.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--P", type=int, default=64)
    ap.add_argument("--B-forward", type=int, default=512)
    ap.add_argument("--B-backward", type=int, default=16)
    ap.add_argument("--qs", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jes", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jes: needs the GPU (no CPU timing)")
    from botorch_amd import kernels
    from botorch_amd.acquisition import qJointEntropySearch
    from botorch_amd.models import SingleTaskGP
    n, d, P = args.n, args.d, args.P
    g = torch.Generator().manual_seed(0)
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    Y = (torch.sin(4 * Xt).sum(-1, keepdim=True) + 0.1 * torch.randn(n, 1, generator=g, dtype=F64))
    model = SingleTaskGP(Xt.to(DEV), Y.to(DEV))
    model.covar_module.lengthscale = torch.full((1, d), 0.5, dtype=F64)
    model.likelihood.noise = torch.tensor([1e-2], dtype=F64)
    model.eval()
    Xo = torch.rand(P, d, generator=g, dtype=F64).to(DEV)
    with torch.no_grad():
        grid = torch.rand(2048, 1, d, generator=g, dtype=F64).to(DEV)
        top = model.posterior(torch.cat([grid, Xo.unsqueeze(1)])).mean.max()
        fo = top + 0.1 + 0.5 * torch.rand(P, 1, generator=g, dtype=F64).to(DEV)
    acqf = qJointEntropySearch(model, Xo, fo)

    def forward_fn(X, route):
        def fn():
            acqf._route = route
            with torch.no_grad():
                return acqf(X)
        return fn

    def backward_fn(X, route):
        def fn():
            acqf._route = route
            Xg = X.detach().requires_grad_(True)
            val = acqf(Xg)
            (gx,) = torch.autograd.grad(val.sum(), Xg)
            return val.detach(), gx
        return fn

    rows = []
    for q in args.qs:
        for what, B, make in (("forward", args.B_forward, forward_fn),
                              ("forward_backward", args.B_backward, backward_fn)):
            X = torch.rand(B, q, d, generator=g, dtype=F64).to(DEV)
            fused, generic = make(X, "fused"), make(X, "generic")
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
            rows.append(dict(what=what, B=B, q=q, fused_ms=t_f, generic_ms=t_g,
                             fused_median_ms=med_f, generic_median_ms=med_g,
                             speedup=round(med_g / med_f, 2), max_rel_difference=agree))
    acqf._route = None
    res = dict(tool="bench_jes", device=torch.cuda.get_device_name(0), n=n, d=d, P=P, kind="rbf",
               runs=args.runs, warmup=args.warmup, reps=args.reps, results=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
