#!/usr/bin/env python3
"""Time qNegIntegratedPosteriorVariance's fused route (bo::nipv_gram: the
cross-covariance with the integration points formed and contracted to its Gram
matrix on the matrix cores) against its generic route (posterior_moments on the
q points and chunks of the integration points, the Gram matrix in torch), on the
GPU, in one process.

Shape (defaults): n = 1024 training points, d = 6, N = 1024 integration points,
RBF; forward alone (no_grad) at B = 512 t-batches and forward + backward (dX)
at B = 16, each for q in {1, 4, 8}.
--runs alternating runs of each route (fused, generic, fused, ...); a run is
the median of --reps calls after --warmup untimed ones, each call between two
HIP events on the current stream.  Per shape: the agreement of the two routes
(values and dX, max relative difference), the peak transient memory of one call
of each route (torch's allocator; the fused route's stream-ordered workspace of
split x B q q resp. split x B q d doubles is added by its formula), and whether
the difference of the medians exceeds the run-to-run range of the five runs
(``fused_wins``: the slowest fused run is faster than the fastest generic run).

Writes one JSON object to --out (default profiles/nipv/bench.json) and prints it
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


def _peak(fn):
    """Peak bytes above the resting level of one call (torch's allocator)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def _workspace_bytes(B, q, d, N, backward):
    """The fused route's stream-ordered workspace: the slice count by size of
    csrc/nipv.hip times the partial output."""
    tiles = -(-B // (16 // q))
    split = max(1, min(-(-256 // tiles), -(-N // 64), -(-N // 16)))
    zlen = 16 * -(-(-(-N // split)) // 16)
    split = -(-N // zlen)
    if split == 1:
        return 0
    return 8 * split * B * q * (q + (d if backward else 0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--B-forward", type=int, default=512)
    ap.add_argument("--B-backward", type=int, default=16)
    ap.add_argument("--qs", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nipv", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nipv: needs the GPU (no CPU timing)")
    from botorch_amd import kernels
    from botorch_amd.acquisition import qNegIntegratedPosteriorVariance
    from botorch_amd.models import SingleTaskGP
    n, d, N = args.n, args.d, args.N
    g = torch.Generator().manual_seed(0)
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    Y = (torch.sin(4 * Xt).sum(-1, keepdim=True) + 0.1 * torch.randn(n, 1, generator=g, dtype=F64))
    model = SingleTaskGP(Xt.to(DEV), Y.to(DEV))
    model.covar_module.lengthscale = torch.full((1, d), 0.5, dtype=F64)
    model.likelihood.noise = torch.tensor([1e-2], dtype=F64)
    model.eval()
    Z = torch.rand(N, d, generator=g, dtype=F64).to(DEV)
    acqf = qNegIntegratedPosteriorVariance(model, Z)

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
            back = what != "forward"
            peak = dict(fused_bytes=_peak(fused) + _workspace_bytes(B, q, d, N, back),
                        fused_workspace_bytes=_workspace_bytes(B, q, d, N, back),
                        generic_bytes=_peak(generic))
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
                             speedup=round(med_g / med_f, 2), fused_wins=max(t_f) < min(t_g),
                             generic_wins=max(t_g) < min(t_f), peak_transient=peak,
                             max_rel_difference=agree))
    acqf._route = None
    res = dict(tool="bench_nipv", device=torch.cuda.get_device_name(0), n=n, d=d, N=N, kind="rbf",
               runs=args.runs, warmup=args.warmup, reps=args.reps, results=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
