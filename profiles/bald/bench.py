#!/usr/bin/env python3
"""Time qBayesianActiveLearningByDisagreement's fused route (bo::bald: every
sample under every component of the mixture posterior in registers) against its
generic route (the same formula in torch on model.posterior, in chunks of
t-batches), on the GPU, in one process.

Shape (defaults, the C5 configuration): n = 256 training points, d = 50, M = 16
SAAS-prior members, Matern-5/2, S = 512 base samples; forward alone (no_grad) at
B = 512 t-batches and forward + backward (dX) at B = 16, each for q in {1, 4, 8}.
--runs alternating runs of each route (fused, generic, fused, ...); a run is
the median of --reps calls after --warmup untimed ones, each call between two
HIP events on the current stream.  Per shape: the agreement of the two routes
(values and dX, max relative difference), the peak transient memory of one call
of each route (torch's allocator, which also serves the fused route's scratch),
and whether the difference of the medians exceeds the run-to-run range of the
runs (``fused_wins``: the slowest fused run is faster than the fastest generic
run).

Writes one JSON object to --out (default profiles/bald/bench.json) and prints it
on one line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--S", type=int, default=512)
    ap.add_argument("--B-forward", type=int, default=512)
    ap.add_argument("--B-backward", type=int, default=16)
    ap.add_argument("--qs", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bald", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profiles/bald/bench.py: needs the GPU (no CPU timing)")
    from botorch_amd import kernels
    from botorch_amd.acquisition import qBayesianActiveLearningByDisagreement
    from botorch_amd.models import SaasFullyBayesianSingleTaskGP, sample_saas_prior
    from botorch_amd.sampling import SobolQMCNormalSampler
    from botorch_amd.test_functions import Hartmann
    n, d, M, S = args.n, args.d, args.M, args.S
    g = torch.Generator().manual_seed(0)
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    Y = Hartmann(negate=True)(Xt[:, :6]).unsqueeze(-1)
    Y = (Y - Y.mean()) / Y.std()
    model = SaasFullyBayesianSingleTaskGP(Xt.to(DEV), Y.to(DEV))
    model.load_mcmc_samples({k: v.to(DEV) for k, v in sample_saas_prior(d, M, seed=0).items()})
    model.eval()
    acqf = qBayesianActiveLearningByDisagreement(
        model, sampler=SobolQMCNormalSampler(torch.Size([S]), seed=0))
    routes = dict(fused=acqf, generic=acqf._generic)

    def forward_fn(X, route):
        def fn():
            with torch.no_grad():
                return routes[route](X)
        return fn

    def backward_fn(X, route):
        def fn():
            Xg = X.detach().requires_grad_(True)
            val = routes[route](Xg)
            (gx,) = torch.autograd.grad(val.sum(), Xg)
            return val.detach(), gx
        return fn

    rows = []
    for q in args.qs:
        for what, B, make in (("forward", args.B_forward, forward_fn),
                              ("forward_backward", args.B_backward, backward_fn)):
            X = torch.rand(B, q, d, generator=g, dtype=F64).to(DEV)
            assert acqf._fused_ok(X)
            fused, generic = make(X, "fused"), make(X, "generic")
            a, b = fused(), generic()
            if what == "forward":
                agree = dict(value=_rel(a, b))
            else:
                agree = dict(value=_rel(a[0], b[0]), dX=_rel(a[1], b[1]))
            del a, b
            kernels.drop_keepalive()
            peak = dict(fused_bytes=_peak(fused), generic_bytes=_peak(generic))
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
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    res = dict(tool="profiles/bald/bench.py", device=torch.cuda.get_device_name(0), n=n, d=d, M=M,
               S=S, kind="matern52", runs=args.runs, warmup=args.warmup, reps=args.reps,
               results=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
