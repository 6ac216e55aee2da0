#!/usr/bin/env python3
"""Time the PairwiseGP paths on the GPU, in one process.

closure    the closure of fit_gpytorch_mll (Laplace value + gradient, ending in its
           device-to-host transfer): the fused route (one bo_pairwise_laplace launch)
           against the torch route on the device, warm-started from the previous MAP
           utility and cold (the win-count start), host clock.  ``iters``: the Newton
           iterations of either start.
posterior  model.posterior forward at B = 512, q = 2, and forward + backward at B = 16,
           q = 2, fused against torch route (HIP events); the Laplace cache is built
           before the clock starts.
fit        a whole fit_gpytorch_mll from the default start at n = 256, a fresh model per
           call (host clock, one call per run).

n = 64, 256, 512 with m = 4 n, and n = 1024 with m = 4096; d = 6.  --runs alternating runs
of each route (a, b, a, ...); a run is the median of --reps calls after --warmup untimed
ones.  ``a_wins``: the slowest run of the fused route beats the fastest of the torch
route.  Writes one JSON object to --out and prints it on one line."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV, F64 = "cuda", torch.float64


def _timed(fn, warmup, reps, events):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        if events:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        else:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def _alternate(a, b, runs, warmup, reps, events):
    ra, rb = [], []
    for _ in range(runs):
        ra.append(_timed(a, warmup, reps, events))
        rb.append(_timed(b, warmup, reps, events))
    return {"a_ms": {"median": statistics.median(ra), "min": min(ra), "max": max(ra)},
            "b_ms": {"median": statistics.median(rb), "min": min(rb), "max": max(rb)},
            "a_wins": max(ra) < min(rb), "b_wins": max(rb) < min(ra)}


def _data(n, m, d):
    g = torch.Generator().manual_seed(n)
    X = torch.rand(n, d, generator=g, dtype=F64)
    util = torch.sin(3.0 * X.sum(-1))
    i = torch.randint(0, n, (m,), generator=g)
    j = (i + 1 + torch.randint(0, n - 1, (m,), generator=g)) % n
    swap = util[i] < util[j]
    return X.to(DEV), torch.stack([torch.where(swap, j, i), torch.where(swap, i, j)], -1).to(DEV)


def _routed(m, route, fn, cold=False):
    def call():
        m._route = route
        if cold:
            m._x0 = None
        try:
            return fn()
        finally:
            m._route = None
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[64, 256, 512, 1024])
    ap.add_argument("--fit-n", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise", "bench.json"))
    args = ap.parse_args()
    from botorch_amd import fit
    from botorch_amd.models import PairwiseGP, PairwiseLaplaceMarginalLogLikelihood
    warnings.simplefilter("ignore")  # (the cap's NumericalWarning, once per closure)
    d, rows = 6, []
    alt = lambda a, b, events: _alternate(a, b, args.runs, args.warmup, args.reps, events)
    for n in args.ns:
        X, comp = _data(n, 4 * n, d)
        m = PairwiseGP(X, comp)
        lay = fit._layout(m)
        x = lay.get()
        hyper = m.hyper_vector().reshape(1, -1).to(DEV)
        iters = {}
        for route in ("fused", "torch"):
            m._route, m._x0 = route, None
            cold = int(m.laplace(hyper, want_grad=True)["iters"][0])
            iters[route] = {"cold": cold, "warm": int(m.laplace(hyper, want_grad=True)["iters"][0])}
        m._route = None
        g = torch.Generator().manual_seed(1)
        Xf = torch.rand(512, 2, d, generator=g, dtype=F64).to(DEV)
        Xb = torch.rand(16, 2, d, generator=g, dtype=F64).to(DEV).requires_grad_(True)
        m._laplace()

        def fwd():
            with torch.no_grad():
                return m.posterior(Xf).distribution.covariance_matrix

        def fwd_bwd():
            post = m.posterior(Xb)
            return torch.autograd.grad(post.mean.sum() + post.distribution.covariance_matrix.sum(), Xb)

        closure = lambda: lay.value_and_grad(x)
        row = {"n": n, "m": 4 * n, "d": d, "newton_iterations": iters,
               "closure_warm_fused_vs_torch": alt(_routed(m, "fused", closure),
                                                  _routed(m, "torch", closure), False),
               "closure_cold_fused_vs_torch": alt(_routed(m, "fused", closure, cold=True),
                                                  _routed(m, "torch", closure, cold=True), False),
               "posterior_fwd_B512_q2_fused_vs_torch": alt(_routed(m, "fused", fwd),
                                                           _routed(m, "torch", fwd), True),
               "posterior_fwd_bwd_B16_q2_fused_vs_torch": alt(_routed(m, "fused", fwd_bwd),
                                                              _routed(m, "torch", fwd_bwd), True)}
        rows.append(row)
        print(json.dumps(row), flush=True)

    X, comp = _data(args.fit_n, 4 * args.fit_n, d)

    def whole_fit(route):
        def call():
            m = PairwiseGP(X, comp)
            m._route = route
            fit.fit_gpytorch_mll(PairwiseLaplaceMarginalLogLikelihood(m.likelihood, m))
        return call

    fit_row = {"n": args.fit_n, "m": 4 * args.fit_n, "d": d,
               "fit_fused_vs_torch": _alternate(whole_fit("fused"), whole_fit("torch"), args.runs, 0, 1,
                                                False)}
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "reps": args.reps,
           "warmup": args.warmup, "rows": rows, "fit": fit_row}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
