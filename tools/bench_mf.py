#!/usr/bin/env python3
"""Time the SingleTaskMultiFidelityGP paths on the GPU, in one process.

closure    the MLL closure (value + gradient) of fit_gpytorch_mll: the fused route
           (bo_ltf_covar, the optimistic factorisation, bo_ainv, bo_ltf_mll_terms)
           against the torch route (autograd), host clock around the closure, which
           ends in its device-to-host transfer.
posterior  model.posterior forward at B = 512, q = 4, and forward + backward at
           B = 16, q = 4, fused against torch route (HIP events).
target     bo_ltf_cross at B = 4096, q = 4 with every query row at target fidelity
           (s = 1: k0 alone) against no row at target fidelity (s = 0.5): HIP events
           around 20 launches enqueued back to back, the figure is the time per launch.

n = 1024 and 4096, d_x = 6, one fidelity column.  --runs alternating runs of each variant (a,
b, a, ...); a run is the median of --reps calls after --warmup untimed ones.
``a_wins``: the slowest run of the first variant beats the fastest of the second.
Writes one JSON object to --out and prints it on one line."""
import argparse
import json
import os
import statistics
import sys
import time

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


def _alternate(a, b, args, events):
    ra, rb = [], []
    for _ in range(args.runs):
        ra.append(_timed(a, args.warmup, args.reps, events))
        rb.append(_timed(b, args.warmup, args.reps, events))
    return {"a_ms": {"median": statistics.median(ra), "min": min(ra), "max": max(ra)},
            "b_ms": {"median": statistics.median(rb), "min": min(rb), "max": max(rb)},
            "a_wins": max(ra) < min(rb), "b_wins": max(rb) < min(ra)}


def _model(n, dx):
    from botorch_amd import fit
    from botorch_amd.models import SingleTaskMultiFidelityGP
    g = torch.Generator().manual_seed(0)
    X = torch.rand(n, dx + 1, generator=g, dtype=F64)
    Y = (torch.sin(4 * X[:, :dx]).sum(-1) - 0.3 * (1 - X[:, dx])
         + 0.05 * torch.randn(n, generator=g, dtype=F64)).unsqueeze(-1)
    m = SingleTaskMultiFidelityGP(X.to(DEV), Y.to(DEV), data_fidelities=[dx])
    lay = fit._layout(m)
    x = lay.get()
    x[0] = 0.05
    x[lay.h0:lay.s0] = 0.5
    lay.set(x)
    return m, lay, x


def _routed(m, route, fn):
    def call():
        m._route = route
        try:
            return fn()
        finally:
            m._route = None
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mf", "bench.json"))
    args = ap.parse_args()
    from botorch_amd import kernels
    dx = 6
    rows = []
    for n in args.ns:
        m, lay, x = _model(n, dx)
        g = torch.Generator().manual_seed(1)

        def queries(B, q=4, s=None):
            X = torch.rand(B, q, dx + 1, generator=g, dtype=F64)
            if s is not None:
                X[..., dx] = s
            return X.to(DEV)

        Xf, Xb = queries(512), queries(16).requires_grad_(True)

        def fwd():
            with torch.no_grad():
                return m.posterior(Xf).mvn.covariance_matrix

        def fwd_bwd():
            post = m.posterior(Xb)
            return torch.autograd.grad(post.mean.sum() + post.mvn.covariance_matrix.sum(), Xb)

        spec, Xt = m.spec(), m.train_inputs[0]
        Xk = {True: queries(4096, s=1.0), False: queries(4096, s=0.5)}

        def cross20(target):
            for _ in range(20):
                kernels.ltf_cross(Xk[target], Xt, spec)

        row = {"n": n, "d_x": dx, "n_f": 1,
               "closure_fused_vs_torch": _alternate(_routed(m, "fused", lambda: lay.value_and_grad(x)),
                                                    _routed(m, "torch", lambda: lay.value_and_grad(x)),
                                                    args, events=False),
               "posterior_fwd_B512_q4_fused_vs_torch": _alternate(_routed(m, "fused", fwd),
                                                                   _routed(m, "torch", fwd), args, True),
               "posterior_fwd_bwd_B16_q4_fused_vs_torch": _alternate(_routed(m, "fused", fwd_bwd),
                                                                      _routed(m, "torch", fwd_bwd), args, True),
               "cross_B4096_q4_all_target_vs_none_per_launch": _alternate(
                   lambda: cross20(True), lambda: cross20(False), args, True)}
        for v in row["cross_B4096_q4_all_target_vs_none_per_launch"].values():
            if isinstance(v, dict):
                v.update({k: t / 20 for k, t in v.items()})
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "reps": args.reps,
           "warmup": args.warmup, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
