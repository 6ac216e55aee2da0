#!/usr/bin/env python3
"""Time risk-averse qExpectedImprovement (CVaR at alpha = 0.8) over a perturbed SingleTaskGP
on the GPU, in one process: the fused route (moments, root, bo_qmc_risk) against the generic
route of the same object (the same moments and root, then S x B x Q samples and the torch
objective), at n = 1024, d = 6, S = 512 and (q, n_w) = (1, 128), (4, 32), (8, 16).

forward    B = 512 t-batches under no_grad.
fwd+bwd    B = 16 t-batches, value and X.grad.

--runs alternating runs of each route (a, b, a, ...); a run is the median of --reps calls
after --warmup untimed ones (HIP events).  ``a_wins``: the slowest run of the fused route
beats the fastest of the generic one.  Writes one JSON object to --out and prints it on one
line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV, F64 = "cuda", torch.float64


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


def _alternate(a, b, args):
    ra, rb = [], []
    for _ in range(args.runs):
        ra.append(_timed(a, args.warmup, args.reps))
        rb.append(_timed(b, args.warmup, args.reps))
    return {"a_ms": {"median": statistics.median(ra), "min": min(ra), "max": max(ra)},
            "b_ms": {"median": statistics.median(rb), "min": min(rb), "max": max(rb)},
            "a_wins": max(ra) < min(rb), "b_wins": max(rb) < min(ra)}


def case(q, n_w, B, grad, args, n=1024, d=6, S=512):
    from botorch_amd.acquisition import _risk_fused_ok, qExpectedImprovement, t_batch_mode
    from botorch_amd.models import SingleTaskGP
    from botorch_amd.risk_measures import CVaR
    from botorch_amd.sampling import SobolQMCNormalSampler
    from botorch_amd.transforms import InputPerturbation
    g = torch.Generator().manual_seed(n_w)
    Xt = torch.rand(n, d, generator=g, dtype=F64)
    Y = torch.sin(3.0 * Xt.sum(-1, keepdim=True)) + 0.05 * torch.randn(n, 1, generator=g, dtype=F64)
    P = 0.1 * torch.randn(n_w, d, generator=g, dtype=F64)
    bounds = torch.tensor([[0.0] * d, [1.0] * d], dtype=F64)
    model = SingleTaskGP(Xt.to(DEV), Y.to(DEV),
                         input_transform=InputPerturbation(P.to(DEV), bounds=bounds.to(DEV))).eval()
    acqf = qExpectedImprovement(model, best_f=-0.5, objective=CVaR(0.8, n_w),
                                sampler=SobolQMCNormalSampler(torch.Size([S]), seed=0))
    acqf.risk_route = "fused"  # both routes are called explicitly below
    X = torch.rand(B, q, d, generator=g, dtype=F64).to(DEV)
    assert _risk_fused_ok(acqf, X, 1)

    def run(route):
        if not grad:
            with torch.no_grad():
                return route(X)
        Xr = X.clone().requires_grad_(True)
        val = route(Xr)
        val.sum().backward()
        return Xr.grad

    fused, generic = (lambda: run(acqf)), (lambda: run(lambda x: acqf._generic_forward(
        t_batch_mode(x))))
    want = generic()
    out = _alternate(fused, generic, args)
    out["max_rel_diff"] = float((fused() - want).abs().max() / want.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "risk", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_risk.py needs the GPU")
    shapes = [(1, 128), (4, 32), (8, 16)]
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "reps": args.reps,
           "forward B=512 (a fused, b generic)": {
               f"q={q}, n_w={w}": case(q, w, 512, False, args) for q, w in shapes},
           "forward + backward B=16 (a fused, b generic)": {
               f"q={q}, n_w={w}": case(q, w, 16, True, args) for q, w in shapes}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
