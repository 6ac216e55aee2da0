#!/usr/bin/env python3
"""Time the input-transform paths on the GPU, in one process.

closure    the closure of fit_gpytorch_mll (value + gradient, ending in its device-to-host
           transfer) of a Normalize + Warp SingleTaskGP, all d = 6 columns warped, at
           n = 1024 and 4096: the fused route (bo_input_warp, cache build, bo_mll_terms,
           bo_mll_dx, bo_input_warp_bwd) against the same closure as a torch composition with
           autograd on the device (host clock).
mll_dx     bo_mll_dx alone on prebuilt operands, the MFMA form against the FMA form, at
           d = 6, 15 and 31 (one per instantiation that has both forms; HIP events).
qlognei    one qLogNoisyExpectedImprovement forward at B = 512, q = 4, n = 1024, d = 6,
           32 baseline points: a Normalize + Warp model against a plain SingleTaskGP of the
           same n (HIP events).
transform  forward + backward of the transform at R = 65536, d = 6: torch.ops.bo.input_warp
           against the torch chain (HIP events).

--runs alternating runs of each route (a, b, a, ...); a run is the median of --reps calls
after --warmup untimed ones.  ``a_wins``: the slowest run of route a beats the fastest of
route b.  Writes one JSON object to --out and prints it on one line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
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


def _model(n, d):
    from botorch_amd.models import SingleTaskGP
    from botorch_amd.transforms import ChainedInputTransform, Normalize, Warp
    g = torch.Generator().manual_seed(n)
    X = 4.0 * torch.rand(n, d, generator=g, dtype=F64) - 1.0
    Y = torch.sin(X.sum(-1, keepdim=True)) + 0.05 * torch.randn(n, 1, generator=g, dtype=F64)
    tf = ChainedInputTransform(normalize=Normalize(d), warp=Warp(list(range(d))))
    return SingleTaskGP(X.to(DEV), Y.to(DEV), input_transform=tf)


def closure_case(n, d, args):
    from botorch_amd import fit
    from botorch_amd.transforms import warp_torch
    model = _model(n, d)
    layout = fit._layout(model)
    x = layout.get()
    x[-2 * d:] = np.linspace(0.7, 1.4, 2 * d)
    norm, warp = layout.norm, layout.warp
    offset, rscale, _, _, _ = norm.columns(d)
    Xraw, y = model.train_inputs[0], model.train_targets

    def fused():
        return fit.mll_value_and_grad(model, x, layout, sync_model=False)

    def composed():
        t = torch.tensor(x, dtype=F64, device=DEV, requires_grad=True)
        Xt = warp_torch(Xraw, offset, rscale, t[2 + 2 * d:], t[2 + d:2 + 2 * d], warp.mask(d),
                        warp._eps)
        ll = fit._mll_torch(Xt, y, t[2:2 + d], t[0], t[1], 1.0, int(model.kind))
        ll.backward()
        return float(ll.detach()), t.grad.cpu().numpy()

    la, ga = fused()
    lb, gb = composed()  # data term only: compare the concentration entries, which carry no prior
    out = _alternate(fused, composed, args.runs, args.warmup, args.reps, events=False)
    out["max_abs_dgrad_conc"] = float(np.abs(ga[-2 * d:] - (-gb[-2 * d:] / n)).max())
    return out


def mll_dx_case(n, d, args):
    from botorch_amd import kernels
    g = torch.Generator().manual_seed(n + 1)
    X = torch.rand(n, d, generator=g, dtype=F64).to(DEV)
    y = torch.randn(n, generator=g, dtype=F64).to(DEV)
    ls = torch.full((d,), 0.4, dtype=F64, device=DEV)
    cache = kernels.build_gp_cache(X, y, ls, 0.05, 0.0)
    Ainv = kernels.ainv(cache)
    forms = [lambda f=f: kernels.mll_dx(0, X, ls, 1.0, Ainv, cache.alpha, form=f) for f in (0, 1)]
    out = _alternate(forms[0], forms[1], args.runs, args.warmup, args.reps, events=True)
    out["max_abs_diff"] = float((forms[0]() - forms[1]()).abs().max())
    return out


def transform_case(R, d, args):
    from botorch_amd import ops  # noqa: F401
    from botorch_amd.transforms import warp_torch
    g = torch.Generator().manual_seed(R)
    X = torch.rand(R, d, generator=g, dtype=F64).to(DEV).requires_grad_(True)
    offset, rscale = torch.zeros(d, dtype=F64, device=DEV), torch.ones(d, dtype=F64, device=DEV)
    a = torch.linspace(0.5, 2.0, d, dtype=F64, device=DEV).requires_grad_(True)
    b = torch.linspace(1.5, 0.6, d, dtype=F64, device=DEV).requires_grad_(True)
    mask = (1 << d) - 1

    def run(op):
        for t in (X, a, b):
            t.grad = None
        op(X, offset, rscale, a, b, mask, 1e-7).sum().backward()

    return _alternate(lambda: run(torch.ops.bo.input_warp), lambda: run(warp_torch), args.runs,
                      args.warmup, args.reps, events=True)


def qlognei_case(n, d, args):
    from botorch_amd.acquisition import qLogNoisyExpectedImprovement
    from botorch_amd.models import SingleTaskGP
    from botorch_amd.sampling import SobolQMCNormalSampler
    warped = _model(n, d).eval()
    plain = SingleTaskGP(warped.train_inputs[0], warped._raw_train_Y).eval()
    g = torch.Generator().manual_seed(7)
    Xb = (4.0 * torch.rand(32, d, generator=g, dtype=F64) - 1.0).to(DEV)
    X = (4.0 * torch.rand(512, 4, d, generator=g, dtype=F64) - 1.0).to(DEV)
    acqs = [qLogNoisyExpectedImprovement(m, Xb, sampler=SobolQMCNormalSampler(torch.Size([512]),
                                                                                seed=0))
            for m in (warped, plain)]

    def run(acq):
        with torch.no_grad():
            return acq(X)

    return _alternate(lambda: run(acqs[0]), lambda: run(acqs[1]), args.runs, args.warmup,
                      args.reps, events=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp.py needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "reps": args.reps,
           "closure (a fused, b torch composition)": {f"n={n}": closure_case(n, 6, args)
                                                      for n in (1024, 4096)},
           "mll_dx (a MFMA form, b FMA form)": {f"n={n}, d={d}": mll_dx_case(n, d, args)
                                                for n in (1024, 4096) for d in (6, 15, 31)},
           "qLogNEI forward B=512 q=4 (a Normalize + Warp model, b plain)": {
               "n=1024": qlognei_case(1024, 6, args)},
           "transform fwd+bwd (a kernel, b torch chain)": {"R=65536": transform_case(65536, 6, args)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
