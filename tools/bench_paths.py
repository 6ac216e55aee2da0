#!/usr/bin/env python3
"""Time the fused pathwise-sample evaluation (kernels.paths_eval, all mode)
against the same values composed from the existing operators, on the GPU, in
one process.

Shape (defaults): R = 65536 points, n = 2048 training points, M = 1024 features,
S = 16 paths, d = 6, RBF.
  fused     one bo_paths_eval launch: the R x M features and the R x n kernel
            rows stay in registers
  unfused   kernels.covar_matrix into R x n, the phases by kernels.gemm into
            R x H, torch.sin / torch.cos into R x M, two kernels.gemm against W
            and V, and the affine output map
--runs alternating runs of each (fused, unfused, fused, ...); a run is the
median of --reps calls after --warmup untimed ones, each call between two HIP
events on the current stream.  Peak transient memory: the rise of
torch.cuda.max_memory_allocated over one call.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


def _peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return rise


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--R", type=int, default=65536)
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--M", type=int, default=1024)
    ap.add_argument("--S", type=int, default=16)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--matern", action="store_true")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_paths: needs the GPU (no CPU timing)")
    from botorch_amd import _lib, kernels
    R, n, M, S, d = args.R, args.n, args.M, args.S, args.d
    kind = _lib.MATERN52 if args.matern else _lib.RBF
    o, c, ymean, ystd = 1.3, 0.2, -0.4, 2.5
    g = torch.Generator(device=DEV).manual_seed(0)
    X = torch.rand(R, d, generator=g, dtype=F64, device=DEV)
    Xt = torch.rand(n, d, generator=g, dtype=F64, device=DEV)
    ls = 0.3 + 0.4 * torch.rand(d, generator=g, dtype=F64, device=DEV)
    Omega = torch.randn(M // 2, d, generator=g, dtype=F64, device=DEV)
    W = torch.randn(S, M, generator=g, dtype=F64, device=DEV)
    V = torch.randn(S, n, generator=g, dtype=F64, device=DEV) / n
    Xts = (Xt / ls).contiguous()
    H = M // 2
    pscale = math.sqrt(2.0 * o / M)

    def fused():
        return kernels.paths_eval(X, ls, Omega, W, Xts, V, kind, o, c, ymean, ystd, 0)

    def unfused():
        K = kernels.covar_matrix(X, Xt, ls, kind, o)                  # R x n
        theta = kernels.gemm(X / ls, Omega, transB=True)              # R x H
        feat = torch.empty(R, M, dtype=F64, device=DEV)
        torch.sin(theta, out=feat[:, :H])
        torch.cos(theta, out=feat[:, H:])
        g_ = kernels.gemm(W, feat, transB=True, alpha=pscale)         # S x R
        g_ = kernels.gemm(V, K, transB=True, beta=1.0, C=g_)
        return ymean + ystd * (c + g_)

    a, b = fused(), unfused()
    agree = ((a - b).abs().max() / b.abs().max()).item()
    del a, b
    kernels.drop_keepalive()
    t_f, t_u = [], []
    for _ in range(args.runs):
        t_f.append(round(_timed(fused, args.warmup, args.reps), 4))
        kernels.drop_keepalive()
        t_u.append(round(_timed(unfused, args.warmup, args.reps), 4))
        kernels.drop_keepalive()
    peak_f, peak_u = _peak_rise(fused), _peak_rise(unfused)
    kernels.drop_keepalive()
    med_f, med_u = statistics.median(t_f), statistics.median(t_u)
    print(json.dumps(dict(tool="bench_paths", device=torch.cuda.get_device_name(0), R=R, n=n, M=M,
                          S=S, d=d, kind="matern52" if args.matern else "rbf", mode="all",
                          runs=args.runs, warmup=args.warmup, reps=args.reps,
                          fused_ms=t_f, unfused_ms=t_u, fused_median_ms=med_f,
                          unfused_median_ms=med_u, speedup=round(med_u / med_f, 2),
                          fused_peak_bytes=peak_f, unfused_peak_bytes=peak_u,
                          max_rel_difference=agree)))


if __name__ == "__main__":
    main()
