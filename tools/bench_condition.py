#!/usr/bin/env python3
"""Time SingleTaskGP.condition_on_observations against the same update done by
a rebuild, on the GPU, in one process.

Per shape (n old points, k new ones, d = 6), medians over --reps timed calls
after --warmup untimed ones, each between two HIP events on the current stream
(the host part of a call lies between the events too: these are call times):
  extend_device_ms   kernels.extend_gp_cache_enqueue alone: the bordered update's
                     launches, no status read-back
  condition_ms       model.condition_on_observations (extension route: the
                     launches, the status read-back, the new model's modules)
  condition_post_ms  the same plus the new model's first posterior
  rebuild_cache_ms   kernels.build_gp_cache on the concatenated data alone
  rebuild_post_ms    a new SingleTaskGP on the concatenated data plus its first
                     posterior (the only route before condition_on_observations)
speedup = rebuild_post_ms / condition_post_ms.  crossover_k: the k at which the
two n = 4096 curves meet (linear between the measured k), rounded down to a
multiple of 16; null when the extension is faster at every measured k.
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda"
F64 = torch.float64
D, LS, NOISE, CONST = 6, 0.35, 1e-3, 0.1


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


def _model(X, Y):
    from botorch_amd.models import SingleTaskGP
    m = SingleTaskGP(X, Y)
    m.covar_module.lengthscale = torch.full((1, D), LS, dtype=F64)
    m.likelihood.noise = torch.tensor([NOISE], dtype=F64)
    m.mean_module.constant = CONST
    return m.eval()


def measure(n, k, warmup, reps):
    from botorch_amd import kernels
    g = torch.Generator().manual_seed(n + k)
    X = torch.rand(n + k, D, generator=g, dtype=F64).to(DEV)
    Y = (torch.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] - X[:, 3:].pow(2).sum(-1)).unsqueeze(-1)
    Xc = torch.rand(4, 4, D, generator=g, dtype=F64).to(DEV)
    src = _model(X[:n], Y[:n])
    src.posterior(Xc)
    c = src._cache
    X2, Y2 = X[n:].contiguous(), Y[n:].contiguous()
    y2 = ((Y2 - src.outcome_transform.means) / src.outcome_transform.stdvs).reshape(-1)
    y_all = torch.cat([src.train_targets, y2])
    ls = torch.full((D,), LS, dtype=F64, device=DEV)

    def extend_device():
        kernels.extend_gp_cache_enqueue(c.kind, c.Xt_scaled, c.L, c.Linv, c.beta, c.alpha,
                                        c.lengthscale, c.outputscale, c.noise, c.constant, X2, y2)

    def condition():
        return src.condition_on_observations(X2, Y2)

    def condition_post():
        new = condition()
        assert new._cache is not None and new._cache.jitter == 0.0  # the extension route
        new.posterior(Xc)

    def rebuild_cache():
        kernels.build_gp_cache(X, y_all, ls, NOISE, CONST, check_nan=False)

    def rebuild_post():
        _model(X, Y).posterior(Xc)

    out = dict(n=n, k=k)
    for name, fn in (("extend_device_ms", extend_device), ("condition_ms", condition),
                     ("condition_post_ms", condition_post), ("rebuild_cache_ms", rebuild_cache),
                     ("rebuild_post_ms", rebuild_post)):
        out[name] = round(_timed(fn, warmup, reps), 4)
        kernels.drop_keepalive()
    out["speedup"] = round(out["rebuild_post_ms"] / out["condition_post_ms"], 2)
    return out


def crossover(rows):
    rows = sorted(rows, key=lambda r: r["k"])
    gap = [r["condition_post_ms"] - r["rebuild_post_ms"] for r in rows]
    if gap[0] >= 0:
        return 0
    for (a, ga), (b, gb) in zip(zip(rows, gap), zip(rows[1:], gap[1:])):
        if gb >= 0:
            kx = a["k"] + (b["k"] - a["k"]) * (-ga) / (gb - ga)
            return int(kx) // 16 * 16
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--extra-k", default="512,1024",
                    help="further k at n = 4096, to find where the curves meet")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_condition: needs the GPU (no CPU timing)")
    from botorch_amd import kernels
    kernels.EXTEND_MAX_K = 1 << 30  # time the extension at every k
    shapes = [(4096, k) for k in (1, 16, 64, 128, 256)] + [(2048, 16)]
    shapes += [(4096, int(k)) for k in args.extra_k.split(",") if k]
    rows = [measure(n, k, args.warmup, args.reps) for n, k in shapes]
    print(json.dumps(dict(tool="bench_condition", device=torch.cuda.get_device_name(0), d=D,
                          warmup=args.warmup, reps=args.reps, results=rows,
                          crossover_k=crossover([r for r in rows if r["n"] == 4096]))))


if __name__ == "__main__":
    main()
