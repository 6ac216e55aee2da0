#!/usr/bin/env python3
"""Time qKnowledgeGradient's two routes on the GPU, in one process (run
nothing else on the GPU beside it).

n = 1024, d = 6, N_f = 64, q in {1, 4, 8}: the forward at B = 512 (the raw
samples of the initialiser) and forward + backward at B = 16 (the restarts),
each on the packed fused route (tiles of <= 16 rows through bo::gp_posterior,
then bo::kg) and on the generic route (the joint posterior through the generic
kernels, the formula in torch).  The routes alternate, --rounds times each
after --warmup untimed calls, --reps timed calls per round between two HIP
events on the current stream (the host part of a call lies between the events
too: these are call times); the figure is the median over all timed calls.

Writes one JSON object to --out (default profiles/kg/bench_kg.json) and prints
it on one line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)
F64 = torch.float64
N, D, N_F = 1024, 6, 64
B_FWD, B_BWD = 512, 16


def _times(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kg", "bench_kg.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kg: needs the GPU (no CPU timing)")
    from botorch_amd import kernels
    from botorch_amd.acquisition import qKnowledgeGradient
    from botorch_amd.models import SingleTaskGP
    from botorch_amd.test_functions import Hartmann
    from botorch_amd.utils_sampling import draw_sobol_samples

    unit = torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)])
    Xtr = draw_sobol_samples(unit, N, 1, seed=0).squeeze(1)
    Ytr = Hartmann(negate=True)(Xtr).unsqueeze(-1)
    model = SingleTaskGP(Xtr.to(DEV), Ytr.to(DEV))
    model.covar_module.lengthscale = torch.full((1, D), 0.35, dtype=F64)
    model.likelihood.noise = torch.tensor([1e-3], dtype=F64)
    model = model.eval()
    acqf = qKnowledgeGradient(model, num_fantasies=N_F)

    def call(route, X):
        Xa, Xf = X[:, :-N_F], X[:, -N_F:]
        Z = acqf.sampler.base_samples_2d(Xa.shape[1], X.device)
        return (acqf._fused if route == "fused" else acqf._generic)(Xa, Xf, Z)

    results = {}
    for q in (1, 4, 8):
        Xf = draw_sobol_samples(unit, B_FWD, q + N_F, seed=q).to(DEV)
        Xb = draw_sobol_samples(unit, B_BWD, q + N_F, seed=100 + q).to(DEV).requires_grad_(True)

        def fwd(route):
            with torch.no_grad():
                return call(route, Xf)

        def fb(route):
            return torch.autograd.grad(call(route, Xb).sum(), Xb)[0]

        rec = {r: dict(fwd=[], fwd_bwd=[]) for r in ("fused", "generic")}
        for rnd in range(args.rounds):
            routes = ["fused", "generic"] if rnd % 2 == 0 else ["generic", "fused"]
            for route in routes:
                rec[route]["fwd"] += _times(lambda: fwd(route), args.warmup, args.reps)
                rec[route]["fwd_bwd"] += _times(lambda: fb(route), args.warmup, args.reps)
        kernels.check_ladder_status(DEV)
        vf, vg = fwd("fused"), fwd("generic")
        gf, gg = fb("fused"), fb("generic")
        T, slots = kernels.kg_tile_plan(q, N_F)
        results[f"q{q}"] = dict(
            T=T, slots=slots, rows_packed=T * (q + slots), rows_joint=q + N_F,
            fused_fwd_ms=round(statistics.median(rec["fused"]["fwd"]), 4),
            generic_fwd_ms=round(statistics.median(rec["generic"]["fwd"]), 4),
            fused_fwd_bwd_ms=round(statistics.median(rec["fused"]["fwd_bwd"]), 4),
            generic_fwd_bwd_ms=round(statistics.median(rec["generic"]["fwd_bwd"]), 4),
            fwd_min_ms=dict(fused=round(min(rec["fused"]["fwd"]), 4),
                            generic=round(min(rec["generic"]["fwd"]), 4)),
            fwd_bwd_min_ms=dict(fused=round(min(rec["fused"]["fwd_bwd"]), 4),
                                generic=round(min(rec["generic"]["fwd_bwd"]), 4)),
            value_max_rel_diff=float(((vf - vg).abs() / vg.abs().clamp_min(1e-12)).max()),
            grad_max_abs_diff=float((gf - gg).abs().max()))
    out = dict(tool="bench_kg", device=torch.cuda.get_device_name(0), n=N, d=D, N_f=N_F,
               B_fwd=B_FWD, B_fwd_bwd=B_BWD, warmup=args.warmup, reps=args.reps,
               rounds=args.rounds, KG_FUSED_QMAX=kernels.KG_FUSED_QMAX, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
