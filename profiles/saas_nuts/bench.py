#!/usr/bin/env python3
"""Time the SAAS potential and the NUTS fit built on it, on the GPU, in one process.

1. The potential per call: the fused kernel (torch.ops.bo.saas_potential, one
   workgroup per chain) against the generic route (mcmc.saas_potential_torch on
   the device), for n in {64, 256, 512}, d = 50, C in {1, 4, 16} chains.  --runs
   alternating runs of each route (fused, generic, fused, ...); a run is the
   median of --reps calls after --warmup untimed ones, each call between two HIP
   events.  ``fused_wins``: the slowest fused run is faster than the fastest
   generic run.  These rows decide the default route per shape.
2. The whole fit at the C5 shape (n = 256, d = 50, Hartmann6 on the first six
   dimensions, the reference's defaults: 512 warmup steps, 256 draws, depth 6,
   thinning 16) for num_chains in {1, 4}: wall time, rounds, leapfrogs,
   divergences, mean acceptance and the median lengthscale of the six active
   dimensions against the other 44.
3. The same sampler driven by saas_potential_torch on host tensors (the
   machine's CPU threads as torch finds them), on a shortened schedule
   (--cpu-warmup, --cpu-samples), with the time per potential round of both.

Writes one JSON object to --out (default profiles/saas_nuts/bench.json) and
prints it on one line.
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def _problem(n, d):
    from botorch_amd.test_functions import Hartmann
    g = torch.Generator().manual_seed(0)
    X = torch.rand(n, d, generator=g, dtype=F64)
    Y = Hartmann(negate=True)(X[:, :6]).unsqueeze(-1)
    return X, (Y - Y.mean()) / Y.std()


def _summary(info, wall):
    rounds = info[0]["total_rounds"]
    return dict(wall_s=round(wall, 2), rounds=rounds,
                leapfrogs_after_warmup=[i["leapfrogs"] for i in info],
                potential_evaluations=[i["rounds"] for i in info],
                divergences=[i["divergences"] for i in info],
                warmup_divergences=[i["warmup_divergences"] for i in info],
                mean_accept=[round(i["mean_accept"], 3) for i in info],
                step_size=[round(i["step_size"], 4) for i in info],
                ms_per_round=round(1e3 * wall / max(rounds, 1), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--ns", type=int, nargs="+", default=[64, 256, 512])
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--Cs", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit-n", type=int, default=256)
    ap.add_argument("--chains", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--cpu-warmup", type=int, default=24)
    ap.add_argument("--cpu-samples", type=int, default=8)
    ap.add_argument("--skip-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saas_nuts", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profiles/saas_nuts/bench.py: needs the GPU")
    from botorch_amd import kernels, ops  # noqa: F401
    from botorch_amd.fit import fit_fully_bayesian_model_nuts
    from botorch_amd.mcmc import run_nuts, saas_potential_fn, saas_potential_torch
    from botorch_amd.models import SaasFullyBayesianSingleTaskGP
    d = args.d
    rows = []
    for n in args.ns:
        X, Y = _problem(n, d)
        Xd, yd = X.to(DEV), Y.squeeze(-1).to(DEV)
        for C in args.Cs:
            z = (4.0 * torch.rand(C, d + 4, generator=torch.Generator().manual_seed(C),
                                  dtype=F64) - 2.0).to(DEV)
            work = torch.empty(kernels.saas_potential_work(n, d, C), dtype=F64, device=DEV)
            fused = lambda: torch.ops.bo.saas_potential(z, Xd, yd, work)  # noqa: E731
            generic = lambda: saas_potential_torch(z, Xd, yd)  # noqa: E731
            (u, g, s), (ur, gr, sr) = fused(), generic()
            assert s.tolist() == sr.tolist() == [0] * C
            agree = dict(U=((u - ur).abs().max() / ur.abs().max()).item(),
                         grad=((g - gr).abs().max() / gr.abs().max()).item())
            t_f, t_g = [], []
            for _ in range(args.runs):
                t_f.append(round(_timed(fused, args.warmup, args.reps), 4))
                t_g.append(round(_timed(generic, args.warmup, args.reps), 4))
            med_f, med_g = statistics.median(t_f), statistics.median(t_g)
            rows.append(dict(n=n, d=d, C=C, fused_ms=t_f, generic_ms=t_g, fused_median_ms=med_f,
                             generic_median_ms=med_g, speedup=round(med_g / med_f, 2),
                             fused_wins=max(t_f) < min(t_g), generic_wins=max(t_g) < min(t_f),
                             max_rel_difference=agree))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    fits, cpu = [], None
    if not args.skip_fit:
        X, Y = _problem(args.fit_n, d)
        for chains in args.chains:
            gp = SaasFullyBayesianSingleTaskGP(X.to(DEV), Y.to(DEV))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit_fully_bayesian_model_nuts(gp, num_chains=chains, seed=0)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            ls = torch.stack([m.covar_module.base_kernel.lengthscale.reshape(-1)
                              for m in gp._members]).cpu()
            med = ls.median(dim=0).values
            fits.append(dict(num_chains=chains, num_mcmc_samples=gp.num_mcmc_samples,
                             median_lengthscale_active=round(med[:6].median().item(), 3),
                             median_lengthscale_other=round(med[6:].median().item(), 3),
                             **_summary(gp.nuts_info, wall)))
            print(json.dumps(fits[-1]), file=sys.stderr, flush=True)
        # the same sampler on the generic route on host tensors, a shortened schedule
        kw = dict(warmup_steps=args.cpu_warmup, num_samples=args.cpu_samples, max_tree_depth=6,
                  seed=0)
        t0 = time.perf_counter()
        _, info = run_nuts(saas_potential_fn(X, Y.squeeze(-1), route="torch"), (1, d + 4), **kw)
        cpu = dict(route="saas_potential_torch on host tensors", threads=torch.get_num_threads(),
                   schedule=kw, **_summary(info, time.perf_counter() - t0))
        t0 = time.perf_counter()
        _, info = run_nuts(saas_potential_fn(X.to(DEV), Y.squeeze(-1).to(DEV)), (1, d + 4), **kw)
        cpu["fused_same_schedule"] = _summary(info, time.perf_counter() - t0)
        print(json.dumps(cpu), file=sys.stderr, flush=True)
    res = dict(tool="profiles/saas_nuts/bench.py", device=torch.cuda.get_device_name(0), d=d,
               runs=args.runs, warmup=args.warmup, reps=args.reps, potential=rows,
               fit=dict(n=args.fit_n, d=d, warmup_steps=512, num_samples=256, max_tree_depth=6,
                        thinning=16, results=fits), host_route=cpu)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
