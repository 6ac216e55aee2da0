#!/usr/bin/env python3
"""Time the MultiTaskGP paths on the GPU, in one process.

closure      the MLL closure (value + gradient) of fit_gpytorch_mll on a
             MultiTaskGP: the fused route (fit.icm_mll_terms: bo_icm_covar, the
             optimistic factorisation, bo_ainv, bo_icm_mll_terms) against the
             generic route (fit.icm_mll_terms_torch), at n = 1024 (768 source +
             256 target points) and n = 4096 (3072 + 1024), d = 6, T = 2 and
             T = 8 (tasks beyond the first two dealt round-robin over the source
             points), rank = T.  Each call is a host clock around the closure,
             which ends in its device-to-host transfer.
fit          one full fit_gpytorch_mll at n = 1024, T = 2 (the default route).
acquisition  one qLogNoisyExpectedImprovement forward at B = 512, q = 4 on the
             task view of a MultiTaskGP beside the same call on a SingleTaskGP
             with the same n (HIP events on the current stream).

--runs alternating runs of each route (fused, generic, fused, ...); a run is the
median of --reps calls after --warmup untimed ones.  ``fused_wins``: the slowest
fused run is faster than the fastest generic run (``generic_wins`` likewise).

Writes one JSON object to --out (default profiles/mtgp/bench.json) and prints it
on one line.
"""
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

DEV = "cuda"
F64 = torch.float64


def _host_timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times)


def _event_timed(fn, warmup, reps):
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


def _data(n, d, T, seed=0):
    """n points, a quarter of them of the target task (index 1), the rest dealt
    over the other tasks; two correlated smooth tasks plus task offsets."""
    g = torch.Generator().manual_seed(seed)
    Xd = torch.rand(n, d, generator=g, dtype=F64)
    n_t = n // 4
    others = [t for t in range(T) if t != 1]
    task = torch.tensor([others[i % len(others)] for i in range(n - n_t)] + [1] * n_t)
    f = torch.sin(4 * Xd).sum(-1) + Xd[:, 0] * Xd[:, 1]
    Y = (f + 0.2 * torch.cos(1.0 * task) * torch.sin(3 * Xd[:, 1])
         + 0.05 * torch.randn(n, generator=g, dtype=F64)).unsqueeze(-1)
    return Xd, task, Y


def _model(n, d, T, seed=0):
    from botorch_amd.models import MultiTaskGP, Standardize
    Xd, task, Y = _data(n, d, T, seed)
    X = torch.cat([Xd, task.to(F64).unsqueeze(-1)], dim=-1)
    torch.manual_seed(seed)
    m = MultiTaskGP(X.to(DEV), Y.to(DEV), task_feature=-1, output_tasks=[1],
                    outcome_transform=Standardize(m=1))
    return m, Xd, Y, task


def _start(layout, T):
    x = layout.get()
    x[0] = 0.05                                              # noise
    x[layout.o + 1:layout.o + 1 + layout.d] = 0.5            # lengthscales
    g = np.random.default_rng(0)
    x[layout.f0:layout.v0] = (0.6 + 0.2 * g.standard_normal((T, T))).reshape(-1) / np.sqrt(T)
    x[layout.v0:] = 0.3
    return x


def bench_closure(args):
    from botorch_amd import fit, kernels
    rows = []
    for n in args.ns:
        for T in args.Ts:
            m, _, _, _ = _model(n, args.d, T)
            lay = fit._ICMLayout(m)
            x = _start(lay, T)

            def closure(route):
                def fn():
                    fit.ICM_ROUTE = route
                    try:
                        return fit.icm_mll_value_and_grad(m, x, lay)
                    finally:
                        fit.ICM_ROUTE = None
                return fn
            fused, generic = closure("fused"), closure("generic")
            (vf, gf), (vg, gg) = fused(), generic()
            agree = dict(value=abs(vf - vg) / max(1.0, abs(vg)),
                         grad=float(np.max(np.abs(gf - gg) / (1e-9 + np.abs(gg)))))
            t_f, t_g = [], []
            for _ in range(args.runs):
                t_f.append(round(_host_timed(fused, args.warmup, args.reps), 4))
                kernels.drop_keepalive()
                t_g.append(round(_host_timed(generic, args.warmup, args.reps), 4))
                kernels.drop_keepalive()
            med_f, med_g = statistics.median(t_f), statistics.median(t_g)
            rows.append(dict(n=n, d=args.d, T=T, rank=T, parameters=int(lay.size), fused_ms=t_f,
                             generic_ms=t_g, fused_median_ms=med_f, generic_median_ms=med_g,
                             speedup=round(med_g / med_f, 2), fused_wins=max(t_f) < min(t_g),
                             generic_wins=max(t_g) < min(t_f), max_rel_difference=agree))
            del m, lay
            torch.cuda.empty_cache()
    return rows


def bench_fit(args):
    from botorch_amd import fit
    n, T = args.ns[0], 2
    times, evals, loss = [], [], []
    for run in range(args.fit_runs + 1):          # the first run is the warm-up
        m, _, _, _ = _model(n, args.d, T)
        lay = fit._ICMLayout(m)
        lay.set(_start(lay, T))
        count = [0]
        inner = fit.icm_mll_value_and_grad

        def counted(*a, **k):
            count[0] += 1
            return inner(*a, **k)
        fit.icm_mll_value_and_grad = counted
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit.fit_gpytorch_mll(fit.ExactMarginalLogLikelihood(m.likelihood, m))
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
        finally:
            fit.icm_mll_value_and_grad = inner
        if run:
            times.append(round(dt, 2))
            evals.append(count[0])
            loss.append(float(inner(m, lay.get(), lay)[0]))
    B = m.task_covar_module.covar_matrix.detach().cpu()
    return dict(n=n, d=args.d, T=T, rank=T, fit_ms=times, fit_median_ms=statistics.median(times),
                closure_evaluations=evals, final_loss=loss,
                task_correlation=float(B[0, 1] / (B[0, 0] * B[1, 1]).sqrt()))


def bench_acquisition(args):
    from botorch_amd import kernels
    from botorch_amd.acquisition import qLogNoisyExpectedImprovement
    from botorch_amd.models import MaternKernel, ScaleKernel, SingleTaskGP
    from botorch_amd.sampling import SobolQMCNormalSampler
    n, d = args.ns[0], args.d
    mt, Xd, Y, task = _model(n, d, 2)
    lay_x = dict(ls=0.5, os=1.2, noise=0.02)
    st = SingleTaskGP(Xd.to(DEV), Y.to(DEV), covar_module=ScaleKernel(MaternKernel(ard_num_dims=d)))
    for m in (mt, st):
        m.covar_module.base_kernel.lengthscale = torch.full((1, d), lay_x["ls"], dtype=F64)
        m.covar_module.outputscale = lay_x["os"]
        m.likelihood.noise = lay_x["noise"]
        m.eval()
    with torch.no_grad():
        mt.task_covar_module.covar_factor.copy_(torch.tensor([[0.9, 0.1], [0.7, 0.4]], dtype=F64))
    mt.task_covar_module.var = torch.tensor([0.2, 0.3], dtype=F64)
    Xb = Xd[task == 1][:64].to(DEV)
    g = torch.Generator().manual_seed(1)
    X = torch.rand(args.B, args.q, d, generator=g, dtype=F64).to(DEV)
    acqs = {}
    for name, m in (("multitask_view", mt), ("singletask", st)):
        acqs[name] = qLogNoisyExpectedImprovement(
            m, X_baseline=Xb, sampler=SobolQMCNormalSampler(sample_shape=torch.Size([128]), seed=3),
            prune_baseline=False)
        assert acqs[name]._fused_ready and acqs[name]._fused_eligible(X)

    def forward(acqf):
        def fn():
            with torch.no_grad():
                return acqf(X)
        return fn
    fns = {k: forward(a) for k, a in acqs.items()}
    times = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, fn in fns.items():
            times[k].append(round(_event_timed(fn, args.warmup, args.reps), 4))
            kernels.drop_keepalive()
    med = {k: statistics.median(v) for k, v in times.items()}
    return dict(n=n, d=d, B=args.B, q=args.q, baseline_points=int(Xb.shape[0]), samples=128,
                multitask_view_ms=times["multitask_view"], singletask_ms=times["singletask"],
                multitask_view_median_ms=med["multitask_view"], singletask_median_ms=med["singletask"],
                ratio=round(med["multitask_view"] / med["singletask"], 3),
                ranges_overlap=not (max(times["multitask_view"]) < min(times["singletask"])
                                    or max(times["singletask"]) < min(times["multitask_view"])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--ns", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--Ts", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--q", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--fit-runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", nargs="*", default=[], choices=["closure", "fit", "acquisition"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtgp", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mtgp: needs the GPU (no CPU timing)")
    res = dict(tool="bench_mtgp", device=torch.cuda.get_device_name(0), runs=args.runs,
               warmup=args.warmup, reps=args.reps)
    if "closure" not in args.skip:
        res["closure"] = bench_closure(args)
    if "fit" not in args.skip:
        res["fit"] = bench_fit(args)
    if "acquisition" not in args.skip:
        res["acquisition"] = bench_acquisition(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
