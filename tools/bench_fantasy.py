#!/usr/bin/env python3
"""Time FantasizedGP.posterior's two routes, and the host loop it replaces, on
the GPU, in one process (run nothing else on the GPU beside it).

n = 1024, d = 6, N_f = 64, q_a in {1, 4, 8}, q in {1, 4}, one set of q points
per fantasy: the forward at B = 512 and forward + backward (to X and X') at
B = 16, each on the packed fused route (tiles of <= 16 rows through
bo::gp_posterior, then bo::fantasy_posterior) and on the generic route (the
joint posterior of [X; X'_f] per fantasy, the formula in torch); and at B = 1
the forward against a host loop of condition_on_observations + posterior over
the N_f fantasies, which is what the same result takes without fantasize.  The
routes alternate, --rounds times each after --warmup untimed calls, --reps
timed calls per round between two HIP events on the current stream (the host
part of a call lies between the events too: these are call times); the figure
is the median over all timed calls.

Writes one JSON object to --out (default profiles/fantasy/bench_fantasy.json)
and prints it on one line.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fantasy", "bench_fantasy.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fantasy: needs the GPU (no CPU timing)")
    from botorch_amd import kernels
    from botorch_amd.models import FantasizedGP, SingleTaskGP
    from botorch_amd.sampling import SobolQMCNormalSampler
    from botorch_amd.test_functions import Hartmann
    from botorch_amd.utils_sampling import draw_sobol_samples

    unit = torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)])
    Xtr = draw_sobol_samples(unit, N, 1, seed=0).squeeze(1)
    Ytr = Hartmann(negate=True)(Xtr).unsqueeze(-1)
    model = SingleTaskGP(Xtr.to(DEV), Ytr.to(DEV))
    model.covar_module.lengthscale = torch.full((1, D), 0.35, dtype=F64)
    model.likelihood.noise = torch.tensor([1e-3], dtype=F64)
    model = model.eval()
    sampler = SobolQMCNormalSampler(torch.Size([N_F]), seed=0)
    fused_rows = FantasizedGP.FUSED_ROWS

    def moments(route, X, Xp):
        FantasizedGP.FUSED_ROWS = fused_rows if route == "fused" else 0
        try:
            post = model.fantasize(X, sampler).posterior(Xp)
        finally:
            FantasizedGP.FUSED_ROWS = fused_rows
        return post.mean, post.covariance_matrix

    def host_loop(X, Xp):
        """What the same moments take without fantasize: one conditioned model
        per fantasy (X: q_a x d, Xp: N_f x q x d)."""
        fm = model.fantasize(X, sampler)
        ymean, ystd = model.outcome_stats()
        Yf = fm.train_targets[:, N:] * ystd + ymean
        out = []
        for f in range(N_F):
            p = model.condition_on_observations(X, Yf[f].unsqueeze(-1)).posterior(Xp[f])
            out.append((p.mean, p.covariance_matrix))
        return torch.stack([m for m, _ in out]), torch.stack([c for _, c in out])

    results = {}
    for q_a in (1, 4, 8):
        for q in (1, 4):
            pts = lambda B, seed: torch.rand(B, q_a + N_F * q, D, dtype=F64,  # noqa: E731
                                             generator=torch.Generator().manual_seed(seed)).to(DEV)
            split = lambda P: (P[:, :q_a], P[:, q_a:].reshape(P.shape[0], N_F, q, D).transpose(0, 1))  # noqa: E731
            Xf, Xpf = split(pts(B_FWD, 10 * q_a + q))
            Pb = pts(B_BWD, 100 + 10 * q_a + q).requires_grad_(True)
            X1, Xp1 = split(pts(1, 200 + 10 * q_a + q))
            X1, Xp1 = X1[0], Xp1[:, 0]

            def fwd(route):
                with torch.no_grad():
                    return moments(route, Xf, Xpf)

            def fb(route):
                m, c = moments(route, *split(Pb))
                return torch.autograd.grad(m.sum() + c.sum(), Pb)[0]

            def one(route):
                with torch.no_grad():
                    return moments(route, X1, Xp1) if route != "loop" else host_loop(X1, Xp1)

            rec = {r: dict(fwd=[], fwd_bwd=[], b1=[]) for r in ("fused", "generic", "loop")}
            for rnd in range(args.rounds):
                routes = ["fused", "generic"] if rnd % 2 == 0 else ["generic", "fused"]
                for route in routes:
                    rec[route]["fwd"] += _times(lambda: fwd(route), args.warmup, args.reps)
                    rec[route]["fwd_bwd"] += _times(lambda: fb(route), args.warmup, args.reps)
                for route in routes + ["loop"]:
                    rec[route]["b1"] += _times(lambda: one(route), min(args.warmup, 1) if route == "loop"
                                               else args.warmup, args.reps)
            kernels.check_ladder_status(DEV)
            (mf, cf), (mg, cg), (ml, cl) = fwd("fused"), fwd("generic"), one("loop")
            m1, c1 = one("fused")
            gf, gg = fb("fused"), fb("generic")
            T, slots = kernels.fantasy_tile_plan(q_a, q, N_F)
            med = lambda r, k: round(statistics.median(rec[r][k]), 4)  # noqa: E731
            results[f"qa{q_a}_q{q}"] = dict(
                T=T, slots=slots, rows_packed=T * (q_a + slots * q), rows_needed=q_a + N_F * q,
                rows_generic=N_F * (q_a + q),
                fused_fwd_ms=med("fused", "fwd"), generic_fwd_ms=med("generic", "fwd"),
                fused_fwd_bwd_ms=med("fused", "fwd_bwd"), generic_fwd_bwd_ms=med("generic", "fwd_bwd"),
                b1_fused_ms=med("fused", "b1"), b1_generic_ms=med("generic", "b1"),
                b1_host_loop_ms=med("loop", "b1"),
                fwd_min_ms=dict(fused=round(min(rec["fused"]["fwd"]), 4),
                                generic=round(min(rec["generic"]["fwd"]), 4)),
                fwd_bwd_min_ms=dict(fused=round(min(rec["fused"]["fwd_bwd"]), 4),
                                    generic=round(min(rec["generic"]["fwd_bwd"]), 4)),
                mean_max_abs_diff=float((mf - mg).abs().max()),
                cov_max_abs_diff=float((cf - cg).abs().max()),
                grad_max_abs_diff=float((gf - gg).abs().max()),
                loop_mean_max_abs_diff=float((m1 - ml).abs().max()),
                loop_cov_max_abs_diff=float((c1 - cl).abs().max()))
    out = dict(tool="bench_fantasy", device=torch.cuda.get_device_name(0), n=N, d=D, N_f=N_F,
               B_fwd=B_FWD, B_fwd_bwd=B_BWD, warmup=args.warmup, reps=args.reps,
               rounds=args.rounds, FUSED_ROWS=fused_rows, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
