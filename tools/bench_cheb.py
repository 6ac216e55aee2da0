"""The fused Chebyshev-scalarization (ParEGO) route against the generic route, in one process.

qLogExpectedImprovement over GenericMCObjective(get_chebyshev_scalarization(...)) (a sampler
per member) and qLogNParEGO (its default sampler, a baseline of the first 64 training points:
the cached-root term F and the per-sample best) on a ModelListGP of Mt SingleTaskGP members
(n = 1024, d = 6, S = 512), Mt in {2, 4, 8}, q in {1, 4, 8}:
the forward at B = 512 and forward + backward at B = 16, the routes alternating, five runs
each (a run: the median of ITERS timed calls after a warm-up); at B = 16 also the fused
route with G = 1 against the chosen G.  Writes profiles/cheb/bench.json.

    python tools/bench_cheb.py [--out profiles/cheb/bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, D, S, RUNS, ITERS = 1024, 6, 512, 5, 5
DEV = torch.device("cuda", 0)
F64 = torch.float64


def build(Mt, kind):
    from botorch_amd import acquisition as A, get_chebyshev_scalarization
    from botorch_amd.models import ModelListGP, SingleTaskGP
    from botorch_amd.objective import GenericMCObjective
    from botorch_amd.sampling import ListSampler, SobolQMCNormalSampler
    g = torch.Generator().manual_seed(Mt)
    X = torch.rand(N, D, dtype=F64, generator=g)
    Y = torch.stack([torch.sin((2.0 + t) * X.sum(-1)) + 0.3 * X[:, t % D] for t in range(Mt)], -1)
    Y = (Y + 0.05 * torch.randn(N, Mt, dtype=F64, generator=g)).to(DEV)
    model = ModelListGP(*[SingleTaskGP(X.to(DEV), Y[:, t:t + 1]) for t in range(Mt)]).eval()
    w = torch.full((Mt,), 1.0 / Mt, dtype=F64, device=DEV)
    if kind == "qLogNParEGO":
        return A.qLogNParEGO(model, X[:64].to(DEV), scalarization_weights=w)
    sampler = ListSampler(*[SobolQMCNormalSampler(torch.Size([S]), seed=t) for t in range(Mt)])
    return A.qLogExpectedImprovement(model, best_f=-0.5, sampler=sampler,
                                     objective=GenericMCObjective(get_chebyshev_scalarization(w, Y)))


def one_run(acqf, X, grad):
    def call():
        if not grad:
            with torch.no_grad():
                return acqf(X)
        Xr = X.clone().requires_grad_(True)
        acqf(Xr).sum().backward()
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(ITERS):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/cheb/bench.json")
    args = ap.parse_args()
    from botorch_amd import kernels
    rows = []
    for Mt, kind in [(m, k) for m in (2, 4, 8) for k in ("qLogExpectedImprovement", "qLogNParEGO")]:
        acqf = build(Mt, kind)
        for q in (1, 4, 8):
            for B, grad in ((512, False), (16, True)):
                X = torch.rand(B, q, D, dtype=F64, generator=torch.Generator().manual_seed(q)).to(DEV)
                variants = [("fused", None), ("generic", None)] + ([("fused", 1)] if grad else [])
                ms = {v: [] for v in variants}
                for _ in range(RUNS):
                    for route, G in variants:
                        acqf.cheb_route, acqf.cheb_groups = route, G
                        ms[(route, G)].append(one_run(acqf, X, grad))
                row = dict(kind=kind, Mt=Mt, q=q, B=B, backward=grad, G=kernels.qmc_cheb_groups(B, S, DEV),
                           fused_ms=ms[("fused", None)], generic_ms=ms[("generic", None)])
                if grad:
                    row["fused_G1_ms"] = ms[("fused", 1)]
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(n=N, d=D, S=S, runs=RUNS, iters=ITERS,
                       device=torch.cuda.get_device_name(0), rows=rows), fh, indent=1)


if __name__ == "__main__":
    main()
