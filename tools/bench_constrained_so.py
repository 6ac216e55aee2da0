#!/usr/bin/env python3
"""Time outcome constraints on the single-objective acquisitions, on the GPU,
in one process (run nothing else on the GPU beside it).

C4's shape with Mt = 2 (n = 2048, d = 6, b = 128, q = 8, S = 128): a model
list of C4's first objective and one constraint member, ``LinearMCObjective([1,
0])``, the constraint f_1 <= 0 with eta = 1e-3.  Medians over --reps timed
calls after --warmup untimed ones, each between two HIP events on the current
stream (the host part of a call lies between the events too: these are call
times).  --rounds repeats the whole set, alternating the order of the routes.

  acquisitions   qLogEI and qLogNEI, forward (no_grad) and forward + backward,
                 three ways on the same commit:
                   generic    the route every constrained call took before the
                              fused one existed: a ListSampler (the only sampler
                              that route accepts on a model list), the fused
                              route switched off; qLogNEI then runs with
                              cache_root=False, a joint (r + q) root per forward
                   lambda     the fused route, the constraint a plain callable
                              (the weights through torch, dfeas back)
                   in_kernel  the fused route, the constraint from
                              get_outcome_constraint_transforms
  kernels        kernels.qmc_feas / qmc_feas_backward (Mt = 2, one constraint,
                 log mode) beside bo_qmc_finalize's own reduction and
                 kernels.qmc_backward at Mt = 1 on the same moments.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

DEV = torch.device("cuda", 0)
F64 = torch.float64
B, Q, S = 128, 8, 128


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
    return round(statistics.median(times), 4)


def _time_acqf(acqf, X, warmup, reps):
    Xg = X.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            return acqf(X)

    def fb():
        return torch.autograd.grad(acqf(Xg).sum(), Xg)[0]

    return dict(fwd_ms=_timed(fwd, warmup, reps), fwd_bwd_ms=_timed(fb, warmup, reps),
                value_sum=float(fwd().sum()), grad_abs_sum=float(fb().abs().sum()))


def _last(Z):
    return Z[..., -1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--baseline", type=int, default=64, help="baseline points of qLogNEI")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_constrained_so: needs the GPU (no CPU timing)")
    from botorch_amd import _lib, acquisition, kernels
    from botorch_amd.acquisition import qLogExpectedImprovement, qLogNoisyExpectedImprovement
    from botorch_amd.models import ModelListGP, SingleTaskGP
    from botorch_amd.objective import LinearMCObjective, get_outcome_constraint_transforms
    from botorch_amd.sampling import ListSampler, SobolQMCNormalSampler
    from botorch_amd.utils_sampling import draw_sobol_samples

    Xtr, Y, ref, ls, noise = bench.c4_problem()
    c = Xtr[:, 0] + 0.5 * torch.sin(3.0 * Xtr[:, 1]) - 0.8
    Ym = torch.stack([Y[:, 0], c], dim=-1)
    members = []
    for t in range(2):
        m = SingleTaskGP(Xtr.to(DEV), Ym[:, t:t + 1].to(DEV))
        m.covar_module.lengthscale = torch.full((1, 6), ls, dtype=F64)
        m.likelihood.noise = torch.tensor([noise], dtype=F64)
        m.mean_module.constant = torch.tensor(bench.CONSTANT, dtype=F64)
        members.append(m.eval())
    model = ModelListGP(*members)
    unit = torch.stack([torch.zeros(6, dtype=F64), torch.ones(6, dtype=F64)])
    X = draw_sobol_samples(unit, B, Q, seed=1).to(DEV)
    Xb = Xtr[: args.baseline].to(DEV)
    best_f = float(Y[:, 0].median())
    lin = get_outcome_constraint_transforms((torch.tensor([[0.0, 1.0]], dtype=F64),
                                             torch.zeros(1, 1, dtype=F64)))
    obj = lambda: LinearMCObjective(torch.tensor([1.0, 0.0], dtype=F64, device=DEV))  # noqa: E731
    single = lambda: SobolQMCNormalSampler(torch.Size([S]), seed=0)  # noqa: E731
    listed = lambda: ListSampler(*[SobolQMCNormalSampler(torch.Size([S]), seed=t) for t in range(2)])  # noqa: E731

    def build(kind, route):
        cons = lin if route == "in_kernel" else [_last]
        kw = dict(objective=obj(), constraints=cons, eta=1e-3,
                  sampler=listed() if route == "generic" else single())
        if kind == "qlogei":
            return qLogExpectedImprovement(model, best_f, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)   # generic: cache_root switched off
            return qLogNoisyExpectedImprovement(model, Xb, **kw)

    plan = acquisition._weighted_so_plan
    acq = {}
    for rnd in range(args.rounds):
        routes = ["generic", "lambda", "in_kernel"]
        if rnd % 2:
            routes.reverse()
        for kind in ("qlogei", "qlognei"):
            for route in routes:
                acquisition._weighted_so_plan = (lambda a: None) if route == "generic" else plan
                try:
                    a = build(kind, route)
                    acq.setdefault(f"{kind}_{route}", []).append(_time_acqf(a, X, args.warmup, args.reps))
                finally:
                    acquisition._weighted_so_plan = plan

    # the kernels alone, on the members' posterior moments at X
    with torch.no_grad():
        posts = [m.posterior(X).distribution for m in members]
        mean = torch.stack([p.mean.reshape(B, Q) for p in posts]).contiguous()
        eye = 1e-8 * torch.eye(Q, dtype=F64, device=DEV)
        L = torch.stack([torch.linalg.cholesky(p.covariance_matrix.reshape(B, Q, Q) + eye)
                         for p in posts]).contiguous()
    Z2 = kernels.sobol_normal(Q * 2, S, 0, DEV)
    Z1 = kernels.sobol_normal(Q, S, 0, DEV)
    dacq = torch.randn(B, generator=torch.Generator().manual_seed(0), dtype=F64).to(DEV)
    lp = (1, 1e-6, 1e-2)
    kw = dict(best_f=best_f, A=[[0.0, 1.0]], rhs=[0.0], eta=[1e-3], log=True, fat=True)
    a2 = kernels.qmc_feas(mean, L, Z2, [1.0, 0.0], **kw)
    a1 = kernels.qmc_feas(mean[:1], L[:1], Z1, [1.0], best_f=best_f, log=True, fat=True)
    kern = dict(Mt=2, k=1, q=Q, S=S, B=B)
    kern["qmc_feas_ms"] = _timed(lambda: kernels.qmc_feas(mean, L, Z2, [1.0, 0.0], **kw),
                                 args.warmup, args.reps)
    kern["qmc_feas_backward_ms"] = _timed(
        lambda: kernels.qmc_feas_backward(mean, L, Z2, [1.0, 0.0], dacq, acq=a2, **kw),
        args.warmup, args.reps)
    kern["qmc_feas_mt1_k0_ms"] = _timed(
        lambda: kernels.qmc_feas(mean[:1], L[:1], Z1, [1.0], best_f=best_f, log=True, fat=True),
        args.warmup, args.reps)
    cache = members[0].prediction_cache()
    ymean, ystd = members[0].outcome_stats()
    pp = kernels.post_partials(cache, X)
    kern["qmc_finalize_qlogei_ms"] = _timed(
        lambda: kernels.qmc_finalize(cache, pp, _lib.QMC_QLOGEI, ymean, ystd, Z=Z1, best_f=best_f,
                                     want_cov=False, want_L=True, log_params=lp),
        args.warmup, args.reps)
    kern["qmc_backward_qlogei_ms"] = _timed(
        lambda: kernels.qmc_backward(_lib.QMC_QLOGEI, mean[0], L[0], Z1, dacq, best_f=best_f,
                                     acq_fwd=a1, log_params=lp), args.warmup, args.reps)
    print(json.dumps(dict(tool="bench_constrained_so", device=torch.cuda.get_device_name(0),
                          warmup=args.warmup, reps=args.reps, rounds=args.rounds,
                          baseline_points=int(Xb.shape[0]), acquisitions=acq, kernels=kern)))


if __name__ == "__main__":
    main()
