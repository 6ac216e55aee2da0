#!/usr/bin/env python3
"""Time outcome constraints on the multi-objective acquisitions, on the GPU, in
one process (run nothing else on the GPU beside it).

C4's shape (ModelListGP of 3 on DTLZ2, n = 2048, d = 6, b = 128, q = 8,
S = 128, ref point -1.1; qNEHVI on the pruned baseline).  Medians over --reps
timed calls after --warmup untimed ones, each between two HIP events on the
current stream (the host part of a call lies between the events too: these
are call times):

  acquisitions   qEHVI and qNEHVI, forward (no_grad) and forward + backward,
                 unconstrained on the 3 members, and with one constraint member
                 added (Mt = 4, objective = outcomes [0, 1, 2], constraint
                 ``lambda Z: Z[..., -1]``, eta = 1e-3) on the same commit.  The
                 cost of a constraint is one more member's posterior plus the
                 weighted kernel plus the weights' torch graph;
                 ``qehvi_outcomes_only`` (the Mt = 4 list and objective without
                 the constraint: all weights 1, no graph) separates the two.
  kernels        kernels.qehvi / qehvi_backward against kernels.qehvi_feas /
                 qehvi_feas_backward alone at equal (m, q, S, B, K): C4's
                 posterior moments and cells, weights uniform in (0, 1).

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

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


def _models(X, Y, ls, noise):
    from botorch_amd.models import SingleTaskGP
    out = []
    for t in range(Y.shape[1]):
        m = SingleTaskGP(X.to(DEV), Y[:, t:t + 1].to(DEV))
        m.covar_module.lengthscale = torch.full((1, 6), ls, dtype=F64)
        m.likelihood.noise = torch.tensor([noise], dtype=F64)
        m.mean_module.constant = torch.tensor(bench.CONSTANT, dtype=F64)
        out.append(m.eval())
    return out


def _time_acqf(acqf, X, warmup, reps):
    Xg = X.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            return acqf(X)

    def fb():
        return torch.autograd.grad(acqf(Xg).sum(), Xg)[0]

    return dict(fwd_ms=_timed(fwd, warmup, reps), fwd_bwd_ms=_timed(fb, warmup, reps),
                value_sum=float(fwd().sum()), grad_abs_sum=float(fb().abs().sum()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_constrained: needs the GPU (no CPU timing)")
    from botorch_amd import kernels
    from botorch_amd.acquisition import (IdentityMCMultiOutputObjective,
                                         qExpectedHypervolumeImprovement,
                                         qNoisyExpectedHypervolumeImprovement)
    from botorch_amd.models import ModelListGP
    from botorch_amd.multi_objective import FastNondominatedPartitioning
    from botorch_amd.sampling import SobolQMCNormalSampler
    from botorch_amd.utils_sampling import draw_sobol_samples

    Xtr, Y, ref, ls, noise = bench.c4_problem()
    # the constraint member: smooth, feasible (<= 0) on about half of the cube
    c = Xtr[:, 0] + 0.5 * torch.sin(3.0 * Xtr[:, 1]) - 0.8
    members = _models(Xtr, torch.cat([Y, c.unsqueeze(-1)], dim=-1), ls, noise)
    plain, full = ModelListGP(*members[:3]), ModelListGP(*members)
    part = FastNondominatedPartitioning(ref, Y)
    unit = torch.stack([torch.zeros(6, dtype=F64), torch.ones(6, dtype=F64)])
    X = draw_sobol_samples(unit, B, Q, seed=1).to(DEV)
    con = dict(objective=IdentityMCMultiOutputObjective(outcomes=[0, 1, 2]),
               constraints=[lambda Z: Z[..., -1]], eta=1e-3)
    sampler = lambda: SobolQMCNormalSampler(torch.Size([S]), seed=0)  # noqa: E731

    acq = {}
    acq["qehvi"] = _time_acqf(qExpectedHypervolumeImprovement(
        plain, ref.tolist(), part, sampler=sampler()), X, args.warmup, args.reps)
    acq["qehvi_constrained"] = _time_acqf(qExpectedHypervolumeImprovement(
        full, ref.tolist(), part, sampler=sampler(), **con), X, args.warmup, args.reps)
    # the same Mt = 4 model list and objective without the constraint: every
    # weight is 1 and no torch graph is built -- one more member's posterior and
    # the weighted kernels through the autograd Function, nothing else
    acq["qehvi_outcomes_only"] = _time_acqf(qExpectedHypervolumeImprovement(
        full, ref.tolist(), part, sampler=sampler(), objective=con["objective"]),
        X, args.warmup, args.reps)
    for name, model, kw in (("qnehvi", plain, {}), ("qnehvi_constrained", full, con)):
        torch.manual_seed(0)
        a = qNoisyExpectedHypervolumeImprovement(model, ref.tolist(), Xtr.to(DEV), prune_baseline=True,
                                                 sampler=sampler(), **kw)
        acq[name] = _time_acqf(a, X, args.warmup, args.reps)
        acq[name]["baseline_points"] = int(a.X_baseline.shape[0])
        acq[name]["cells_per_sample"] = int(a.cell_lower_bounds.shape[1])
    for k in ("qehvi", "qnehvi"):
        for f in ("fwd_ms", "fwd_bwd_ms"):
            acq[k + "_constrained"][f.replace("_ms", "_ratio")] = round(
                acq[k + "_constrained"][f] / acq[k][f], 3)

    # the kernels alone: C4's posterior moments of the 3 objective members
    with torch.no_grad():
        posts = [m.posterior(X).distribution for m in members[:3]]
        mean = torch.stack([p.mean.reshape(B, Q) for p in posts]).contiguous()
        eye = 1e-8 * torch.eye(Q, dtype=F64, device=DEV)
        L = torch.stack([torch.linalg.cholesky(p.covariance_matrix.reshape(B, Q, Q) + eye)
                         for p in posts]).contiguous()
    Z = kernels.sobol_normal(Q * 3, S, 0, DEV)
    lo, hi = [t.to(DEV, F64).contiguous() for t in part.get_hypercell_bounds()]
    g = torch.Generator().manual_seed(0)
    w = torch.rand(S, B, Q, generator=g, dtype=F64).to(DEV)
    dacq = torch.randn(B, generator=g, dtype=F64).to(DEV)
    oi = (0, 1, 2)
    kern = dict(m=3, q=Q, S=S, B=B, K=int(lo.shape[0]))
    kern["qehvi_ms"] = _timed(lambda: kernels.qehvi(mean, L, Z, lo, hi), args.warmup, args.reps)
    kern["qehvi_feas_ms"] = _timed(lambda: kernels.qehvi_feas(mean, L, Z, lo, hi, w, oi),
                                   args.warmup, args.reps)
    kern["qehvi_backward_ms"] = _timed(lambda: kernels.qehvi_backward(mean, L, Z, lo, hi, dacq),
                                       args.warmup, args.reps)
    kern["qehvi_feas_backward_ms"] = _timed(
        lambda: kernels.qehvi_feas_backward(mean, L, Z, lo, hi, w, oi, dacq), args.warmup, args.reps)
    kern["forward_ratio"] = round(kern["qehvi_feas_ms"] / kern["qehvi_ms"], 3)
    kern["backward_ratio"] = round(kern["qehvi_feas_backward_ms"] / kern["qehvi_backward_ms"], 3)
    ones = torch.ones_like(w)
    kern["unit_weights_bitwise_equal"] = bool(torch.equal(
        kernels.qehvi(mean, L, Z, lo, hi), kernels.qehvi_feas(mean, L, Z, lo, hi, ones, oi)))
    print(json.dumps(dict(tool="bench_constrained", device=torch.cuda.get_device_name(0),
                          warmup=args.warmup, reps=args.reps, acquisitions=acq, kernels=kern)))


if __name__ == "__main__":
    main()
