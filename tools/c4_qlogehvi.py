#!/usr/bin/env python3
"""qLogEHVI / qLogNEHVI beside plain qEHVI / qNEHVI at the C4 shape
(ModelListGP of 3 on DTLZ2, n = 2048, d = 6, S = 128, b = 128, the
partitioning's own cells; qNEHVI with the pruned baseline) for q = 4 and q = 8:
forward and forward + backward per call, HIP events after a warm-up, the
classes alternating within every repetition, the median of the repetitions
(development tool; the figures of DESIGN.md's qLogEHVI section).

Also the reduction alone at q = 4, b = 8 (where the torch composition fits in
memory): bo_qlogehvi (+ backward) against the same value composed from
botorch_amd.safe_math torch ops on the device (tests/logehvi_restatement.py,
the restatement the tests pin to the reference).  argv: reps steps."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tests.logehvi_restatement import log_qehvi_from_samples  # noqa: E402
from botorch_amd import kernels  # noqa: E402
from botorch_amd.acquisition import (qExpectedHypervolumeImprovement,  # noqa: E402
                                     qLogExpectedHypervolumeImprovement,
                                     qLogNoisyExpectedHypervolumeImprovement,
                                     qNoisyExpectedHypervolumeImprovement)
from botorch_amd.models import ModelListGP, SingleTaskGP  # noqa: E402
from botorch_amd.multi_objective import FastNondominatedPartitioning  # noqa: E402
from botorch_amd.sampling import SobolQMCNormalSampler  # noqa: E402
from botorch_amd.utils_sampling import draw_sobol_samples  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda", 0)
f64 = torch.float64
S, b = 128, 128
X, Y, ref_point, ls, noise = bench.c4_problem()


def stgp(t):
    m = SingleTaskGP(X.to(dev), Y[:, t:t + 1].to(dev))
    m.covar_module.lengthscale = torch.full((1, X.shape[-1]), ls, dtype=f64)
    m.likelihood.noise = torch.tensor([noise], dtype=f64)
    return m.eval()


model = ModelListGP(*[stgp(t) for t in range(3)])
part = FastNondominatedPartitioning(ref_point, Y)
sampler = lambda: SobolQMCNormalSampler(torch.Size([S]), seed=0)  # noqa: E731
acqfs = {
    "qEHVI": qExpectedHypervolumeImprovement(model, ref_point.tolist(), part, sampler=sampler()),
    "qLogEHVI": qLogExpectedHypervolumeImprovement(model, ref_point.tolist(), part, sampler=sampler()),
    "qNEHVI": qNoisyExpectedHypervolumeImprovement(model, ref_point.tolist(), X.to(dev),
                                                   sampler=sampler(), prune_baseline=True),
    "qLogNEHVI": qLogNoisyExpectedHypervolumeImprovement(model, ref_point.tolist(), X.to(dev),
                                                         sampler=sampler(), prune_baseline=True),
}
print("cells", part.get_hypercell_bounds()[0].shape[0], "qNEHVI cells per sample (max)",
      acqfs["qNEHVI"].cell_lower_bounds.shape[1], "baseline", acqfs["qNEHVI"].X_baseline.shape[0],
      flush=True)


def event_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def alternate(fns, warmup=2):
    """Median ms per call of every fn: all warmed up, then ``reps`` rounds in
    which the fns take turns."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(event_ms(fn, steps))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in ts.items()}


unit = torch.stack([torch.zeros(6, dtype=f64), torch.ones(6, dtype=f64)])
for q in (4, 8):
    Xd = draw_sobol_samples(unit, b, q, seed=1).to(dev)
    Xg = Xd.clone().requires_grad_(True)
    fwd, fb = {}, {}
    for name, acqf in acqfs.items():
        def f(acqf=acqf):
            with torch.no_grad():
                return acqf(Xd)

        def g(acqf=acqf):
            return torch.autograd.grad(acqf(Xg).sum(), Xg)[0]
        fwd[name], fb[name] = f, g
    with torch.no_grad():
        vals = {k: float(f().mean()) for k, f in fwd.items()}
    print(f"q = {q}: mean value", {k: round(v, 6) for k, v in vals.items()}, flush=True)
    for tag, fns in (("forward", fwd), ("forward+backward", fb)):
        for k, (med, lo_, hi_) in alternate(fns).items():
            print(f"q = {q} {tag:>16s} {k:>10s}: {med:8.3f} ms  (min {lo_:.3f}, max {hi_:.3f})", flush=True)


# ---- the reduction alone: the kernel against torch ops on the device (q = 4, b = 8) ----
q, b8 = 4, 8
g = torch.Generator().manual_seed(0)
mean = (-0.6 + 0.2 * torch.randn(3, b8, q, generator=g, dtype=f64)).to(dev)
L = (0.1 * torch.tril(torch.randn(3, b8, q, q, generator=g, dtype=f64))).to(dev)
Z = torch.randn(S, q * 3, generator=g, dtype=f64).to(dev)
lo, hi = (t.to(dev).contiguous() for t in part.get_hypercell_bounds())
dacq = torch.ones(b8, dtype=f64, device=dev)


def samples(mean_, L_):
    return mean_.permute(1, 2, 0).unsqueeze(0) + torch.einsum("tbpj,sjt->sbpt", L_.tril(), Z.reshape(S, q, 3))


def kernel_fwd():
    return kernels.qlogehvi(mean, L, Z, lo, hi)


def kernel_fb():
    acq, hvi = kernels.qlogehvi(mean, L, Z, lo, hi)
    return kernels.qlogehvi_backward(mean, L, Z, lo, hi, acq, hvi, dacq)


def torch_fwd():
    with torch.no_grad():
        return log_qehvi_from_samples(samples(mean, L), lo, hi)


mg, Lg = mean.clone().requires_grad_(True), L.clone().requires_grad_(True)


def torch_fb():
    return torch.autograd.grad(log_qehvi_from_samples(samples(mg, Lg), lo, hi).sum(), (mg, Lg))


dv = (kernel_fwd()[0] - torch_fwd()).abs().max().item()
dg = (kernel_fb()[0] - torch_fb()[0]).abs().max().item()
print(f"reduction alone, q = {q}, b = {b8}, K = {lo.shape[0]}: kernel vs torch max|dvalue| = {dv:.2e}, "
      f"max|d dmean| = {dg:.2e}", flush=True)
for k, (med, lo_, hi_) in alternate({"kernel forward": kernel_fwd, "torch forward": torch_fwd,
                                     "kernel forward+backward": kernel_fb,
                                     "torch forward+backward": torch_fb}).items():
    print(f"reduction q = {q} b = {b8} {k:>24s}: {med:8.3f} ms  (min {lo_:.3f}, max {hi_:.3f})", flush=True)
print("done", flush=True)
