#!/usr/bin/env python3
"""C3 (n = 4096, q = 16, B = 512, S = 512) timings of qSimpleRegret,
qProbabilityOfImprovement and qUpperConfidenceBound beside qEI on the same tree
(development tool): forward-only and forward + backward,
HIP events around 20 back-to-back calls after warm-ups, five repetitions with
the classes alternating.  Prints a summary; argv[1]: a path for the JSON."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from botorch_amd.acquisition import (qExpectedImprovement, qProbabilityOfImprovement,  # noqa: E402
                                     qSimpleRegret, qUpperConfidenceBound)
from botorch_amd.sampling import SobolQMCNormalSampler  # noqa: E402

dev = torch.device("cuda", 0)
w = bench.make_workload("qei", dev)
model = w.acqf.model
smp = lambda: SobolQMCNormalSampler(torch.Size([bench.MC]), seed=0)  # noqa: E731
# qPI's best_f at the median qSR value so the sigmoids are not all saturated
Xd = w.Xc.to(dev)
sr = qSimpleRegret(model, sampler=smp())
with torch.no_grad():
    med = float(sr(Xd).median())
acqs = {
    "qEI": qExpectedImprovement(model, w.best_f, sampler=smp()),
    "qSR": sr,
    "qPI": qProbabilityOfImprovement(model, med, sampler=smp()),
    "qUCB": qUpperConfidenceBound(model, 0.2, sampler=smp()),
}


def fwd(a):
    with torch.no_grad():
        return a(Xd)


def fwd_bwd(a):
    X = Xd.detach().requires_grad_(True)
    (g,) = torch.autograd.grad(a(X).sum(), X)
    return g


def timed(fn, a, steps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn(a)
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


for a in acqs.values():  # warm-up, every shape and route
    for _ in range(5):
        fwd(a)
        fwd_bwd(a)
torch.cuda.synchronize(dev)
out = {k: {"fwd_ms": [], "fwd_bwd_ms": []} for k in acqs}
for rep in range(5):
    for k, a in acqs.items():
        out[k]["fwd_ms"].append(timed(fwd, a))
        out[k]["fwd_bwd_ms"].append(timed(fwd_bwd, a))
for k, v in out.items():
    v["fwd_ms_median"] = statistics.median(v["fwd_ms"])
    v["fwd_bwd_ms_median"] = statistics.median(v["fwd_bwd_ms"])
    with torch.no_grad():
        val = acqs[k](Xd)
    v["finite"] = bool(torch.isfinite(val).all())
    v["value_range"] = [float(val.min()), float(val.max())]
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
for k, v in out.items():
    print(k, "fwd %.4f ms  fwd+bwd %.4f ms" % (v["fwd_ms_median"], v["fwd_bwd_ms_median"]),
          "spread fwd", min(v["fwd_ms"]), max(v["fwd_ms"]), "range", v["value_range"])
