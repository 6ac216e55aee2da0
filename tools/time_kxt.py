#!/usr/bin/env python3
"""K*x^T build (kxt_build_kernel) timed on its own, across builds of the
library: C3 (b = 512, q = 16, n = 4096; bo_post_kxt_rows), C4 (b = 128, q = 8,
n = 2048, three members; bo_post_kxt_rows_members) and C2 (b = 64, q = 8,
n = 1024; bo_post_kxt_rows, the small grid -- BO_KXT_SMALL is read once per
library).  HIP events around every call, the libraries interleaved over
ROUNDS rounds; per library and shape the median, minimum and maximum in us and
whether Kt and Xq equal the first library's bit for bit.  Beside them the time
of a plain device fill of C3's 268 MB (torch zero_, median of 10): the write
rate the build is held against.

  tools/time_kxt.py [NAME=PATH ...]     (default: CUR = the tree's library)
"""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, CALLS = 3, 20
SHAPES = {"C3": (512, 16, 4096, 1), "C4": (128, 8, 2048, 3), "C2": (64, 8, 1024, 1)}
D = 6
P = ctypes.c_void_p
dev = torch.device("cuda", 0)


def load(path):
    h = ctypes.CDLL(path)
    h.bo_post_kxt_rows.argtypes = [ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P,
                                   ctypes.c_int64, ctypes.c_double, P, P, P]
    h.bo_post_kxt_rows_members.argtypes = [ctypes.c_int, ctypes.c_int, P, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, P, P, P, ctypes.c_int64, P, P, P]
    return h


def problem(B, q, n, nm):
    g = torch.Generator().manual_seed(B + n)
    X = torch.rand(B, q, D, dtype=torch.float64, generator=g).to(dev)
    Qp = 1 << (q - 1).bit_length()
    nrows_pad = -(-B * Qp // 128) * 128
    np_ = -(-n // 128) * 128
    mem = []
    for m in range(nm):
        Xt = torch.zeros(n, 8, dtype=torch.float64)
        ls = torch.full((D,), 0.5 + 0.1 * m, dtype=torch.float64)
        Xt[:, :D] = torch.rand(n, D, dtype=torch.float64, generator=g) / ls
        mem.append((ls.to(dev), Xt.to(dev), 1.0 + 0.5 * m,
                    torch.empty(nrows_pad, 8, dtype=torch.float64, device=dev),
                    torch.empty(np_, nrows_pad, dtype=torch.float64, device=dev)))
    return X, mem


def call(h, X, mem, n):
    B, q, _ = X.shape
    st = P(torch._C._cuda_getCurrentRawStream(0))
    if len(mem) == 1:
        ls, Xt, os_, Xq, Kt = mem[0]
        rc = h.bo_post_kxt_rows(0, P(X.data_ptr()), B, q, D, P(ls.data_ptr()), P(Xt.data_ptr()), n, os_,
                                P(Xq.data_ptr()), P(Kt.data_ptr()), st)
    else:
        nm = len(mem)
        A = P * nm
        rc = h.bo_post_kxt_rows_members(
            nm, 0, P(X.data_ptr()), B, q, D, A(*[m[0].data_ptr() for m in mem]),
            A(*[m[1].data_ptr() for m in mem]), (ctypes.c_double * nm)(*[m[2] for m in mem]), n,
            A(*[m[3].data_ptr() for m in mem]), A(*[m[4].data_ptr() for m in mem]), st)
    if rc:
        raise SystemExit(f"kxt call failed: {rc}")


def timed(fn, calls):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in ev]


def main():
    libs = [a.split("=", 1) for a in sys.argv[1:]] or [["CUR", os.path.join(ROOT, "botorch_amd",
                                                                            "libbotorch_amd.so")]]
    libs = [(name, load(path)) for name, path in libs]
    out = {}
    fill = torch.empty(4096 * 8192, dtype=torch.float64, device=dev)
    for _ in range(3):
        fill.zero_()
    t = timed(fill.zero_, 10)
    out["fill_268MB_us"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2),
                            "max": round(max(t), 2)}
    del fill
    for sname, (B, q, n, nm) in SHAPES.items():
        X, mem = problem(B, q, n, nm)
        ref = None
        times = {name: [] for name, _ in libs}
        same = {}
        for name, h in libs:
            for m in mem:
                m[3].fill_(float("nan"))
                m[4].fill_(float("nan"))
            for _ in range(5):
                call(h, X, mem, n)
            torch.cuda.synchronize()
            got = [(m[3].clone(), m[4].clone()) for m in mem]
            if ref is None:
                ref = got
            same[name] = all(torch.equal(a, c) and torch.equal(b, e) for (a, b), (c, e) in zip(got, ref))
        for _ in range(ROUNDS):
            for name, h in libs:
                times[name] += timed(lambda: call(h, X, mem, n), CALLS)
        out[sname] = {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                             "max_us": round(max(v), 2), "equal_to_first": same[name]}
                      for name, v in times.items()}
        del X, mem, ref
    print(json.dumps(out))


if __name__ == "__main__":
    main()
