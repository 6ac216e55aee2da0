"""bo_qlogehvi / bo_qlogehvi_backward alone (kernels.qlogehvi,
kernels.qlogehvi_backward) against CPU fp64 autograd through the torch
restatement of the reference's log-space reduction
(tests/logehvi_restatement.py, pinned to the reference by
tests/test_logehvi_golden.py) on f = mean + L z (+ F), with a random
mixed-sign dacq.  The reference is never another route of the library.

Bound: the project's kernel-against-torch bound, max|got - ref| <= 1e-9 max|ref|
+ 1e-10 over whole arrays.  The kernel sums the subsets of one parity in mask
order where the reference sums them per subset size; permuting points and
subsets moves the fp64 reference itself by <= 7e-15 on the log value and 5e-14
relative on the gradient, far inside the bound.

Shapes: each the smallest that reaches a distinct code path (q bucket edges,
every m, several sample passes, sample split on / off in either kernel, cells
in LDS / through cache, one cell, per-sample cells with zero padding, F with
Qp > q, weights with a member map, both fat values and both default tau_max).
The forward splits a t-batch's samples over H = min(8, 1024 / B, S) workgroups
and the backward over min(8, 256 / B, S) (the launchers of csrc/qlogehvi.hip,
restated in ``launch_plan``), so the forward runs unsplit only from B = 513 and
the backward from B = 129; test_cases_reach_their_paths checks every case's
plan."""
import math

import pytest
import torch

from tests.logehvi_restatement import (log_hvi_per_sample, samples_from_roots)

F64 = torch.float64


def staircase_cells(m, n, nz=1, centre=0.7, seed=0):
    """Hand-made non-dominated cells above the reference point 0: the n + 1
    cells of an n-point m = 2 staircase front near ``centre`` (lower corner
    (x_i, y_{i+1}), upper (x_{i+1}, inf)), times nz slabs in every further
    objective (the last one unbounded) -> lo, hi ((n + 1) nz^(m-2) x m)."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.sort(centre + 0.3 * (torch.rand(n, generator=g, dtype=F64) - 0.5)).values
    y = torch.sort(centre + 0.3 * (torch.rand(n, generator=g, dtype=F64) - 0.5), descending=True).values
    inf = torch.tensor([math.inf], dtype=F64)
    zero = torch.zeros(1, dtype=F64)
    xs, ys = torch.cat([zero, x, inf]), torch.cat([y, zero])
    lo = torch.stack([xs[:-1], ys], -1)
    hi = torch.stack([xs[1:], inf.expand(n + 1)], -1)
    for _ in range(m - 2):
        edges = torch.cat([zero, torch.sort(centre + 0.3 * (torch.rand(nz - 1, generator=g, dtype=F64)
                                                            - 0.5)).values, inf])
        K = lo.shape[0]
        lo = torch.cat([lo.repeat_interleave(nz, 0), edges[:-1].repeat(K).unsqueeze(-1)], -1)
        hi = torch.cat([hi.repeat_interleave(nz, 0), edges[1:].repeat(K).unsqueeze(-1)], -1)
    return lo.contiguous(), hi.contiguous()


# name -> spec; defaults below
CASES = {
    # q bucket edges at m = 2, S = 5, B = 3, K = 9
    "q1": dict(q=1), "q4": dict(q=4), "q5": dict(q=5), "q8": dict(q=8),
    # every m at q = 3
    "m2": dict(m=2, q=3), "m3": dict(m=3, q=3, nfront=3, nz=2), "m4": dict(m=4, q=3, nfront=2, nz=2),
    # several sample passes per workgroup
    "passes": dict(q=8, m=4, S=256, B=1, nfront=0, nz=2),
    # no sample split in the forward (1024 / B < 2: the in-kernel logmeanexp) and the
    # backward; forward split (H = 3) with the backward unsplit; both split
    "nosplit": dict(q=2, S=4, B=513), "nosplit_bwd": dict(q=2, S=4, B=257),
    "split": dict(q=2, S=4, B=3),
    # cells beyond the LDS cap (K m = 1200 > 1024), read through cache
    "manycells": dict(q=2, m=3, S=4, nfront=19, nz=20),
    # single cell (an empty front)
    "onecell": dict(q=2, nfront=0),
    # per-sample cells, half of the samples padded by 2 zero cells
    "persample": dict(q=3, per_sample=True), "persample_m3": dict(q=2, m=3, nz=2, per_sample=True),
    # F present with Qp > q
    "withF": dict(q=3, Qp=5), "withF_persample": dict(q=2, m=3, nz=2, Qp=3, per_sample=True),
    # weights with a member map; some logw exactly 0.0
    "weights_map": dict(q=3, Mt=3, out_idx=(2, 0), logw=True),
    "weights_map_F": dict(q=5, Mt=3, out_idx=(2, 0), logw=True, Qp=6, per_sample=True),
    # both fat values and both default tau_max on the q = 4 case
    "q4_nofat": dict(q=4, fat=False), "q4_tau3": dict(q=4, tau_max=1e-3),
    "q4_nofat_tau3": dict(q=4, fat=False, tau_max=1e-3), "q4_nofat_w": dict(q=4, fat=False, logw=True),
    # the hopeless set: plain qEHVI exactly zero
    "hopeless": dict(q=4, kind="hopeless"), "hopeless_nofat": dict(q=4, kind="hopeless", fat=False),
    "hopeless_q8_m3": dict(q=8, m=3, nz=2, kind="hopeless", tau_max=1e-3),
}
DEFAULTS = dict(q=2, m=2, S=5, B=3, nfront=8, nz=1, per_sample=False, Qp=0, Mt=None, out_idx=None,
                logw=False, fat=True, tau_relu=1e-6, tau_max=1e-2, kind="mixed")


def build_case(name):
    """CPU inputs of the case (a dict of tensors and options)."""
    c = dict(DEFAULTS, **CASES[name])
    q, m, S, B = c["q"], c["m"], c["S"], c["B"]
    Mt = c["Mt"] or m
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    centre, spread = (0.6, 0.25) if c["kind"] == "mixed" else (0.2, 0.02)
    # f = mean + L z (+ F) is centre + spread N(0, 1) per entry
    has_F = c["Qp"] > 0
    part = spread / math.sqrt(3.0 if has_F else 2.0)
    mean = centre + part * rn(Mt, B, q)
    L = torch.tril(rn(Mt, B, q, q))
    L = part * L / L.norm(dim=-1, keepdim=True).clamp_min(1e-3)
    L = L + torch.diag_embed(torch.full((Mt, B, q), 1e-3, dtype=F64))
    Z = rn(S, q * Mt)
    F = None
    if has_F:
        F = part * rn(Mt, S, B * c["Qp"] + 3)  # ldF > B Qp
    if c["per_sample"]:
        # every sample its own front; the even samples' fronts are smaller by
        # two cells and padded with lo = hi = 0 (BoxDecompositionList's padding)
        slabs = c["nz"] ** (m - 2)
        per = [staircase_cells(m, 3 - (s % 2 == 0) * (2 // slabs), c["nz"], seed=s) for s in range(S)]
        Kmax = max(p[0].shape[0] for p in per)
        lo, hi = torch.zeros(S, Kmax, m, dtype=F64), torch.zeros(S, Kmax, m, dtype=F64)
        for s, (l_, h_) in enumerate(per):
            lo[s, : l_.shape[0]], hi[s, : l_.shape[0]] = l_, h_
    else:
        lo, hi = staircase_cells(m, c["nfront"], c["nz"])
    logw = None
    if c["logw"]:
        w = torch.rand(S, B, q, generator=g, dtype=F64).clamp_min(1e-3)
        w[torch.rand(S, B, q, generator=g, dtype=F64) < 0.3] = 1.0
        logw = w.log()
    dacq = rn(B)
    dacq[0] = -abs(dacq[0]) - 0.1
    if B > 1:
        dacq[1] = abs(dacq[1]) + 0.1
    c.update(name=name, Mt=Mt, mean=mean, L=L, Z=Z, F=F, lo=lo.contiguous(), hi=hi.contiguous(),
             logw=logw, dacq=dacq, out_idx=tuple(c["out_idx"] or range(m)))
    return c


def reference(c):
    """CPU fp64 autograd through the restatement -> acq, hvi, dmean, dL, dF, dlogw."""
    leaves = [c["mean"].clone().requires_grad_(True), c["L"].clone().requires_grad_(True)]
    if c["F"] is not None:
        leaves.append(c["F"].clone().requires_grad_(True))
    logw = c["logw"].clone().requires_grad_(True) if c["logw"] is not None else None
    if logw is not None:
        leaves.append(logw)
    f = samples_from_roots(leaves[0], leaves[1], c["Z"], leaves[2] if c["F"] is not None else None,
                           c["Qp"])
    obj = f[..., list(c["out_idx"])]
    hvi = log_hvi_per_sample(obj, c["lo"], c["hi"], logw, c["fat"], c["tau_relu"], c["tau_max"])
    acq = torch.logsumexp(hvi, dim=0) - math.log(hvi.shape[0])
    grads = list(torch.autograd.grad(acq, leaves, c["dacq"]))
    out = dict(acq=acq.detach(), hvi=hvi.detach(), dmean=grads.pop(0), dL=grads.pop(0))
    out["dF"] = grads.pop(0) if c["F"] is not None else None
    out["dlogw"] = grads.pop(0) if logw is not None else None
    return out


def check(name, got, ref):
    """The bound on every output; every reference non-trivial."""
    for k, r in ref.items():
        if r is None:
            assert got[k] is None, (name, k)
            continue
        gk = got[k].detach().cpu()
        assert gk.shape == r.shape, (name, k, gk.shape, r.shape)
        assert torch.isfinite(r).all() and r.abs().max() > 0, f"{name}/{k}: trivial reference"
        scale = r.abs().max().item()
        dev = (gk - r).abs().max().item()
        print(f"{name:>18s} {k:>6s}: max|ref| = {scale:.3e}  max|got - ref| = {dev:.3e} "
              f"(bound {1e-9 * scale + 1e-10:.3e})")
        assert torch.isfinite(gk).all(), (name, k)
        assert dev <= 1e-9 * scale + 1e-10, (name, k, dev, scale)


def run_kernels(c, dev):
    from botorch_amd import kernels
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    args = [t(c[k]) for k in ("mean", "L", "Z", "lo", "hi")]
    kw = dict(out_idx=c["out_idx"], logw=t(c["logw"]), F=t(c["F"]), Qp=c["Qp"], fat=c["fat"],
              tau_relu=c["tau_relu"], tau_max=c["tau_max"])
    acq, hvi = kernels.qlogehvi(*args, **kw)
    dmean, dL, dF, dlogw = kernels.qlogehvi_backward(*args, acq, hvi, t(c["dacq"]), **kw)
    return dict(acq=acq, hvi=hvi, dmean=dmean, dL=dL, dF=dF, dlogw=dlogw)


def launch_plan(c):
    """What the launchers of csrc/qlogehvi.hip choose for the case through
    kernels.qlogehvi / qlogehvi_backward (whose workspaces allow H = 8):
    sample split of the forward and of the backward, samples per workgroup,
    q bucket, cells staged in LDS."""
    B, S, q, m = c["B"], c["S"], c["q"], c["m"]
    shared = c["lo"].dim() == 2
    return dict(H_fwd=max(1, min(8, max(1, 1024 // B), S)), H_bwd=max(1, min(8, max(1, 256 // B), S)),
                qb=4 if q <= 4 else 8, lds=shared and c["lo"].shape[-2] * m <= 1024)


def test_cases_reach_their_paths():
    """The shapes above do exercise what they are named for (CPU)."""
    from botorch_amd.kernels import QLOGEHVI_QMAX
    plans = {n: launch_plan(build_case(n)) for n in CASES}
    assert all(build_case(n)["q"] <= QLOGEHVI_QMAX for n in CASES) and QLOGEHVI_QMAX == 8
    # sample split: off in both kernels, off in the backward only, on in both
    assert (plans["nosplit"]["H_fwd"], plans["nosplit"]["H_bwd"]) == (1, 1)
    assert plans["nosplit_bwd"]["H_fwd"] > 1 and plans["nosplit_bwd"]["H_bwd"] == 1
    assert plans["split"]["H_fwd"] > 1 and plans["split"]["H_bwd"] > 1
    # several passes of 16 samples per workgroup, in both kernels
    assert 256 // plans["passes"]["H_fwd"] > 16 and 256 // plans["passes"]["H_bwd"] > 16
    # q bucket edges and every (m, bucket) the dispatch has
    assert [plans[n]["qb"] for n in ("q1", "q4", "q5", "q8")] == [4, 4, 8, 8]
    reached = {(build_case(n)["m"], plans[n]["qb"]) for n in CASES}
    assert {(2, 4), (2, 8), (3, 4), (3, 8), (4, 4), (4, 8)} <= reached
    # cells in LDS, through cache (too many; per sample)
    assert plans["q4"]["lds"] and not plans["manycells"]["lds"] and not plans["persample"]["lds"]
    c = build_case("manycells")
    assert c["lo"].shape == (400, 3) and 400 * 3 > 1024
    assert build_case("onecell")["lo"].shape == (1, 2)
    assert build_case("q8")["lo"].shape[0] <= 9
    assert build_case("passes")["lo"].shape == (4, 4)
    for n in ("persample", "persample_m3", "withF_persample", "weights_map_F"):
        c = build_case(n)
        pad = ((c["lo"] == 0).all(-1) & (c["hi"] == 0).all(-1)).sum(-1)
        assert (pad >= 2).sum() >= c["S"] // 2 and (pad == 0).any(), n
    c = build_case("weights_map")
    assert (c["logw"] == 0).any() and (c["logw"] < 0).any() and c["Mt"] == 3
    c = build_case("hopeless")
    f = samples_from_roots(c["mean"], c["L"], c["Z"])
    assert ((torch.minimum(f.unsqueeze(-2), c["hi"]) - c["lo"]).clamp_min(0).prod(-1) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_qlogehvi_kernels_match_cpu_autograd(name):
    c = build_case(name)
    ref = reference(c)
    got = run_kernels(c, torch.device("cuda"))
    check(name, got, ref)
    # the members outside the map receive no gradient
    others = [i for i in range(c["Mt"]) if i not in c["out_idx"]]
    if others:
        assert (got["dmean"][others] == 0).all() and (got["dL"][others] == 0).all()


@pytest.mark.gpu
def test_qlogehvi_argument_errors():
    from botorch_amd import kernels
    c = build_case("q8")
    dev = torch.device("cuda")
    mean, L, Z = (torch.zeros(2, 1, 9, dtype=F64, device=dev), torch.zeros(2, 1, 9, 9, dtype=F64, device=dev),
                  torch.zeros(4, 18, dtype=F64, device=dev))
    with pytest.raises(ValueError, match="q <= 8"):
        kernels.qlogehvi(mean, L, Z, c["lo"].to(dev), c["hi"].to(dev))
    with pytest.raises(ValueError, match="temperatures"):
        kernels.qlogehvi(c["mean"].to(dev), c["L"].to(dev), c["Z"].to(dev), c["lo"].to(dev),
                         c["hi"].to(dev), tau_max=0.0)
