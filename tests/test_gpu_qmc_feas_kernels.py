"""bo_qmc_feas / bo_qmc_feas_backward alone (kernels.qmc_feas,
kernels.qmc_feas_backward) against CPU fp64 autograd through the torch
restatement of the constrained single-objective reductions
(tests/constrained_so_restatement.py, pinned to the reference by
tests/test_constrained_so_cpu.py) on f = mean + L z (+ F), with a random
mixed-sign dacq.  The reference is never another route of the library.

Bound: the project's kernel-against-torch bound, max|got - ref| <= 1e-9 max|ref|
+ 1e-10 over whole arrays.

Shapes: defaults q = 2, Mt = 2, k = 1, S = 5, B = 3; each case the smallest
that reaches a distinct path.  The launcher of csrc/qmc_feas.hip has one plan:
a workgroup per t-batch, the q bucket 4 / 8 / 16, and the samples in chunks of
min(256, S, (8000 - fixed) / per) with fixed = Mt q^2 + Mt q + 88 + 512 doubles
and per = (q Mt | 1) doubles per sample, plus (q (k + 1) | 1) in the backward (k
= 0 with an external weight tensor); ``launch_plan`` restates it and
test_cases_reach_their_paths checks every case's plan."""
import pytest
import torch

from tests.constrained_so_restatement import constrained_acq_from_samples, samples_from_roots

F64 = torch.float64

BASE = {
    # q bucket edges
    "q1": dict(q=1), "q4": dict(q=4), "q5": dict(q=5), "q8": dict(q=8), "q9": dict(q=9),
    "q16": dict(q=16),
    # one member, eight members (q = 16: the smallest chunk, several passes at S = 45)
    "mt1": dict(Mt=1), "mt8": dict(Mt=8, q=3), "mt8_q16_k8": dict(Mt=8, q=16, k=8, S=45, B=2),
    # eight constraints with distinct etas
    "k8": dict(k=8, Mt=3),
    # objective weights that are no unit vector, one negative
    "cmix": dict(Mt=3, c=(0.7, -0.4, 0.2), k=2),
    # several sample passes, the last one ragged; exactly one full chunk; S below the lanes
    "passes": dict(S=300, B=1), "fullchunk": dict(S=256, B=1), "ragged_q8": dict(q=8, Mt=4, k=2, S=301, B=1),
    # F with Qp > q and one best_f per sample (qNEI's inputs)
    "withF": dict(q=3, Qp=5, ps=True), "withF_mt3": dict(q=2, Mt=3, Qp=2, ps=True, k=2),
    # the external weight tensor: some weights exactly 1; in plain mode whole
    # samples with weight exactly 0 on points with a positive improvement
    "ext": dict(q=3, ext=True), "ext_F": dict(q=4, Mt=3, ext=True, Qp=6, ps=True),
    # no constraint at all
    "k0": dict(k=0),
}
CASES = {}
for _n, _spec in BASE.items():
    CASES[_n] = dict(_spec, log=False)
    CASES[_n + "_log"] = dict(_spec, log=True)
CASES.update({
    # plain mode with the fat sigmoid
    "q4_fatsig": dict(q=4, fat=True, log=False),
    # both fat values and both default tau_max in log mode
    "q4_log_nofat": dict(q=4, log=True, fat=False), "q4_log_tau3": dict(q=4, log=True, tau_max=1e-3),
    "q4_log_nofat_tau3": dict(q=4, log=True, fat=False, tau_max=1e-3),
    "ext_log_nofat": dict(q=3, ext=True, log=True, fat=False),
    # every point far below best_f and infeasible
    "hopeless": dict(q=4, log=True, kind="hopeless"),
    "hopeless_nofat": dict(q=4, log=True, fat=False, kind="hopeless"),
})
DEFAULTS = dict(q=2, Mt=2, k=1, S=5, B=3, log=False, fat=None, ext=False, Qp=0, ps=False, c=None,
                tau_relu=1e-6, tau_max=1e-2, kind="mixed")


def build_case(name):
    """CPU inputs of the case (a dict of tensors and options)."""
    c = dict(DEFAULTS, **CASES[name])
    if c["fat"] is None:
        c["fat"] = c["log"]          # the classes' defaults: qEI logistic, qLogEI fat
    q, Mt, k, S, B = c["q"], c["Mt"], c["k"], c["S"], c["B"]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    has_F = c["Qp"] > 0
    part = 0.25 / (3.0 if has_F else 2.0) ** 0.5
    mean = part * rn(Mt, B, q)
    L = torch.tril(rn(Mt, B, q, q))
    L = part * L / L.norm(dim=-1, keepdim=True).clamp_min(1e-3)
    L = L + torch.diag_embed(torch.full((Mt, B, q), 1e-3, dtype=F64))
    Z = rn(S, q * Mt)
    F = part * rn(Mt, S, B * c["Qp"] + 3) if has_F else None   # ldF > B Qp
    cw = torch.tensor(c["c"], dtype=F64) if c["c"] is not None else torch.eye(Mt, dtype=F64)[0]
    hopeless = c["kind"] == "hopeless"
    best_f = 5.0 if hopeless else -0.1
    best_f_s = best_f + 0.1 * rn(S) if c["ps"] else None
    # constraints a_i . f <= rhs_i on samples of spread 0.25: etas of that order
    # give weights all over (0, 1); the hopeless set lies 3 outside
    A = rn(k, Mt) if k else None
    # (several constraints: each looser, so that their product still reaches 1)
    rhs = (0.1 * rn(k) + 0.12 * (k - 1) - (3.0 + A.abs().sum(-1) if hopeless else 0.0)) if k else None
    eta = torch.tensor([0.02 * 1.3 ** i for i in range(k)], dtype=F64) if k else None
    feas = None
    if c["ext"]:
        A = rhs = eta = None
        w = torch.rand(S, B, q, generator=g, dtype=F64).clamp_min(1e-3)
        w[torch.rand(S, B, q, generator=g, dtype=F64) < 0.3] = 1.0
        if not c["log"]:
            w[::3] = 0.0
        feas = w.log() if c["log"] else w
    dacq = rn(B)
    dacq[0] = -abs(dacq[0]) - 0.1
    if B > 1:
        dacq[1] = abs(dacq[1]) + 0.1
    c.update(name=name, mean=mean, L=L, Z=Z, F=F, cw=cw, best_f=best_f, best_f_s=best_f_s, A=A,
             rhs=rhs, eta=eta, feas=feas, dacq=dacq)
    return c


def _constraints(c):
    from botorch_amd.objective import get_outcome_constraint_transforms
    if c["A"] is None:
        return None
    return get_outcome_constraint_transforms((c["A"], c["rhs"].unsqueeze(-1)))


def reference(c, log=None):
    """CPU fp64 autograd through the restatement -> acq, dmean, dL, dF, dfeas."""
    log = c["log"] if log is None else log
    leaves = [c["mean"].clone().requires_grad_(True), c["L"].clone().requires_grad_(True)]
    if c["F"] is not None:
        leaves.append(c["F"].clone().requires_grad_(True))
    feas = c["feas"].clone().requires_grad_(True) if c["feas"] is not None else None
    if feas is not None:
        leaves.append(feas)
    f = samples_from_roots(leaves[0], leaves[1], c["Z"], leaves[2] if c["F"] is not None else None,
                           c["Qp"])
    acq = constrained_acq_from_samples(
        f, c["cw"], c["best_f_s"] if c["best_f_s"] is not None else c["best_f"], _constraints(c),
        c["eta"], log=log, fat=c["fat"], tau_relu=c["tau_relu"], tau_max=c["tau_max"], feas=feas)
    grads = list(torch.autograd.grad(acq, leaves, c["dacq"], allow_unused=True))
    out = dict(acq=acq.detach(), dmean=grads.pop(0), dL=grads.pop(0))
    out["dF"] = grads.pop(0) if c["F"] is not None else None
    out["dfeas"] = grads.pop(0) if feas is not None else None
    return out


def check(name, got, ref, trivial_ok=()):
    """The bound on every output; every reference non-trivial."""
    for k, r in ref.items():
        if r is None:
            assert got[k] is None, (name, k)
            continue
        gk = got[k].detach().cpu()
        assert gk.shape == r.shape, (name, k, gk.shape, r.shape)
        assert torch.isfinite(r).all(), f"{name}/{k}: reference not finite"
        assert k in trivial_ok or r.abs().max() > 0, f"{name}/{k}: trivial reference"
        scale = r.abs().max().item()
        dev = (gk - r).abs().max().item()
        print(f"{name:>20s} {k:>6s}: max|ref| = {scale:.3e}  max|got - ref| = {dev:.3e} "
              f"(bound {1e-9 * scale + 1e-10:.3e})")
        assert torch.isfinite(gk).all(), (name, k)
        assert dev <= 1e-9 * scale + 1e-10, (name, k, dev, scale)


def run_kernels(c, dev, log=None, backward=True):
    from botorch_amd import kernels
    log = c["log"] if log is None else log
    t = lambda x: None if x is None else x.to(dev)  # noqa: E731
    args = [t(c[k]) for k in ("mean", "L", "Z")] + [c["cw"].tolist()]
    kw = dict(best_f=c["best_f"], best_f_s=t(c["best_f_s"]),
              A=c["A"].tolist() if c["A"] is not None else None,
              rhs=c["rhs"].tolist() if c["rhs"] is not None else None,
              eta=c["eta"].tolist() if c["eta"] is not None else None, feas=t(c["feas"]), F=t(c["F"]),
              Qp=c["Qp"], log=log, fat=c["fat"], tau_relu=c["tau_relu"], tau_max=c["tau_max"])
    acq = kernels.qmc_feas(*args, **kw)
    if not backward:
        return dict(acq=acq)
    dmean, dL, dF, dfeas = kernels.qmc_feas_backward(*args, t(c["dacq"]), acq=acq, **kw)
    return dict(acq=acq, dmean=dmean, dL=dL, dF=dF, dfeas=dfeas)


def launch_plan(c):
    """What the launcher of csrc/qmc_feas.hip chooses for the case: the q
    bucket and the samples per LDS chunk of the forward and of the backward."""
    q, Mt, S = c["q"], c["Mt"], c["S"]
    k = 0 if c["ext"] else c["k"]
    fixed = Mt * q * q + Mt * q + 88 + 512
    zs, gs = (q * Mt) | 1, (q * (k + 1)) | 1
    return dict(qb=4 if q <= 4 else 8 if q <= 8 else 16,
                chunk_fwd=max(1, min(256, S, (8000 - fixed) // zs)),
                chunk_bwd=max(1, min(256, S, (8000 - fixed) // (zs + gs))))


def test_cases_reach_their_paths():
    """The shapes above do exercise what they are named for (CPU)."""
    from botorch_amd import kernels
    assert (kernels.QMC_FEAS_QMAX, kernels.QMC_FEAS_MTMAX, kernels.QMC_FEAS_KMAX) == (16, 8, 8)
    cs = {n: build_case(n) for n in CASES}
    plans = {n: launch_plan(c) for n, c in cs.items()}
    assert [plans[n]["qb"] for n in ("q1", "q4", "q5", "q8", "q9", "q16")] == [4, 4, 8, 8, 16, 16]
    # every (bucket, log, external) instantiation the dispatch has
    reached = {(plans[n]["qb"], c["log"], c["ext"]) for n, c in cs.items()}
    assert {(qb, lg, False) for qb in (4, 8, 16) for lg in (False, True)} <= reached
    assert {(4, False, True), (4, True, True)} <= reached
    # sample passes: several with a ragged last one, exactly one, a fraction of one
    for n in ("passes", "passes_log"):
        assert plans[n]["chunk_fwd"] == plans[n]["chunk_bwd"] == 256 and cs[n]["S"] % 256 != 0
    assert plans["fullchunk"]["chunk_bwd"] == 256 == cs["fullchunk"]["S"]
    p = plans["ragged_q8"]
    assert p["chunk_bwd"] < p["chunk_fwd"] < 256 and 301 % p["chunk_bwd"] and 301 % p["chunk_fwd"]
    # the largest configuration: LDS allows 19 samples a pass in the backward, 40 in the forward
    p = plans["mt8_q16_k8"]
    assert (p["chunk_fwd"], p["chunk_bwd"]) == (40, 19) and cs["mt8_q16_k8"]["S"] > 2 * 19
    assert plans["mt1"]["chunk_bwd"] == 5       # S below the lanes: one partial pass
    c = cs["k8"]
    assert c["A"].shape == (8, 3) and len(set(c["eta"].tolist())) == 8
    c = cs["cmix"]
    assert (c["cw"] < 0).any() and (c["cw"] != 0).sum() == 3
    for n in ("withF", "withF_mt3", "ext_F"):
        assert cs[n]["F"] is not None and cs[n]["best_f_s"] is not None
    assert cs["withF"]["Qp"] > cs["withF"]["q"] and cs["ext_F"]["Qp"] > cs["ext_F"]["q"]
    # external weights: exactly 1 somewhere; plain: exactly 0 on points with a
    # positive improvement in samples whose maximum is therefore a tie at 0
    for n in ("ext", "ext_F"):
        c = cs[n]
        f = samples_from_roots(c["mean"], c["L"], c["Z"], c["F"], c["Qp"])
        bf = c["best_f_s"].reshape(-1, 1, 1) if c["best_f_s"] is not None else c["best_f"]
        imp = torch.einsum("...m, m", [f, c["cw"]]) - bf
        w = c["feas"]
        assert (w == 1).any() and ((w == 0) & (imp > 0)).any()
        assert (reference(c)["dfeas"][w == 0] > 0).any() or (reference(c)["dfeas"][w == 0] < 0).any()
        assert (cs[n + "_log"]["feas"] == 0).any() and (cs[n + "_log"]["feas"] < 0).any()
    # the weights of the in-kernel cases spread over (0, 1)
    for n in ("q4", "k8", "cmix", "q16_log"):
        c = cs[n]
        from botorch_amd.objective import compute_smoothed_feasibility_indicator
        w = compute_smoothed_feasibility_indicator(
            _constraints(c), samples_from_roots(c["mean"], c["L"], c["Z"]), c["eta"], fat=c["fat"])
        assert (w < 0.3).any() and (w > 0.7).any(), n
    # hopeless: the plain value exactly 0, the log value finite with a gradient
    for n in ("hopeless", "hopeless_nofat"):
        r = reference(cs[n])
        assert (reference(cs[n], log=False)["acq"] == 0).all()
        assert torch.isfinite(r["acq"]).all() and r["dmean"].abs().max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_qmc_feas_kernels_match_cpu_autograd(name):
    c = build_case(name)
    ref = reference(c)
    dev = torch.device("cuda")
    got = run_kernels(c, dev)
    check(name, got, ref)
    # bitwise reproducible from run to run
    again = run_kernels(c, dev)
    for k, v in got.items():
        assert v is None or torch.equal(v, again[k]), (name, k)
    if c["kind"] == "hopeless":
        plain = run_kernels(c, dev, log=False, backward=False)
        assert (plain["acq"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("log", [False, True])
def test_unconstrained_equals_qmc_finalize(log):
    """No constraints, c = e_0, Mt = 1: the value bo_qmc_finalize computes from
    the same mean / L / Z in QEI and QLOGEI mode."""
    from botorch_amd import _lib, kernels
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(5)
    n, B, q, S = 40, 3, 4, 33
    X = torch.rand(n, 3, generator=g, dtype=F64).to(dev)
    y = torch.randn(n, generator=g, dtype=F64).to(dev)
    ls = torch.full((3,), 0.4, dtype=F64, device=dev)
    cache = kernels.build_gp_cache(X, y, ls, 1e-2, 0.1, outputscale=1.3)
    Xc = torch.rand(B, q, 3, generator=g, dtype=F64).to(dev)
    Z = torch.randn(S, q, generator=g, dtype=F64).to(dev)
    pp = kernels.post_partials(cache, Xc)
    lp = (1, 1e-6, 1e-2)
    out = kernels.qmc_finalize(cache, pp, _lib.QMC_QLOGEI if log else _lib.QMC_QEI, 0.0, 1.0, Z=Z,
                               best_f=0.3, want_cov=False, want_L=True, log_params=lp if log else None)
    acq = kernels.qmc_feas(out["mean"][None], out["L"][None], Z, [1.0], best_f=0.3, log=log, fat=True,
                           tau_relu=lp[1], tau_max=lp[2])
    ref = out["acq"]
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    dev_ = (acq - ref).abs().max().item()
    print(f"qmc_feas against qmc_finalize ({'log' if log else 'plain'}): max diff {dev_:.3e}, "
          f"max|ref| {ref.abs().max().item():.3e}")
    assert dev_ <= 1e-9 * ref.abs().max().item() + 1e-10


@pytest.mark.gpu
def test_qmc_feas_library_argument_errors():
    """The C entry's own checks (reached with the wrapper's bypassed)."""
    import ctypes
    from botorch_amd import _lib
    from botorch_amd.kernels import _qmc_feas_args, _stream
    dev = torch.device("cuda")
    c = build_case("q4")
    a = _qmc_feas_args(c["mean"].to(dev), c["L"].to(dev), c["Z"].to(dev), c["cw"].tolist(), 0.0, None,
                       c["A"].tolist(), c["rhs"].tolist(), c["eta"].tolist(), None, None, 0, False,
                       False, 1e-6, 1e-2)
    a.q = 17
    assert _lib.lib().bo_qmc_feas_v(ctypes.byref(a), _stream(dev)) == _lib.BO_ERR_ARG
    assert b"q <= 16" in _lib.lib().bo_last_error()
