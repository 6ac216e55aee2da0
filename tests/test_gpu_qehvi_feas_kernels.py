"""The feasibility-weighted qEHVI kernels (bo_qehvi_feas_v /
bo_qehvi_feas_backward_v), called directly through ``kernels.qehvi_feas`` and
``kernels.qehvi_feas_backward``, against CPU fp64 torch autograd through a
plain restatement of qExpectedHypervolumeImprovement._compute_qehvi WITH its
feasibility weights (acquisition/multi_objective/monte_carlo.py:276-315):

  HVI_s,b = sum_k sum_{T} (-1)^{|T|+1} prod_{p in T} w[s,b,p]
                          prod_t max(min(u_kt, min_{p in T} f[s,b,p,t]) - l_kt, 0)

applied to f = mean + L z (+ F) and a leaf w, with a random mixed-sign dacq.

The reference is never another route of the library.  Every output array is
compared whole under  max|got - ref| <= 1e-9 max|ref| + 1e-10  (the project's
bound for a kernel against torch), every case asserts that its reference is
non-trivial and every comparison prints its measured deviation.  Weights are
uniform in (0, 1) with some entries exactly 0.0 and some exactly 1.0 (a
saturated or underflowed sigmoid): the gradient w.r.t. such a weight is formed
without dividing by it.
"""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
RTOL, ATOL = 1e-9, 1e-10


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k) + 1
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F64)


def _cotangent(g, *shape):
    """Random cotangent: mixed sign and (three or more entries) one exact 0.0."""
    c = _randn(g, *shape)
    v = c.view(-1)
    n = v.numel()
    if n == 1:
        v[0] = v[0].abs() + 0.25
    else:
        v[0] = v[0].abs() + 0.1
        v[n - 1] = -(v[n - 1].abs() + 0.1)
        if n >= 3:
            v[n // 2] = 0.0
    return c


def _weights(g, S, B, q):
    """Uniform (0, 1) with about one entry in eight exactly 0.0 and one in
    eight exactly 1.0 (at least one of each where there are three entries)."""
    w = _rand(g, S, B, q)
    pick = _rand(g, S, B, q)
    w[pick < 0.125] = 0.0
    w[pick > 0.875] = 1.0
    v = w.view(-1)
    if v.numel() >= 3:
        v[1] = 0.0
        v[2] = 1.0
    return w


def _pow2(q):
    Qp = 1
    while Qp < q:
        Qp *= 2
    return Qp


def _check(tag, name, got, ref, half_nonzero=False, rtol=RTOL, atol=ATOL):
    got = got.detach().cpu()
    ref = ref.detach()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    scale = ref.abs().max().item()
    dev = (got - ref).abs().max().item()
    nz = (ref != 0).double().mean().item()
    print(f"[{tag}] {name}: max|got-ref| = {dev:.3e}  max|ref| = {scale:.3e}  "
          f"rel = {dev / scale if scale > 0 else float('nan'):.3e}  nonzero = {nz:.2f}")
    assert scale > 0, f"{name}: trivial reference"
    if half_nonzero:
        assert nz >= 0.5, f"{name}: only {nz:.2f} of the reference is non-zero"
    assert dev <= rtol * scale + atol, f"{name}: {dev:.3e} > {rtol} * {scale:.3e} + {atol}"


def weighted_qehvi_from_samples(obj, w, cell_lower, cell_upper):
    """monte_carlo.py:276-315 with feas_subsets.prod: obj S x b x q x m, w
    S x b x q, cells K x m (shared) or S x K x m (one set per sample).  -> b."""
    S, b, q, m = obj.shape
    per_sample = cell_lower.dim() == 3
    K = cell_lower.shape[-2]
    view = (S, 1, K, 1, m) if per_sample else (1, 1, K, 1, m)
    total = torch.zeros(S, b, K, dtype=obj.dtype)
    for i in range(1, q + 1):
        idx = torch.tensor(list(itertools.combinations(range(q), i)), dtype=torch.long)
        sub = obj[:, :, idx.view(-1), :].view(S, b, idx.shape[0], i, m)
        ov = sub.min(dim=-2).values                                   # S x b x C x m
        ov = torch.minimum(ov.unsqueeze(-3), cell_upper.view(view))   # S x b x K x C x m
        lengths = (ov - cell_lower.view(view)).clamp_min(0.0)
        areas = lengths.prod(dim=-1)                                  # S x b x K x C
        wsub = w[:, :, idx.view(-1)].view(S, b, idx.shape[0], i).prod(dim=-1)
        areas = areas * wsub.unsqueeze(-2)
        total = total + (-1) ** (i + 1) * areas.sum(dim=-1)
    return total.sum(dim=-1).mean(dim=0)


def _case(m, q, S, B, K, per_sample=False, with_F=False, Mt=None, out_idx=None, w=None):
    """Inputs over Mt members (objective t = member out_idx[t]) and the
    reference value and gradients w.r.t. mean, L, w (and F)."""
    Mt = m if Mt is None else Mt
    out_idx = list(range(m)) if out_idx is None else list(out_idx)
    g = _gen(21, m, q, S, B, K, per_sample, with_F, Mt, *out_idx)
    mean = (0.5 * _randn(g, Mt, B, q)).requires_grad_(True)
    L = (0.3 * _randn(g, Mt, B, q, q).tril() + torch.eye(q, dtype=F64)).requires_grad_(True)
    Z = _randn(g, S, q * Mt)
    cshape = (S, K, m) if per_sample else (K, m)
    lo = -2.0 * _rand(g, *cshape)
    hi = lo + 2.0 * _rand(g, *cshape)
    if K == 1:     # one cell: wide enough that the samples meet it
        lo, hi = lo - 3.0, hi + 1.0
    dacq = _cotangent(g, B)
    w = (_weights(g, S, B, q) if w is None else w.clone()).requires_grad_(True)
    leaves = [mean, L, w]
    f = mean.permute(1, 2, 0).unsqueeze(0) + torch.einsum("tbpj,sjt->sbpt", L, Z.view(S, q, Mt))
    Fk, Qp = None, 0
    if with_F:
        Qp = _pow2(q)
        ldF = B * Qp + 3                      # ldF > B Qp
        Fk = (0.3 * _randn(g, Mt, S, ldF)).requires_grad_(True)
        leaves.append(Fk)
        f = f + Fk[:, :, : B * Qp].view(Mt, S, B, Qp)[..., :q].permute(1, 2, 3, 0)
    acq = weighted_qehvi_from_samples(f[..., out_idx], w, lo, hi)
    grads = torch.autograd.grad(acq, leaves, dacq)
    return dict(mean=mean.detach(), L=L.detach(), Z=Z, lo=lo, hi=hi, dacq=dacq, w=w.detach(),
                Fk=Fk.detach() if with_F else None, Qp=Qp, acq=acq.detach(), dmean=grads[0],
                dL=grads[1], dw=grads[2], dF=grads[3] if with_F else None, out_idx=out_idx, Mt=Mt)


def _dv(t):
    return t.to(DEV) if t is not None else None


def _run(c, **out):
    from botorch_amd import kernels
    args = [_dv(c[k]) for k in ("mean", "L", "Z", "lo", "hi", "w")]
    acq = kernels.qehvi_feas(*args, c["out_idx"], F=_dv(c["Fk"]), Qp=c["Qp"])
    res = kernels.qehvi_feas_backward(*args, c["out_idx"], _dv(c["dacq"]), F=_dv(c["Fk"]),
                                      Qp=c["Qp"], **out)
    return acq, res


def _check_case(tag, c, acq, res, half=True):
    q = c["mean"].shape[-1]
    low = torch.ones(q, q, dtype=torch.bool).tril()
    _check("bo_qehvi_feas", f"{tag} acq", acq, c["acq"], half)
    _check("bo_qehvi_feas_backward", f"{tag} dmean", res[0], c["dmean"])
    dL = res[1].cpu()
    _check("bo_qehvi_feas_backward", f"{tag} dL (lower)", dL[..., low], c["dL"][..., low])
    assert (dL[..., ~low] == 0).all(), "dL: strict upper triangle not zero"
    if c["Fk"] is not None:
        _check("bo_qehvi_feas_backward", f"{tag} dF", res[2], c["dF"])
    _check("bo_qehvi_feas_backward", f"{tag} dfeas", res[-1], c["dw"])


# m, q, S, B, K, per-sample cells, F
CASES = [
    (2, 1, 1, 1, 1, False, False),       # smallest shape
    (3, 2, 3, 1, 8, False, False),       # S below the sample split
    (4, 5, 24, 3, 20, False, False),     # q <= 8 bucket, m = 4
    (4, 12, 16, 2, 16, False, False),    # q = 12 bucket, sample split
    (2, 3, 16, 2, 600, False, False),    # cells read from global memory
    (2, 2, 8, 300, 4, False, False),     # no backward split
    (3, 4, 16, 2, 10, True, True),       # per-sample cells with F, ldF > B Qp
]


@pytest.mark.parametrize("m,q,S,B,K,per_sample,with_F", CASES)
def test_weighted_value_and_backward(m, q, S, B, K, per_sample, with_F):
    c = _case(m, q, S, B, K, per_sample, with_F)
    if c["w"].numel() >= 3:
        assert (c["w"] == 0).any() and (c["w"] == 1).any()
    acq, res = _run(c)
    tag = f"m={m} q={q} S={S} B={B} K={K}" + (" per-sample F" if with_F else "")
    _check_case(tag, c, acq, res, half=B > 1)


def test_output_map_writes_objective_slices_only():
    """Mt = 5 members, objectives = members (3, 0), zm = 5: values and
    gradients against the reference on f[..., (3, 0)], with dmean / dL / dF
    pre-filled with a sentinel that must survive outside the objective slices."""
    m, q, S, B, K, Mt, oi = 2, 3, 16, 2, 12, 5, (3, 0)
    c = _case(m, q, S, B, K, per_sample=True, with_F=True, Mt=Mt, out_idx=oi)
    SENT = -7.25
    dmean = torch.full((Mt, B, q), SENT, dtype=F64, device=DEV)
    dL = torch.full((Mt, B, q, q), SENT, dtype=F64, device=DEV)
    dF = torch.full(tuple(c["Fk"].shape), SENT, dtype=F64, device=DEV)
    acq, res = _run(c, dmean=dmean, dL=dL, dF=dF)
    rest = [t for t in range(Mt) if t not in oi]
    for name, o in (("dmean", res[0]), ("dL", res[1]), ("dF", res[2])):
        assert (o[rest] == SENT).all(), f"{name}: a slice of a non-objective member was written"
    # dF: the kernel writes rows b Qp + p (p < q) of the objective slices only
    Qp = c["Qp"]
    pad = torch.ones_like(res[2], dtype=torch.bool)
    pad[:, :, : B * Qp].view(Mt, S, B, Qp)[..., :q] = False
    assert (res[2][pad] == SENT).all(), "dF: padding written"
    zero = lambda t: torch.where(t == SENT, torch.zeros_like(t), t)  # noqa: E731
    res = (zero(res[0]), zero(res[1]), zero(res[2]), res[3])
    assert (c["dmean"][rest] == 0).all() and (c["dL"][rest] == 0).all()
    _check_case("Mt=5 out_idx=(3,0)", c, acq, res)


# The plain and the weighted launches share one launcher.  B = 2: every launch
# splits the samples (forward: B <= 512, backward: B <= 128); B = 600: none does.
@pytest.mark.parametrize("m,q,S,B,K", [(3, 4, 16, 5, 30), (2, 12, 16, 2, 16), (2, 2, 16, 2, 3),
                                       (2, 2, 16, 600, 3)])
def test_unit_weights_match_unweighted_kernels(m, q, S, B, K):
    """(a) all weights exactly 1.0: the unweighted kernels' acq, dmean, dL."""
    from botorch_amd import kernels
    c = _case(m, q, S, B, K, w=torch.ones(S, B, q, dtype=F64))
    acq, res = _run(c)
    args = [_dv(c[k]) for k in ("mean", "L", "Z", "lo", "hi")]
    acq0 = kernels.qehvi(*args).cpu()
    dmean0, dL0 = [o.cpu() for o in kernels.qehvi_backward(*args, _dv(c["dacq"]))]
    same = [torch.equal(a.cpu(), b) for a, b in ((acq, acq0), (res[0], dmean0), (res[1], dL0))]
    print(f"[unit weights] m={m} q={q}: bit-identical acq / dmean / dL = {same}")
    _check("unit weights", "acq", acq, acq0)
    _check("unit weights", "dmean", res[0], dmean0)
    _check("unit weights", "dL", res[1], dL0)
    _check_case(f"unit weights m={m} q={q}", c, acq, res)


@pytest.mark.parametrize("p", [0, 1, 3])
def test_zero_weight_drops_the_point(p):
    """(b) w[:, :, p] = 0 equals the same problem without point p (q - 1
    points): values to 1e-12 relative."""
    from botorch_amd import kernels
    m, q, S, B, K = 3, 4, 16, 3, 25
    g = _gen(22, p)
    mean = 0.5 * _randn(g, m, B, q)
    L = torch.diag_embed(0.5 + _rand(g, m, B, q))     # independent points: dropping one is exact
    Z = _randn(g, S, q, m)
    lo = -2.0 * _rand(g, K, m)
    hi = lo + 2.0 * _rand(g, K, m)
    w = 0.05 + 0.9 * _rand(g, S, B, q)
    w[:, :, p] = 0.0
    keep = [i for i in range(q) if i != p]
    full = kernels.qehvi_feas(_dv(mean), _dv(L), _dv(Z.reshape(S, -1)), _dv(lo), _dv(hi), _dv(w),
                              range(m)).cpu()
    less = kernels.qehvi_feas(_dv(mean[..., keep]), _dv(L[..., keep, :][..., keep].contiguous()),
                              _dv(Z[:, keep].reshape(S, -1)), _dv(lo), _dv(hi),
                              _dv(w[..., keep].contiguous()), range(m)).cpu()
    assert (less.abs() > 0).all()
    _check("zero weight", f"p={p}: q points with w_p = 0 vs q - 1 points", full, less, rtol=1e-12,
           atol=0.0)


def test_known_answers():
    """(c) the reference's own constrained qEHVI values (test_monte_carlo.py:
    608-711): ref point (0, 0), the cells of the front
    [[4,5],[5,5],[8.5,3.5],[8.5,3],[9,1]], one sample (6.5, 4.5), weights from
    the smoothed indicator of the reference's constraint lists.  The
    unconstrained improvement of (6.5, 4.5) is 1.5."""
    from botorch_amd import kernels
    from botorch_amd.objective import compute_smoothed_feasibility_indicator
    Y = torch.tensor([[4.0, 5.0], [5.0, 5.0], [8.5, 3.5], [8.5, 3.0], [9.0, 1.0]], dtype=F64)
    from botorch_amd.multi_objective import FastNondominatedPartitioning
    lo, hi = FastNondominatedPartitioning(torch.zeros(2, dtype=F64), Y).get_hypercell_bounds()
    lo, hi = lo.to(F64).contiguous(), hi.to(F64).contiguous()
    sample = torch.tensor([6.5, 4.5], dtype=F64)
    sig = lambda x: 1.0 / (1.0 + math.exp(-x))  # noqa: E731

    def run(q, cons, eta, expect):
        samples = sample.view(1, 1, 1, 2).expand(1, 1, q, 2).contiguous()
        w = compute_smoothed_feasibility_indicator(cons, samples, torch.as_tensor(eta, dtype=F64)
                                                   if not isinstance(eta, float) else eta, fat=False)
        mean = sample.view(2, 1, 1).expand(2, 1, q).contiguous()
        L = torch.zeros(2, 1, q, q, dtype=F64)
        Z = torch.zeros(1, 2 * q, dtype=F64)
        acq = kernels.qehvi_feas(_dv(mean), _dv(L), _dv(Z), _dv(lo), _dv(hi), _dv(w.to(F64)),
                                 (0, 1)).cpu()
        dev = abs(acq.item() - expect)
        print(f"[known answers] q={q} eta={eta}: got {acq.item():.15g} expected {expect:.15g} "
              f"|diff| = {dev:.2e}")
        assert dev <= 1e-12

    zero = lambda Z: torch.zeros_like(Z[..., -1])  # noqa: E731
    run(1, [zero], 1e-3, 0.75)                                         # w = sigmoid(0) = 1/2
    run(1, [zero, zero], 1e-3, 0.375)                                  # w = 1/4
    run(2, [zero], 1e-3, 1.5 * (2 * 0.5 - 0.25))       # two equal points: 2 w a - w^2 a, a = 1.5
    run(1, [lambda Z: torch.ones_like(Z[..., -1])] * 2, 1.0, 1.5 * sig(-1.0) ** 2)
    run(1, [lambda Z: torch.ones_like(Z[..., -1])] * 2, [1.0, 10.0], 1.5 * sig(-1.0) * sig(-0.1))
    run(1, [lambda Z: -100.0 * torch.ones_like(Z[..., -1])], 1e-3, 1.5)
    run(1, [lambda Z: 100.0 * torch.ones_like(Z[..., -1])], 1e-3, 0.0)
