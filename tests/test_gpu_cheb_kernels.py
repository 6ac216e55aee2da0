"""bo_qmc_cheb and bo_qmc_cheb_backward against the restatement (tests/cheb_restatement.py).
The bound of each output is 10 x the largest disagreement of the restatement's two forms over
CASES, as max |x - y| / max |y|, computed here from the restatement alone."""
import pytest
import torch

from tests import cheb_restatement as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# (q, Mt, S, B, k, neg, outside, G, chunk, log, fat, noisy, ext): one axis at a time from BASE;
# ext: the caller's feasibility tensor in place of the constraint table, and its cotangent
BASE = dict(q=3, Mt=3, S=80, B=3, k=2, neg=True, outside=False, G=1, chunk=32, log=True,
            fat=True, noisy=True, ext=False)
VARY = [{}, dict(q=1), dict(q=5), dict(q=16), dict(Mt=2), dict(Mt=8), dict(Mt=4, outside=True),
        dict(S=1), dict(S=17), dict(B=1), dict(G=3), dict(G=3, chunk=16), dict(k=0),
        dict(neg=False), dict(log=False), dict(log=False, noisy=False), dict(noisy=False),
        dict(fat=False), dict(chunk=0), dict(ext=True), dict(ext=True, log=False, G=3),
        dict(q=16, Mt=8, S=80, B=3, k=2, G=3)]
CASES = [tuple({**BASE, **v}.values()) for v in VARY]
NAMES = ("acq", "dmean", "dL", "dF", "dfeas")


def _err(got, want):
    return float((got.cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _case(case):
    q, Mt, S, B, k, neg, outside, G, chunk, log, fat, noisy, ext = case
    c = ref.make_case(q, Mt, S, B, k, neg, outside, noisy, seed=7, ext=ext)
    return c, torch.linspace(0.5, 1.5, B, dtype=torch.float64)


@pytest.fixture(scope="module")
def restated():
    """Per case the form-0 outputs, and per output the file's bound."""
    want, worst = {}, dict.fromkeys(NAMES, 0.0)
    for case in CASES:
        c, dacq = _case(case)
        log, fat = case[9], case[10]
        assert ref.smallest_gap(c, log, fat) > 1e-9  # no max can flip at rounding
        want[case] = ref.value_and_grads(c, log, fat, dacq, form=0)
        other = ref.value_and_grads(c, log, fat, dacq, form=1)
        for name, x, y in zip(NAMES, other, want[case]):
            if y is not None:
                worst[name] = max(worst[name], _err(x, y))
    return want, {name: 10.0 * v for name, v in worst.items()}


def _run(case, c, dacq):
    from botorch_amd import kernels
    q, Mt, S, B, k, neg, outside, G, chunk, log, fat, noisy, ext = case
    ca, cb = ref.affine(c)
    dev = lambda t: None if t is None else t.to(DEV)
    kw = dict(best_f=c["best_f"], best_f_s=dev(c["best_f_s"]), A=c["A"].tolist(),
              rhs=c["rhs"].tolist(), eta=c["eta"], F=dev(c["F"]), Qp=c["Qp"] if noisy else 0,
              log=log, fat=fat, tau_relu=ref.TAU_RELU, tau_max=ref.TAU_MAX, G=G, chunk=chunk,
              feas=dev(ref.feas_input(c, log)))
    m, l, z = dev(c["mean"]), dev(c["L"]), dev(c["Z"])
    acq = kernels.qmc_cheb(m, l, z, ca, cb, ref.ALPHA, **kw)
    return (acq,) + kernels.qmc_cheb_backward(m, l, z, ca, cb, ref.ALPHA, dev(dacq), acq=acq, **kw)


@pytest.mark.parametrize("case", CASES, ids=[str(v) for v in VARY])
def test_value_and_gradients(case, restated):
    want, bound = restated
    c, dacq = _case(case)
    got = _run(case, c, dacq)
    errs = {n: _err(g, w) for n, g, w in zip(NAMES, got, want[case]) if w is not None}
    print("errors:", errs, "bounds:", bound)
    assert all(errs[n] <= bound[n] for n in errs)
    assert torch.equal(got[2], got[2].tril())


def test_same_groups_bitwise_equal():
    case = tuple({**BASE, "G": 3, "chunk": 16}.values())
    c, dacq = _case(case)
    first, again = _run(case, c, dacq), _run(case, c, dacq)
    assert all(torch.equal(x, y) for x, y in zip(first, again) if x is not None)
