"""qLogEHVI / qLogNEHVI on the CPU (acquisition/multi_objective/logei.py): the
torch restatement of the log-space reduction (tests/logehvi_restatement.py,
which composes botorch_amd.safe_math) against the reference's own outputs
(tests/golden/golden_logehvi.npz, made by make_golden_logehvi.py from the
reference safe_math), values and gradients; the new safe_math functions; the
reference's known answers; the classes' argument checks."""
import math
import os

import numpy as np
import pytest
import torch

from tests.golden.make_golden_logehvi import TAUS, case_table
from tests.logehvi_restatement import log_hvi_per_sample, log_qehvi_from_samples

F64 = torch.float64
CASES = case_table()


@pytest.fixture(scope="module")
def golden_log():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                "golden_logehvi.npz"))


def test_case_table_covers_the_required_axes(golden_log):
    tags = {c[0] for c in CASES}
    for tag in tags:     # every case is recorded
        assert f"{tag}_acq" in golden_log.files and f"{tag}_dobj" in golden_log.files
    assert len(tags) == len(CASES)
    for m in (2, 3):
        for q in (1, 2, 3, 4):
            assert any(c[1] == f"m{m}q{q}" for c in CASES)
    assert {c[2] for c in CASES} == {True, False}
    assert {TAUS[c[3]] for c in CASES} == {(1e-6, 1e-2), (1e-6, 1e-3), (1e-3, 1e-1)}
    assert {c[4] for c in CASES} == {True, False} and {c[5] for c in CASES} == {True, False}
    assert any(c[1] == "hopeless" for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_matches_reference(golden_log, case):
    tag, inp, fat, tk, per_sample, with_w = case
    tau_relu, tau_max = TAUS[tk]
    obj = torch.from_numpy(golden_log[f"{inp}_obj"]).clone().requires_grad_(True)
    logw = (torch.from_numpy(golden_log[f"{inp}_logw"]).clone().requires_grad_(True)
            if with_w else None)
    sfx = "_s" if per_sample else ""
    lo, hi = (torch.from_numpy(golden_log[f"{inp}_{k}{sfx}"]) for k in ("lo", "hi"))
    if per_sample:  # at least half of the samples carry zero padding cells
        assert ((lo == 0).all(-1) & (hi == 0).all(-1)).any(-1).sum() >= lo.shape[0] // 2
    if with_w:
        assert (logw == 0).any() and (logw < 0).any()
    acq = log_qehvi_from_samples(obj, lo, hi, logw, fat, tau_relu, tau_max)
    grads = torch.autograd.grad(acq.sum(), [obj] + ([logw] if with_w else []))
    ref = torch.from_numpy(golden_log[f"{tag}_acq"])
    assert torch.isfinite(ref).all()
    torch.testing.assert_close(acq.detach(), ref, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(grads[0], torch.from_numpy(golden_log[f"{tag}_dobj"]),
                               rtol=1e-9, atol=1e-12)
    if with_w:
        torch.testing.assert_close(grads[1], torch.from_numpy(golden_log[f"{tag}_dlogw"]),
                                   rtol=1e-9, atol=1e-12)


def test_hopeless_set_is_finite_where_plain_qehvi_is_zero(golden_log):
    """Candidates centred at 0.2 below a front near 0.7: no sample clears a
    cell's lower corner (plain qEHVI exactly 0), the log value is finite with
    a finite, non-zero gradient."""
    obj = torch.from_numpy(golden_log["hopeless_obj"])
    lo, hi = (torch.from_numpy(golden_log[f"hopeless_{k}"]) for k in ("lo", "hi"))
    # the plain improvement: every (sample, point, cell) box is empty
    boxes = (torch.minimum(obj.unsqueeze(-2), hi) - lo).clamp_min(0).prod(-1)
    assert (boxes == 0).all()
    for fat in (True, False):
        tag = f"hopeless_{'fat' if fat else 'nofat'}_d_sh_u"
        acq, g = golden_log[f"{tag}_acq"], golden_log[f"{tag}_dobj"]
        assert np.isfinite(acq).all() and (acq < -10).all()
        assert np.isfinite(g).all() and (np.abs(g).max() > 0)


def test_new_safe_math_functions_match_reference(golden_log):
    """Each added function against the reference's own outputs (``fn_*`` of
    golden_logehvi.npz: a tie, a -inf entry, both temperatures), values at
    1e-12 and the minima's gradients at 1e-9."""
    from botorch_amd import safe_math as sm
    t = lambda k: torch.from_numpy(golden_log[k])  # noqa: E731
    val = dict(rtol=1e-12, atol=1e-12)
    x, y, z = t("fn_x"), t("fn_y"), t("fn_z")
    assert (x[0, 1] == x[0, 3]) and x[1, 2] == -math.inf
    for tau in (1e-1, 1e-3):
        k = f"{tau:g}"
        torch.testing.assert_close(sm.fatmin(x, dim=-1, tau=tau), t(f"fn_fatmin_{k}"), **val)
        torch.testing.assert_close(sm.smooth_amin(x, dim=-1, tau=tau), t(f"fn_smooth_amin_{k}"), **val)
        torch.testing.assert_close(sm.fatminimum(x, y, tau=tau), t(f"fn_fatminimum_{k}"), **val)
        for name in ("fatmin", "smooth_amin"):
            xf = x[2:].clone().requires_grad_(True)
            (gx,) = torch.autograd.grad(getattr(sm, name)(xf, dim=-1, tau=tau).sum(), xf)
            torch.testing.assert_close(gx, t(f"fn_{name}_{k}_grad"), rtol=1e-9, atol=1e-12)
    torch.testing.assert_close(sm.logplusexp(x, y), t("fn_logplusexp"), **val)
    torch.testing.assert_close(sm.log1mexp(z), t("fn_log1mexp"), rtol=1e-12, atol=0)
    xf, yf = x[2:], y[2:]
    torch.testing.assert_close(sm.logdiffexp(torch.minimum(xf, yf) - 0.5, torch.maximum(xf, yf)),
                               t("fn_logdiffexp"), **val)
    ninf = torch.full((3,), -math.inf, dtype=F64)
    ref = t("fn_logdiffexp_inf")
    got = sm.logdiffexp(ninf, torch.cat([ninf[:1], x[3, :2]]))
    assert got[0] == ref[0] == -math.inf
    torch.testing.assert_close(got[1:], ref[1:], rtol=0, atol=0)


def test_new_safe_math_functions():
    """Identities of the added functions (safe_math.py:72-121, 276-283,
    355-419) beside the fixtures above, which pin their composition."""
    from botorch_amd import safe_math as sm
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 5, generator=g, dtype=F64)
    y = torch.randn(6, 5, generator=g, dtype=F64)
    torch.testing.assert_close(sm.fatmin(x, dim=-1, tau=0.1), -sm.fatmax(-x, dim=-1, tau=0.1),
                               rtol=0, atol=0)
    torch.testing.assert_close(sm.smooth_amin(x, dim=-1, tau=0.1),
                               -0.1 * torch.logsumexp(-x / 0.1, dim=-1))
    torch.testing.assert_close(sm.fatminimum(x, y, tau=0.05),
                               sm.fatmin(torch.stack([x, y], -1), dim=-1, tau=0.05), rtol=0, atol=0)
    # a smooth minimum lies below the minimum, within the temperature's reach
    for f in (sm.fatmin, sm.smooth_amin):
        v = f(x, dim=-1, tau=1e-3)
        assert (v <= x.amin(-1)).all() and (x.amin(-1) - v < 1e-3 * math.log(5) + 1e-12).all()
    # a single entry is returned as it is
    torch.testing.assert_close(sm.fatmin(x[:, :1], dim=-1, tau=1e-3), x[:, 0], rtol=0, atol=0)
    torch.testing.assert_close(sm.logplusexp(x, y), torch.logaddexp(x, y))
    ninf = torch.full((3,), -math.inf, dtype=F64)
    assert (sm.logplusexp(ninf, ninf) == -math.inf).all()
    torch.testing.assert_close(sm.logplusexp(ninf, x[0, :3]), x[0, :3])
    z = -torch.logspace(-12, 2, 57, dtype=F64)
    # log(-expm1(z)) is exact to an ulp of 1 - e^z: absolutely 1.1e-16 at the far end,
    # where log1mexp itself is -e^z
    torch.testing.assert_close(sm.log1mexp(z), torch.log(-torch.expm1(z)), rtol=1e-14, atol=2.3e-16)
    torch.testing.assert_close(sm.log1mexp(z[-2:]), -torch.exp(z[-2:]), rtol=1e-14, atol=0)
    assert sm.log1mexp(torch.tensor(-math.inf, dtype=F64)).item() == 0.0
    a, b = x - 3.0, x
    torch.testing.assert_close(sm.logdiffexp(a, b), torch.log(b.exp() - a.exp()), rtol=1e-12, atol=1e-12)
    assert (sm.logdiffexp(ninf, ninf) == -math.inf).all()
    torch.testing.assert_close(sm.logdiffexp(ninf, x[0, :3]), x[0, :3], rtol=0, atol=0)
    # the infinity contract of the anchored minimum: a -inf entry makes the slice -inf
    w = torch.tensor([[0.5, -math.inf, 1.0], [0.5, 0.25, 1.0]], dtype=F64, requires_grad=True)
    v = sm.fatmin(w, dim=-1, tau=0.1)
    assert v[0].item() == -math.inf and math.isfinite(v[1].item())
    (gw,) = torch.autograd.grad(v[1], w)
    assert torch.isfinite(gw).all()


@pytest.mark.parametrize("fat", [True, False])
@pytest.mark.parametrize("q", [1, 2])
def test_known_answers_zero_samples(golden, fat, q):
    """test/acquisition/multi_objective/test_logei.py:41-144: the front
    [[4,5],[5,5],[8.5,3.5],[8.5,3],[9,1]], reference point 0 and all-zero samples
    (every MC draw the same).  Plain qEHVI is 0; the log value is finite;
    exp(value) lies in (0, tau_relu] with the fat tails and underflows to exactly
    0 without them."""
    from botorch_amd.safe_math import TAU_MAX, TAU_RELU
    for part in ("nd", "fnd"):
        lo = torch.from_numpy(golden[f"ehvi_m2_{part}_lower"])
        hi = torch.from_numpy(golden[f"ehvi_m2_{part}_upper"])
        for S in (1, 2):
            obj = torch.zeros(S, 1, q, 2, dtype=F64, requires_grad=True)
            v = log_qehvi_from_samples(obj, lo, hi, None, fat, TAU_RELU, TAU_MAX)
            assert v.shape == (1,) and math.isfinite(v.item())
            e = v.exp().item()
            if fat:
                assert 0 < e <= TAU_RELU
            else:
                assert e == 0
            (g,) = torch.autograd.grad(v.sum(), obj)
            assert torch.isfinite(g).all()
            hv = log_hvi_per_sample(obj.detach(), lo, hi, None, fat, TAU_RELU, TAU_MAX)
            assert hv.shape == (S, 1) and torch.isfinite(hv).all()


# ---- the classes' argument checks, before any device work ------------------------------
class _Member:
    num_outputs = 1

    def prediction_cache(self, *a, **k):
        raise AssertionError("device work before the argument checks")

    posterior = outcome_stats = prediction_cache


class _ModelList(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.models = [_Member() for _ in range(n)]
        self.num_outputs = n

    def posterior(self, *a, **k):
        raise AssertionError("device work before the argument checks")


class _Partitioning:
    num_outcomes = 2

    def get_hypercell_bounds(self):
        raise AssertionError("device work before the argument checks")


def _make(kind, ref_point=(0.0, 0.0), **kw):
    from botorch_amd.acquisition import (qLogExpectedHypervolumeImprovement,
                                         qLogNoisyExpectedHypervolumeImprovement)
    model = _ModelList(2)
    if kind == "qlogehvi":
        return qLogExpectedHypervolumeImprovement(model, list(ref_point), _Partitioning(), **kw)
    return qLogNoisyExpectedHypervolumeImprovement(model, list(ref_point),
                                                   torch.zeros(4, 6, dtype=F64), **kw)


def test_log_classes_are_not_nonnegative():
    from botorch_amd import acquisition as A
    from botorch_amd.optim import is_nonnegative
    for cls in (A.qLogExpectedHypervolumeImprovement, A.qLogNoisyExpectedHypervolumeImprovement):
        assert cls._log is True
        assert not is_nonnegative(object.__new__(cls))
    assert issubclass(A.qLogExpectedHypervolumeImprovement, A.qExpectedHypervolumeImprovement)
    assert issubclass(A.qLogNoisyExpectedHypervolumeImprovement,
                      A.qNoisyExpectedHypervolumeImprovement)
    assert A.qExpectedHypervolumeImprovement._log is False


def test_constructor_defaults_follow_the_reference():
    """logei.py:54-67, 327-347."""
    import inspect
    from botorch_amd import acquisition as A
    p = inspect.signature(A.qLogExpectedHypervolumeImprovement.__init__).parameters
    assert (p["eta"].default, p["fat"].default, p["tau_relu"].default, p["tau_max"].default) == (
        1e-2, True, 1e-6, 1e-2)
    p = inspect.signature(A.qLogNoisyExpectedHypervolumeImprovement.__init__).parameters
    assert (p["eta"].default, p["fat"].default, p["tau_relu"].default, p["tau_max"].default) == (
        1e-3, True, 1e-6, 1e-3)
    assert (p["prune_baseline"].default, p["alpha"].default, p["cache_pending"].default,
            p["max_iep"].default, p["incremental_nehvi"].default, p["cache_root"].default) == (
        False, 0.0, True, 0, True, True)


@pytest.mark.parametrize("kind", ["qlogehvi", "qlognehvi"])
def test_constructor_rejects_bad_ref_point_and_temperatures(kind):
    with pytest.raises(ValueError, match="(?i)reference point|ref_point"):
        _make(kind, ref_point=(0.0,) if kind == "qlognehvi" else (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="tau_max is non-positive"):
        _make(kind, tau_max=0.0)
    with pytest.raises(ValueError, match="tau_relu is non-positive"):
        _make(kind, tau_relu=-1e-6)
    with pytest.raises(ValueError, match="tau_max is not a scalar"):
        _make(kind, tau_max=torch.tensor([1e-2, 1e-3]))
