"""The analytic family without a GPU: the ABI record and its refusals, the
restatement (tests/analytic_restatement.py) and the package's safe_math functions
against the reference's own outputs and the 80-digit truth
(tests/golden/golden_analytic.npz), the classes on a CPU model against the
formulae written out by hand, and their validation."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import analytic_restatement as ar

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_analytic.npz")


@pytest.fixture(scope="module")
def G():
    return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


# ---- ABI ------------------------------------------------------------------------------------
def test_analytic_record_symbols_and_ops():
    from botorch_amd import _lib, kernels, ops
    lib = _lib.lib()
    assert _lib.ARG_RECORDS["BoAnalyticArgs"] is _lib.AnalyticArgs
    assert lib.bo_struct_size(b"BoAnalyticArgs") == ctypes.sizeof(_lib.AnalyticArgs)
    for sym in ("bo_analytic_v", "bo_analytic_backward_v"):
        assert sym in _lib.exported_symbols() and hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert "analytic" in ops.OPS and "analytic_backward" in ops.OPS
    assert lib.bo_version() == _lib.ABI_VERSION == 12  # a pure addition
    assert kernels.AN_CMAX == _lib.AN_CMAX == 15 and kernels.AN_MT_MAX == 16
    assert (kernels.AN_LOG_EI, kernels.AN_EI, kernels.AN_LOG_PI, kernels.AN_PI, kernels.AN_UCB,
            kernels.AN_STD) == (ar.LOG_EI, ar.EI, ar.LOG_PI, ar.PI, ar.UCB, ar.STD)
    assert (kernels.AN_CON_LOWER, kernels.AN_CON_UPPER, kernels.AN_CON_BOTH) == (0, 1, 2)


def test_analytic_abi_refusals():
    """Header discipline and argument errors, refused before any launch (no
    device is touched: the pointers are host memory that nothing reads)."""
    from botorch_amd import _lib
    lib = _lib.lib()
    d = torch.zeros(64, dtype=F64)
    a = _lib.AnalyticArgs()
    a.abi_version = _lib.ABI_VERSION + 1
    assert lib.bo_analytic_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG

    def args(ncon=1, member=1, kind=2, lower=0.0, upper=1.0, **kw):
        base = dict(mode=0, Mt=2, obj=0, ncon=ncon, best_f_stride=0, R=4, mean=d, var=d, best_f=d,
                    w=1.0, beta=0.0, min_var=1e-12, acq=d, dacq=d, dmean=d, dvar=d)
        base.update(kw)
        rec = _lib.AnalyticArgs(**base)
        for c in range(min(ncon, 16)):
            rec.con_member[c], rec.con_kind[c] = (member, kind) if c == 0 else (c + 1, 0)
            rec.con_lower[c], rec.con_upper[c] = lower, upper
        return rec

    bads = [(dict(Mt=17), "1 <= Mt"), (dict(Mt=0), "1 <= Mt"), (dict(mode=6), "mode"),
            (dict(mode=-1), "mode"), (dict(ncon=16, Mt=16), "ncon"), (dict(member=0), "objective"),
            (dict(member=2), "member < Mt"), (dict(upper=0.0), "upper > lower"),
            (dict(kind=3), "kind"), (dict(min_var=0.0), "min_var"), (dict(w=0.5), "+1 or -1"),
            (dict(beta=-1.0), "beta"), (dict(best_f_stride=2), "best_f_stride"),
            (dict(obj=2), "obj"), (dict(R=-1), "R"), (dict(mean=None), "required"),
            (dict(var=None), "required"), (dict(best_f=None), "best_f"),
            (dict(ncon=2, Mt=3, member=2), "more than one")]
    for bad, text in bads:
        for fn in (lib.bo_analytic_v, lib.bo_analytic_backward_v):
            assert fn(ctypes.byref(args(**bad)), None) == _lib.BO_ERR_ARG, bad
            assert text in lib.bo_last_error().decode(), (bad, lib.bo_last_error())
    assert lib.bo_analytic_v(ctypes.byref(args(acq=None)), None) == _lib.BO_ERR_ARG
    for name in ("dacq", "dmean", "dvar"):
        assert lib.bo_analytic_backward_v(ctypes.byref(args(**{name: None})),
                                          None) == _lib.BO_ERR_ARG
    # R = 0 returns at once, before any pointer is looked at
    for fn in (lib.bo_analytic_v, lib.bo_analytic_backward_v):
        assert fn(ctypes.byref(args(R=0, mean=None, var=None, acq=None, dacq=None)),
                  None) == _lib.BO_OK


def test_analytic_op_fake_shapes():
    from botorch_amd import ops  # noqa: F401
    e = lambda *s: torch.empty(*s, device="meta", dtype=F64)  # noqa: E731
    Mt, R = 3, 37
    args = (e(Mt, R), e(Mt, R), e(R), ar.LOG_EI, 0, 1.0, 0.0, 1e-12, [1, 2], [0.0, 0.0],
            [1.0, 0.0], [ar.BOTH, ar.LOWER])
    assert torch.ops.bo.analytic(*args).shape == (R,)
    assert [t.shape for t in torch.ops.bo.analytic_backward(e(R), *args)] == [(Mt, R), (Mt, R)]
    args = (e(1, R), e(1, R), None, ar.STD, 0, -1.0, 0.0, 1e-12, [], [], [], [])
    assert torch.ops.bo.analytic(*args).shape == (R,)


def test_wrapper_checks_before_native(monkeypatch):
    from botorch_amd import _lib, kernels

    def boom(*a, **k):
        raise AssertionError("the native library was touched")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(kernels, "lib", boom)
    kernels.analytic_check(16, ar.LOG_EI, 3, [(j, 0.0, 1.0, ar.BOTH) for j in range(16) if j != 3])
    for kw, text in [(dict(Mt=17, mode=0), "Mt"), (dict(Mt=2, mode=6), "mode"),
                     (dict(Mt=2, mode=0, min_var=0.0), "min_var"),
                     (dict(Mt=2, mode=0, constraints=[(0, 0.0, 1.0, 2)]), "objective"),
                     (dict(Mt=2, mode=0, constraints=[(1, 1.0, 1.0, 2)]), "upper > lower"),
                     (dict(Mt=16, mode=0, constraints=[(1, 0.0, 0.0, 0)] * 16), "at most 15"),
                     (dict(Mt=3, mode=0, constraints=[(1, 0.0, 0.0, 0)] * 2), "more than one"),
                     (dict(Mt=2, mode=0, w=0.0), r"\+1 or -1")]:
        with pytest.raises(ValueError, match=text):
            kernels.analytic_check(**kw)


# ---- the leaf functions against the golden columns -------------------------------------------
def _value_and_grad(f, *xs):
    xs = [x.clone().requires_grad_(True) for x in xs]
    y = f(*xs)
    return y.detach(), torch.autograd.grad(y.sum(), xs)


def _impls():
    from botorch_amd import safe_math as sm
    return [("restatement", ar.log_ei, ar.log_ndtr, ar.log_prob_normal_in),
            ("safe_math", sm.log_ei_helper, sm.log_ndtr, sm.log_prob_normal_in)]


@pytest.mark.parametrize("which", [0, 1])
def test_leaf_functions_match_the_reference(G, which):
    """Values at rtol 1e-12, atol 1e-12 (the project's golden bound); gradients
    at rtol 1e-9, atol 1e-12: the same composition, so the same rounding."""
    name, log_ei, log_ndtr, log_prob_normal_in = _impls()[which]
    cases = [("log_ei", log_ei, (G["lei_u"],), G["lei_ref"], (G["lei_ref_grad"],)),
             ("log_ndtr", log_ndtr, (G["lnd_x"],), G["lnd_ref"], (G["lnd_ref_grad"],)),
             ("log_prob_normal_in", log_prob_normal_in, (G["lpn_ab"][:, 0], G["lpn_ab"][:, 1]),
              G["lpn_ref"], (G["lpn_ref_da"], G["lpn_ref_db"]))]
    for fname, f, xs, want, want_grads in cases:
        got, grads = _value_and_grad(f, *xs)
        assert torch.isfinite(got).all(), (name, fname)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12, msg=f"{name} {fname}")
        for g, wg in zip(grads, want_grads):
            assert torch.isfinite(g).all(), (name, fname)
            torch.testing.assert_close(g, wg, rtol=1e-9, atol=1e-12, msg=f"{name} {fname} grad")


def test_restatement_values_against_the_truth(G):
    """Within 64 x the reference's worst recorded value error (relative to
    max(1, |truth|)): the restatement is the reference's composition, on this
    host's libm."""
    lim = 64 * max(G["lei_ref_err"].max().item(), G["lnd_ref_err"].max().item())
    for f, xs, truth in [(ar.log_ei, (G["lei_u"],), G["lei_true"]),
                         (ar.log_ndtr, (G["lnd_x"],), G["lnd_true"])]:
        err = ((f(*xs) - truth).abs() / truth.abs().clamp_min(1.0)).max().item()
        print(f"{f.__name__}: {err:.3e} (limit {lim:.3e})")
        assert err <= lim
    ab, truth = G["lpn_ab"], G["lpn_true"]
    err = (ar.log_prob_normal_in(ab[:, 0], ab[:, 1]) - truth).abs() / truth.abs().clamp_min(1.0)
    plim = 64 * G["lpn_ref_err"].max().item()
    assert err.max().item() <= plim, (err, plim)


def test_other_safe_math_functions():
    from botorch_amd import safe_math as sm
    x = torch.tensor([-1e100, -1e8, -40.0, -3.0, 0.0, 0.5, 4.0, 30.0], dtype=F64,
                     requires_grad=True)
    for f in (sm.log_phi, sm.log_ndtr, sm.log_erfc, sm.log_erfcx, sm.standard_normal_log_hazard):
        y = f(x)
        (g,) = torch.autograd.grad(y.sum(), x)
        assert torch.isfinite(y).all() and torch.isfinite(g).all(), f.__name__
    assert sm.log_Phi is sm.log_ndtr
    mid = torch.tensor([-3.0, 0.0, 0.5, 4.0], dtype=F64)
    torch.testing.assert_close(sm.log_erfc(mid), torch.erfc(mid).log(), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(sm.log_erfcx(mid), torch.special.erfcx(mid).log(), rtol=1e-12,
                               atol=1e-13)
    torch.testing.assert_close(sm.standard_normal_log_hazard(mid),
                               (sm.phi(mid) / sm.ndtr(-mid)).log(), rtol=1e-12, atol=1e-13)
    with pytest.raises(TypeError, match="log_Phi only supports"):
        sm.log_ndtr(torch.zeros(2, dtype=torch.float16))
    with pytest.raises(TypeError, match="LogExpectedImprovement only supports"):
        sm.log_ei_helper(torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="not all a < b"):
        sm.log_prob_normal_in(torch.ones(2, dtype=F64), torch.ones(2, dtype=F64))


def test_restatement_modes_and_constraints_by_hand():
    """The six modes and the three constraint kinds against the naive formulae,
    where those are accurate (|u| of order 1)."""
    g = torch.Generator().manual_seed(3)
    Mt, R = 4, 9
    mean = torch.randn(Mt, R, generator=g, dtype=F64)
    var = 0.2 + torch.rand(Mt, R, generator=g, dtype=F64)
    bf = 0.3 * torch.randn(R, generator=g, dtype=F64)
    cons = [(0, -1.0, 0.0, ar.LOWER), (3, 0.0, 1.5, ar.UPPER), (2, -1.5, 1.0, ar.BOTH)]
    sg = var.sqrt()
    feas = (1 - ar.Phi((-1.0 - mean[0]) / sg[0])) * ar.Phi((1.5 - mean[3]) / sg[3]) * (
        ar.Phi((1.0 - mean[2]) / sg[2]) - ar.Phi((-1.5 - mean[2]) / sg[2]))
    for w in (1.0, -1.0):
        u = w * (mean[1] - bf) / sg[1]
        ei = sg[1] * (ar.phi(u) + u * ar.Phi(u))
        want = {ar.LOG_EI: (ei * feas).log(), ar.EI: ei * feas, ar.LOG_PI: (ar.Phi(u) * feas).log(),
                ar.PI: ar.Phi(u) * feas, ar.UCB: (w * mean[1] + math.sqrt(0.7) * sg[1]) * feas,
                ar.STD: w * sg[1] * feas}
        for mode, val in want.items():
            got = ar.analytic(mean, var, bf, mode, obj=1, w=w, beta=0.7, constraints=cons)
            torch.testing.assert_close(got, val, rtol=1e-11, atol=1e-13, msg=f"mode {mode} w {w}")


# ---- the classes on a CPU model ----------------------------------------------------------------
class _Posterior:
    def __init__(self, mean, variance):
        self.mean, self.variance = mean, variance


class _TorchGP:
    """An exact RBF GP with m independent outputs in plain torch (n = 12, d = 2).
    The noise keeps sigma above 0.2, so |u| stays below 10 on the unit square and
    the naive formulae the classes are compared with are accurate there."""

    def __init__(self, m=1, n=12, d=2):
        g = torch.Generator().manual_seed(11 + m)
        self.X = torch.rand(n, d, generator=g, dtype=F64)
        self.Y = torch.stack([1.4 * (3.0 * self.X.sum(-1) + t).sin() for t in range(m)], dim=-1)
        self.ls, self.noise = 0.3, 0.05
        self.num_outputs = m
        K = self._k(self.X, self.X) + self.noise * torch.eye(n, dtype=F64)
        self.Kinv = torch.linalg.inv(K)

    def _k(self, A, B):
        return torch.exp(-0.5 * torch.cdist(A / self.ls, B / self.ls).square())

    def posterior(self, X, posterior_transform=None, **kw):
        assert posterior_transform is None
        X = X.to(F64)
        Ks = self._k(X, self.X)                                       # ... x q x n
        mean = Ks @ (self.Kinv @ self.Y)                              # ... x q x m
        var = 1.0 - ((Ks @ self.Kinv) * Ks).sum(-1, keepdim=True)
        return _Posterior(mean, var.expand(mean.shape))


def _moments(model, X):
    p = model.posterior(X)
    mean = p.mean.squeeze(-2)
    return mean, p.variance.squeeze(-2).clamp_min(1e-12).sqrt()


def _Xs():
    g = torch.Generator().manual_seed(5)
    return [torch.rand(7, 1, 2, generator=g, dtype=F64), torch.rand(3, 2, 1, 2, generator=g, dtype=F64)]


@pytest.mark.parametrize("maximize", [True, False])
def test_single_output_classes_by_hand(maximize):
    from botorch_amd.acquisition import (LogExpectedImprovement, LogProbabilityOfImprovement,
                                         PosteriorStandardDeviation, ScalarizedPosteriorMean)
    model = _TorchGP()
    w = 1.0 if maximize else -1.0
    for X in _Xs():
        batch = X.shape[:-2]
        mean, sigma = _moments(model, X)
        mean, sigma = mean.squeeze(-1), sigma.squeeze(-1)
        for best_f in (0.4, 0.4 + 0.1 * torch.arange(batch[-1], dtype=F64)):
            u = w * (mean - best_f) / sigma
            lei = LogExpectedImprovement(model, best_f, maximize=maximize)(X)
            lpi = LogProbabilityOfImprovement(model, best_f, maximize=maximize)(X)
            assert lei.shape == lpi.shape == batch
            torch.testing.assert_close(lei, (sigma * (ar.phi(u) + u * ar.Phi(u))).log(),
                                       rtol=1e-10, atol=1e-12)
            torch.testing.assert_close(lpi, ar.Phi(u).log(), rtol=1e-10, atol=1e-12)
        std = PosteriorStandardDeviation(model, maximize=maximize)(X)
        torch.testing.assert_close(std, w * sigma, rtol=1e-13, atol=0)
    X = torch.rand(4, 3, 2, dtype=F64)
    wts = torch.tensor([0.5, -1.0, 2.0], dtype=F64)
    spm = ScalarizedPosteriorMean(model, wts)(X)
    torch.testing.assert_close(spm, model.posterior(X).mean.squeeze(-1) @ wts, rtol=1e-13, atol=0)
    # float32 X: computed in fp64, returned in X's dtype
    X32 = _Xs()[0].to(torch.float32)
    acqf = LogExpectedImprovement(model, 0.4, maximize=maximize)
    out = acqf(X32)
    assert out.dtype == torch.float32
    torch.testing.assert_close(out, acqf(X32.to(F64)).to(torch.float32), rtol=0, atol=0)
    assert acqf._log and LogProbabilityOfImprovement._log
    assert acqf.best_f.dtype == F64 and "best_f" in dict(acqf.named_buffers())


@pytest.mark.parametrize("maximize", [True, False])
def test_constrained_classes_by_hand(maximize):
    from botorch_amd.acquisition import (ConstrainedExpectedImprovement,
                                         LogConstrainedExpectedImprovement)
    model = _TorchGP(m=3)
    w = 1.0 if maximize else -1.0
    for constraints in ({0: (-0.5, None)}, {2: (None, 0.8)}, {0: (-1.0, 1.2)},
                        {0: (-0.5, None), 2: (-1.0, 0.9)}):
        for X in _Xs():
            mean, sigma = _moments(model, X)
            best_f = 0.2 + 0.05 * torch.arange(X.shape[-3], dtype=F64)
            u = w * (mean[..., 1] - best_f) / sigma[..., 1]
            cei_hand = sigma[..., 1] * (ar.phi(u) + u * ar.Phi(u))
            for k, (lo, hi) in constraints.items():
                p_hi = 1.0 if hi is None else ar.Phi((hi - mean[..., k]) / sigma[..., k])
                p_lo = 0.0 if lo is None else ar.Phi((lo - mean[..., k]) / sigma[..., k])
                cei_hand = cei_hand * (p_hi - p_lo)
            cei = ConstrainedExpectedImprovement(model, best_f, 1, constraints, maximize)(X)
            lcei = LogConstrainedExpectedImprovement(model, best_f, 1, constraints, maximize)(X)
            assert cei.shape == lcei.shape == X.shape[:-2]
            torch.testing.assert_close(cei, cei_hand, rtol=1e-10, atol=1e-14)
            torch.testing.assert_close(lcei, cei_hand.log(), rtol=1e-10, atol=1e-11)
    acqf = LogConstrainedExpectedImprovement(model, 0.1, 1, {0: (-0.5, None), 2: (-1.0, 0.9)})
    assert acqf._log and not ConstrainedExpectedImprovement._log
    assert acqf.con_lower_inds.tolist() == [0] and acqf.con_both_inds.tolist() == [2]
    assert acqf.con_lower.tolist() == [-0.5] and acqf.con_both.tolist() == [[-1.0, 0.9]]
    assert acqf._an_members() == [1, 0, 2]
    assert acqf._an_constraints() == [(1, -0.5, 0.0, ar.LOWER), (2, -1.0, 0.9, ar.BOTH)]
    assert acqf.posterior_transform is None and acqf.objective_index == 1


def test_validation():
    import botorch_amd
    from botorch_amd import acquisition as A
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.optim import is_nonnegative
    model, model3 = _TorchGP(), _TorchGP(m=3)
    for cls in (A.LogConstrainedExpectedImprovement, A.ConstrainedExpectedImprovement):
        with pytest.raises(ValueError, match="There must be at least one constraint."):
            cls(model3, 0.0, 1, {})
        with pytest.raises(ValueError,
                           match="Output corresponding to objective should not be a constraint."):
            cls(model3, 0.0, 1, {1: (0.0, None)})
        with pytest.raises(ValueError, match="Upper bound is less than the lower bound."):
            cls(model3, 0.0, 1, {0: (1.0, 1.0)})
    acqfs = [A.LogExpectedImprovement(model, 0.0), A.LogProbabilityOfImprovement(model, 0.0),
             A.PosteriorStandardDeviation(model),
             A.LogConstrainedExpectedImprovement(model3, 0.0, 1, {0: (0.0, None)}),
             A.ConstrainedExpectedImprovement(model3, 0.0, 1, {0: (0.0, None)}),
             A.ScalarizedPosteriorMean(model, torch.ones(1, dtype=F64))]
    assert [is_nonnegative(a) for a in acqfs] == [False, False, False, False, True, False]
    for a in acqfs:
        with pytest.raises(UnsupportedError, match="do not account for X_pending"):
            a.set_X_pending(torch.rand(1, 2, dtype=F64))
        assert a.X_pending is None
    for a in acqfs[:5]:
        assert a._route is None and not a._fused_applies(torch.rand(3, 1, 2, dtype=F64))
        with pytest.raises(AssertionError, match="q=1"):
            a(torch.rand(3, 2, 2, dtype=F64))
        a._route = "fused"  # no quiet fall-back: the fused route on a foreign model is an error
        with pytest.raises(UnsupportedError, match="exact GP"):
            a(torch.rand(3, 1, 2, dtype=F64))
    for cls in (A.LogExpectedImprovement, A.LogProbabilityOfImprovement):
        with pytest.raises(UnsupportedError, match="Must specify a posterior transform"):
            cls(model3, 0.0)
    with pytest.raises(UnsupportedError, match="Must specify a posterior transform"):
        A.PosteriorStandardDeviation(model3)
    for name in ("LogExpectedImprovement", "LogProbabilityOfImprovement",
                 "LogConstrainedExpectedImprovement", "ConstrainedExpectedImprovement",
                 "PosteriorStandardDeviation", "ScalarizedPosteriorMean"):
        assert name in botorch_amd.__all__ and getattr(botorch_amd, name) is getattr(A, name)


def test_log_ei_where_ei_vanishes():
    """Ten length-scales from the data with best_f = max(Y) + 50 sigma_y: EI is
    exactly 0 with a zero gradient, LogEI finite with a finite non-zero one."""
    from botorch_amd.acquisition import ExpectedImprovement, LogExpectedImprovement
    model = _TorchGP()
    best_f = (model.Y.max() + 50.0 * model.Y.std()).item()
    X = (model.X.max(0).values + 10.0 * model.ls).reshape(1, 1, 2).requires_grad_(True)
    ei = ExpectedImprovement(model, best_f)(X)
    (g,) = torch.autograd.grad(ei.sum(), X)
    assert ei.item() == 0.0 and not g.any()
    lei = LogExpectedImprovement(model, best_f)(X)
    (g,) = torch.autograd.grad(lei.sum(), X)
    assert math.isfinite(lei.item()) and lei.item() < -700.0
    assert torch.isfinite(g).all() and g.abs().min().item() > 0.0
