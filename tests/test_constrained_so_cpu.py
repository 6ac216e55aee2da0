"""The constrained single-objective reductions without a GPU: the torch
restatement the GPU tests use as their reference (tests/
constrained_so_restatement.py) against the reference's recorded outputs
(golden_constrained_so.npz, made by tests/golden/make_golden_constrained_so.py),
``get_outcome_constraint_transforms`` and the recogniser of its callables, and
the argument checks of the kernel wrappers, which run before any device work.

Bars: values rtol / atol 1e-12, gradients w.r.t. the samples rtol 1e-9 / atol
1e-12 (the bars of test_logehvi_golden.py)."""
import os
from functools import partial

import numpy as np
import pytest
import torch

from botorch_amd import kernels
from botorch_amd.objective import (_linear_outcome_constraints, _oc,
                                   get_outcome_constraint_transforms)

from .constrained_so_restatement import constrained_acq_from_samples

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_constrained_so.npz"))


def _t(name):
    return torch.from_numpy(GOLD[name])


def _constraints():
    return get_outcome_constraint_transforms((_t("A"), _t("b")))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("ps", [False, True])
@pytest.mark.parametrize("fat", [False, True])
@pytest.mark.parametrize("log", [False, True])
def test_restatement_matches_reference(log, fat, ps, k):
    tag = f"{'log' if log else 'plain'}_f{int(fat)}_{'ps' if ps else 'sc'}_k{k}"
    x = _t("samples").clone().requires_grad_(True)
    eta = 1e-3 if k == 1 else _t("eta2")       # a float, or one entry per constraint
    acq = constrained_acq_from_samples(x, _t("c"), _t("bf_s") if ps else _t("bf"),
                                       _constraints()[:k], eta, log=log, fat=fat)
    (gx,) = torch.autograd.grad(acq.sum(), x)
    torch.testing.assert_close(acq.detach(), _t(f"{tag}_acq"), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gx, _t(f"{tag}_dsamples"), rtol=1e-9, atol=1e-12)
    assert gx.abs().max() > 0


def test_outcome_constraint_transforms_match_reference():
    cons = _constraints()
    assert len(cons) == 2
    vals = torch.stack([f(_t("samples")) for f in cons])
    torch.testing.assert_close(vals, _t("oc_vals"), rtol=1e-12, atol=1e-12)
    # broadcasting: q x Mt in, q out
    one = torch.stack([f(_t("samples")[0, 0]) for f in cons])
    assert one.shape == (2, _t("samples").shape[2])
    torch.testing.assert_close(one, _t("oc_bcast"), rtol=1e-12, atol=1e-12)


def test_outcome_constraint_transforms_none():
    assert get_outcome_constraint_transforms(None) is None


def test_recogniser():
    A, b = _t("A"), _t("b")
    cons = get_outcome_constraint_transforms((A, b))
    got = _linear_outcome_constraints(cons)
    assert got is not None
    assert got[0] == A.tolist() and got[1] == b.reshape(-1).tolist()
    assert _linear_outcome_constraints(cons[:1]) == ([A[0].tolist()], [float(b[0])])

    def lam(Y):
        return Y[..., 1]

    assert _linear_outcome_constraints([lam]) is None
    assert _linear_outcome_constraints([cons[0], lam]) is None            # mixed
    assert _linear_outcome_constraints([partial(_oc, A[0])]) is None       # rhs unbound
    assert _linear_outcome_constraints([partial(torch.mul, A[0], b[0])]) is None
    assert _linear_outcome_constraints(None) is None
    assert _linear_outcome_constraints([]) is None


def _roots(Mt=2, B=3, q=2, S=5):
    g = torch.Generator().manual_seed(0)
    return (torch.randn(Mt, B, q, generator=g, dtype=torch.double),
            torch.randn(Mt, B, q, q, generator=g, dtype=torch.double).tril(),
            torch.randn(S, q * Mt, generator=g, dtype=torch.double))


@pytest.mark.parametrize("kw,match", [
    (dict(Mt=9), "Mt <= 8"),
    (dict(q=17), "q <= 16"),
    (dict(k=9), "at most 8"),
    (dict(c_len=3), "one objective weight per member"),
    (dict(eta=0.0), "eta must be positive"),
    (dict(both=True), "not both"),
    (dict(feas_shape=(5, 3, 3)), "feas must be S x B x q"),
    (dict(bfs=4), "one value per sample"),
])
def test_wrapper_argument_checks(kw, match):
    Mt, q = kw.get("Mt", 2), kw.get("q", 2)
    mean, L, Z = _roots(Mt=Mt, q=q)
    k = kw.get("k", 1)
    args = dict(c=[1.0] * kw.get("c_len", Mt), A=[[1.0] * Mt] * k, rhs=[0.0] * k,
                eta=[kw.get("eta", 1e-3)] * k)
    if kw.get("both"):
        args["feas"] = torch.ones(5, 3, q, dtype=torch.double)
    if "feas_shape" in kw:
        args.update(A=None, rhs=None, eta=None, feas=torch.ones(kw["feas_shape"], dtype=torch.double))
    if "bfs" in kw:
        args["best_f_s"] = torch.zeros(kw["bfs"], dtype=torch.double)
    with pytest.raises(ValueError, match=match):
        kernels.qmc_feas(mean, L, Z, **args)
    with pytest.raises(ValueError, match=match):
        kernels.qmc_feas_backward(mean, L, Z, dacq=torch.ones(3, dtype=torch.double), **args)


def test_backward_needs_forward_value_in_log_mode():
    mean, L, Z = _roots()
    with pytest.raises(ValueError, match="forward's acq"):
        kernels.qmc_feas_backward(mean, L, Z, [1.0, 0.0], torch.ones(3, dtype=torch.double),
                                  log=True)


@pytest.mark.parametrize("Mt", [1, 2])
def test_callable_constraint_weights_keep_their_graph(Mt):
    """_feas_weights inside an autograd Function's forward (grad mode off around
    it): the weights stay a differentiable function of the leaves -- for one
    member they come out non-contiguous, and a copy made outside the enabled
    grad mode dropped the graph (and with it the constraint path's gradient)."""
    from botorch_amd import acquisition as A
    B, q, S = 4, 3, 6
    plan = A._WeightedSOPlan([None] * Mt, [1.0] * Mt, [lambda Z: Z[..., -1]], None, False)
    plan.set_eta(0.05)
    g = torch.Generator().manual_seed(Mt)
    mean = torch.randn(Mt, B, q, generator=g, dtype=torch.double)
    L = torch.randn(Mt, B, q, q, generator=g, dtype=torch.double)
    Z = torch.randn(S, q * Mt, generator=g, dtype=torch.double)
    with torch.no_grad():
        w, leaves = A._feas_weights(plan, mean, L, Z, None, 0, True)
    assert w.requires_grad and w.is_contiguous()
    dm, dl = torch.autograd.grad(w.sum(), leaves)
    assert dm.abs().max() > 0 and dl.abs().max() > 0
