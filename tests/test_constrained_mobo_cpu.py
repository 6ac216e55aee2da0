"""Host-side pieces of outcome constraints for qEHVI / qNEHVI (no GPU):
the outcome-selecting identity objective, the BoQehviFeasArgs record, the
box decomposition of a masked point set, and the constructors' argument
errors, which are raised before any device work."""
import ctypes

import pytest
import torch

F64 = torch.float64


# ---- IdentityMCMultiOutputObjective(outcomes=, num_outcomes=) -------------------------
def test_identity_objective_selects_outcomes():
    from botorch_amd.acquisition import IdentityMCMultiOutputObjective
    g = torch.Generator().manual_seed(0)
    samples = torch.randn(4, 3, 2, 5, generator=g, dtype=F64)
    assert IdentityMCMultiOutputObjective()(samples) is samples
    assert not hasattr(IdentityMCMultiOutputObjective(), "outcomes")
    obj = IdentityMCMultiOutputObjective(outcomes=[3, 0])
    assert torch.equal(obj(samples), samples[..., [3, 0]])
    assert obj.outcomes.dtype == torch.long and obj.outcomes.tolist() == [3, 0]
    neg = IdentityMCMultiOutputObjective(outcomes=[0, -1, -4], num_outcomes=5)
    assert neg.outcomes.tolist() == [0, 4, 1]
    assert torch.equal(neg(samples, X=None), samples[..., [0, 4, 1]])


def test_identity_objective_argument_errors():
    from botorch_amd.acquisition import IdentityMCMultiOutputObjective
    from botorch_amd.exceptions import BotorchError, BotorchTensorDimensionError
    with pytest.raises(BotorchError, match="num_outcomes is required"):
        IdentityMCMultiOutputObjective(outcomes=[0, -1])
    for bad in ([], [1]):
        with pytest.raises(BotorchTensorDimensionError, match="at least two outcomes"):
            IdentityMCMultiOutputObjective(outcomes=bad)
        with pytest.raises(ValueError):          # the reference's error is a ValueError too
            IdentityMCMultiOutputObjective(outcomes=bad)


# ---- the C record ----------------------------------------------------------------------
def test_feas_record_layout():
    from botorch_amd import _lib
    assert "BoQehviFeasArgs" in _lib.ARG_RECORDS
    rec = _lib.ARG_RECORDS["BoQehviFeasArgs"]
    lib = _lib.lib()
    assert lib.bo_struct_size(b"BoQehviFeasArgs") == ctypes.sizeof(rec)
    # the fields of BoQehviArgs first, unchanged, then the new ones
    base = _lib.ARG_RECORDS["BoQehviArgs"]
    assert rec._fields_[: len(base._fields_)] == base._fields_
    assert [f[0] for f in rec._fields_[len(base._fields_):]] == ["feas", "dfeas", "Mt", "zm", "zld",
                                                               "out_idx"]
    assert lib.bo_struct_size(b"BoQehviArgs") == ctypes.sizeof(base)
    for sym in ("bo_qehvi_feas_v", "bo_qehvi_feas_backward_v"):
        assert sym in _lib.exported_symbols()
    # header discipline: a wrong abi_version / struct_size is refused before any launch
    a = rec(B=1, q=1, m=2, S=1)
    a.abi_version = _lib.ABI_VERSION + 1
    assert lib.bo_qehvi_feas_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    a = rec(B=1, q=1, m=2, S=1)
    a.struct_size = 8
    assert lib.bo_qehvi_feas_backward_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    # argument errors likewise: no feas, a non-injective output map
    a = rec(B=1, q=1, m=2, S=1, Mt=3, zm=3, zld=3)
    assert lib.bo_qehvi_feas_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert b"feas" in lib.bo_last_error()
    dummy = torch.zeros(8, dtype=F64)
    a = rec(B=1, q=1, m=2, S=1, Mt=3, zm=3, zld=3, feas=dummy)
    a.out_idx[0] = a.out_idx[1] = 2
    assert lib.bo_qehvi_feas_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert b"injective" in lib.bo_last_error()


# ---- masked point sets decompose as the filtered ones -------------------------------------
@pytest.mark.parametrize("fill", ["ref", "-inf"])
@pytest.mark.parametrize("m", [2, 3])
def test_masked_rows_give_the_cells_of_the_filtered_set(m, fill):
    """qNEHVI with constraints decomposes every sample's FEASIBLE baseline
    points (hypervolume.py:749-751).  bo_nd_partition_host keeps only the points
    strictly above the reference point, so the batched call on the full S x n x m
    array with the infeasible rows overwritten (reference point, or -inf)
    returns, cell for cell, what the call on each sample's filtered rows
    returns, padded with empty cells to the common count."""
    from botorch_amd import kernels
    S, n = 6, 12
    g = torch.Generator().manual_seed(10 + m)
    Y = torch.rand(S, n, m, generator=g, dtype=F64) + 0.05
    ref = torch.full((m,), 0.1, dtype=F64)
    feas = torch.rand(S, n, generator=g) < 0.6
    feas[2] = False                       # a sample with no feasible point at all
    feas[4] = True
    assert feas.any(dim=1).sum() == S - 1 and not feas.all()
    masked = Y.clone()
    masked[~feas] = ref if fill == "ref" else torch.full((m,), float("-inf"), dtype=F64)
    lo, hi = kernels.nd_partition_host(masked, ref)
    K = lo.shape[1]
    counts = []
    for s in range(S):
        rows = Y[s][feas[s]]
        if rows.shape[0] == 0:
            # test_monte_carlo.py:976-994: no point above ref -> the one cell [ref, inf)
            lo_s, hi_s = ref.view(1, m), torch.full((1, m), float("inf"), dtype=F64)
        else:
            lo_s, hi_s = kernels.nd_partition_host(rows, ref)
        k = lo_s.shape[0]
        counts.append(k)
        assert k <= K
        assert torch.equal(lo[s, :k], lo_s) and torch.equal(hi[s, :k], hi_s), f"sample {s}"
        assert (lo[s, k:] == 0).all() and (hi[s, k:] == 0).all(), f"sample {s}: padding"
    assert max(counts) == K and min(counts) == 1 and len(set(counts)) > 1


# ---- constructor errors, before any device work ----------------------------------------
class _Member:
    """A model-list member whose every device-facing call fails the test."""

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


def _make(kind, **kw):
    from botorch_amd.acquisition import (qExpectedHypervolumeImprovement,
                                         qNoisyExpectedHypervolumeImprovement)
    model = _ModelList(3)
    if kind == "qehvi":
        return qExpectedHypervolumeImprovement(model, [0.0, 0.0], _Partitioning(), **kw)
    return qNoisyExpectedHypervolumeImprovement(model, [0.0, 0.0], torch.zeros(4, 6, dtype=F64), **kw)


@pytest.mark.parametrize("kind", ["qehvi", "qnehvi"])
def test_constructor_errors_precede_device_work(kind):
    from botorch_amd.acquisition import IdentityMCMultiOutputObjective
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.objective import MCObjective
    obj = IdentityMCMultiOutputObjective(outcomes=[0, 1])
    con = [lambda Z: Z[..., -1]]
    with pytest.raises(ValueError, match="do not match"):
        _make(kind, objective=obj, constraints=con, eta=torch.tensor([1e-3, 1e-2]))
    with pytest.raises(ValueError, match="do not match"):
        _make(kind, objective=obj, constraints=con * 2, eta=torch.tensor([1e-3]))
    for eta in (0.0, -1e-3, torch.tensor([-1.0])):
        with pytest.raises(ValueError, match="positive"):
            _make(kind, objective=obj, constraints=con, eta=eta)

    class Other(MCObjective):
        def forward(self, samples, X=None):
            return samples[..., :2] * 2.0

    with pytest.raises(UnsupportedError, match="constraints"):
        _make(kind, objective=Other(), constraints=con)
    # the reference point counts the objective's outcomes, not the members
    with pytest.raises(ValueError, match="reference point"):
        _make(kind, objective=IdentityMCMultiOutputObjective(outcomes=[0, 1, 2]), constraints=con)
