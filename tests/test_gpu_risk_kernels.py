"""bo_qmc_risk and bo_qmc_risk_backward against the restatement."""
import ctypes

import pytest
import torch

from tests import risk_restatement as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# 10 x the largest disagreement of the restatement's two forms over CASES, as
# max |x - y| / max |y| (measured: 1.49e-15 on acq, 1.88e-14 on dmean, 3.34e-14 on dL; the
# kernel's largest errors against form 0 are in DESIGN.md section 29)
ACQ_TOL, DMEAN_TOL, DL_TOL = 1.49e-14, 1.88e-13, 3.34e-13


def _err(got, want):
    return float((got.cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("q,n_w,k,S,B,kind,mode,fat", ref.CASES)
def test_value_and_gradients(q, n_w, k, S, B, kind, mode, fat):
    from botorch_amd import kernels
    from botorch_amd.safe_math import TAU_MAX, TAU_RELU
    mean, L, Z = ref.make_inputs(q, n_w, S, B)
    best_f, margin = ref.well_separated(mean, L, Z, q, n_w, k, kind, mode)
    assert margin > 1e-6  # no selection can flip at rounding: a condition on the inputs
    dacq = torch.linspace(0.5, 1.5, B, dtype=torch.float64)
    want = ref.value_and_grads(mean, L, Z, q, n_w, k, kind, mode, best_f, fat, dacq)
    args = (q, n_w, k, kind, mode, best_f, fat, TAU_RELU, TAU_MAX)
    m, l, z = mean.to(DEV), L.to(DEV), Z.to(DEV)
    acq = kernels.qmc_risk(m, l, z, *args)
    dmean, dL = kernels.qmc_risk_backward(dacq.to(DEV), acq, m, l, z, *args)
    errs = [_err(g, w) for g, w in zip((acq, dmean, dL), want)]
    print("errors (acq, dmean, dL):", errs)
    assert errs[0] <= ACQ_TOL and errs[1] <= DMEAN_TOL and errs[2] <= DL_TOL
    assert torch.equal(dL, dL.tril())
    # a second call, and every row alone, to the bit
    assert torch.equal(acq, kernels.qmc_risk(m, l, z, *args))
    again = kernels.qmc_risk_backward(dacq.to(DEV), acq, m, l, z, *args)
    assert torch.equal(dmean, again[0]) and torch.equal(dL, again[1])
    for b in range(B if B > 1 else 0):
        one = kernels.qmc_risk(m[b:b + 1], l[b:b + 1], z, *args)
        assert torch.equal(one, acq[b:b + 1])
        g = kernels.qmc_risk_backward(dacq[b:b + 1].to(DEV), one, m[b:b + 1], l[b:b + 1], z, *args)
        assert torch.equal(g[0], dmean[b:b + 1]) and torch.equal(g[1], dL[b:b + 1])


@pytest.mark.parametrize("entry", ["bo_qmc_risk", "bo_qmc_risk_backward"])
@pytest.mark.parametrize("how", ["Q129", "n_w1", "abi", "size"])
def test_refusals(entry, how):
    from botorch_amd import _lib
    q, n_w = {"Q129": (3, 43), "n_w1": (4, 1)}.get(how, (2, 4))
    Q = q * n_w
    t = torch.zeros(Q * Q + 8, dtype=torch.float64, device=DEV)
    a = _lib.QmcRiskArgs(q=q, n_w=n_w, k=1, kind=0, mode=_lib.QMC_QSR, fat=1, B=1, S=1, mean=t, L=t,
                         Z=t, tau_relu=1.0, tau_max=1.0, acq=t, dacq=t, dmean=t, dL=t)
    if how == "abi":
        a.abi_version += 1
    if how == "size":
        a.struct_size -= 8
    lib = _lib.lib()
    assert getattr(lib, entry)(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert lib.bo_last_error().decode().startswith(entry + ":")
