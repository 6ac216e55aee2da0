"""Generate ``golden_constrained_so.npz``: the reference's constrained
single-objective MC reductions (qEI / qLogEI with scalar ``best_f``, qNEI /
qLogNEI with one ``best_f`` per sample) on recorded samples, values and
gradients, and its linear outcome-constraint callables on their own.

Runs ONLY in the development container, where the reference tree exists (see
``_refload.py``).  The acquisition modules themselves pull in gpytorch and
cannot be imported, so ``ref_acq`` below composes the reference's own leaf
functions step by step as SampleReducingMCAcquisitionFunction does
(acquisition/monte_carlo.py:253-330; logei.py:219-234, 509-534): the outcome
constraints of ``botorch.utils.constraints``, the smoothed feasibility
indicator of ``botorch.utils.objective`` and the smooth functions of
``botorch.utils.safe_math``.

Usage:  python tests/golden/make_golden_constrained_so.py

Inputs: ``samples`` (S x b x q x Mt), ``c`` (Mt), ``bf`` (scalar), ``bf_s`` (S),
``A`` (2 x Mt), ``b`` (2 x 1), ``eta2`` (2).  Per case ``<tag>`` =
``{plain,log}_f{fat}_{sc,ps}_k{1,2}``: ``<tag>_acq`` (b) and ``<tag>_dsamples``,
the gradient of acq.sum().  k1 takes the first constraint with eta = 1e-3, k2
both with ``eta2``.  ``oc_vals`` (2 x S x b x q): the callables' outputs;
``oc_bcast`` their outputs on ``samples[0, 0]`` (q x Mt).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

S, B, Q, MT = 8, 2, 3, 3
TAU_RELU, TAU_MAX = 1e-6, 1e-2


def ref_acq(sm, objmod, samples, c, best_f, constraints, eta, log, fat):
    obj = torch.einsum("...m, m", [samples, c])                     # LinearMCObjective
    bf = best_f.reshape(-1, 1) if best_f.dim() == 1 else best_f    # sample_shape x batch
    diff = obj - bf.unsqueeze(-1)
    if log:                                                         # logei.py:509-534
        val = (sm.log_fatplus if fat else sm.log_softplus)(diff, tau=TAU_RELU)
    else:                                                           # monte_carlo.py:405-414
        val = diff.clamp_min(0)
    ind = objmod.compute_smoothed_feasibility_indicator(            # monte_carlo.py:305-330
        constraints=constraints, samples=samples, eta=eta, log=log, fat=fat)
    val = val.add(ind) if log else val.mul(ind)
    if log:                                                         # logei.py:122, 209-223
        val = (sm.fatmax if fat else sm.smooth_amax)(val, dim=-1, tau=TAU_MAX)
        return sm.logmeanexp(val, dim=0)
    return val.amax(dim=-1).mean(dim=0)


def main():
    sm = _refload.load("botorch.utils.safe_math")
    objmod = _refload.load("botorch.utils.objective")
    conmod = _refload.load("botorch.utils.constraints")
    g = torch.Generator().manual_seed(53)
    dd = dict(generator=g, dtype=torch.double)
    samples = 0.4 * torch.randn(S, B, Q, MT, **dd)
    samples[..., 1] *= 0.02           # constraint values within a few eta of the boundary
    samples[0, 0, :, 0] = -3.0        # a sample whose points all lie below best_f
    c = torch.tensor([1.0, 0.25, -0.5], dtype=torch.double)
    bf = torch.tensor(-0.1, dtype=torch.double)
    bf_s = -0.1 + 0.2 * torch.randn(S, **dd)
    A = torch.tensor([[0.0, 1.0, 0.0], [0.5, 0.0, 1.0]], dtype=torch.double)
    b = torch.tensor([[0.0], [0.3]], dtype=torch.double)
    eta2 = torch.tensor([1e-2, 0.5], dtype=torch.double)
    out = {"samples": samples.numpy(), "c": c.numpy(), "bf": bf.numpy(), "bf_s": bf_s.numpy(),
           "A": A.numpy(), "b": b.numpy(), "eta2": eta2.numpy()}
    cons = conmod.get_outcome_constraint_transforms((A, b))
    assert conmod.get_outcome_constraint_transforms(None) is None
    out["oc_vals"] = torch.stack([f(samples) for f in cons]).numpy()
    out["oc_bcast"] = torch.stack([f(samples[0, 0]) for f in cons]).numpy()
    for log in (False, True):
        for fat in (False, True):
            for ps in (False, True):
                for k in (1, 2):
                    tag = f"{'log' if log else 'plain'}_f{int(fat)}_{'ps' if ps else 'sc'}_k{k}"
                    x = samples.clone().requires_grad_(True)
                    acq = ref_acq(sm, objmod, x, c, bf_s if ps else bf, cons[:k],
                                  1e-3 if k == 1 else eta2, log, fat)
                    (gx,) = torch.autograd.grad(acq.sum(), x)
                    assert torch.isfinite(acq).all() and torch.isfinite(gx).all(), tag
                    assert gx.abs().max() > 0, tag
                    if not log:
                        assert (acq > 0).all(), tag
                    out[f"{tag}_acq"] = acq.detach().numpy()
                    out[f"{tag}_dsamples"] = gx.numpy()
    path = os.path.join(HERE, "golden_constrained_so.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
