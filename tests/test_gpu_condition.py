"""condition_on_observations on the device: the bordered cache update
(bo_gp_cache_extend) against the fp64 CPU oracle on the concatenated data and
against a full rebuild (reference: botorch/models/gpytorch.py:468-531,
models/model_list_gp_regression.py:58-129).

Inputs follow tests/test_gpu_models_widen.py::_data: d = 4, lengthscales
[0.5, 0.6, 0.7, 0.8], constant 0.2, noise 1e-2 in standardised units.  Each
(n, k, kernel) case is built once and shared by the tests below."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
LS = [0.5, 0.6, 0.7, 0.8]
CONST, NOISE, OS_MATERN = 0.2, 1e-2, 1.3
RBF, MATERN = 0, 1

# (n, k): within one padded order; across 128 -> 256 with a full MFMA tile of
# new rows; n exactly a padded order and one new row; two blocks, the second
# of one row; three blocks; many row tiles (np 1152)
CASES = [(100, 5, RBF), (120, 16, RBF), (128, 1, RBF), (300, 17, RBF), (300, 40, RBF),
         (1100, 16, RBF), (120, 16, MATERN), (300, 17, MATERN)]


def _data(n, m=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(n, 4, generator=g, dtype=F64)
    cols = [torch.sin(3 * X[:, 0] + t) + X[:, 1] * (t + 1) - X[:, 2] ** 2 for t in range(m)]
    Y = torch.stack(cols, dim=-1) + 0.05 * torch.randn(n, m, generator=g, dtype=F64)
    Yvar = 1e-3 + 0.02 * torch.rand(n, m, generator=g, dtype=F64)
    return X, Y, Yvar


def _set_hypers(m, noise=NOISE):
    getattr(m.covar_module, "base_kernel", m.covar_module).lengthscale = torch.tensor([LS], dtype=F64)
    m.mean_module.constant = CONST
    if noise is not None:
        m.likelihood.noise = torch.tensor([noise], dtype=F64)
    return m.eval()


def _model(X, Y, kind, Yvar=None, **kw):
    from botorch_amd.models import MaternKernel, ScaleKernel, SingleTaskGP
    covar = None
    if kind == MATERN:
        covar = ScaleKernel(MaternKernel(ard_num_dims=4), outputscale=OS_MATERN)
    m = SingleTaskGP(X.to(DEV), Y.to(DEV), None if Yvar is None else Yvar.to(DEV),
                     covar_module=covar, **kw)
    return _set_hypers(m, None if Yvar is not None else NOISE)


def _oracle(Xall, y_std, noise, kind, mean, std):
    """The fp64 CPU oracle on the concatenated data with the SOURCE model's
    standardisation statistics."""
    from oracle.gp import ExactGPOracle, GPHyper
    orc = ExactGPOracle(Xall, y_std, GPHyper(torch.tensor(LS, dtype=F64), noise, CONST,
                                             OS_MATERN if kind == MATERN else 1.0, kind),
                        standardize=False)
    orc.ymean, orc.ystd = mean.reshape(1, 1), std.reshape(1, 1)
    return orc


def _test_points():
    return torch.rand(5, 3, 4, generator=torch.Generator().manual_seed(3), dtype=F64)


def _check_posterior(model, orc, noise_var):
    """Case 1's tolerances: those of test_fixed_noise_posterior_matches_oracle."""
    Xc = _test_points()
    post = model.posterior(Xc.to(DEV))
    mean_ref, cov_ref = orc.posterior(Xc)
    mean, cov = post.mean.squeeze(-1).cpu(), post.distribution.covariance_matrix.cpu()
    print("posterior: max |dmean| %.3e, max |dcov| %.3e"
          % ((mean - mean_ref).abs().max(), (cov - cov_ref).abs().max()))
    torch.testing.assert_close(mean, mean_ref, rtol=1e-9, atol=1e-10)
    torch.testing.assert_close(cov, cov_ref, rtol=1e-8, atol=1e-10)
    pn = model.posterior(Xc.to(DEV), observation_noise=True)
    extra = noise_var * float(orc.ystd.squeeze()) ** 2
    torch.testing.assert_close(pn.distribution.covariance_matrix.cpu(),
                               cov_ref + extra * torch.eye(3, dtype=F64), rtol=1e-8, atol=1e-10)
    torch.testing.assert_close(pn.mean.squeeze(-1).cpu(), mean_ref, rtol=1e-9, atol=1e-10)


@functools.lru_cache(maxsize=None)
def _case(n, k, kind):
    """Source model with a built cache, its conditioned model, and the oracle."""
    X, Y, _ = _data(n + k, seed=n + k)
    src = _model(X[:n], Y[:n], kind)
    Xc = _test_points().to(DEV)
    before = src.posterior(Xc)
    before = (before.mean.clone(), before.distribution.covariance_matrix.clone())
    old = src._cache
    assert old is not None and src._cache_key == src._key()
    names = ("L", "Linv", "U", "beta", "alpha")
    old_arrays = {a: getattr(old, a).clone() for a in names}
    cond = src.condition_on_observations(X[n:].to(DEV), Y[n:].to(DEV))
    ext = cond._cache
    took_extension = ext is not None and cond._cache_key == cond._key()
    after = src.posterior(Xc)
    after = (after.mean.clone(), after.distribution.covariance_matrix.clone())
    mean = src.outcome_transform.means.cpu().reshape(())
    std = src.outcome_transform.stdvs.cpu().reshape(())
    y_std = ((Y - mean) / std).squeeze(-1)
    orc = _oracle(X, y_std, NOISE, kind, mean, std)
    return dict(X=X, Y=Y, y_std=y_std, src=src, cond=cond, ext=ext, old=old,
                old_arrays=old_arrays, before=before, after=after, orc=orc,
                took_extension=took_extension, n=n, k=k, kind=kind)


@pytest.mark.parametrize("n,k,kind", CASES)
def test_posterior_parity(n, k, kind):
    c = _case(n, k, kind)
    assert c["took_extension"], "the conditioned model's cache must come from the extension"
    cond = c["cond"]
    assert not cond.training and cond.train_inputs[0].shape == (n + k, 4)
    assert cond._cache.n == n + k and cond._cache.jitter == 0.0
    assert cond._cache is not c["old"]
    _check_posterior(cond, c["orc"], NOISE)


def _reldev(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("n,k,kind", CASES)
def test_cache_parity(n, k, kind):
    """Extension vs build_gp_cache on the concatenated data; bound: 8 x the
    rebuild's own deviation from the fp64 CPU oracle (max-abs difference over
    max-abs value, per array).  Linv' and U' over the whole np' x np' buffers."""
    from botorch_amd import kernels
    c = _case(n, k, kind)
    ext, orc, N = c["ext"], c["orc"], n + k
    assert c["took_extension"]
    reb = kernels.build_gp_cache(c["X"].to(DEV), c["y_std"].to(DEV),
                                 torch.tensor(LS, dtype=F64, device=DEV), NOISE, CONST, kind=kind,
                                 outputscale=OS_MATERN if kind == MATERN else 1.0)
    assert reb.jitter == 0.0 and ext.np == reb.np == kernels.padded_order(N)
    Linv_o = orc.LinvT.mT.contiguous()
    beta_o = Linv_o @ (c["y_std"] - CONST)
    oracle = dict(Linv=Linv_o, U=orc.LinvT, L=orc.L, beta=beta_o, alpha=orc.alpha)
    failures = []
    for name in ("Linv", "U", "L", "beta", "alpha"):
        e, r = getattr(ext, name).cpu(), getattr(reb, name).cpu()
        if name == "L":
            e, r = torch.tril(e), torch.tril(r)
        assert e.shape == r.shape
        lead = (slice(0, N), slice(0, N)) if e.dim() == 2 else (slice(0, N),)
        dev_reb = _reldev(r[lead], oracle[name])
        dev_ext = _reldev(e[lead], oracle[name])
        diff = _reldev(e, r)  # whole buffers: padding and the opposite triangle too
        print(f"n={n} k={k} kind={kind} {name}: rebuild-vs-oracle {dev_reb:.3e}, "
              f"extension-vs-oracle {dev_ext:.3e}, extension-vs-rebuild {diff:.3e}")
        if not diff <= 8 * dev_reb:
            failures.append((name, diff, dev_reb))
    assert not failures, failures
    # the padding a fresh build leaves: identity on the diagonal, zeros elsewhere
    for name in ("Linv", "U"):
        e = getattr(ext, name).cpu()
        assert torch.equal(e[N:, N:], torch.eye(ext.np - N, dtype=F64))
        assert not e[N:, :N].any() and not e[:N, N:].any()
    assert not torch.triu(ext.Linv.cpu(), 1).any() and not torch.tril(ext.U.cpu(), -1).any()
    assert torch.equal(ext.Xt_scaled.cpu(), reb.Xt_scaled.cpu())


@pytest.mark.parametrize("n,k,kind", [(100, 5, RBF), (120, 16, RBF), (300, 40, RBF)])
def test_copy_semantics(n, k, kind):
    c = _case(n, k, kind)
    ext, old = c["ext"], c["old"]
    assert torch.equal(ext.L[:n, :n], old.L[:n, :n])
    assert torch.equal(ext.Linv[:n, :n], old.Linv[:n, :n])
    assert c["src"]._cache is old
    for name, arr in c["old_arrays"].items():
        assert torch.equal(getattr(old, name), arr), name
    assert torch.equal(c["before"][0], c["after"][0])
    assert torch.equal(c["before"][1], c["after"][1])
    assert c["src"].train_inputs[0].shape == (n, 4)


def test_fixed_noise():
    n, k = 120, 16
    X, Y, Yvar = _data(n + k, seed=7)
    src = _model(X[:n], Y[:n], RBF, Yvar=Yvar[:n])
    src.posterior(_test_points().to(DEV))
    mean = src.outcome_transform.means.cpu().reshape(())
    std = src.outcome_transform.stdvs.cpu().reshape(())
    with pytest.raises(RuntimeError, match="requires a `noise` kwarg"):
        src.condition_on_observations(X[n:].to(DEV), Y[n:].to(DEV))
    nv = Yvar / std ** 2  # ``noise`` is taken as already transformed
    cond = src.condition_on_observations(X[n:].to(DEV), Y[n:].to(DEV), noise=nv[n:].to(DEV))
    assert cond._cache is not None and cond._cache_key == cond._key()
    assert cond.likelihood.noise.shape == (n + k,)
    orc = _oracle(X, ((Y - mean) / std).squeeze(-1), nv.squeeze(-1), RBF, mean, std)
    _check_posterior(cond, orc, float(nv.mean()))


def test_multi_output_and_model_list():
    from botorch_amd.models import ModelListGP, SingleTaskGP
    n, k = 100, 5
    X, Y, _ = _data(n + k, m=2, seed=9)
    multi = SingleTaskGP(X[:n].to(DEV), Y[:n].to(DEV))
    singles = [SingleTaskGP(X[:n].to(DEV), Y[:n, t:t + 1].to(DEV)) for t in range(2)]
    for t in range(2):
        for mm in (multi.models[t], singles[t]):
            mm.covar_module.lengthscale = torch.tensor([[0.4 + 0.1 * t, 0.6, 0.7, 0.9]], dtype=F64)
            mm.mean_module.constant = 0.1 * t
            mm.likelihood.noise = torch.tensor([1e-2 * (t + 1)], dtype=F64)
    multi.eval()
    lst = ModelListGP(*[s.eval() for s in singles])
    Xc = _test_points().to(DEV)
    multi.posterior(Xc), lst.posterior(Xc)  # the sources' caches
    X2, Y2 = X[n:].to(DEV), Y[n:].to(DEV)
    ref = [s.condition_on_observations(X2, Y2[:, t:t + 1]).posterior(Xc).mean[..., 0]
           for t, s in enumerate(singles)]
    cm = multi.condition_on_observations(X2, Y2)
    assert cm.num_outputs == 2 and cm.train_targets.shape == (2, n + k)
    assert all(mm._cache is not None and mm._cache_key == mm._key() for mm in cm.models)
    pm = cm.posterior(Xc).mean
    assert pm.shape == (5, 3, 2)
    cl = lst.condition_on_observations([X2, X2], Y2)
    pl = cl.posterior(Xc).mean
    for t in range(2):
        torch.testing.assert_close(pm[..., t], ref[t], rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(pl[..., t], ref[t], rtol=1e-12, atol=1e-13)
    assert multi.train_targets.shape == (2, n)


def test_twice_in_a_row():
    """(100, 5) then (105, 16) against the 21 points at once."""
    c = _case(100, 5, RBF)
    X, Y, _ = _data(16, seed=11)
    Xn = torch.cat([c["X"][100:], X]).to(DEV)
    Yn = torch.cat([c["Y"][100:], Y]).to(DEV)
    twice = c["cond"].condition_on_observations(Xn[5:], Yn[5:])
    once = c["src"].condition_on_observations(Xn, Yn)
    for mdl in (twice, once):
        assert mdl._cache is not None and mdl._cache_key == mdl._key() and mdl._cache.n == 121
    assert torch.equal(twice.train_targets, once.train_targets)
    Xc = _test_points().to(DEV)
    pt, po = twice.posterior(Xc), once.posterior(Xc)
    torch.testing.assert_close(pt.mean, po.mean, rtol=1e-9, atol=1e-10)
    torch.testing.assert_close(pt.distribution.covariance_matrix,
                               po.distribution.covariance_matrix, rtol=1e-8, atol=1e-10)
    mean = c["src"].outcome_transform.means.cpu().reshape(())
    std = c["src"].outcome_transform.stdvs.cpu().reshape(())
    Xall, Yall = torch.cat([c["X"][:100], Xn.cpu()]), torch.cat([c["Y"][:100], Yn.cpu()])
    orc = _oracle(Xall, ((Yall - mean) / std).squeeze(-1), NOISE, RBF, mean, std)
    _check_posterior(twice, orc, NOISE)


def _scratch_model(src, Xall, Yall, kind):
    """A model built from scratch on the concatenated data with the source's
    hyperparameters and standardisation statistics (its cache: a full build)."""
    s = _model(Xall, Yall, kind)
    ot = src.outcome_transform
    s.outcome_transform.means = ot.means.clone()
    s.outcome_transform.stdvs = ot.stdvs.clone()
    s.train_targets = ((Yall.to(DEV) - ot.means) / ot.stdvs).squeeze(-1)
    return s


def test_acquisition_on_conditioned_model():
    from botorch_amd.acquisition import qExpectedImprovement
    from botorch_amd.sampling import SobolQMCNormalSampler
    n, k = 300, 16
    X, Y, _ = _data(n + k, seed=13)
    src = _model(X[:n], Y[:n], RBF)
    src.posterior(_test_points().to(DEV))
    cond = src.condition_on_observations(X[n:].to(DEV), Y[n:].to(DEV))
    assert cond._cache is not None and cond._cache_key == cond._key()
    scratch = _scratch_model(src, X, Y, RBF)
    bf = float(Y.mean())
    Xq = torch.rand(8, 4, 4, generator=torch.Generator().manual_seed(2), dtype=F64)
    out = []
    for mdl in (cond, scratch):
        acqf = qExpectedImprovement(mdl, bf, sampler=SobolQMCNormalSampler(torch.Size([64]), seed=4))
        Xg = Xq.to(DEV).requires_grad_(True)
        v = acqf(Xg)
        (g,) = torch.autograd.grad(v.sum(), Xg)
        out.append((v.detach().cpu(), g.cpu()))
    assert int((out[1][0] > 0).sum()) > 0
    # the project's forward and gradient tolerances against the oracle
    torch.testing.assert_close(out[0][0], out[1][0], rtol=1e-7, atol=1e-12)
    torch.testing.assert_close(out[0][1], out[1][1], rtol=1e-5, atol=1e-8)


def test_routing_crossover_zero_takes_the_rebuild(monkeypatch):
    from botorch_amd import kernels
    c = _case(120, 16, RBF)
    monkeypatch.setattr(kernels, "EXTEND_MAX_K", 0)
    cond = c["src"].condition_on_observations(c["X"][120:].to(DEV), c["Y"][120:].to(DEV))
    assert cond._cache is None  # built lazily, as any model's
    _check_posterior(cond, c["orc"], NOISE)
    assert cond._cache is not None and cond._cache.n == 136


def test_jittered_source_cache_takes_the_rebuild():
    """The duplicated-points input of test_gpu_chol_batched.py (K + 0 I singular:
    the ladder adds jitter): the conditioned model is the full rebuild's."""
    from botorch_amd.exceptions import NumericalWarning
    from botorch_amd.models import GaussianLikelihood, RBFKernel, ScaleKernel, SingleTaskGP
    g = torch.Generator().manual_seed(3)
    X = torch.rand(300, 6, generator=g, dtype=F64)
    X[150:] = X[:150]  # duplicated points
    Y = torch.sin(X.sum(-1)).unsqueeze(-1)
    X2 = torch.rand(16, 6, generator=g, dtype=F64)
    Y2 = torch.sin(X2.sum(-1)).unsqueeze(-1)

    def build(Xa, Ya):
        m = SingleTaskGP(Xa.to(DEV), Ya.to(DEV), likelihood=GaussianLikelihood(initial=0.0),
                         covar_module=ScaleKernel(RBFKernel(ard_num_dims=6), outputscale=1.3),
                         outcome_transform=None)
        m.covar_module.base_kernel.lengthscale = torch.full((1, 6), 0.4, dtype=F64)
        m.mean_module.constant = 0.1
        return m.eval()

    Xc = torch.rand(5, 3, 6, generator=g, dtype=F64).to(DEV)
    src = build(X, Y)
    with pytest.warns(NumericalWarning):
        src.posterior(Xc)
    with pytest.warns(NumericalWarning):
        cond = src.condition_on_observations(X2.to(DEV), Y2.to(DEV))
    full = build(torch.cat([X, X2]), torch.cat([Y, Y2]))
    with pytest.warns(NumericalWarning):
        pf = full.posterior(Xc)
    from botorch_amd import kernels
    reb = kernels.build_gp_cache  # the full rebuild's jitter, read back
    with pytest.warns(NumericalWarning):
        ref_cache = reb(full.train_inputs[0], full.train_targets, torch.full((6,), 0.4, dtype=F64,
                        device=DEV), 0.0, 0.1, outputscale=1.3)
    assert cond._cache is not None and cond._cache.jitter == ref_cache.jitter > 0
    pc = cond.posterior(Xc)
    torch.testing.assert_close(pc.mean, pf.mean, rtol=1e-9, atol=1e-10)
    torch.testing.assert_close(pc.distribution.covariance_matrix,
                               pf.distribution.covariance_matrix, rtol=1e-8, atol=1e-10)
