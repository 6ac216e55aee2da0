"""qBayesianActiveLearningByDisagreement without a GPU: the ABI record and
symbols, the ABI's refusals, the fake shapes of the ops, the two forms of the
restatement (tests/bald_restatement.py) against each other and against known
answers, the generic route's torch formula on host tensors (values and dX)
against the restatement, MultivariateNormal.log_prob, the mixture moments and
quantiles of GaussianMixturePosterior, the constructor errors, pending points
and the output shape."""
import ctypes
import math

import pytest
import torch

from tests import bald_restatement as br

F64 = torch.float64


def test_bald_record_and_symbols():
    from botorch_amd import _lib, ops
    lib = _lib.lib()
    assert "BoBaldArgs" in _lib.ARG_RECORDS
    assert lib.bo_struct_size(b"BoBaldArgs") == ctypes.sizeof(_lib.BaldArgs)
    for sym in ("bo_bald_v", "bo_bald_backward_v"):
        assert sym in _lib.exported_symbols()
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert "bald" in ops.OPS and "bald_backward" in ops.OPS
    assert lib.bo_version() == _lib.ABI_VERSION == 12  # a pure addition


def test_bald_abi_refusals():
    """Header discipline and argument errors, refused before any launch."""
    from botorch_amd import _lib
    lib = _lib.lib()
    a = _lib.BaldArgs(M=2, q=1, S=1, B=1)
    a.abi_version = _lib.ABI_VERSION + 1
    assert lib.bo_bald_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    assert "ABI" in lib.bo_last_error().decode()
    a = _lib.BaldArgs(M=2, q=1, S=1, B=1)
    a.struct_size -= 8
    assert lib.bo_bald_backward_v(ctypes.byref(a), None) == _lib.BO_ERR_ARG
    dummy = torch.zeros(64, dtype=F64)
    ok = dict(M=2, q=2, S=3, B=2, mean=dummy, L=dummy, Z=dummy, out=dummy, dout=dummy,
              dmean=dummy, dL=dummy, work=dummy, work_size=64)
    bads = [(dict(M=0), "M <= 64"), (dict(M=65), "M <= 64"), (dict(q=0), "q <= 16"),
            (dict(q=17), "q <= 16"), (dict(S=0), "1 <= S"), (dict(S=(1 << 20) + 1), "1 <= S"),
            (dict(B=0), "B >= 1"), (dict(B=-1), "B >= 1"), (dict(B=1 << 30), "B M < 2^31"),
            (dict(work=None), "work of at least"), (dict(work_size=3), "work of at least")]
    bads += [({name: None}, "mean, L and Z are required") for name in ("mean", "L", "Z")]
    for bad, text in bads:
        for fn in (lib.bo_bald_v, lib.bo_bald_backward_v):
            assert fn(ctypes.byref(_lib.BaldArgs(**{**ok, **bad})), None) == _lib.BO_ERR_ARG, bad
            assert text in lib.bo_last_error().decode(), (bad, lib.bo_last_error())
    # the backward's scratch holds the per-sample log-sum-exp: B M S doubles
    assert lib.bo_bald_backward_v(ctypes.byref(_lib.BaldArgs(**{**ok, "work_size": 11})),
                                  None) == _lib.BO_ERR_ARG
    assert "at least 12 doubles" in lib.bo_last_error().decode()
    assert lib.bo_bald_v(ctypes.byref(_lib.BaldArgs(**{**ok, "out": None})),
                         None) == _lib.BO_ERR_ARG
    assert "out is required" in lib.bo_last_error().decode()
    for name in ("dout", "dmean", "dL"):
        assert lib.bo_bald_backward_v(ctypes.byref(_lib.BaldArgs(**{**ok, name: None})),
                                      None) == _lib.BO_ERR_ARG
        assert "dout, dmean and dL are required" in lib.bo_last_error().decode()


def test_bald_wrapper_limits():
    """kernels.bald_check names the limit it refuses, on the host."""
    from botorch_amd import kernels
    for args, text in (((65, 2, 8), "M <= 64"), ((0, 2, 8), "M <= 64"), ((4, 17, 8), "q <= 16"),
                       ((4, 0, 8), "q <= 16"), ((4, 2, 0), "1 <= S"), ((4, 2, 8, -1), "B >= 0")):
        with pytest.raises(ValueError, match=text):
            kernels.bald_check(*args)
    kernels.bald_check(64, 16, 4096, 0)


def test_bald_op_fake_shapes():
    meta = dict(device="meta", dtype=F64)
    B, M, q, S = 7, 5, 3, 19
    e = lambda *s: torch.empty(*s, **meta)  # noqa: E731
    args = (e(M * B, q), e(M * B, q, q), e(S, q), M)
    assert torch.ops.bo.bald(*args).shape == (B, M)
    dmean, dL = torch.ops.bo.bald_backward(e(B, M), *args)
    assert dmean.shape == (M * B, q) and dL.shape == (M * B, q, q)


def _members(case, standardize=False):
    from oracle.acquisition import saas_members
    X, Y, smp, Xc, Z = br.problem(*case, standardize=standardize)
    return saas_members(X, Y, smp, standardize=standardize), Xc, Z


@pytest.mark.parametrize("case", br.CASES)
def test_restatement_forms_agree(case):
    members, Xc, Z = _members(case)
    a, b = br.bald_members(members, Xc, Z, "exp"), br.bald_members(members, Xc, Z, "lse")
    print(f"{case}: exp form vs log-sum-exp form, largest difference {(a - b).abs().max():.3e}")
    assert torch.isfinite(a).all() and (a - b).abs().max() <= 1e-14


def _random_mixture(B, M, q, seed=0):
    g = torch.Generator().manual_seed(seed)
    mean = torch.randn(B, M, q, generator=g, dtype=F64)
    A = torch.randn(B, M, q, q, generator=g, dtype=F64)
    return mean, A @ A.mT + torch.eye(q, dtype=F64), g


def test_known_answers():
    """M = 1 is exactly 0; identical components give 0; q = 1 components with
    unit variance and means 40 apart never overlap, so the mutual information is
    log M; through both forms where the exp form is finite."""
    mean, cov, g = _random_mixture(3, 1, 4)
    Z = torch.randn(32, 4, generator=g, dtype=F64)
    assert br.bald(mean, cov, Z, "lse").abs().max() == 0.0
    assert br.bald(mean, cov, Z, "exp").abs().max() < 4e-15  # (log(exp(l)) rounds)
    mean, cov, _ = _random_mixture(2, 1, 3, seed=1)
    Z = torch.randn(16, 3, generator=g, dtype=F64)
    for form in ("exp", "lse"):
        v = br.bald(mean.expand(2, 5, 3), cov.expand(2, 5, 3, 3), Z, form)
        assert v.abs().max() < 1e-13
    for M in (2, 3, 5):
        mean = 40.0 * torch.arange(M, dtype=F64).view(1, M, 1)
        cov = torch.ones(1, M, 1, 1, dtype=F64)
        Z = torch.randn(64, 1, generator=g, dtype=F64)
        for form in ("exp", "lse"):
            got = br.bald(mean, cov, Z, form).item()
            print(f"M = {M} ({form}): {got:.16e} against log M = {math.log(M):.16e}")
            assert abs(got - math.log(M)) < 4e-15


@pytest.mark.parametrize("standardize", [False, True])
@pytest.mark.parametrize("case", br.CASES)
def test_generic_formula_on_host_tensors(case, standardize):
    """The torch formula of ``_generic`` on host tensors (the members' moments at
    X with the noise on the diagonal, torch's Cholesky, y = mu + L z) against the
    restatement: values and dX."""
    from botorch_amd.acquisition import _bald_value
    members, Xc, Z = _members(case, standardize)
    Xa = Xc.clone().requires_grad_(True)
    mean, cov = br.member_moments(members, Xa)
    L = torch.linalg.cholesky(cov)
    y = mean.unsqueeze(0) + torch.einsum("bmij,sj->sbmi", L, Z)
    got = _bald_value(mean, L, y).mean(-1)
    (ga,) = torch.autograd.grad(got.sum(), Xa)
    Xb = Xc.clone().requires_grad_(True)
    ref = br.bald_members(members, Xb, Z)
    (gb,) = torch.autograd.grad(ref.sum(), Xb)
    print(f"{case} standardize={standardize}: value err {(got - ref).abs().max():.3e} "
          f"(max |ref| {ref.abs().max():.3e}), dX err {(ga - gb).abs().max():.3e} "
          f"(max |dX| {gb.abs().max():.3e})")
    assert gb.abs().max() > 1e-6
    torch.testing.assert_close(got.detach(), ref.detach(), rtol=1e-7, atol=1e-8)
    torch.testing.assert_close(ga, gb, rtol=1e-5, atol=1e-8)


def test_mvn_log_prob_matches_torch():
    from botorch_amd.posteriors import MultivariateNormal
    mean, cov, g = _random_mixture(3, 4, 5, seed=2)
    mvn = MultivariateNormal(mean, cov)
    mvn._scale_tril = torch.linalg.cholesky(cov)  # (the property's ladder is a device kernel)
    ref = torch.distributions.MultivariateNormal(mean, covariance_matrix=cov)
    for shape in ((3, 4, 5), (5,), (7, 3, 4, 5), (4, 6, 3, 1, 5)):
        v = torch.randn(*shape, generator=g, dtype=F64)
        got, want = mvn.log_prob(v), ref.log_prob(v)
        assert got.shape == want.shape
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def _mixture_posterior(B, M, q, seed=3):
    from botorch_amd.posteriors import GaussianMixturePosterior, MultivariateNormal
    mean, cov, _ = _random_mixture(B, M, q, seed=seed)
    return GaussianMixturePosterior(MultivariateNormal(mean, cov)), mean, cov


def test_mixture_moments():
    post, mean, cov = _mixture_posterior(3, 4, 5)
    assert post.batch_range == (0, -1)
    assert post.mean.shape == (3, 4, 5, 1)
    torch.testing.assert_close(post.mixture_mean, mean.mean(1).unsqueeze(-1), rtol=0, atol=1e-15)
    var = cov.diagonal(dim1=-2, dim2=-1)
    want = var.mean(1) + (mean ** 2).mean(1) - mean.mean(1) ** 2
    torch.testing.assert_close(post.mixture_variance, want.unsqueeze(-1), rtol=1e-13, atol=1e-14)
    dev = mean - mean.mean(1, keepdim=True)
    want = cov.mean(1) + torch.einsum("bmi,bmj->bij", dev, dev) / 4
    torch.testing.assert_close(post.mixture_covariance_matrix, want, rtol=1e-13, atol=1e-14)
    # the covariance's diagonal is the variance
    torch.testing.assert_close(post.mixture_covariance_matrix.diagonal(dim1=-2, dim2=-1),
                               post.mixture_variance.squeeze(-1), rtol=1e-12, atol=1e-13)


def test_mixture_quantile():
    post, mean, cov = _mixture_posterior(3, 4, 5)
    sd = cov.diagonal(dim1=-2, dim2=-1).sqrt()
    normal = torch.distributions.Normal(mean, sd)
    for level in (0.05, 0.5, 0.9):
        x = post.quantile(torch.tensor(level, dtype=F64))
        assert x.shape == (3, 5, 1)
        cdf = normal.cdf(x.squeeze(-1).unsqueeze(1)).mean(1)   # the mixture cdf at the quantile
        assert (cdf - level).abs().max() <= 1e-6
    both = post.quantile(torch.tensor([0.25, 0.75], dtype=F64))
    assert both.shape == (2, 3, 5, 1) and (both[0] < both[1]).all()
    # one component: the normal quantile itself
    post1, mean1, cov1 = _mixture_posterior(2, 1, 3, seed=4)
    sd1 = cov1.diagonal(dim1=-2, dim2=-1).sqrt()
    want = torch.distributions.Normal(mean1, sd1).icdf(torch.tensor(0.3, dtype=F64))
    got = post1.quantile(torch.tensor(0.3, dtype=F64))
    assert got.shape == (2, 3, 1)
    torch.testing.assert_close(got.squeeze(-1), want.squeeze(1), rtol=1e-14, atol=1e-14)
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"range \(0, 1\)"):
            post.quantile(torch.tensor(bad, dtype=F64))


def test_batched_bisect_refuses_a_target_outside_the_bounds():
    from botorch_amd.posteriors import batched_bisect
    bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=F64)
    with pytest.raises(ValueError, match="not contained in the interval"):
        batched_bisect(lambda x: x, 2.0, bounds)
    x = batched_bisect(lambda x: x ** 3, 0.3, bounds)
    assert (x ** 3 - 0.3).abs().max() <= 1e-6


class _Fitted:
    """A stand-in for a fitted ensemble model on the host: M fixed Gaussians per
    t-batch whose means move with X (so that pending points show)."""

    _is_fully_bayesian = True
    _is_ensemble = True
    training = False
    num_mcmc_samples = 3

    def posterior(self, X, observation_noise=False, posterior_transform=None):
        from botorch_amd.posteriors import GaussianMixturePosterior, MultivariateNormal
        assert observation_noise is True
        q = X.shape[-2]
        scale = torch.arange(1, 4, dtype=F64).view(3, 1)
        mean = X.sum(-1).unsqueeze(-2) * scale                        # ... x M x q
        cov = (torch.eye(q, dtype=F64) * scale.view(3, 1, 1) + 0.1).expand(*mean.shape, q)
        mvn = MultivariateNormal(mean, cov)
        mvn._scale_tril = torch.linalg.cholesky(cov)
        return GaussianMixturePosterior(mvn)


class _HostSampler:
    """Base samples S x q shared by every component and t-batch, on the host."""

    sample_shape = torch.Size([16])

    def __call__(self, post):
        mean, L = post.distribution.loc, post.distribution.scale_tril
        Z = torch.randn(16, mean.shape[-1], generator=torch.Generator().manual_seed(5), dtype=F64)
        return (mean + torch.einsum("...ij,sj->s...i", L, Z)).unsqueeze(-1)


def test_constructor_errors():
    from botorch_amd.acquisition import (FullyBayesianAcquisitionFunction,
                                         qBayesianActiveLearningByDisagreement)
    from botorch_amd.models import SaasFullyBayesianSingleTaskGP

    class Plain:
        _is_fully_bayesian = False

    for cls in (FullyBayesianAcquisitionFunction, qBayesianActiveLearningByDisagreement):
        with pytest.raises(ValueError, match="Fully Bayesian acquisition functions require "
                                             "a SaasFullyBayesianSingleTaskGP to run."):
            cls(Plain())
    unfitted = SaasFullyBayesianSingleTaskGP(torch.rand(5, 2, dtype=F64),
                                             torch.rand(5, 1, dtype=F64))
    with pytest.raises(RuntimeError, match="Model has not been fitted"):
        qBayesianActiveLearningByDisagreement(unfitted)
    acqf = qBayesianActiveLearningByDisagreement(_Fitted())
    assert acqf.sample_shape == torch.Size([512]) and acqf.posterior_transform is None


def test_pending_points_and_shapes_on_host():
    """Host input takes ``_generic``: pending points join every t-batch, extra
    batch dimensions come back, and the exports resolve."""
    import botorch_amd
    from botorch_amd.acquisition import qBayesianActiveLearningByDisagreement as BALD
    assert botorch_amd.qBayesianActiveLearningByDisagreement is BALD
    assert botorch_amd.GaussianMixturePosterior.__name__ == "GaussianMixturePosterior"
    assert issubclass(BALD, botorch_amd.FullyBayesianAcquisitionFunction)
    g = torch.Generator().manual_seed(6)
    X = torch.rand(2, 3, 2, 4, generator=g, dtype=F64)
    Xp = torch.rand(2, 4, generator=g, dtype=F64)
    acqf = BALD(_Fitted(), sampler=_HostSampler())
    v = acqf(X)
    assert v.shape == (2, 3) and torch.isfinite(v).all()
    torch.testing.assert_close(acqf(X[1, 2]), v[1, 2].reshape(1), rtol=1e-13, atol=1e-14)
    pend = BALD(_Fitted(), sampler=_HostSampler(), X_pending=Xp)
    joined = torch.cat([X, Xp.expand(2, 3, 2, 4)], dim=-2)
    torch.testing.assert_close(pend(X), acqf(joined), rtol=0, atol=0)
    assert (pend(X) - v).abs().min() > 1e-6
    pend.set_X_pending(None)
    torch.testing.assert_close(pend(X), v, rtol=0, atol=0)
    assert acqf(torch.empty(0, 2, 4, dtype=F64)).shape == (0,)
    # the value through the restatement from the same moments
    post = _Fitted().posterior(X.reshape(-1, 2, 4), observation_noise=True)
    Z = torch.randn(16, 2, generator=torch.Generator().manual_seed(5), dtype=F64)
    ref = br.bald(post.distribution.loc, post.distribution.covariance_matrix, Z)
    torch.testing.assert_close(v.reshape(-1), ref, rtol=1e-7, atol=1e-8)
