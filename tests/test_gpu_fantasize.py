"""SingleTaskGP.fantasize / FantasizedGP.posterior on the device: against the
product's own condition_on_observations, against CPU autograd through the
oracle and the restatement (tests/fantasy_restatement.py), against
qKnowledgeGradient, both routes, the variants, and acquisition functions put on
a fantasy model.

n = 40, d = 3 (d = 10 for the generic route), Standardize on (mean != 0, std !=
1), one seed.  Bars (the project's product-against-oracle bars): values rtol
1e-6 / atol 1e-8; gradients and the generic route rtol 1e-5 / atol 1e-8.  The
fused tests make ``_generic`` raise, so a silent fall-back fails."""
import functools

import pytest
import torch

from tests.fantasy_restatement import fantasy_moments

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
VAL = dict(rtol=1e-6, atol=1e-8)
GRAD = dict(rtol=1e-5, atol=1e-8)
GENERIC = dict(rtol=1e-5, atol=1e-8)
SEED = 5
N, LS, NOISE, CONST = 40, 0.4, 1e-2, 0.1


# ---- data, model, reference -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(d=3, fixed=False, standardize=True):
    """(X, Y, Yvar or None, oracle) on the CPU."""
    from oracle.gp import ExactGPOracle, GPHyper, standardize_fit
    g = torch.Generator().manual_seed(11)
    X = torch.rand(N, d, generator=g, dtype=F64)
    Y = 3.0 + 2.0 * torch.sin(3 * X.sum(-1, keepdim=True)) + 0.1 * torch.randn(N, 1, generator=g, dtype=F64)
    ymean, ystd = standardize_fit(Y) if standardize else (torch.zeros(1), torch.ones(1))
    Yvar, noise = None, NOISE
    if fixed:
        Yvar = (0.5 + torch.rand(N, 1, generator=g, dtype=F64)) * 2e-2 * ystd.item() ** 2
        noise = (Yvar / ystd.item() ** 2).squeeze(-1)
    orc = ExactGPOracle(X, Y, GPHyper(torch.full((d,), LS, dtype=F64), noise, CONST),
                        standardize=standardize)
    if standardize:
        assert abs(float(orc.ymean)) > 1 and abs(float(orc.ystd) - 1) > 0.1
    return X, Y, Yvar, orc


@functools.lru_cache(maxsize=None)
def _model(d=3, fixed=False, standardize=True):
    from botorch_amd.models import SingleTaskGP
    X, Y, Yvar, _ = _data(d, fixed, standardize)
    kw = {} if standardize else dict(outcome_transform=None)
    m = SingleTaskGP(X.to(DEV), Y.to(DEV), None if Yvar is None else Yvar.to(DEV), **kw)
    m.covar_module.lengthscale = torch.full((1, d), LS, dtype=F64)
    if not fixed:
        m.likelihood.noise = torch.tensor([NOISE], dtype=F64)
    m.mean_module.constant = CONST
    return m.eval()


def _sampler(N_f):
    from botorch_amd.sampling import SobolQMCNormalSampler
    return SobolQMCNormalSampler(torch.Size([N_f]), seed=SEED)


def _base_samples(q_a, N_f):
    from oracle.sampling import draw_sobol_normal_samples
    return draw_sobol_normal_samples(q_a, N_f, SEED)


def _outcome_noise(orc, q_a, noise_tf=None):
    """s'^2 per fantasised row in outcome space."""
    s2 = float(orc.ystd) ** 2
    if noise_tf is not None:
        return noise_tf.reshape(-1).expand(q_a) * s2
    n = orc.h.noise
    return torch.full((q_a,), float(n.mean() if torch.is_tensor(n) else n) * s2, dtype=F64)


def oracle_moments(orc, X, Xp, N_f, noise_tf=None):
    """(mean N_f x b x q, cov F x b x q x q) of the fantasy models by the oracle
    and the restatement; X b x q_a x d, Xp b x q x d (shared) or N_f x b x q x d."""
    b, q_a, d = X.shape
    groups = Xp.unsqueeze(1) if Xp.dim() == 3 else Xp.transpose(0, 1)       # b x F x q x d
    joint = torch.cat([X.unsqueeze(1).expand(b, groups.shape[1], q_a, d), groups], dim=-2)
    mean, cov = orc.posterior(joint)
    m, c = fantasy_moments(mean, cov, _base_samples(q_a, N_f), _outcome_noise(orc, q_a, noise_tf), q_a)
    return m.transpose(0, 1), c.transpose(0, 1)


def _points(b, q_a, q, N_f, d=3, shared=False):
    g = torch.Generator().manual_seed(b * 1000 + q_a * 100 + q * 10 + N_f)
    X = torch.rand(b, q_a, d, generator=g, dtype=F64)
    Xp = torch.rand(*(() if shared else (N_f,)), b, q, d, generator=g, dtype=F64)
    return X, Xp


@functools.lru_cache(maxsize=None)
def reference(b, q_a, q, N_f, d=3, shared=False, fixed=False, standardize=True):
    """(X, Xp, c1, c2, mean, cov, dX, dXp) of the oracle restatement, computed
    once and shared: the gradients are those of (mean c1).sum() + (cov c2).sum()."""
    orc = _data(d, fixed, standardize)[3]
    X, Xp = _points(b, q_a, q, N_f, d, shared)
    g = torch.Generator().manual_seed(3)
    c1 = torch.randn(N_f, b, q, generator=g, dtype=F64)
    c2 = torch.randn(N_f, b, q, q, generator=g, dtype=F64)
    Xo, Xpo = X.clone().requires_grad_(True), Xp.clone().requires_grad_(True)
    mean, cov = oracle_moments(orc, Xo, Xpo, N_f)
    loss = (mean * c1).sum() + (cov.expand(N_f, b, q, q) * c2).sum()
    gX, gXp = torch.autograd.grad(loss, (Xo, Xpo))
    assert gX.abs().max() > 1e-6 and gXp.abs().max() > 1e-6
    return X, Xp, c1, c2, mean.detach(), cov.detach().expand(N_f, b, q, q), gX, gXp


def _no_generic(monkeypatch):
    from botorch_amd.models import FantasizedGP

    def boom(self, *a):
        raise AssertionError("the generic route was taken")
    monkeypatch.setattr(FantasizedGP, "_generic", boom)


def _no_fused(monkeypatch):
    from botorch_amd.models import FantasizedGP

    def boom(self, *a):
        raise AssertionError("the fused route was taken")
    monkeypatch.setattr(FantasizedGP, "_fused", boom)


def _moments_and_grads(model, X, Xp, N_f, c1, c2, **kw):
    Xd, Xpd = X.to(DEV).requires_grad_(True), Xp.to(DEV).requires_grad_(True)
    fm = model.fantasize(Xd, _sampler(N_f), **kw)
    post = fm.posterior(Xpd)
    mean, cov = post.mean, post.covariance_matrix
    loss = (mean.squeeze(-1) * c1.to(DEV)).sum() + (cov * c2.to(DEV)).sum()
    gX, gXp = torch.autograd.grad(loss, (Xd, Xpd))
    return mean.detach().cpu(), cov.detach().cpu(), gX.cpu(), gXp.cpu()


# ---- against the product's own conditioning --------------------------------------------
@pytest.mark.parametrize("shared", [True, False])
def test_against_condition_on_observations(shared, monkeypatch):
    """b = 2, q_a = 2, q = 3, N_f = 3: every fantasy model's posterior equals the
    posterior of model.condition_on_observations(X[b], Y_f[b]), one fantasy and
    one t-batch at a time, with Y_f = mu(X) + L z_f read from fm.train_targets."""
    _no_generic(monkeypatch)
    b, q_a, q, N_f = 2, 2, 3, 3
    model = _model()
    model.posterior(torch.rand(1, 3, dtype=F64, device=DEV))  # a valid cache: the bordered update
    X, Xp = _points(b, q_a, q, N_f, shared=shared)
    X, Xp = X.to(DEV), Xp.to(DEV)
    fm = model.fantasize(X, _sampler(N_f))
    assert fm.batch_shape == torch.Size([N_f, b])
    ymean, ystd = model.outcome_stats()
    tt = fm.train_targets
    assert tt.shape == (N_f, b, N + q_a) and fm.train_inputs[0].shape == (N_f, b, N + q_a, 3)
    assert torch.equal(tt[1, 1, :N], model.train_targets)
    Yf = tt[..., N:] * ystd + ymean
    with torch.no_grad():
        post = fm.posterior(Xp)
    assert post.mean.shape == (N_f, b, q, 1) and post.covariance_matrix.shape == (N_f, b, q, q)
    if shared:  # the covariance does not depend on the fantasy: an expanded view
        assert post.covariance_matrix.stride(0) == 0
    for f in range(N_f):
        for i in range(b):
            cm = model.condition_on_observations(X[i], Yf[f, i].unsqueeze(-1))
            with torch.no_grad():
                ref = cm.posterior(Xp[i] if shared else Xp[f, i])
            torch.testing.assert_close(post.mean[f, i], ref.mean, **VAL)
            torch.testing.assert_close(post.covariance_matrix[f, i], ref.covariance_matrix, **VAL)


# ---- against the oracle: values and gradients ---------------------------------------------
@pytest.mark.parametrize("b, q_a, q, N_f, shared",
                         [(2, 2, 3, 3, False), (2, 2, 3, 3, True), (1, 8, 4, 3, False),
                          (2, 5, 11, 2, False)])
def test_fused_values_and_gradients(b, q_a, q, N_f, shared, monkeypatch):
    _no_generic(monkeypatch)
    X, Xp, c1, c2, m_ref, c_ref, gX_ref, gXp_ref = reference(b, q_a, q, N_f, shared=shared)
    mean, cov, gX, gXp = _moments_and_grads(_model(), X, Xp, N_f, c1, c2)
    assert mean.shape == (N_f, b, q, 1) and cov.shape == (N_f, b, q, q)
    torch.testing.assert_close(mean.squeeze(-1), m_ref, **VAL)
    torch.testing.assert_close(cov, c_ref, **VAL)
    torch.testing.assert_close(gX, gX_ref, **GRAD)
    torch.testing.assert_close(gXp, gXp_ref, **GRAD)


@pytest.mark.parametrize("b, q_a, q, N_f, d, shared",
                         [(2, 9, 8, 3, 3, False), (2, 2, 3, 3, 10, False), (2, 2, 3, 3, 10, True)])
def test_generic_route(b, q_a, q, N_f, d, shared, monkeypatch):
    _no_fused(monkeypatch)
    X, Xp, c1, c2, m_ref, c_ref, gX_ref, gXp_ref = reference(b, q_a, q, N_f, d, shared)
    mean, cov, gX, gXp = _moments_and_grads(_model(d), X, Xp, N_f, c1, c2)
    torch.testing.assert_close(mean.squeeze(-1), m_ref, **GENERIC)
    torch.testing.assert_close(cov, c_ref, **GENERIC)
    torch.testing.assert_close(gX, gX_ref, **GENERIC)
    torch.testing.assert_close(gXp, gXp_ref, **GENERIC)


def test_fused_and_generic_routes_agree(monkeypatch):
    from botorch_amd.models import FantasizedGP
    b, q_a, q, N_f = 2, 2, 3, 3
    X, Xp, c1, c2, *_ = reference(b, q_a, q, N_f)
    fused = _moments_and_grads(_model(), X, Xp, N_f, c1, c2)
    monkeypatch.setattr(FantasizedGP, "FUSED_ROWS", 0)
    _no_fused(monkeypatch)
    generic = _moments_and_grads(_model(), X, Xp, N_f, c1, c2)
    for a, g in zip(fused, generic):
        torch.testing.assert_close(a, g, **GENERIC)


# ---- against existing code --------------------------------------------------------------
@pytest.mark.parametrize("b, q_a, N_f", [(3, 2, 5), (2, 4, 13)])
def test_equals_knowledge_gradient(b, q_a, N_f, monkeypatch):
    """q = 1: the mean over the fantasies of the fantasy models' posterior mean
    at one point each is qKnowledgeGradient's value, and the gradients agree."""
    from botorch_amd.acquisition import qKnowledgeGradient
    _no_generic(monkeypatch)
    model = _model()
    X_full = torch.rand(b, q_a + N_f, 3, generator=torch.Generator().manual_seed(b), dtype=F64)
    Xk = X_full.to(DEV).requires_grad_(True)
    kg = qKnowledgeGradient(model, num_fantasies=N_f, sampler=_sampler(N_f))(Xk)
    (g_kg,) = torch.autograd.grad(kg.sum(), Xk)
    Xd = X_full.to(DEV).requires_grad_(True)
    fm = model.fantasize(Xd[:, :q_a], _sampler(N_f))
    X_fantasies = Xd[:, q_a:].permute(1, 0, 2)              # N_f x b x d, as the reference splits
    val = fm.posterior(X_fantasies.unsqueeze(-2)).mean.mean(0).reshape(b)
    (g_fm,) = torch.autograd.grad(val.sum(), Xd)
    torch.testing.assert_close(val.detach(), kg.detach(), **VAL)
    torch.testing.assert_close(g_fm, g_kg, **GRAD)


# ---- variants ---------------------------------------------------------------------------
def test_fixed_noise_model(monkeypatch):
    _no_generic(monkeypatch)
    X, Xp, c1, c2, m_ref, c_ref, gX_ref, gXp_ref = reference(2, 2, 3, 3, fixed=True)
    mean, cov, gX, gXp = _moments_and_grads(_model(fixed=True), X, Xp, 3, c1, c2)
    torch.testing.assert_close(mean.squeeze(-1), m_ref, **VAL)
    torch.testing.assert_close(cov, c_ref, **VAL)
    torch.testing.assert_close(gX, gX_ref, **GRAD)
    torch.testing.assert_close(gXp, gXp_ref, **GRAD)


def test_standardize_off(monkeypatch):
    _no_generic(monkeypatch)
    X, Xp, c1, c2, m_ref, c_ref, gX_ref, gXp_ref = reference(2, 2, 3, 3, standardize=False)
    mean, cov, gX, gXp = _moments_and_grads(_model(standardize=False), X, Xp, 3, c1, c2)
    torch.testing.assert_close(mean.squeeze(-1), m_ref, **VAL)
    torch.testing.assert_close(cov, c_ref, **VAL)
    torch.testing.assert_close(gX, gX_ref, **GRAD)


@pytest.mark.parametrize("rows", [1, 2])
def test_observation_noise_tensor(rows, monkeypatch):
    """A 1 x 1 or q_a x 1 noise in the standardised space, per fantasised row."""
    _no_generic(monkeypatch)
    b, q_a, q, N_f = 2, 2, 3, 3
    orc = _data()[3]
    X, Xp = _points(b, q_a, q, N_f)
    noise_tf = torch.tensor([[5e-3], [8e-2]], dtype=F64)[:rows]
    m_ref, c_ref = oracle_moments(orc, X, Xp, N_f, noise_tf)
    fm = _model().fantasize(X.to(DEV), _sampler(N_f), observation_noise=noise_tf.to(DEV))
    with torch.no_grad():
        post = fm.posterior(Xp.to(DEV))
    torch.testing.assert_close(post.mean.squeeze(-1).cpu(), m_ref, **VAL)
    torch.testing.assert_close(post.covariance_matrix.cpu(), c_ref, **VAL)
    assert (m_ref - oracle_moments(orc, X, Xp, N_f)[0]).abs().max() > 1e-4  # the noise matters


def test_fp32_inputs_compute_in_fp64(monkeypatch):
    _no_generic(monkeypatch)
    b, q_a, q, N_f = 2, 2, 3, 3
    X, Xp = _points(b, q_a, q, N_f)
    X32, Xp32 = X.float(), Xp.float()
    m_ref, c_ref = oracle_moments(_data()[3], X32.double(), Xp32.double(), N_f)
    Xd = X32.to(DEV).requires_grad_(True)
    post = _model().fantasize(Xd, _sampler(N_f)).posterior(Xp32.to(DEV))
    assert post.mean.dtype == F64
    torch.testing.assert_close(post.mean.squeeze(-1).detach().cpu(), m_ref, **VAL)
    torch.testing.assert_close(post.covariance_matrix.detach().cpu(), c_ref, **VAL)
    (g,) = torch.autograd.grad(post.mean.sum(), Xd)
    assert g.dtype == torch.float32 and g.abs().max() > 0


def test_observation_noise_and_posterior_transform(monkeypatch):
    from botorch_amd.objective import ScalarizedPosteriorTransform
    _no_generic(monkeypatch)
    b, q_a, q, N_f = 2, 2, 3, 3
    orc = _data()[3]
    X, Xp = _points(b, q_a, q, N_f)
    m_ref, c_ref = oracle_moments(orc, X, Xp, N_f)
    fm = _model().fantasize(X.to(DEV), _sampler(N_f))
    with torch.no_grad():
        noisy = fm.posterior(Xp.to(DEV), observation_noise=True)
        tf = fm.posterior(Xp.to(DEV), posterior_transform=ScalarizedPosteriorTransform(
            torch.tensor([-2.0], dtype=F64, device=DEV), offset=0.5))
    s2 = _outcome_noise(orc, q_a)[0]
    torch.testing.assert_close(noisy.mean.squeeze(-1).cpu(), m_ref, **VAL)
    torch.testing.assert_close(noisy.covariance_matrix.cpu(), c_ref + s2 * torch.eye(q, dtype=F64), **VAL)
    torch.testing.assert_close(tf.mean.squeeze(-1).cpu(), 0.5 - 2.0 * m_ref, **VAL)
    torch.testing.assert_close(tf.covariance_matrix.cpu(), 4.0 * c_ref, **VAL)


def test_unbatched_and_broadcast_shapes(monkeypatch):
    """X q_a x d gives batch_shape (N_f,); a 1 in place of b or of N_f and a
    q x d set broadcast."""
    _no_generic(monkeypatch)
    b, q_a, q, N_f = 2, 2, 3, 3
    orc = _data()[3]
    X, Xp = _points(b, q_a, q, N_f)
    model = _model()
    with torch.no_grad():
        fm0 = model.fantasize(X[0].to(DEV), _sampler(N_f))
        assert fm0.batch_shape == torch.Size([N_f])
        p0 = fm0.posterior(Xp[:, 0].to(DEV))                      # N_f x q x d: one set per fantasy
        p1 = fm0.posterior(Xp[0, 0].to(DEV))                      # q x d: shared
        fm = model.fantasize(X.to(DEV), _sampler(N_f))
        p2 = fm.posterior(Xp[:, :1].to(DEV))                      # N_f x 1 x q x d
        p3 = fm.posterior(Xp[:1, :1].to(DEV))                     # 1 x 1 x q x d
    m0, c0 = oracle_moments(orc, X[:1], Xp[:, :1], N_f)
    assert p0.mean.shape == (N_f, q, 1)
    torch.testing.assert_close(p0.mean.squeeze(-1).cpu(), m0[:, 0], **VAL)
    torch.testing.assert_close(p0.covariance_matrix.cpu(), c0[:, 0], **VAL)
    m1, c1 = oracle_moments(orc, X[:1], Xp[0, :1], N_f)
    assert p1.mean.shape == (N_f, q, 1) and p1.covariance_matrix.shape == (N_f, q, q)
    torch.testing.assert_close(p1.mean.squeeze(-1).cpu(), m1[:, 0], **VAL)
    m2, _ = oracle_moments(orc, X, Xp[:, :1].expand(N_f, b, q, 3), N_f)
    assert p2.mean.shape == (N_f, b, q, 1)
    torch.testing.assert_close(p2.mean.squeeze(-1).cpu(), m2, **VAL)
    m3, c3 = oracle_moments(orc, X, Xp[0, :1].expand(b, q, 3), N_f)
    assert p3.mean.shape == (N_f, b, q, 1)
    torch.testing.assert_close(p3.mean.squeeze(-1).cpu(), m3, **VAL)
    torch.testing.assert_close(p3.covariance_matrix.cpu(), c3.expand(N_f, b, q, q), **VAL)


# ---- acquisition functions on a fantasy model ---------------------------------------------
def _mc_reference(post, acqf, best_f=None):
    """E over the acquisition's own base samples of max_j (Y_j [- best_f]_+), in
    torch on the CPU from the posterior's moments."""
    mean, cov = post.mean.squeeze(-1).detach().cpu(), post.covariance_matrix.detach().cpu()
    Zb = acqf.sampler.base_samples.cpu()                      # S x 1 x 1 x q
    samples = mean + torch.einsum("...ij,s...j->s...i", torch.linalg.cholesky(cov),
                                  Zb.expand(Zb.shape[0], *mean.shape))
    obj = samples if best_f is None else (samples - best_f).clamp_min(0)
    return obj.amax(dim=-1).mean(dim=0)


def test_acquisition_functions_on_a_fantasy_model():
    from botorch_amd.acquisition import PosteriorMean, qExpectedImprovement, qSimpleRegret
    from botorch_amd.sampling import SobolQMCNormalSampler
    b, q_a, N_f, d = 2, 2, 3, 3
    model = _model()
    g = torch.Generator().manual_seed(8)
    X = torch.rand(b, q_a, d, generator=g, dtype=F64).to(DEV).requires_grad_(True)
    Xp = torch.rand(b, 2, d, generator=g, dtype=F64).to(DEV)
    fm = model.fantasize(X, _sampler(N_f))
    best_f = float(_data()[1].median())
    mk = lambda: SobolQMCNormalSampler(torch.Size([64]), seed=2)  # noqa: E731
    post = fm.posterior(Xp)
    qei = qExpectedImprovement(fm, best_f, sampler=mk())
    v = qei(Xp)
    assert v.shape == (N_f, b) and (v > 0).any()
    torch.testing.assert_close(v.detach().cpu(), _mc_reference(post, qei, best_f), **GRAD)
    qsr = qSimpleRegret(fm, sampler=mk())
    v = qsr(Xp)
    assert v.shape == (N_f, b)
    torch.testing.assert_close(v.detach().cpu(), _mc_reference(post, qsr), **GRAD)
    # PosteriorMean is analytic, q = 1
    pm = PosteriorMean(fm)(Xp[:, :1])
    assert pm.shape == (N_f, b)
    torch.testing.assert_close(pm, fm.posterior(Xp[:, :1]).mean.reshape(N_f, b), rtol=0, atol=0)
    # a one-step look-ahead value and its gradient to the fantasised points
    look = qsr(Xp).mean(0)
    (gX,) = torch.autograd.grad(look.sum(), X)
    assert look.shape == (b,) and gX.shape == X.shape
    assert torch.isfinite(gX).all() and gX.abs().max() > 1e-6
    eps = 1e-6  # central difference along one direction
    dirn = torch.randn(X.shape, generator=g, dtype=F64).to(DEV)
    with torch.no_grad():
        up = qSimpleRegret(model.fantasize(X + eps * dirn, _sampler(N_f)), sampler=mk())(Xp).mean(0).sum()
        dn = qSimpleRegret(model.fantasize(X - eps * dirn, _sampler(N_f)), sampler=mk())(Xp).mean(0).sum()
    torch.testing.assert_close((gX * dirn).sum(), (up - dn) / (2 * eps), rtol=1e-4, atol=1e-7)


def test_repeated_backward_needs_no_retain_graph():
    b, q_a, q, N_f = 2, 2, 3, 3
    X, Xp = _points(b, q_a, q, N_f)
    Xd, Xpd = X.to(DEV).requires_grad_(True), Xp.to(DEV).requires_grad_(True)
    fm = _model().fantasize(Xd, _sampler(N_f))
    grads = []
    for _ in range(2):
        post = fm.posterior(Xpd)
        (post.mean.sum() + post.covariance_matrix.sum()).backward()
        grads.append((Xd.grad.clone(), Xpd.grad.clone()))
        Xd.grad = Xpd.grad = None
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert grads[0][0].abs().max() > 0 and grads[0][1].abs().max() > 0


def test_source_hyperparameter_change_is_seen():
    """The fantasy model holds a reference: a change of the source model's
    hyperparameters shows up in the next posterior."""
    from botorch_amd.models import SingleTaskGP
    X, Y, _, _ = _data()
    m = SingleTaskGP(X.to(DEV), Y.to(DEV)).eval()
    Xa, Xp = _points(2, 2, 3, 3)
    fm = m.fantasize(Xa.to(DEV), _sampler(3))
    with torch.no_grad():
        before = fm.posterior(Xp.to(DEV)).mean.clone()
        m.covar_module.lengthscale = torch.full((1, 3), 0.2, dtype=F64)
        after = fm.posterior(Xp.to(DEV)).mean
        ref = m.fantasize(Xa.to(DEV), _sampler(3)).posterior(Xp.to(DEV)).mean
    assert (before - after).abs().max() > 1e-3 and torch.equal(after, ref)
