"""botorch_amd.pathwise on the device: Matheron paths of small models (n = 48,
d = 3) against the torch restatement (tests/pathwise_restatement.py) fed the
path's own Omega, W and V, the update weights against a CPU cholesky_solve, the
paths' sample moments against the exact ones, and the layers on top
(optimize_posterior_samples, get_optimal_samples, PathwiseThompsonSampling,
get_matheron_path_model, MaxPosteriorSampling).

Bounds: values, the project's kernel-against-torch bound max|got - ref| <=
1e-9 max|ref| + 1e-10; gradients, the project's gradient bar rtol 1e-5 (atol
1e-8); V, 1e-8 relative in the max norm (noise 1e-2 on standardised targets:
cond(A) <= (n + s2) / s2 ~ 5e3, i.e. ~1e-12 of rounding); the sample mean
within 5 standard errors and the sample variance within 5 sqrt(2 / (S - 1)) of
the exact variance under the drawn features (pure sampling error, S = 2048)."""
import functools
import math

import pytest
import torch

from tests import pathwise_restatement as pr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
N, D = 48, 3
NOISE = 1e-2
GRAD = dict(rtol=1e-5, atol=1e-8)
CASES = ["default", "scale_matern", "fixed_noise", "no_transform"]


def _bound(got, ref, what):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    lim = 1e-9 * ref.abs().max().item() + 1e-10
    print(f"{what}: max err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def _data(m=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(N, D, generator=g, dtype=F64)
    cols = [3.0 + 2.0 * torch.sin(3.0 * X[:, 0] + t) + X[:, 1] * X[:, 2] - 0.5 * t * X[:, 1]
            for t in range(m)]
    Y = torch.stack(cols, dim=-1) + 0.05 * torch.randn(N, m, generator=g, dtype=F64)
    return X, Y


def _set(m, ls, noise=NOISE, const=0.1):
    base = getattr(m.covar_module, "base_kernel", m.covar_module)
    base.lengthscale = torch.tensor([ls], dtype=F64)
    if noise is not None:
        m.likelihood.noise = torch.tensor([noise], dtype=F64)
    m.mean_module.constant = const
    return m.eval()


def _model(case="default", seed=0, col=0, m=1):
    from botorch_amd.models import MaternKernel, ScaleKernel, SingleTaskGP
    X, Y = _data(max(m, col + 1), seed)
    Y = Y[:, col:col + m]
    X, Y = X.to(DEV), Y.to(DEV)
    ls = [0.4, 0.6, 0.8]
    if case == "default":
        return _set(SingleTaskGP(X, Y), ls)
    if case == "scale_matern":
        cov = ScaleKernel(MaternKernel(ard_num_dims=D), outputscale=1.7)
        return _set(SingleTaskGP(X, Y, covar_module=cov), ls)
    if case == "fixed_noise":
        g = torch.Generator().manual_seed(4)
        Yvar = Y.var() * NOISE * (1.0 + torch.rand(N, 1, generator=g, dtype=F64)).to(DEV)
        return _set(SingleTaskGP(X, Y, Yvar), ls, noise=None)
    assert case == "no_transform"
    return _set(SingleTaskGP(X, Y, outcome_transform=None), ls, const=3.0)


def _restate(model, paths, X):
    """S x R restatement values from the path's own buffers."""
    ls, o, _, c = model.hyper()
    ymean, ystd = model.outcome_stats()
    pp, up = paths.paths["prior_paths"], paths.paths["update_paths"]
    return pr.path_values(int(model.kind), X.cpu(), model.train_inputs[0].cpu(), ls.cpu(), o, c,
                          ymean, ystd, pp.feature_map.weight.cpu(), pp.weight.cpu(),
                          up.weight.cpu())


@pytest.mark.parametrize("case", CASES)
def test_path_matches_restatement(case):
    from botorch_amd.pathwise import MatheronPath, draw_kernel_feature_paths, draw_matheron_paths
    torch.manual_seed(11)
    model = _model(case)
    S, M = 5, 64
    paths = draw_matheron_paths(model, torch.Size([S]),
                                prior_sampler=functools.partial(draw_kernel_feature_paths,
                                                                num_features=M))
    assert isinstance(paths, MatheronPath)
    pp, up = paths.paths["prior_paths"], paths.paths["update_paths"]
    assert pp.feature_map.weight.shape == (M // 2, D) and pp.weight.shape == (S, M)
    assert up.weight.shape == (S, N)
    g = torch.Generator().manual_seed(2)
    X = torch.rand(40, D, generator=g, dtype=F64)
    # X without sample dims: every path at every point, S x 40
    _bound(paths(X.to(DEV)), _restate(model, paths, X), f"{case} all")
    Xb = X.view(2, 20, D)  # batch dims pass through: S x 2 x 20
    _bound(paths(Xb.to(DEV)), _restate(model, paths, X).view(S, 2, 20), f"{case} all, batched")
    # X with the leading sample shape: path s on its own 8 points, S x 8
    Xs = X.view(S, 8, D)
    ref = torch.stack([_restate(model, paths, Xs[s])[s] for s in range(S)])
    _bound(paths(Xs.to(DEV)), ref, f"{case} mapped")
    # the parts add up (the prior in the transformed space, the update alone)
    ymean, ystd = model.outcome_stats()
    _bound(ymean + ystd * (pp(X.to(DEV)) + up(X.to(DEV))), _restate(model, paths, X),
           f"{case} prior + update")


def test_default_draw_has_1024_features_and_no_sample_dim():
    from botorch_amd.pathwise import draw_matheron_paths
    torch.manual_seed(3)
    model = _model()
    paths = draw_matheron_paths(model, torch.Size())
    assert paths.paths["prior_paths"].weight.shape == (1, 1024)
    X = torch.rand(7, D, dtype=F64)
    out = paths(X.to(DEV))
    assert out.shape == (7,)
    _bound(out, _restate(model, paths, X)[0], "no sample dims")


@pytest.mark.parametrize("case", ["default", "fixed_noise"])
def test_update_weights_match_cpu_solve(case):
    from botorch_amd.pathwise import draw_kernel_feature_paths, gaussian_update
    torch.manual_seed(5)
    model = _model(case)
    S = 6
    prior = draw_kernel_feature_paths(model, torch.Size([S]), num_features=64)
    Xt = model.train_inputs[0]
    with torch.no_grad():
        sample_values = prior(Xt)
    assert sample_values.shape == (S, N)
    ls, o, noise, c = model.hyper()
    if case == "fixed_noise":
        noise = model.likelihood.noise.detach().cpu()
        assert noise.min() >= 0.9 * NOISE  # the conditioning argument of the bound
    g = torch.Generator().manual_seed(6)
    eps = torch.randn(S, N, generator=g, dtype=F64) * torch.as_tensor(noise, dtype=F64).sqrt()
    upd = gaussian_update(model, sample_values, noise_values=eps.to(DEV))
    ref = pr.update_weights(int(model.kind), Xt.cpu(), ls.cpu(), o, noise,
                            model.train_targets.cpu(), sample_values.cpu(), eps)
    err = (upd.weight.cpu() - ref).abs().max().item()
    print(f"V {case}: max err {err:.3e} of {ref.abs().max().item():.3e}")
    assert err <= 1e-8 * ref.abs().max().item()
    # drawn noise: another V, same shape
    drawn = gaussian_update(model, sample_values)
    assert drawn.weight.shape == (S, N) and not torch.equal(drawn.weight, upd.weight)


@pytest.fixture(scope="module")
def many_paths():
    from botorch_amd.pathwise import draw_kernel_feature_paths, draw_matheron_paths
    torch.manual_seed(7)
    model = _model("default")
    paths = draw_matheron_paths(model, torch.Size([2048]),
                                prior_sampler=functools.partial(draw_kernel_feature_paths,
                                                                num_features=256))
    g = torch.Generator().manual_seed(8)
    X = torch.rand(8, D, generator=g, dtype=F64)
    with torch.no_grad():
        f = paths(X.to(DEV)).cpu()
    return model, paths, X, f


def test_path_mean_is_posterior_mean(many_paths):
    model, _, X, f = many_paths
    S = f.shape[0]
    mu = model.posterior(X.to(DEV)).mean.detach().cpu().reshape(-1)
    dev = (f.mean(0) - mu).abs()
    lim = 5.0 * f.std(0) / math.sqrt(S)
    print("mean deviation / limit:", (dev / lim).tolist())
    assert (dev <= lim).all()


def test_path_variance_is_exact_under_the_features(many_paths):
    model, paths, X, f = many_paths
    S = f.shape[0]
    ls, o, noise, _ = model.hyper()
    ls, Xt = ls.cpu(), model.train_inputs[0].cpu()
    _, ystd = model.outcome_stats()
    Omega = paths.paths["prior_paths"].feature_map.weight.cpu()
    kind = int(model.kind)
    A = pr.noisy_covariance(kind, Xt, ls, o, noise)
    B = torch.linalg.solve(A, pr.kernel_matrix(kind, Xt, X, ls, o))  # n x 8: A^{-1} k(Xt, x)
    resid = pr.features(X, Omega, ls, o) - B.T @ pr.features(Xt, Omega, ls, o)  # 8 x M
    exact = ystd ** 2 * ((resid ** 2).sum(-1) + noise * (B ** 2).sum(0))
    rel = (f.var(0) / exact - 1.0).abs()
    lim = 5.0 * math.sqrt(2.0 / (S - 1))
    print("variance deviation:", rel.tolist(), "limit", lim)
    assert (rel <= lim).all()


@pytest.mark.parametrize("case", ["default", "scale_matern"])
def test_gradient_of_mapped_paths(case):
    from botorch_amd.pathwise import draw_kernel_feature_paths, draw_matheron_paths
    torch.manual_seed(9)
    model = _model(case)
    S, P = 4, 5
    paths = draw_matheron_paths(model, torch.Size([S]),
                                prior_sampler=functools.partial(draw_kernel_feature_paths,
                                                                num_features=64))
    g = torch.Generator().manual_seed(10)
    X = torch.rand(S, P, D, generator=g, dtype=F64)
    dout = torch.randn(S, P, generator=g, dtype=F64)
    Xd = X.to(DEV).requires_grad_(True)
    (got,) = torch.autograd.grad((paths(Xd) * dout.to(DEV)).sum(), Xd)
    Xc = X.clone().requires_grad_(True)
    ref = torch.stack([_restate(model, paths, Xc[s])[s] for s in range(S)])
    (want,) = torch.autograd.grad((ref * dout).sum(), Xc)
    torch.testing.assert_close(got.cpu(), want, **GRAD)
    # all mode through the module as well
    Xa = X.view(-1, D).to(DEV).requires_grad_(True)
    da = torch.randn(S, S * P, generator=g, dtype=F64)
    (got,) = torch.autograd.grad((paths(Xa) * da.to(DEV)).sum(), Xa)
    Xc = X.view(-1, D).clone().requires_grad_(True)
    (want,) = torch.autograd.grad((_restate(model, paths, Xc) * da).sum(), Xc)
    torch.testing.assert_close(got.cpu(), want, **GRAD)


@pytest.mark.parametrize("maximize", [True, False])
def test_optimize_posterior_samples(maximize):
    from torch.quasirandom import SobolEngine
    from botorch_amd.pathwise import (draw_kernel_feature_paths, draw_matheron_paths,
                                      optimize_posterior_samples)
    torch.manual_seed(12)
    model = _model("default")
    S, raw = 4, 64
    paths = draw_matheron_paths(model, torch.Size([S]),
                                prior_sampler=functools.partial(draw_kernel_feature_paths,
                                                                num_features=64))
    bounds = torch.tensor([[0.0, 0.1, 0.0], [1.0, 0.9, 0.5]], dtype=F64, device=DEV)
    torch.manual_seed(13)  # fixes the raw candidate set (an unseeded scrambled Sobol draw)
    X_opt, f_opt = optimize_posterior_samples(paths, bounds, raw_samples=raw, num_restarts=4,
                                              maximize=maximize, options={"maxiter": 30})
    assert X_opt.shape == (S, D) and f_opt.shape == (S, 1)
    assert (X_opt >= bounds[0]).all() and (X_opt <= bounds[1]).all()
    with torch.no_grad():
        again = paths(X_opt.unsqueeze(-2))  # S x 1 x d: path s at its own optimiser
    torch.testing.assert_close(f_opt, again, rtol=0.0, atol=1e-12)
    torch.manual_seed(13)
    unit = SobolEngine(dimension=D, scramble=True).draw(raw, dtype=F64).to(DEV)
    cand = bounds[0] + (bounds[1] - bounds[0]) * unit
    with torch.no_grad():
        raw_values = paths(cand)  # S x raw
    if maximize:
        assert (f_opt.squeeze(-1) >= raw_values.max(-1).values).all()
    else:
        assert (f_opt.squeeze(-1) <= raw_values.min(-1).values).all()


def test_get_optimal_samples_shapes():
    from botorch_amd.pathwise import get_optimal_samples
    torch.manual_seed(14)
    model = _model("scale_matern")
    bounds = torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)]).to(DEV)
    X_opt, f_opt = get_optimal_samples(model, bounds, num_optima=3, raw_samples=32, num_restarts=2)
    assert X_opt.shape == (3, D) and f_opt.shape == (3, 1)
    assert torch.isfinite(X_opt).all() and torch.isfinite(f_opt).all()


def test_pathwise_thompson_sampling():
    from botorch_amd.acquisition import PathwiseThompsonSampling
    from botorch_amd.optim import optimize_acqf
    torch.manual_seed(15)
    model = _model("default")
    ts = PathwiseThompsonSampling(model)
    bounds = torch.stack([torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)]).to(DEV)
    cand, val = optimize_acqf(ts, bounds, q=3, num_restarts=2, raw_samples=16,
                              options={"maxiter": 20})
    assert cand.shape == (3, D) and ts.batch_size == 3
    X = torch.rand(5, 3, D, dtype=F64, device=DEV)
    with torch.no_grad():
        v0 = ts(X)
        assert v0.shape == (5,) and torch.equal(ts(X), v0)
        # point i on draw i, summed
        path = ts.samples
        want = sum(path(X[:, i:i + 1].unsqueeze(-2).expand(5, 3, 1, D).contiguous())[:, i, 0, 0]
                   for i in range(3))
        torch.testing.assert_close(v0, want, rtol=0.0, atol=1e-12)
        ts.redraw()
        assert not torch.equal(ts(X), v0)
    with pytest.raises(ValueError, match="The batch size of PathwiseThompsonSampling should not "
                                         "change during a forward pass - was 3, now 2"):
        ts(X[:, :2])


@pytest.mark.parametrize("kind", ["model_list", "multi_output"])
def test_matheron_path_model_with_posterior_mean(kind):
    from botorch_amd.acquisition import PosteriorMean
    from botorch_amd.models import ModelListGP, SingleTaskGP
    from botorch_amd.objective import ScalarizedPosteriorTransform
    from botorch_amd.pathwise import PathList, draw_matheron_paths, get_matheron_path_model
    torch.manual_seed(16)
    m = 2
    if kind == "model_list":
        model = ModelListGP(_model("default", col=0), _model("scale_matern", col=1)).eval()
    else:
        X, Y = _data(m)
        model = SingleTaskGP(X.to(DEV), Y.to(DEV))
        for mm in model.models:
            _set(mm, [0.4, 0.6, 0.8])
        model.eval()
    b, q = 4, 3
    X = torch.rand(b, q, D, dtype=F64, device=DEV)
    paths = draw_matheron_paths(model, torch.Size())
    assert isinstance(paths, PathList) and len(paths.paths) == m
    out = paths(X)
    if kind == "model_list":
        assert isinstance(out, list) and all(o.shape == (b, q) for o in out)
    else:
        assert out.shape == (b, q, m)
    path_model = get_matheron_path_model(model)
    assert path_model.num_outputs == m
    post = path_model.posterior(X)
    assert post.mean.shape == (b, q, m) and not post.variance.any()
    w = torch.tensor([1.0, -0.5], dtype=F64, device=DEV)
    acq = PosteriorMean(path_model, posterior_transform=ScalarizedPosteriorTransform(w))
    X1 = X[:, :1]
    val = acq(X1)
    assert val.shape == (b,)
    torch.testing.assert_close(val, (path_model.posterior(X1).mean @ w).reshape(b),
                               rtol=0.0, atol=1e-12)


def test_max_posterior_sampling_on_the_device():
    from botorch_amd.generation import MaxPosteriorSampling
    torch.manual_seed(17)
    model = _model("default")
    X = torch.rand(20, D, dtype=F64, device=DEV)
    with torch.no_grad():
        s = MaxPosteriorSampling(model)(X, num_samples=4)
        u = MaxPosteriorSampling(model, replacement=False)(X, num_samples=4)
    assert s.shape == (4, D) and u.shape == (4, D)
    assert all((X == r).all(-1).any() for r in torch.cat([s, u]))
    assert torch.unique(u, dim=0).shape[0] == 4


def test_all_mode_memory_stays_at_the_output():
    """One all-mode evaluation at R = 32768, n = 1024, M = 1024, S = 16 raises the
    peak by at most 4 (bytes of X + bytes of out) ~ 23 MB; the unfused R x n and
    R x M arrays would take 512 MB."""
    from botorch_amd import kernels
    R, n, M, S, d = 32768, 1024, 1024, 16, 6
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=F64, device=DEV)  # noqa: E731
    X, Xts, ls = rnd(R, d).abs(), rnd(n, d), torch.ones(d, dtype=F64, device=DEV)
    Omega, W, V = rnd(M // 2, d), rnd(S, M), rnd(S, n)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = kernels.paths_eval(X, ls, Omega, W, Xts, V)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    budget = 4 * (X.numel() + out.numel()) * 8
    print(f"peak rise {rise / 2**20:.1f} MiB, budget {budget / 2**20:.1f} MiB")
    assert out.shape == (S, R) and torch.isfinite(out).all()
    assert rise <= budget
