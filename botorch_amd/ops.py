"""PyTorch custom operators (``torch.ops.bo.*``) over the C ABI.

SURVEY.md section 8(b) asks for the hot path "bound as PyTorch-ROCm custom
ops": this module registers them with ``torch.library`` (schema, ROCm kernel,
fake/meta implementation for tracing, and an autograd formula for the
differentiable ones).  The model and acquisition classes call these ops; each
op's implementation is the ctypes binding of ``include/botorch_amd.h`` through
``botorch_amd.kernels`` (device pointers, the current HIP stream), so the ops
and the C ABI are one path, not two.

Ops (reference computation each replaces):
  bo::sobol_normal    SobolEngine + NormalQMCEngine draw        (sampling/qmc.py:60-98)
  bo::gp_cache        L, L^{-1}, L^{-T}, beta, alpha (+ jitter)  ([G] prediction caches,
                                                                 models/gpytorch.py:446)
  bo::gp_cache_extend the caches after k more observations, by the bordered
                      update of the old ones                    (models/gpytorch.py:468-531)
  bo::chol_jitter     psd_safe_cholesky of a batch (+ autograd)  ([G] psd_safe_cholesky)
  bo::post_partials   column-tile partials of R R^T and R beta  ([G] exact_predictive_covar)
  bo::qmc_finalize    posterior moments / q x q root / MC reduction
  bo::gp_posterior    outcome-space mean and covariance (+ autograd, posteriors/gpytorch.py)
  bo::qmc_acq         fused qEI / qLogEI / qSR / qPI / qUCB value of B t-batches
                      (+ autograd, acquisition/monte_carlo.py:405-414, 648-871,
                      logei.py:137-234; qPI's tau travels in tau_relu, qUCB's
                      beta' in best_f and the base samples' mean in best_f_s)
  bo::qehvi           inclusion-exclusion qEHVI on the hypercells (+ autograd,
                      multi_objective/monte_carlo.py:230-317)
  bo::mll             exact marginal log likelihood data term and its gradient
                      (optim/closures/model_closures.py:171-184)
  bo::kg              one-shot qKnowledgeGradient value of packed posterior moments
                      (+ autograd, acquisition/knowledge_gradient.py:151-207)
  bo::fantasy_posterior  mean and covariance of N_f fantasy models per t-batch from
                      packed posterior moments (+ autograd, models/model.py:328-407)
  bo::paths_eval      S Matheron paths at R points, features and kernel rows fused
                      (+ autograd in X, sampling/pathwise/posterior_samplers.py:198-224)
  bo::jes             mean conditional entropy of R points over P optima, the
                      rank-one conditioned moments fused with the entropy chain
                      (+ autograd in X, mu, var; acquisition/joint_entropy_search.py:
                      195-265; its launches go through bo::jes_native in C++)
  bo::mes             qMaxValueEntropy's information gain of R rows from their posterior
                      mean and variance (+ autograd in mu, var;
                      acquisition/max_value_entropy_search.py:399-515)
  bo::gibbon          GIBBON's quality and repulsion terms of R rows (+ autograd in mu,
                      var, A; max_value_entropy_search.py:537-664)
  bo::mv_quantiles    the three quantiles the Gumbel max-value sampler fits, one launch
                      (max_value_entropy_search.py:994-1010, in place of brentq on host copies)
  bo::nipv_gram       Gram matrices C_b C_b^T of the posterior cross-covariance of every
                      t-batch with N integration points, C never stored (+ autograd in
                      X; acquisition/active_learning.py:40-135)
  bo::bald            mixture entropy minus component entropies of an ensemble's Gaussian
                      posteriors at every t-batch, the M x S x M log-densities in registers
                      (+ autograd in mean, L; acquisition/bayesian_active_learning.py:52-126)
  bo::analytic        LogEI / EI / LogPI / PI / UCB / posterior standard deviation of R rows,
                      with up to 15 outcome constraints, from the members' posterior means
                      and variances in one launch (+ analytic autograd in mean, var;
                      acquisition/analytic.py:357-420, 528-608, 960-1053, 1182-1220)
  bo::saas_potential  U = -log p(z, Y) of the SAAS GP and its closed-form gradient for a batch
                      of NUTS chains, one workgroup per chain (models/fully_bayesian.py:168-247;
                      its launch goes through bo::saas_potential_native in C++)
  bo::icm_covar       training covariance of the ICM multi-task GP as the padded Cholesky
                      input (models/multitask.py:301-312)
  bo::icm_mll_terms   row terms of its marginal log likelihood with T task bins per row for
                      d ll / d B (the closure of fit_gpytorch_mll on a MultiTaskGP)
  bo::icm_task_view   the prediction caches of one output task, scaled so that the
                      single-task posterior kernels compute that task's posterior
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from . import _lib, kernels

F64 = torch.float64


def _geometry(B, q, n):
    """bo_post_geometry restated for symbolic shapes (the fake implementations
    run under tracing): (Qp, nrows_pad, nC) of B t-batches of q <= 16 points
    against n training points -- 16-row t-batch tiles padded to 128 rows,
    128-column training tiles."""
    Qp = 1
    while Qp < q:
        Qp *= 2
    return Qp, ((B * Qp + 127) // 128) * 128, (n + 127) // 128


def _padded(n: int) -> int:
    return ((n + 127) // 128) * 128


def _cache_from(Xt, Xt_scaled, lengthscale, U, beta, alpha, kind, outputscale, constant,
                Linv=None) -> kernels.GPCache:
    n, d = Xt.shape
    np_ = U.shape[0]
    empty = U.new_empty(0)
    return kernels.GPCache(kind, n, d, np_, Xt, Xt_scaled, lengthscale, float(outputscale), 0.0,
                           float(constant), empty, Linv if Linv is not None else empty, U, beta,
                           alpha, 0.0)


def _pp_from(B, q, n, Xq, Spart, mpart, Rt) -> kernels.PostPartials:
    Qp, nrows_pad, nC = kernels.geometry(B, q, n)
    return kernels.PostPartials(B, q, Qp, nrows_pad, nC, Xq, Spart, mpart,
                                Rt if Rt.numel() else None)


# ---- bo::sobol_normal ------------------------------------------------------------------
@torch.library.custom_op("bo::sobol_normal", mutates_args=(), device_types="cuda")
def sobol_normal(state: Tensor, shift: Tensor, n: int, skip: int, first_f32: bool) -> Tensor:
    """n x D standard-normal Sobol points from SobolEngine's scrambled direction
    numbers (state D x 30, int64) and digital shift (D, int64)."""
    dim = shift.shape[0]
    out = torch.empty(n, dim, dtype=F64, device=state.device)
    kernels.check(kernels.lib().bo_sobol_normal(kernels._p(state.contiguous()),
                                                kernels._p(shift.contiguous()), dim, n, skip,
                                                int(first_f32), kernels._p(out),
                                                kernels._stream(state.device)), "sobol_normal")
    return out


@sobol_normal.register_fake
def _(state, shift, n, skip, first_f32):
    return state.new_empty(n, shift.shape[0], dtype=F64)


# ---- bo::gp_cache --------------------------------------------------------------------------
@torch.library.custom_op("bo::gp_cache", mutates_args=(), device_types="cuda")
def gp_cache(Xt: Tensor, y: Tensor, lengthscale: Tensor, outputscale: float, noise: float,
             constant: float, kind: int, noise_vec: Optional[Tensor] = None
             ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(L, L^{-1}, U = L^{-T}: np x np; beta, alpha: n; Xt_scaled: n x 8; jitter: 1).
    noise_vec (n): a fixed-noise likelihood's observed variances (noise ignored)."""
    c = kernels.build_gp_cache(Xt, y, lengthscale, noise if noise_vec is None else noise_vec,
                               constant, kind=kind,
                               outputscale=outputscale)
    jit = torch.full((1,), c.jitter, dtype=F64, device=Xt.device)
    return c.L, c.Linv, c.U, c.beta, c.alpha, c.Xt_scaled, jit


@gp_cache.register_fake
def _(Xt, y, lengthscale, outputscale, noise, constant, kind, noise_vec=None):
    n = Xt.shape[0]
    np_ = _padded(n)
    mk = lambda *s: Xt.new_empty(*s, dtype=F64)  # noqa: E731
    return mk(np_, np_), mk(np_, np_), mk(np_, np_), mk(n), mk(n), mk(n, kernels.DP), mk(1)


# ---- bo::gp_cache_extend -------------------------------------------------------------------
@torch.library.custom_op("bo::gp_cache_extend", mutates_args=(), device_types="cuda")
def gp_cache_extend(Xt_scaled: Tensor, L: Tensor, Linv: Tensor, beta: Tensor, alpha: Tensor,
                    lengthscale: Tensor, X_new: Tensor, y_new: Tensor, outputscale: float,
                    noise: float, constant: float, kind: int, noise_vec: Optional[Tensor] = None
                    ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The caches of the model conditioned on X_new (k x d), y_new (k) by the
    bordered update of the old ones (condition_on_observations,
    models/gpytorch.py:468-531): (L', L'^{-1}, U': np' x np' at the padded order
    of n + k; beta', alpha': n + k; Xt_scaled': (n + k) x 8; info: 1, nonzero when
    the k x k border was not p.d.).  The inputs are only read."""
    return kernels.extend_gp_cache_enqueue(kind, Xt_scaled, L, Linv, beta, alpha, lengthscale,
                                           outputscale, noise, constant, X_new, y_new, noise_vec)


@gp_cache_extend.register_fake
def _(Xt_scaled, L, Linv, beta, alpha, lengthscale, X_new, y_new, outputscale, noise, constant,
      kind, noise_vec=None):
    m = Xt_scaled.shape[0] + X_new.shape[0]
    np_ = _padded(m)
    mk = lambda *s: L.new_empty(*s, dtype=F64)  # noqa: E731
    return (mk(np_, np_), mk(np_, np_), mk(np_, np_), mk(m), mk(m), mk(m, kernels.DP),
            L.new_empty(1, dtype=torch.int32))


# ---- bo::chol_jitter -------------------------------------------------------------------------
@torch.library.custom_op("bo::chol_jitter", mutates_args=(), device_types="cuda")
def chol_jitter(A: Tensor) -> Tensor:
    """psd_safe_cholesky of (..., k, k): jitter ladder per member; NotPSDError
    (with the reference's message) when the ladder is exhausted."""
    return kernels.chol_jitter(A.contiguous())


@chol_jitter.register_fake
def _(A):
    return torch.empty_like(A)


@torch.library.custom_op("bo::chol_backward", mutates_args=(), device_types="cuda")
def chol_backward(L: Tensor, dL: Tensor) -> Tensor:
    """dA of A = L L^T (torch.linalg.cholesky's backward), batched, k <= 64."""
    q = L.shape[-1]
    batch = L.shape[:-2]
    dA = kernels.chol_backward(L.reshape(-1, q, q).contiguous(),
                               dL.reshape(-1, q, q).tril().contiguous())
    return dA.reshape(*batch, q, q)


@chol_backward.register_fake
def _(L, dL):
    return torch.empty_like(L)


def _chol_setup(ctx, inputs, output):
    ctx.save_for_backward(output)


def _chol_bwd(ctx, dL):
    (L,) = ctx.saved_tensors
    return torch.ops.bo.chol_backward(L, dL)


chol_jitter.register_autograd(_chol_bwd, setup_context=_chol_setup)


# ---- bo::post_partials / bo::qmc_finalize (the primitive posterior pair) ------------------------
@torch.library.custom_op("bo::post_partials", mutates_args=(), device_types="cuda")
def post_partials(X: Tensor, Xt: Tensor, Xt_scaled: Tensor, U: Tensor, beta: Tensor,
                  lengthscale: Tensor, kind: int, outputscale: float,
                  store_R: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Column-tile partials of R R^T and R beta for X (B x q x d), R = K*x L^{-T}:
    (Spart nC x B Qp/16 x 16 x 16, mpart nC x B Qp, Xq B Qp x 8, R^T or empty)."""
    c = _cache_from(Xt, Xt_scaled, lengthscale, U, beta, beta, kind, outputscale, 0.0)
    pp = kernels.post_partials(c, X, store_R=store_R, small=False)  # the schema's nC partials
    Rt = pp.Rt if pp.Rt is not None else X.new_empty(0, dtype=F64)
    return pp.Spart, pp.mpart, pp.Xq, Rt


@post_partials.register_fake
def _(X, Xt, Xt_scaled, U, beta, lengthscale, kind, outputscale, store_R):
    B, q, _ = X.shape
    Qp, nrows_pad, nC = _geometry(B, q, Xt.shape[0])
    mk = lambda *s: X.new_empty(*s, dtype=F64)  # noqa: E731
    return (mk(nC, nrows_pad // 16, 16, 16), mk(nC, nrows_pad), mk(nrows_pad, kernels.DP),
            mk(nC * 128, nrows_pad) if store_R else mk(0))


@torch.library.custom_op("bo::qmc_finalize", mutates_args=(), device_types="cuda")
def qmc_finalize(Spart: Tensor, mpart: Tensor, Xq: Tensor, Z: Optional[Tensor],
                 best_f_s: Optional[Tensor], B: int, q: int, n: int, kind: int, mode: int,
                 outputscale: float, constant: float, ymean: float, ystd: float, best_f: float,
                 fat: bool, tau_relu: float, tau_max: float
                 ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Per t-batch: moments (outcome space), jittered q x q root and, in the MC
    modes, the acquisition value: (acq, mean, cov, L, info, jitter)."""
    pp = _pp_from(B, q, n, Xq, Spart, mpart, Xq.new_empty(0))
    c = kernels.GPCache(kind, n, 0, 0, Xq, Xq, Xq, float(outputscale), 0.0, float(constant),
                        Xq, Xq, Xq, Xq, Xq, 0.0)
    out = kernels.qmc_finalize(c, pp, mode, ymean, ystd, Z=Z, best_f=best_f, best_f_s=best_f_s,
                               want_mean=True, want_cov=True, want_L=True,
                               log_params=(fat, tau_relu, tau_max))
    def e(dtype=F64):
        return Xq.new_empty(0, dtype=dtype)
    return (out["acq"] if out["acq"] is not None else e(), out["mean"], out["cov"], out["L"],
            out["info"] if out["info"] is not None else e(torch.int32),
            out["jitter"] if out["jitter"] is not None else e())


@qmc_finalize.register_fake
def _(Spart, mpart, Xq, Z, best_f_s, B, q, n, kind, mode, outputscale, constant, ymean, ystd,
      best_f, fat, tau_relu, tau_max):
    mk = lambda *s: Xq.new_empty(*s, dtype=F64)  # noqa: E731
    mc = mode in _lib.MC_MODES
    post = mode == _lib.QMC_POSTERIOR
    return (mk(B) if mc else mk(0), mk(B, q), mk(B, q, q), mk(B, q, q),
            Xq.new_empty(0 if post else B, dtype=torch.int32), mk(0 if post else B))


# ---- bo::gp_posterior ----------------------------------------------------------------------
@torch.library.custom_op("bo::gp_posterior", mutates_args=(), device_types="cuda")
def gp_posterior(X: Tensor, Xt: Tensor, Xt_scaled: Tensor, U: Tensor, Linv: Tensor, beta: Tensor,
                 alpha: Tensor, lengthscale: Tensor, kind: int, outputscale: float,
                 constant: float, ymean: float, ystd: float, need_grad: bool
                 ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(mean B x q, cov B x q x q) of the outcome-space exact posterior
    ([G] exact_predictive_mean/covar + Standardize.untransform_posterior), plus
    what the gradient needs when need_grad: (Xq, R^T, W) (else empty)."""
    c = _cache_from(Xt, Xt_scaled, lengthscale, U, beta, alpha, kind, outputscale, constant, Linv)
    pp = kernels.post_partials(c, X, store_R=need_grad)
    out = kernels.qmc_finalize(c, pp, _lib.QMC_POSTERIOR, ymean, ystd)
    if not need_grad:
        return (out["mean"], out["cov"], X.new_empty(0, dtype=F64), X.new_empty(0, dtype=F64),
                X.new_empty(0, dtype=F64))
    W = kernels.w_matrix(c, pp)
    Wt = W.t if W.kmajor else W.t.T.contiguous()  # stored k-major (np x B Qp) either way
    return out["mean"], out["cov"], pp.Xq, pp.Rt, Wt


@gp_posterior.register_fake
def _(X, Xt, Xt_scaled, U, Linv, beta, alpha, lengthscale, kind, outputscale, constant, ymean,
      ystd, need_grad):
    B, q, _ = X.shape
    mk = lambda *s: X.new_empty(*s, dtype=F64)  # noqa: E731
    if not need_grad:
        return mk(B, q), mk(B, q, q), mk(0), mk(0), mk(0)
    Qp, nrows_pad, nC = _geometry(B, q, Xt.shape[0])
    return (mk(B, q), mk(B, q, q), mk(nrows_pad, kernels.DP), mk(nC * 128, nrows_pad),
            mk(U.shape[0], nrows_pad))


@torch.library.custom_op("bo::gp_posterior_backward", mutates_args=(), device_types="cuda")
def gp_posterior_backward(dmean: Tensor, dcov: Tensor, Xq: Tensor, Rt: Tensor, Wt: Tensor,
                          Xt: Tensor, Xt_scaled: Tensor, alpha: Tensor, lengthscale: Tensor,
                          kind: int, outputscale: float, ystd: float, q: int) -> Tensor:
    """dX (B x q x d) of the posterior moments: dK*x = s dmean alpha^T - G W,
    reduced through dk/dx over the training points (bo_post_backward)."""
    B = dmean.shape[0]
    c = _cache_from(Xt, Xt_scaled, lengthscale, Wt, alpha, alpha, kind, outputscale, 0.0)
    pp = _pp_from(B, q, Xt.shape[0], Xq, Xq, Xq, Rt)
    return kernels.post_backward(c, pp, kernels.WMat(Wt, True), dmean.contiguous(),
                                 dcov.contiguous(), ystd)


@gp_posterior_backward.register_fake
def _(dmean, dcov, Xq, Rt, Wt, Xt, Xt_scaled, alpha, lengthscale, kind, outputscale, ystd, q):
    return dmean.new_empty(dmean.shape[0], q, Xt.shape[1])


def _post_setup(ctx, inputs, output):
    X, Xt, Xt_scaled, U, Linv, beta, alpha, lengthscale, kind, outputscale, constant, ymean, ystd, \
        need_grad = inputs
    _, _, Xq, Rt, Wt = output
    # the saved intermediates carry no gradient: without this autograd would
    # zero-fill a grad for each of them (R^T and W^T: 268 MB each at C3)
    ctx.mark_non_differentiable(Xq, Rt, Wt)
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(Xq, Rt, Wt, Xt, Xt_scaled, alpha, lengthscale)
    ctx.meta = (kind, outputscale, ystd, X.shape[0], X.shape[1])


def _post_bwd(ctx, dmean, dcov, *_):
    Xq, Rt, Wt, Xt, Xt_scaled, alpha, lengthscale = ctx.saved_tensors
    kind, outputscale, ystd, B, q = ctx.meta
    if Rt.numel() == 0:
        raise RuntimeError("bo::gp_posterior was called with need_grad=False")
    if dmean is None and dcov is None:
        return (None,) * 14
    if dmean is None:
        dmean = Wt.new_zeros(B, q)
    if dcov is None:
        dcov = Wt.new_zeros(B, q, q)
    dX = torch.ops.bo.gp_posterior_backward(dmean, dcov, Xq, Rt, Wt, Xt, Xt_scaled, alpha,
                                            lengthscale, kind, outputscale, ystd, q)
    return (dX,) + (None,) * 13


gp_posterior.register_autograd(_post_bwd, setup_context=_post_setup)


# ---- bo::qmc_acq (fused qEI / qLogEI) -------------------------------------------------------
@torch.library.custom_op("bo::qmc_acq", mutates_args=(), device_types="cuda")
def qmc_acq(X: Tensor, Xt: Tensor, Xt_scaled: Tensor, U: Tensor, Linv: Tensor, beta: Tensor,
            alpha: Tensor, lengthscale: Tensor, Z: Tensor, best_f_s: Optional[Tensor], kind: int,
            mode: int, outputscale: float, constant: float, ymean: float, ystd: float,
            best_f: float, fat: bool, tau_relu: float, tau_max: float, need_grad: bool,
            Ainv: Optional[Tensor] = None
            ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """MC acquisition value (B) of B t-batches on the fused path: posterior
    partials, finalisation with the per-member jitter ladder, reparameterised
    Sobol samples and the qEI / qLogEI reduction, one launch each.  With
    need_grad also (mean, L, Xq, R^T) for the registered backward (the W^T slot
    stays empty: the backward forms W itself); the last output is the ladder
    status tensor (info).  Ainv (forward only): the model's full A^{-1}
    (kernels.quad_ainv) where the quad plan applies to this geometry."""
    # the whole host sequence is one native call (csrc/torch/bo_torch.cpp)
    n = Xt.shape[0]
    out = _lib.torch_ops().qmc_acq_native(
        X.contiguous(), Xt_scaled, U, Linv, beta, lengthscale, Z.reshape(-1, X.shape[1]).contiguous(),
        best_f_s, kind, mode, n, outputscale, constant, ymean, ystd, best_f, fat, tau_relu, tau_max,
        need_grad, kernels.kxt_cap(X.device), False, Ainv, alpha)
    acq, mean, L, Xq, Rt, Wt, jit, info, _ = out
    return acq, mean, L, Xq, Rt, Wt, jit, info


@qmc_acq.register_fake
def _(X, Xt, Xt_scaled, U, Linv, beta, alpha, lengthscale, Z, best_f_s, kind, mode, outputscale,
      constant, ymean, ystd, best_f, fat, tau_relu, tau_max, need_grad, Ainv=None):
    B, q, _ = X.shape
    mk = lambda *s: X.new_empty(*s, dtype=F64)  # noqa: E731
    info = X.new_empty(B, dtype=torch.int32)
    if not need_grad:
        return mk(B), mk(0), mk(0), mk(0), mk(0), mk(0), mk(B), info
    Qp, nrows_pad, nC = _geometry(B, q, Xt.shape[0])
    # R^T's layout is carried by its shape (csrc/torch/bo_torch.cpp): blocked
    # where the backward's fused W -> dX pass applies
    Rt = (mk(nC * 8, nrows_pad // 16, 256) if kernels.rt_blocked_plan(B, q, Xt.shape[0])
          else mk(nC * 128, nrows_pad))
    return (mk(B), mk(B, q), mk(B, q, q), mk(nrows_pad, kernels.DP), Rt, mk(0), mk(B), info)


@torch.library.custom_op("bo::qmc_acq_backward", mutates_args=(), device_types="cuda")
def qmc_acq_backward(dacq: Tensor, acq: Tensor, mean: Tensor, L: Tensor, Z: Tensor,
                     best_f_s: Optional[Tensor], Xq: Tensor, Rt: Tensor, Linv: Tensor, U: Tensor,
                     Xt: Tensor, Xt_scaled: Tensor, alpha: Tensor, lengthscale: Tensor, kind: int,
                     mode: int, outputscale: float, ystd: float, best_f: float, fat: bool,
                     tau_relu: float, tau_max: float) -> Tensor:
    """dX of qmc_acq: the reduction + sampling + q x q Cholesky backward
    (bo_qmc_backward), then the posterior backward with W = R L^-1 reduced into
    dX as it is formed (bo_post_w_dx) -- one native call
    (bo::qmc_acq_backward_native)."""
    return _lib.torch_ops().qmc_acq_backward_native(
        dacq.contiguous(), acq, mean, L, Z.reshape(-1, mean.shape[1]).contiguous(), best_f_s, Xq,
        Rt, Linv, U, Xt_scaled, alpha, lengthscale, kind, mode, Xt.shape[1], Xt.shape[0],
        outputscale, ystd, best_f, fat, tau_relu, tau_max)


@qmc_acq_backward.register_fake
def _(dacq, acq, mean, L, Z, best_f_s, Xq, Rt, Linv, U, Xt, Xt_scaled, alpha, lengthscale, kind,
      mode, outputscale, ystd, best_f, fat, tau_relu, tau_max):
    return mean.new_empty(mean.shape[0], mean.shape[1], Xt.shape[1])


def _acq_setup(ctx, inputs, output):
    (X, Xt, Xt_scaled, U, Linv, beta, alpha, lengthscale, Z, best_f_s, kind, mode, outputscale,
     constant, ymean, ystd, best_f, fat, tau_relu, tau_max, need_grad, *_) = inputs
    acq, mean, L, Xq, Rt, Wt, jit, info = output
    # only acq is differentiable; unmaterialised grads keep autograd from
    # zero-filling R^T (268 MB at C3) on every backward
    ctx.mark_non_differentiable(mean, L, Xq, Rt, Wt, jit, info)
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(acq, mean, L, Z, Xq, Rt, Linv, U, Xt, Xt_scaled, alpha, lengthscale)
    ctx.best_f_s = best_f_s
    ctx.meta = (kind, mode, outputscale, ystd, best_f, fat, tau_relu, tau_max)


def _acq_bwd(ctx, dacq, *_):
    acq, mean, L, Z, Xq, Rt, Linv, U, Xt, Xt_scaled, alpha, lengthscale = ctx.saved_tensors
    if Rt.numel() == 0:
        raise RuntimeError("bo::qmc_acq was called with need_grad=False")
    kind, mode, outputscale, ystd, best_f, fat, tau_relu, tau_max = ctx.meta
    if dacq is None:
        return (None,) * 22
    dX = torch.ops.bo.qmc_acq_backward(dacq, acq, mean, L, Z, ctx.best_f_s, Xq, Rt, Linv, U, Xt,
                                       Xt_scaled, alpha, lengthscale, kind, mode, outputscale,
                                       ystd, best_f, fat, tau_relu, tau_max)
    # the forward's deferred ladder status, now that the backward is queued
    # (waits only for the forward's event; raises NotPSDError / warns here)
    if not torch.cuda.is_current_stream_capturing():
        kernels.check_ladder_status(dX.device)
    return (dX,) + (None,) * 21


qmc_acq.register_autograd(_acq_bwd, setup_context=_acq_setup)


class QmcAcqGrad(torch.autograd.Function):
    """bo::qmc_acq with need_grad, as a plain autograd Function: the same two
    native calls (qmc_acq_native, qmc_acq_backward_native) and the semantics
    of _acq_setup / _acq_bwd (only acq differentiable, no materialised zero
    grads, the ladder status read once the backward is queued), without the
    torch.library autograd wrapper around the registered op -- its per-call
    schema handling (fill_defaults over 22 arguments) and redispatch cost ~90
    us of host time per C2 forward + backward (tools/host_c2_fwd_bwd.py), the
    per-iteration path of gen_candidates_scipy.  The registered op stays the
    interface for opcheck / fake tensors and the forward-only calls."""

    @staticmethod
    def forward(ctx, X, Xt, Xt_scaled, U, Linv, beta, alpha, lengthscale, Z, best_f_s, kind, mode,
                outputscale, constant, ymean, ystd, best_f, fat, tau_relu, tau_max):
        out = _lib.torch_ops().qmc_acq_native(
            X.contiguous(), Xt_scaled, U, Linv, beta, lengthscale,
            Z.reshape(-1, X.shape[1]).contiguous(), best_f_s, kind, mode, Xt.shape[0], outputscale,
            constant, ymean, ystd, best_f, fat, tau_relu, tau_max, True, kernels.kxt_cap(X.device),
            False, None, alpha)
        acq, mean, L, Xq, Rt, _, jit, info, _ = out
        ctx.mark_non_differentiable(jit, info)
        ctx.set_materialize_grads(False)
        # every tensor through save_for_backward (the output acq included): a
        # tensor held as a plain ctx attribute, above all an output, forms an
        # output -> grad_fn -> ctx -> output cycle that keeps R^T (268 MB at C3)
        # and the whole graph alive until the cyclic GC runs, and skips the
        # saved-tensor version check on the cached U / L^-1 / alpha
        ctx.save_for_backward(acq, mean, L, Z, Xq, Rt, Linv, U, Xt_scaled, alpha, lengthscale,
                              best_f_s)
        ctx.meta = (kind, mode, outputscale, ystd, best_f, fat, tau_relu, tau_max, Xt.shape[1],
                    Xt.shape[0])
        return acq, jit, info

    @staticmethod
    def backward(ctx, dacq, *_):
        if dacq is None:
            return (None,) * 20
        acq, mean, L, Z, Xq, Rt, Linv, U, Xt_scaled, alpha, lengthscale, best_f_s = \
            ctx.saved_tensors
        kind, mode, outputscale, ystd, best_f, fat, tau_relu, tau_max, d, n = ctx.meta
        dX = _lib.torch_ops().qmc_acq_backward_native(
            dacq.contiguous(), acq, mean, L, Z.reshape(-1, mean.shape[1]).contiguous(), best_f_s,
            Xq, Rt, Linv, U, Xt_scaled, alpha, lengthscale, kind, mode, d, n, outputscale, ystd,
            best_f, fat, tau_relu, tau_max)
        if not torch.cuda.is_current_stream_capturing():
            kernels.check_ladder_status(dX.device)
        return (dX,) + (None,) * 19


# ---- bo::qehvi ---------------------------------------------------------------------------
@torch.library.custom_op("bo::qehvi", mutates_args=(), device_types="cuda")
def qehvi(mean: Tensor, L: Tensor, Z: Tensor, cell_lo: Tensor, cell_hi: Tensor) -> Tensor:
    """qEHVI (B) of m independent outputs: mean m x B x q, roots m x B x q x q,
    Z S x (q m), hypercells K x m (or S x K x m)."""
    return kernels.qehvi(mean, L, Z, cell_lo, cell_hi)


@qehvi.register_fake
def _(mean, L, Z, cell_lo, cell_hi):
    return mean.new_empty(mean.shape[1])


@torch.library.custom_op("bo::qehvi_backward", mutates_args=(), device_types="cuda")
def qehvi_backward(dacq: Tensor, mean: Tensor, L: Tensor, Z: Tensor, cell_lo: Tensor,
                   cell_hi: Tensor) -> Tuple[Tensor, Tensor]:
    return kernels.qehvi_backward(mean, L, Z, cell_lo, cell_hi, dacq)


@qehvi_backward.register_fake
def _(dacq, mean, L, Z, cell_lo, cell_hi):
    return torch.empty_like(mean), torch.empty_like(L)


def _qehvi_setup(ctx, inputs, output):
    mean, L, Z, cell_lo, cell_hi = inputs
    ctx.save_for_backward(mean, L, Z, cell_lo, cell_hi)


def _qehvi_bwd(ctx, dacq):
    mean, L, Z, lo, hi = ctx.saved_tensors
    dmean, dL = torch.ops.bo.qehvi_backward(dacq, mean, L, Z, lo, hi)
    return dmean, dL, None, None, None


qehvi.register_autograd(_qehvi_bwd, setup_context=_qehvi_setup)


# ---- bo::mll -----------------------------------------------------------------------------------
@torch.library.custom_op("bo::mll", mutates_args=(), device_types="cuda")
def mll(Xt: Tensor, y: Tensor, lengthscale: Tensor, noise: float, constant: float,
        outputscale: float, kind: int, noise_vec: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Data term of the exact marginal log likelihood, log N(y | c, K + s2 I)
    (no priors, not divided by n), and its gradient w.r.t. [noise, constant,
    lengthscale_1..d, (outputscale)]: one Cholesky + inverse (task DAG), the
    triangular A^{-1} = U U^T and one bo_mll_terms pass.  noise_vec (n): a
    fixed-noise likelihood (K + diag(noise_vec); the noise entry of the
    gradient is then meaningless and unused)."""
    from .fit import mll_terms
    val, grad = mll_terms(Xt, y, lengthscale, noise if noise_vec is None else noise_vec,
                          constant, outputscale, kind)
    return (torch.tensor([val], dtype=F64, device=Xt.device),
            torch.as_tensor(grad, dtype=F64).to(Xt.device))


@mll.register_fake
def _(Xt, y, lengthscale, noise, constant, outputscale, kind, noise_vec=None):
    d = Xt.shape[1]
    return Xt.new_empty(1, dtype=F64), Xt.new_empty(d + 3, dtype=F64)


# ---- bo::kg (one-shot knowledge gradient, posterior-mean inner value) -------------------------
@torch.library.custom_op("bo::kg", mutates_args=(), device_types="cuda")
def kg(mean: Tensor, cov: Tensor, Z: Tensor, noise: float, q_a: int, slots: int
       ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(acq B, values B x N_f) of the packed moments mean (B T) x q', cov (B T)
    x q' x q' (kernels.kg_tile_plan, q' = q_a + slots) and the fantasy base
    samples Z (N_f x q_a), plus (L, W) for the backward and the ladder's
    (jitter, info) per restart."""
    o = kernels.kg(mean, cov, Z, noise, q_a, slots)
    return o["acq"], o["values"], o["L"], o["W"], o["jitter"], o["info"]


@kg.register_fake
def _(mean, cov, Z, noise, q_a, slots):
    N_f = Z.shape[0]
    B = mean.shape[0] // ((N_f + slots - 1) // slots)
    mk = lambda *s: mean.new_empty(*s, dtype=F64)  # noqa: E731
    return (mk(B), mk(B, N_f), mk(B, q_a, q_a), mk(B, N_f, q_a), mk(B),
            mean.new_empty(B, dtype=torch.int32))


@torch.library.custom_op("bo::kg_backward", mutates_args=(), device_types="cuda")
def kg_backward(dacq: Tensor, dvalues: Optional[Tensor], cov: Tensor, L: Tensor, W: Tensor,
                slots: int) -> Tuple[Tensor, Tensor]:
    return kernels.kg_backward(cov, L, W, dacq, slots, dvalues)


@kg_backward.register_fake
def _(dacq, dvalues, cov, L, W, slots):
    return cov.new_empty(cov.shape[0], cov.shape[1]), torch.empty_like(cov)


def _kg_setup(ctx, inputs, output):
    mean, cov, Z, noise, q_a, slots = inputs
    _, _, L, W, jitter, info = output
    ctx.mark_non_differentiable(L, W, jitter, info)
    ctx.set_materialize_grads(False)
    ctx.save_for_backward(cov, L, W)
    ctx.slots = slots


def _kg_bwd(ctx, dacq, dvalues, *_):
    cov, L, W = ctx.saved_tensors
    if dacq is None and dvalues is None:
        return (None,) * 6
    if dacq is None:
        dacq = W.new_zeros(W.shape[0])
    dmean, dcov = torch.ops.bo.kg_backward(dacq, dvalues, cov, L, W, ctx.slots)
    return dmean, dcov, None, None, None, None


kg.register_autograd(_kg_bwd, setup_context=_kg_setup)


# ---- bo::fantasy_posterior (batched fantasy models from packed posterior moments) --------------
@torch.library.custom_op("bo::fantasy_posterior", mutates_args=(), device_types="cuda")
def fantasy_posterior(mean: Tensor, cov: Tensor, Z: Tensor, noise: Tensor, q_a: int, q: int,
                      slots: int, shared: bool
                      ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(mean_out B x N_f x q, cov_out B x F x q x q) of the fantasy models from
    the packed moments mean (B T) x q', cov (B T) x q' x q' (kernels.
    fantasy_tile_plan, q' = q_a + slots q), the fantasy base samples Z (N_f x
    q_a) and the fantasy noise (q_a or B x q_a), plus (L, V) for the backward
    and the ladder's (jitter, info) per t-batch.  F = 1 with ``shared``."""
    o = kernels.fantasy_posterior(mean, cov, Z, noise, q_a, q, slots, shared)
    return o["mean_out"], o["cov_out"], o["L"], o["V"], o["jitter"], o["info"]


@fantasy_posterior.register_fake
def _(mean, cov, Z, noise, q_a, q, slots, shared):
    N_f = Z.shape[0]
    F = 1 if shared else N_f
    B = mean.shape[0] // ((F + slots - 1) // slots)
    mk = lambda *s: mean.new_empty(*s, dtype=F64)  # noqa: E731
    return (mk(B, N_f, q), mk(B, F, q, q), mk(B, q_a, q_a), mk(B, F, q, q_a), mk(B),
            mean.new_empty(B, dtype=torch.int32))


@torch.library.custom_op("bo::fantasy_posterior_backward", mutates_args=(), device_types="cuda")
def fantasy_posterior_backward(dmean_out: Tensor, dcov_out: Tensor, Z: Tensor, L: Tensor,
                               V: Tensor, slots: int, shared: bool
                               ) -> Tuple[Tensor, Tensor, Tensor]:
    return kernels.fantasy_posterior_backward(Z, L, V, dmean_out, dcov_out, slots, shared,
                                              need_dZ=True)


@fantasy_posterior_backward.register_fake
def _(dmean_out, dcov_out, Z, L, V, slots, shared):
    B, F, q, q_a = V.shape
    T, qp = (F + slots - 1) // slots, q_a + slots * q
    return V.new_empty(B * T, qp), V.new_empty(B * T, qp, qp), torch.empty_like(Z)


def _fantasy_setup(ctx, inputs, output):
    mean, cov, Z, noise, q_a, q, slots, shared = inputs
    _, _, L, V, jitter, info = output
    ctx.mark_non_differentiable(L, V, jitter, info)
    ctx.save_for_backward(Z, L, V)
    ctx.slots, ctx.shared = slots, shared


def _fantasy_bwd(ctx, dmean_out, dcov_out, *_):
    Z, L, V = ctx.saved_tensors
    dmean, dcov, dZ = torch.ops.bo.fantasy_posterior_backward(
        dmean_out, dcov_out, Z, L, V, ctx.slots, ctx.shared)
    return dmean, dcov, (dZ if ctx.needs_input_grad[2] else None), None, None, None, None, None


fantasy_posterior.register_autograd(_fantasy_bwd, setup_context=_fantasy_setup)


# ---- bo::paths_eval (Matheron paths at R points, fused features + kernel rows) -----------------
@torch.library.custom_op("bo::paths_eval", mutates_args=(), device_types="cuda")
def paths_eval(X: Tensor, lengthscale: Tensor, Omega: Tensor, W: Tensor,
               Xt_scaled: Optional[Tensor], V: Optional[Tensor], kind: int, outputscale: float,
               constant: float, ymean: float, ystd: float, inner: int) -> Tensor:
    """S pathwise posterior samples at the rows of X (R x d): S x R (inner = 0)
    or, with row r on path (r // inner) % S, R values (kernels.paths_eval).
    Differentiable in X only: Omega, W and V are buffers of the draw."""
    return kernels.paths_eval(X, lengthscale, Omega, W, Xt_scaled, V, kind, outputscale, constant,
                              ymean, ystd, inner)


@paths_eval.register_fake
def _(X, lengthscale, Omega, W, Xt_scaled, V, kind, outputscale, constant, ymean, ystd, inner):
    R = X.shape[0]
    return X.new_empty((R,) if inner else (W.shape[0], R), dtype=F64)


@torch.library.custom_op("bo::paths_eval_backward", mutates_args=(), device_types="cuda")
def paths_eval_backward(dout: Tensor, X: Tensor, lengthscale: Tensor, Omega: Tensor, W: Tensor,
                        Xt_scaled: Optional[Tensor], V: Optional[Tensor], kind: int,
                        outputscale: float, ystd: float, inner: int) -> Tensor:
    return kernels.paths_eval_backward(dout, X, lengthscale, Omega, W, Xt_scaled, V, kind,
                                       outputscale, ystd, inner)


@paths_eval_backward.register_fake
def _(dout, X, lengthscale, Omega, W, Xt_scaled, V, kind, outputscale, ystd, inner):
    return X.new_empty(X.shape, dtype=F64)


def _paths_setup(ctx, inputs, output):
    X, lengthscale, Omega, W, Xt_scaled, V, kind, outputscale, _, _, ystd, inner = inputs
    ctx.save_for_backward(X, lengthscale, Omega, W, Xt_scaled, V)
    ctx.consts = (kind, outputscale, ystd, inner)


def _paths_bwd(ctx, dout):
    X, lengthscale, Omega, W, Xt_scaled, V = ctx.saved_tensors
    dX = None
    if ctx.needs_input_grad[0]:
        dX = torch.ops.bo.paths_eval_backward(dout.contiguous(), X, lengthscale, Omega, W,
                                              Xt_scaled, V, *ctx.consts)
    return (dX,) + (None,) * 11


paths_eval.register_autograd(_paths_bwd, setup_context=_paths_setup)


# ---- bo::jes (joint entropy search, lower bound: mean conditional entropy per row) -------------
def _jes_dense(X, mu, var, lengthscale, Xt_scaled, Xopt_scaled, V, g, sinv, wf, tau2):
    """The tensor arguments of bo::jes[_backward]_native, contiguous, after
    kernels.jes_check's limits (a ValueError before any native call)."""
    if X.dim() != 2 or Xopt_scaled.dim() != 2:
        raise ValueError("jes: X must be R x d and Xopt_scaled P x d")
    kernels.jes_check(X.shape[1], Xopt_scaled.shape[0], X.shape[0])
    return tuple(None if t is None else t.contiguous()
                 for t in (X, mu, var, lengthscale, Xt_scaled, Xopt_scaled, V, g, sinv, wf, tau2))


@torch.library.custom_op("bo::jes", mutates_args=(), device_types="cuda")
def jes(X: Tensor, mu: Tensor, var: Tensor, lengthscale: Tensor, Xt_scaled: Optional[Tensor],
        Xopt_scaled: Tensor, V: Optional[Tensor], g: Tensor, sinv: Tensor, wf: Tensor,
        tau2: Tensor, kind: int, outputscale: float, w: float) -> Tensor:
    """H (R): the mean over the P optima of log(vt_ij) / 2 at the rows of X
    (R x d) with current posterior mean mu and variance var (R each)
    (kernels.jes).  Differentiable in X (through the covariance with the
    optima), mu and var; the optima's tensors are buffers of the construction.
    One native call (bo::jes_native, csrc/torch/bo_torch.cpp) after the host's
    limit checks."""
    n = 0 if V is None else V.shape[-1]
    args = _jes_dense(X, mu, var, lengthscale, Xt_scaled if n else None, Xopt_scaled,
                      V if n else None, g, sinv, wf, tau2)
    return _lib.torch_ops().jes_native(*args, kind, outputscale, w)


@jes.register_fake
def _(X, mu, var, lengthscale, Xt_scaled, Xopt_scaled, V, g, sinv, wf, tau2, kind, outputscale,
      w):
    return X.new_empty((X.shape[0],), dtype=F64)


@torch.library.custom_op("bo::jes_backward", mutates_args=(), device_types="cuda")
def jes_backward(dout: Tensor, X: Tensor, mu: Tensor, var: Tensor, lengthscale: Tensor,
                 Xt_scaled: Optional[Tensor], Xopt_scaled: Tensor, V: Optional[Tensor], g: Tensor,
                 sinv: Tensor, wf: Tensor, tau2: Tensor, kind: int, outputscale: float,
                 w: float) -> Tuple[Tensor, Tensor, Tensor]:
    n = 0 if V is None else V.shape[-1]
    args = _jes_dense(X, mu, var, lengthscale, Xt_scaled if n else None, Xopt_scaled,
                      V if n else None, g, sinv, wf, tau2)
    dX, dmu, dvar = _lib.torch_ops().jes_backward_native(dout.contiguous(), *args, kind,
                                                         outputscale, w)
    return dX, dmu, dvar


@jes_backward.register_fake
def _(dout, X, mu, var, lengthscale, Xt_scaled, Xopt_scaled, V, g, sinv, wf, tau2, kind,
      outputscale, w):
    return (X.new_empty(X.shape, dtype=F64), X.new_empty((X.shape[0],), dtype=F64),
            X.new_empty((X.shape[0],), dtype=F64))


def _jes_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:11])
    ctx.consts = inputs[11:]


def _jes_bwd(ctx, dout):
    dX = dmu = dvar = None
    if any(ctx.needs_input_grad[:3]):
        dX, dmu, dvar = torch.ops.bo.jes_backward(dout.contiguous(), *ctx.saved_tensors,
                                                  *ctx.consts)
    return (dX, dmu, dvar) + (None,) * 11


jes.register_autograd(_jes_bwd, setup_context=_jes_setup)


# ---- bo::mes, bo::gibbon, bo::mv_quantiles (max-value entropy search) ----------------------------
def _mes_dense(mu, var, fstar, z):
    """The tensor arguments of bo::mes[_backward]_native, contiguous, after
    kernels.mes_check's limits (a ValueError before any native call)."""
    if mu.dim() != 1 or fstar.dim() != 1 or z.dim() != 1:
        raise ValueError("mes: mu, fstar and z must be vectors")
    kernels.mes_check(fstar.shape[0], z.shape[0], mu.shape[0])
    return tuple(t.contiguous() for t in (mu, var, fstar, z))


@torch.library.custom_op("bo::mes", mutates_args=(), device_types="cuda")
def mes(mu: Tensor, var: Tensor, fstar: Tensor, z: Tensor, kappa: float, var_h0: float,
        zsq_mean: float, tau2: float, w: float) -> Tensor:
    """ig (R): qMaxValueEntropy's information gain of R rows with posterior mean
    mu and variance var (R each), S_M max values fstar and S_m base samples z
    (kernels.mes; kappa, var_h0, zsq_mean = kernels.mes_host_constants(z)).
    Differentiable in mu and var."""
    return _lib.torch_ops().mes_native(*_mes_dense(mu, var, fstar, z), kappa, var_h0, zsq_mean,
                                       tau2, w)


@mes.register_fake
def _(mu, var, fstar, z, kappa, var_h0, zsq_mean, tau2, w):
    return mu.new_empty((mu.shape[0],), dtype=F64)


@torch.library.custom_op("bo::mes_backward", mutates_args=(), device_types="cuda")
def mes_backward(dout: Tensor, mu: Tensor, var: Tensor, fstar: Tensor, z: Tensor, kappa: float,
                 var_h0: float, zsq_mean: float, tau2: float, w: float) -> Tuple[Tensor, Tensor]:
    dmu, dvar = _lib.torch_ops().mes_backward_native(dout.contiguous(),
                                                     *_mes_dense(mu, var, fstar, z), kappa,
                                                     var_h0, zsq_mean, tau2, w)
    return dmu, dvar


@mes_backward.register_fake
def _(dout, mu, var, fstar, z, kappa, var_h0, zsq_mean, tau2, w):
    return mu.new_empty((mu.shape[0],), dtype=F64), mu.new_empty((mu.shape[0],), dtype=F64)


def _mes_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:4])
    ctx.consts = inputs[4:]


def _mes_bwd(ctx, dout):
    dmu = dvar = None
    if any(ctx.needs_input_grad[:2]):
        dmu, dvar = torch.ops.bo.mes_backward(dout.contiguous(), *ctx.saved_tensors, *ctx.consts)
    return (dmu, dvar) + (None,) * 7


mes.register_autograd(_mes_bwd, setup_context=_mes_setup)


def _gibbon_dense(mu, var, A, Binv, fstar):
    if mu.dim() != 1 or fstar.dim() != 1:
        raise ValueError("gibbon: mu and fstar must be vectors")
    m = 0 if A is None else A.shape[-1]
    kernels.gibbon_check(fstar.shape[0], m, mu.shape[0])
    if m and Binv is None:
        raise ValueError("gibbon: A and Binv go together")
    return (mu.contiguous(), var.contiguous(), A.contiguous() if m else None,
            Binv.contiguous() if m else None, fstar.contiguous())


@torch.library.custom_op("bo::gibbon", mutates_args=(), device_types="cuda")
def gibbon(mu: Tensor, var: Tensor, A: Optional[Tensor], Binv: Optional[Tensor], fstar: Tensor,
           tau2: float, w: float) -> Tensor:
    """acq (R): GIBBON's value of R rows (kernels.gibbon); with A (R x m) and
    Binv (m x m) the repulsion term of m pending points is added.
    Differentiable in mu, var and A."""
    return _lib.torch_ops().gibbon_native(*_gibbon_dense(mu, var, A, Binv, fstar), tau2, w)


@gibbon.register_fake
def _(mu, var, A, Binv, fstar, tau2, w):
    return mu.new_empty((mu.shape[0],), dtype=F64)


@torch.library.custom_op("bo::gibbon_backward", mutates_args=(), device_types="cuda")
def gibbon_backward(dout: Tensor, mu: Tensor, var: Tensor, A: Optional[Tensor],
                    Binv: Optional[Tensor], fstar: Tensor, tau2: float,
                    w: float) -> Tuple[Tensor, Tensor, Tensor]:
    """(dmu, dvar, dA); dA is R x m (R x 0 without pending points)."""
    dmu, dvar, dA = _lib.torch_ops().gibbon_backward_native(
        dout.contiguous(), *_gibbon_dense(mu, var, A, Binv, fstar), tau2, w)
    return dmu, dvar, dA


@gibbon_backward.register_fake
def _(dout, mu, var, A, Binv, fstar, tau2, w):
    R = mu.shape[0]
    return (mu.new_empty((R,), dtype=F64), mu.new_empty((R,), dtype=F64),
            mu.new_empty((R, 0 if A is None else A.shape[-1]), dtype=F64))


def _gibbon_setup(ctx, inputs, output):
    ctx.present = [t is not None for t in inputs[:5]]  # (A and Binv may be None)
    ctx.save_for_backward(*[t for t in inputs[:5] if t is not None])
    ctx.consts = inputs[5:]


def _gibbon_bwd(ctx, dout):
    dmu = dvar = dA = None
    if any(ctx.needs_input_grad[:3]):
        saved = iter(ctx.saved_tensors)
        tensors = [next(saved) if p else None for p in ctx.present]
        dmu, dvar, dA = torch.ops.bo.gibbon_backward(dout.contiguous(), *tensors, *ctx.consts)
        if tensors[2] is None:
            dA = None
    return (dmu, dvar, dA) + (None,) * 4


gibbon.register_autograd(_gibbon_bwd, setup_context=_gibbon_setup)


@torch.library.custom_op("bo::mv_quantiles", mutates_args=(), device_types="cuda")
def mv_quantiles(mu: Tensor, sigma: Tensor, have_bounds: bool, lo: float,
                 hi: float) -> Tuple[Tensor, Tensor]:
    """(y (3), status (3) int32): the y with sum_i log Phi((y - mu_i) / sigma_i)
    = log p for p = 0.25, 0.5, 0.75 by one on-device bisection launch
    (kernels.mv_quantiles); a non-zero status word means the end points did not
    bracket (kernels.mv_quantiles_raise turns it into brentq's ValueError)."""
    if mu.dim() != 1 or mu.shape[0] < 1 or tuple(sigma.shape) != tuple(mu.shape):
        raise ValueError("mv_quantiles: mu and sigma must have N >= 1 entries each")
    y, status = _lib.torch_ops().mv_quantiles_native(mu.contiguous(), sigma.contiguous(),
                                                     have_bounds, lo, hi)
    return y, status


@mv_quantiles.register_fake
def _(mu, sigma, have_bounds, lo, hi):
    return mu.new_empty((3,), dtype=F64), mu.new_empty((3,), dtype=torch.int32)


# ---- bo::nipv_gram (integrated posterior variance: cross-covariance Gram matrices) ---------------
@torch.library.custom_op("bo::nipv_gram", mutates_args=(), device_types="cuda")
def nipv_gram(X: Tensor, q: int, lengthscale: Tensor, Xt_scaled: Optional[Tensor],
              Z_scaled: Tensor, V: Optional[Tensor], kind: int, outputscale: float,
              split: int) -> Tensor:
    """G (B x q x q): C_b C_b^T of the t-batches of q rows of X (R x d, R = B q)
    with c(x_i, z) the posterior covariance of x_i and integration point z
    (kernels.nipv_gram).  Differentiable in X only: Z_scaled and V are buffers of
    the construction."""
    return kernels.nipv_gram(X, q, lengthscale, Xt_scaled, Z_scaled, V, kind, outputscale, split)


@nipv_gram.register_fake
def _(X, q, lengthscale, Xt_scaled, Z_scaled, V, kind, outputscale, split):
    return X.new_empty((X.shape[0] // q, q, q), dtype=F64)


@torch.library.custom_op("bo::nipv_gram_backward", mutates_args=(), device_types="cuda")
def nipv_gram_backward(dG: Tensor, X: Tensor, q: int, lengthscale: Tensor,
                       Xt_scaled: Optional[Tensor], Z_scaled: Tensor, V: Optional[Tensor],
                       kind: int, outputscale: float, split: int) -> Tensor:
    return kernels.nipv_gram_backward(dG, X, q, lengthscale, Xt_scaled, Z_scaled, V, kind,
                                      outputscale, split)


@nipv_gram_backward.register_fake
def _(dG, X, q, lengthscale, Xt_scaled, Z_scaled, V, kind, outputscale, split):
    return X.new_empty(X.shape, dtype=F64)


def _nipv_setup(ctx, inputs, output):
    X, q, lengthscale, Xt_scaled, Z_scaled, V, kind, outputscale, split = inputs
    ctx.save_for_backward(X, lengthscale, Xt_scaled, Z_scaled, V)
    ctx.consts = (q, kind, outputscale, split)


def _nipv_bwd(ctx, dG):
    X, lengthscale, Xt_scaled, Z_scaled, V = ctx.saved_tensors
    q, kind, outputscale, split = ctx.consts
    dX = None
    if ctx.needs_input_grad[0]:
        dX = torch.ops.bo.nipv_gram_backward(dG.contiguous(), X, q, lengthscale, Xt_scaled,
                                             Z_scaled, V, kind, outputscale, split)
    return (dX,) + (None,) * 8


nipv_gram.register_autograd(_nipv_bwd, setup_context=_nipv_setup)


# ---- bo::bald (BALD over a Gaussian-mixture posterior) -------------------------------------------
@torch.library.custom_op("bo::bald", mutates_args=(), device_types="cuda")
def bald(mean: Tensor, L: Tensor, Z: Tensor, M: int) -> Tensor:
    """out (B x M) = H_b - C_bm from the components' means (M B x q), Cholesky
    roots (M B x q x q) and the shared base samples Z (S x q) (kernels.bald).
    Differentiable in mean and L."""
    return kernels.bald(mean, L, Z, M)


@bald.register_fake
def _(mean, L, Z, M):
    return mean.new_empty((mean.shape[0] // M, M), dtype=F64)


@torch.library.custom_op("bo::bald_backward", mutates_args=(), device_types="cuda")
def bald_backward(dout: Tensor, mean: Tensor, L: Tensor, Z: Tensor, M: int) -> Tuple[Tensor, Tensor]:
    return kernels.bald_backward(dout, mean, L, Z, M)


@bald_backward.register_fake
def _(dout, mean, L, Z, M):
    return mean.new_empty(mean.shape, dtype=F64), L.new_empty(L.shape, dtype=F64)


def _bald_setup(ctx, inputs, output):
    mean, L, Z, M = inputs
    ctx.save_for_backward(mean, L, Z)
    ctx.M = M


def _bald_bwd(ctx, dout):
    mean, L, Z = ctx.saved_tensors
    dmean, dL = torch.ops.bo.bald_backward(dout.contiguous(), mean, L, Z, ctx.M)
    return dmean, dL, None, None


bald.register_autograd(_bald_bwd, setup_context=_bald_setup)


# ---- bo::analytic (the analytic q = 1 family on the posterior moments) ---------------------------
def _analytic_dense(mean, var, best_f, mode, obj, w, beta, min_var, con_member, con_lower,
                    con_upper, con_kind):
    """The arguments of bo::analytic[_backward]_native after kernels.analytic_check's
    limits (a ValueError before any native call)."""
    if mean.dim() != 2 or tuple(var.shape) != tuple(mean.shape):
        raise ValueError("analytic: mean and var must be Mt x R each")
    cons = list(zip(con_member, con_lower, con_upper, con_kind))
    if not len(cons) == len(con_member) == len(con_lower) == len(con_upper) == len(con_kind):
        raise ValueError("analytic: the constraint lists must have one length")
    kernels.analytic_check(mean.shape[0], mode, obj, cons, min_var, w, beta)
    if mode <= kernels.AN_PI:
        if best_f is None or best_f.numel() not in (1, mean.shape[1]):
            raise ValueError(f"analytic: best_f must have 1 or R = {mean.shape[1]} entries")
        best_f = best_f.reshape(-1).contiguous()
    else:
        best_f = None
    return (mean.contiguous(), var.contiguous(), best_f, mode, obj, w, beta, min_var,
            list(con_member), list(con_lower), list(con_upper), list(con_kind))


@torch.library.custom_op("bo::analytic", mutates_args=(), device_types="cuda")
def analytic(mean: Tensor, var: Tensor, best_f: Optional[Tensor], mode: int, obj: int, w: float,
             beta: float, min_var: float, con_member: List[int], con_lower: List[float],
             con_upper: List[float], con_kind: List[int]) -> Tensor:
    """acq (R): the analytic acquisition ``mode`` (kernels.AN_*) of R rows from
    the members' posterior means and variances (Mt x R each) with the constraint
    table given as four lists (kernels.analytic).  Differentiable in mean and
    var."""
    return _lib.torch_ops().analytic_native(*_analytic_dense(
        mean, var, best_f, mode, obj, w, beta, min_var, con_member, con_lower, con_upper, con_kind))


@analytic.register_fake
def _(mean, var, best_f, mode, obj, w, beta, min_var, con_member, con_lower, con_upper, con_kind):
    return mean.new_empty((mean.shape[1],), dtype=F64)


@torch.library.custom_op("bo::analytic_backward", mutates_args=(), device_types="cuda")
def analytic_backward(dacq: Tensor, mean: Tensor, var: Tensor, best_f: Optional[Tensor], mode: int,
                      obj: int, w: float, beta: float, min_var: float, con_member: List[int],
                      con_lower: List[float], con_upper: List[float],
                      con_kind: List[int]) -> Tuple[Tensor, Tensor]:
    dmean, dvar = _lib.torch_ops().analytic_backward_native(dacq.contiguous(), *_analytic_dense(
        mean, var, best_f, mode, obj, w, beta, min_var, con_member, con_lower, con_upper, con_kind))
    return dmean, dvar


@analytic_backward.register_fake
def _(dacq, mean, var, best_f, mode, obj, w, beta, min_var, con_member, con_lower, con_upper,
      con_kind):
    return mean.new_empty(mean.shape, dtype=F64), mean.new_empty(mean.shape, dtype=F64)


def _analytic_setup(ctx, inputs, output):
    ctx.has_best_f = inputs[2] is not None
    ctx.save_for_backward(*[t for t in inputs[:3] if t is not None])
    ctx.consts = inputs[3:]


def _analytic_bwd(ctx, dacq):
    dmean = dvar = None
    if any(ctx.needs_input_grad[:2]):
        mean, var = ctx.saved_tensors[:2]
        best_f = ctx.saved_tensors[2] if ctx.has_best_f else None
        dmean, dvar = torch.ops.bo.analytic_backward(dacq.contiguous(), mean, var, best_f,
                                                     *ctx.consts)
    return (dmean, dvar) + (None,) * 10


analytic.register_autograd(_analytic_bwd, setup_context=_analytic_setup)


# ---- bo::saas_potential (the SAAS log-density and its gradient, for NUTS) -------------------------
@torch.library.custom_op("bo::saas_potential", mutates_args=(), device_types="cuda")
def saas_potential(z: Tensor, X: Tensor, y: Tensor,
                   work: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(U (C), grad (C x (d + 4)), status (C, int32)) of the SAAS potential at
    the rows of z over X (n x d), y (n) (kernels.saas_potential).  It returns its
    own gradient: no autograd."""
    kernels.saas_potential_check(X.shape[0], X.shape[1], z.shape[0])
    U, grad, status = _lib.torch_ops().saas_potential_native(
        z.contiguous(), X.contiguous(), y.contiguous(), work)
    return U, grad, status


@saas_potential.register_fake
def _(z, X, y, work=None):
    C = z.shape[0]
    return (z.new_empty((C,), dtype=F64), z.new_empty(z.shape, dtype=F64),
            z.new_empty((C,), dtype=torch.int32))


# ---- bo::icm_* (multi-task GP, intrinsic coregionalisation model: icm.hip) ---------------------
@torch.library.custom_op("bo::icm_covar", mutates_args=(), device_types="cuda")
def icm_covar(X: Tensor, task: Tensor, lengthscale: Tensor, B: Tensor, kind: int,
              outputscale: float, noise: float, noise_vec: Optional[Tensor] = None) -> Tensor:
    """The ICM training covariance outputscale kbar(X, X) * B[task, task] + diag(noise
    + noise_vec) as the padded np x np lower Cholesky input (identity pad)."""
    return kernels.icm_covar(X, task, lengthscale, B, kind, outputscale, noise, noise_vec)


@icm_covar.register_fake
def _(X, task, lengthscale, B, kind, outputscale, noise, noise_vec=None):
    np_ = _padded(X.shape[0])
    return X.new_empty(np_, np_, dtype=F64)


@torch.library.custom_op("bo::icm_mll_terms", mutates_args=(), device_types="cuda")
def icm_mll_terms(X: Tensor, task: Tensor, lengthscale: Tensor, B: Tensor, kind: int,
                  outputscale: float, L: Tensor, Ainv: Tensor, alpha: Tensor,
                  beta: Tensor) -> Tensor:
    """Row terms of the ICM marginal log likelihood, n x (d + 5 + T): bo_mll_terms'
    columns with the task covariance as a factor of every pair, then T task bins."""
    return kernels.icm_mll_partials(X, task, lengthscale, B, kind, outputscale, L, Ainv, alpha,
                                    beta)


@icm_mll_terms.register_fake
def _(X, task, lengthscale, B, kind, outputscale, L, Ainv, alpha, beta):
    return X.new_empty(X.shape[0], X.shape[1] + 5 + B.shape[0], dtype=F64)


@torch.library.custom_op("bo::icm_task_view", mutates_args=(), device_types="cuda")
def icm_task_view(U: Tensor, alpha: Tensor, task: Tensor, B: Tensor, t: int
                  ) -> Tuple[Tensor, Tensor, Tensor]:
    """(D U, (D U)^T, D alpha) with D = diag(B[t, task] / B[t, t]): the caches of
    output task t of a MultiTaskGP as the single-task posterior kernels read them."""
    return kernels.icm_task_view_arrays(U, alpha, task, B, t)


@icm_task_view.register_fake
def _(U, alpha, task, B, t):
    return U.new_empty(U.shape), U.new_empty(U.shape), alpha.new_empty(alpha.shape)


OPS: List[str] = ["sobol_normal", "gp_cache", "gp_cache_extend", "chol_jitter", "chol_backward",
                  "post_partials", "qmc_finalize", "gp_posterior", "gp_posterior_backward",
                  "qmc_acq", "qmc_acq_backward", "qehvi", "qehvi_backward", "mll", "kg",
                  "kg_backward", "paths_eval", "paths_eval_backward", "jes", "jes_backward", "mes",
                  "mes_backward", "gibbon", "gibbon_backward", "mv_quantiles", "nipv_gram",
                  "nipv_gram_backward", "bald", "bald_backward", "analytic", "analytic_backward",
                  "saas_potential", "fantasy_posterior", "fantasy_posterior_backward", "icm_covar",
                  "icm_mll_terms", "icm_task_view"]
