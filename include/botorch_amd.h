/*
 * botorch_amd -- C ABI of the MI355X (gfx950) GP-posterior + MC-acquisition
 * hot path.  Plain pointers and sizes only; every pointer argument named for
 * a tensor is a DEVICE pointer (HBM) unless documented as host; every `stream`
 * is a hipStream_t passed as void* (enqueue only -- the calls never
 * synchronise, except bo_gp_cache_build, which reads the Cholesky status back
 * once per jitter attempt, as the reference's psd_safe_cholesky does).
 *
 * All matrices are row-major fp64.  Return value: BO_OK (0) or a BO_ERR_*
 * code; bo_last_error() describes the last failure of the calling thread.
 *
 * The reference (anand-12/botorch @ 2024-10-08) is pure Python over
 * GPyTorch/linear_operator; it has no FFI.  Each entry point cites the
 * reference interface whose computation it replaces; INTEGRATION.md shows the
 * ctypes binding (botorch_amd/_lib.py) a maintainer adds on the reference side.
 */
#ifndef BOTORCH_AMD_H
#define BOTORCH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BO_ABI_VERSION 12

/* status codes */
#define BO_OK 0
#define BO_ERR_ARG 1
#define BO_ERR_HIP 2
#define BO_ERR_NOT_PSD 3 /* maps to NotPSDError (botorch/exceptions/errors.py) */
#define BO_ERR_NAN 4     /* maps to NanError */

/* kernel families (botorch/models/utils/gpytorch_modules.py:100-127,
 * botorch/models/fully_bayesian.py:81-92) */
#define BO_KIND_RBF 0
#define BO_KIND_MATERN52 1

/* bo_gemm_f64 flags: structure of the operands (zero regions are skipped) */
#define BO_GEMM_LOWER_C 1 /* write only C[m][n] with m >= n */
#define BO_GEMM_A_LOWER 2 /* op(A)[m][k] == 0 for k > m */
#define BO_GEMM_B_UPPER 4 /* op(B)[k][n] == 0 for k > n */
#define BO_GEMM_A_UPPER 8 /* op(A)[m][k] == 0 for k < m */
#define BO_GEMM_B_LOWER 16 /* op(B)[k][n] == 0 for k < n */

/* layouts of the stored R^T (BoPostPartialsArgs.rt_layout): row-major
 * (nC*128) x nrows_pad, or blocked in the posterior kernel's MFMA accumulator
 * order -- 16 x 16 blocks (training block kb, test block ib) at
 * (kb * nrows_pad / 16 + ib) * 256, element (k, i) of a block at
 * ((k % 16) / 4) * 64 + (k % 4) * 16 + i % 16 -- so every store and every
 * load of it is one 512-B segment per instruction.  bo_post_w_dx reads the
 * blocked layout; every other consumer (bo_post_w, bo_post_w_split,
 * bo_gemm_f64) the row-major one. */
#define BO_RT_ROWMAJOR 0
#define BO_RT_BLOCKED 1

/* qmc modes */
#define BO_QMC_POSTERIOR 0
#define BO_QMC_QEI 1
#define BO_QMC_QNEI 2
#define BO_QMC_CHOL 3 /* finalise + jittered q x q Cholesky only (no MC) */
#define BO_QMC_QLOGEI 4  /* qLogExpectedImprovement (acquisition/logei.py:137-234) */
#define BO_QMC_QLOGNEI 5 /* qLogNoisyExpectedImprovement, cached root (logei.py:236-507) */
/* The rest of the sample-reducing family (acquisition/monte_carlo.py:648-871).
 * They reuse the parameter slots of bo_qmc_finalize_v / bo_qmc_backward_v:
 *   mode      best_f           tau_relu   best_f_s
 *   QSR       ignored          ignored    ignored
 *   QPI       best_f           tau (> 0)  ignored
 *   QUCB      beta' =          ignored    zbar (q doubles, not NULL):
 *             sqrt(beta pi/2)             zbar[j] = mean_s Z[s][j]
 * (fat, tau_max, Tm, F, dF, acq_fwd are not read). */
#define BO_QMC_QSR 6  /* qSimpleRegret: mean_s max_a f */
#define BO_QMC_QPI 7  /* qProbabilityOfImprovement: mean_s max_a sigmoid((f - best_f) / tau) */
#define BO_QMC_QUCB 8 /* qUpperConfidenceBound: mean_s max_a (fbar_a + beta' |f_a - fbar_a|),
                       * fbar = mean_s f (the sample mean, as the reference's obj.mean(dim=0)) */

const char* bo_last_error(void);
int bo_version(void);

/* Hardware probe of the fp64 MFMA accumulator map; out: 64 x 8 doubles (the
 * layout the kernels assume, checked by tests/test_gpu_kernels.py).  The
 * timing/trace probes of the development tools are not part of this ABI: they
 * live in tools/bo_tools.h (tools/libbotorch_amd_tools.so, `make tools`). */
int bo_probe_mfma_f64_layout(double* out, void* stream);

/* Peak-rate probe: `blocks` x 256 threads, each wave issuing iters x 8
 * independent fp64 MFMAs (2048 flop each).  out: 1 double (kept live). */
int bo_probe_mfma_f64_rate(int blocks, int iters, double* out, void* stream);


/* Queue of the Cholesky task DAG for T = np/64 tile rows (HOST function, no
 * device work): 4 ints per task (type | fin << 8, k, j, i0 | i1 << 16) into
 * out (capacity cap tasks); returns the task count. */
int bo_chol_dag_tasks(int T, int* out, int cap);
/* The same queue with the A^{-1} tasks (bo_cholesky_inverse_ainv). */
int bo_chol_dag_tasks_ainv(int T, int* out, int cap);

/* Batched C = alpha op(A) op(B) + beta C on the fp64 matrix cores (strides sA,
 * sB, sC between batch members).  Building block of the Cholesky/inverse and
 * of the qNEI cross-covariance; replaces the dense torch.matmul calls inside
 * [G] linear_operator (e.g. MatmulLinearOperator under
 * botorch/models/gpytorch.py:446). */
int bo_gemm_f64(int transA, int transB, int M, int N, int K, double alpha, const double* A,
                int64_t lda, int64_t sA, const double* B, int64_t ldb, int64_t sB,
                double beta, double* C, int64_t ldc, int64_t sC, int batch, int flags,
                void* stream);

/* K[i][j] = outputscale * k(X1_i, X2_j) + diag_add * [i == j] over a rows x cols
 * extent with an identity pad beyond (n1, n2); mode bit 1 zeroes the strict
 * upper triangle.  X1: n1 x d, X2: n2 x d, lengthscale: d.
 * Replaces [G] RBFKernel/MaternKernel(+ScaleKernel).forward
 * (SingleTaskGP.forward, botorch/models/gp_regression.py:249-254). */
int bo_covar_matrix(int kind, const double* X1, int64_t n1, const double* X2, int64_t n2,
                    int d, const double* lengthscale, double outputscale, double diag_add,
                    int mode, double* K, int64_t ldk, int64_t rows, int64_t cols, void* stream);

/* Padded order np used by every n x n cache below (multiple of 128). */
int64_t bo_padded_order(int64_t n);

/* Two-level batched covariance (batch z = o * inner + i, o < outer, i < inner):
 * K[o][i] (n1 x n2, leading dim ldk, at K + o sKo + i sKi) =
 *   os[o soo + i soi] * k((X1[o][i] - X2[o][i]) / ls[o][i]),
 * X1 at X1 + o s1o + i s1i (n1 x d), X2 likewise, ls at ls + o slo + i sli (d).
 * Strides are in elements (0 = shared); d <= 512.  The SAAS ensemble's K*x of all M
 * members and K** of all M x B t-batches (models/fully_bayesian.py:276-281),
 * one launch each. */
int bo_covar_batched(int kind, const double* X1, int64_t s1o, int64_t s1i, int n1,
                     const double* X2, int64_t s2o, int64_t s2i, int n2, int d, const double* ls,
                     int64_t slo, int64_t sli, const double* os, int64_t soo, int64_t soi,
                     double* K, int64_t sKo, int64_t sKi, int64_t ldk, int outer, int inner,
                     void* stream);

/* In-place blocked Cholesky of the lower-stored SPD matrix A (np x np, upper
 * triangle zero) and its explicit inverse Linv (np x np).  work: np x np
 * scratch.  *info (device int) = 0 or the 1-based order of the first failing
 * leading minor (torch.linalg.cholesky_ex convention; a NaN pivot fails at its
 * own column).
 * Contract on the buffers (tests/test_gpu_chol_accuracy.py): the caller gives
 * A with a zero strict upper triangle and, for an order n < np, the identity
 * in rows and columns >= n; Linv may hold anything.  With info = 0 the call
 * has written every entry of Linv and leaves both A and Linv lower triangular
 * (strict upper triangle exactly zero) with the identity pad in rows and
 * columns >= n bit for bit, so Linv^T is usable over all np columns. */
int bo_cholesky_inverse(double* A, double* Linv, double* work, int64_t np, int* info,
                        void* stream);
/* bo_cholesky_inverse plus A^{-1} = L^{-T} L^{-1} (the lower 64 x 64 tiles,
 * diagonal tiles whole) in the SAME persistent launch (round 5): the MLL
 * gradient's tr(A^{-1} dK/dtheta) (botorch/optim/closures/model_closures.py:
 * 171-184 -> [G] ExactMarginalLogLikelihood's backward).  Its tile products run
 * as soon as the rows of L^{-1} they read are final, in the CUs the
 * factorisation's chain-bound tail leaves idle.  work >= (16 + 5 (np/64)^2)
 * 4-byte counters. */
int bo_cholesky_inverse_ainv(double* A, double* Linv, double* Ainv, double* work, int64_t np,
                             int* info, void* stream);

/* nb independent bo_cholesky_inverse problems in ONE persistent launch: A and
 * Linv hold nb np x np matrices back to back, info nb device ints, work >=
 * (16 + 4 nb (np/64)^2) * 4 bytes.  The matrices' task queues are interleaved,
 * so one matrix's diagonal chain overlaps the others' MFMA updates.  Results
 * are bit-identical to nb separate calls.  Replaces the per-output
 * factorisations of a batched multi-output GP ([G] batched
 * psd_safe_cholesky over the output batch, models/gpytorch.py:327-355) and of
 * a ModelListGP's members (models/model_list_gp_regression.py). */
int bo_cholesky_inverse_batched(double* A, double* Linv, double* work, int nb, int64_t np,
                                int* info, void* stream);

/* psd_safe_cholesky of one n x n matrix ([G] linear_operator, the ladder of
 * botorch/__init__.py:47): factor A + jitter I for jitter = 0, jitter0,
 * 10 jitter0, ... (max_tries increments).  L, Linv, work: np x np (identity
 * pad); jitter_used: HOST double.  Used for the joint posterior over the qNEI
 * baseline (acquisition/cached_cholesky.py:94-120, acquisition/utils.py:245-349). */
int bo_cholesky_jitter(const double* A, int64_t n, double* L, double* Linv, double* work,
                       int max_tries, double jitter0, double* jitter_used, int* info_dev,
                       void* stream);

/* Outcome of a batched jitter ladder (info, jitter: B entries from
 * bo_qmc_finalize_v / bo_chol_small): out[0] = max info (0: all factored),
 * out[1] = max jitter added.  One launch; the caller reads 16 bytes back, as
 * [G] psd_safe_cholesky's torch.any(info) check does. */
int bo_ladder_status(const int* info, const double* jitter, int64_t B, double* out, void* stream);

/* Pinned, device-mapped, coherent host memory (zeroed): *host for the CPU,
 * *dev for kernels -- the status words bo_qmc_finalize_v folds a ladder's
 * outcome into (BoQmcFinalizeArgs.status_out), read by the host after a
 * stream sync without a status launch or copy (a ModelListGP's members in
 * the qEHVI forward).  bo_pinned_free releases it. */
int bo_pinned_alloc(int64_t bytes, void** host, void** dev);
/* bo_qmc_finalize_v in BO_QMC_CHOL mode (mean + jittered q x q root) for
 * nm <= 8 models of one shape and kernel kind in ONE launch: per member its
 * rows Xq[m], partials Spart[m] / mpart[m] (nparts as BoQmcFinalizeArgs.nparts),
 * scalars and outputs; status_out (optional, with status_count) per member as
 * BoQmcFinalizeArgs.status_out; Tm / F (optional, with r, ldT, ldF): each
 * member's cached-root qNEHVI terms as BoQmcFinalizeArgs.Tm / F.  A
 * ModelListGP's members in the qEHVI / qNEHVI forward. */
int bo_qmc_finalize_members(int nm, int kind, int B, int q, const double* const* Xq,
                            const double* const* Spart, const double* const* mpart, int64_t n,
                            const double* outputscale, const double* constant, const double* ymean,
                            const double* ystd, int max_tries, double jitter0,
                            double* const* mean_out, double* const* L_out, int* const* info_out,
                            double* const* jitter_out, int nparts, double* const* status_out,
                            int* const* status_count, const double* const* Tm, int r,
                            int64_t ldT, const double* const* F, int64_t ldF, void* stream);
int bo_pinned_free(void* host);

/* Pareto masks of S point sets (Y: S x n x m, m <= 8; out: S x n bytes, 1 =
 * non-dominated): no other point is >= in every objective and > in one
 * (maximize; <= / < otherwise); dedup also drops later copies of equal points.
 * botorch/utils/multi_objective/pareto.py:16-64 over the S joint samples of
 * prune_inferior_points_multi_objective (acquisition/multi_objective/utils.py:77-161). */
int bo_pareto_mask(const double* Y, int64_t S, int n, int m, int maximize, int dedup,
                   unsigned char* out, void* stream);

/* Batched small psd_safe_cholesky (q <= 64), ladder applied per member
 * ([G] MultivariateNormal root_decomposition, posteriors/gpytorch.py:121-123).
 * A, L: B x q x q; info (B, nullable), jitter (B, nullable). */
int bo_chol_small(const double* A, int64_t B, int q, int max_tries, double jitter0, double* L,
                  int* info, double* jitter, void* stream);

/* K[b] = outputscale * k(X[b], X[b]) (+ diag_add I), X: B x q x d, K: B x q x q. */
int bo_covar_blocks(int kind, const double* X, int64_t B, int q, int d,
                    const double* lengthscale, double outputscale, double diag_add, double* K,
                    void* stream);

/* B = A^T for n x n matrices with leading dimension ld. */
int bo_transpose(const double* A, double* B, int64_t n, int64_t ld, void* stream);

/* y[i] = sum_k M[i][k] (x[k] - xshift), i, k < n. */
int bo_gemv(const double* M, int64_t ld, int64_t n, const double* x, double xshift, double* y,
            void* stream);
/* bo_gemv for a triangular M (uplo 1: lower, 2: upper), reading only the
 * triangle; bit-identical to bo_gemv on the same (zero-filled) matrix.  The
 * cache builds' beta = L^{-1}(y - c). */
int bo_gemv_tri(const double* M, int64_t ld, int64_t n, const double* x, double xshift, double* y,
                int uplo, void* stream);
/* y = M^T (x - xshift) for a lower-triangular M (y[c] = sum_{k >= c} M[k][c]
 * (x[k] - xshift)) read column-wise, without forming M^T: the caches' alpha =
 * L^{-T} beta = (K + s2 I)^{-1}(y - c), [G] mean_cache (botorch/models/
 * gpytorch.py:446; the MLL closure, optim/closures/model_closures.py:171-184,
 * forms no L^{-T}).  work >= bo_gemv_lt_work(n) doubles. */
int bo_gemv_lt_work(int64_t n, int64_t* work_elems);
int bo_gemv_lt(const double* M, int64_t ld, int64_t n, const double* x, double xshift, double* y,
               double* work, void* stream);

/* Xs[i][t] = (X[i][t] - center[t]) / lengthscale[t] for t < d, 0 for d <= t < dp
 * (center may be NULL). */
int bo_scale_inputs(const double* X, int64_t n, int d, const double* lengthscale,
                    const double* center, int dp, double* Xs, void* stream);

/* Exact-GP training caches of an eval-mode SingleTaskGP ([G]
 * DefaultPredictionStrategy.mean_cache / covar_cache, reached at
 * botorch/models/gpytorch.py:446 under gpt_posterior_settings,
 * botorch/models/utils/assorted.py:286-298):
 *   L = psd_safe_cholesky(K + noise I)   (jitter ladder: 0, then jitter0*10^i,
 *                                          i < max_tries; botorch/__init__.py:47)
 *   Linv = L^{-1},  U = L^{-T} (covar_cache),
 *   beta = L^{-1}(y - constant),  alpha = U beta (mean_cache).
 * Xt: n x d, y: n (standardized targets).  L, Linv, U: np x np device buffers,
 * beta, alpha: n.  jitter_used: HOST double (may be NULL).  info_dev: device int.
 * Returns BO_ERR_NOT_PSD when the ladder is exhausted. */
int bo_gp_cache_build(int kind, const double* Xt, int64_t n, int d, const double* lengthscale,
                      double outputscale, double noise, double constant, const double* y,
                      double* L, double* Linv, double* U, double* beta, double* alpha,
                      int max_tries, double jitter0, double* jitter_used, int* info_dev,
                      void* stream);
/* The same caches under a fixed-noise likelihood (SingleTaskGP with train_Yvar,
 * botorch/models/gp_regression.py:187-194 -> [G] FixedNoiseGaussianLikelihood):
 * K + diag(noise_vec), noise_vec: n observed variances (device, standardised
 * like the targets), then the same jitter ladder. */
int bo_gp_cache_build_fixed(int kind, const double* Xt, int64_t n, int d,
                            const double* lengthscale, double outputscale,
                            const double* noise_vec, double constant, const double* y, double* L,
                            double* Linv, double* U, double* beta, double* alpha, int max_tries,
                            double jitter0, double* jitter_used, int* info_dev, void* stream);

/* The caches of the n + k point model from those of the n point model, for
 * Model.condition_on_observations (botorch/models/gpytorch.py:468-531,
 * botorch/models/model.py:149 -> [G] ExactGP.get_fantasy_model), without
 * refactoring: the new factor is the old one with a k-row border,
 *   B = K(X2, X1) L^{-T},  S = K(X2, X2) + noise - B B^T,  L22 = chol(S),
 *   C = -L22^{-1} B L^{-1},
 *   L' = [[L, 0], [B, L22]],  Linv' = [[Linv, 0], [C, L22^{-1}]],  U' = Linv'^T,
 *   beta' = [beta; b2],  b2 = L22^{-1}(y2 - constant - B beta),
 *   alpha' = [alpha + C^T b2; L22^{-T} b2],
 * applied in blocks of <= 16 rows (O(n^2 k) flops, a few streaming passes over
 * L^{-1}).  The old caches (Xt_scaled: n x 8; L, Linv: leading dimension ld;
 * beta, alpha: n) are only read.  X_new: k x d (d <= 8, original scale), y_new:
 * k standardised targets, noise: the likelihood's variance, or noise_vec (k
 * observed variances, may be NULL) under a fixed-noise likelihood.  Outputs at
 * the new padded order np' = bo_padded_order(n + k), leading dimension ld_out
 * >= np': Xt_scaled_out (n + k) x 8, L_out / Linv_out / U_out np' rows, beta_out
 * / alpha_out n + k; every element of the np' x np' blocks is written, with
 * the identity pad and zero opposite triangle bo_gp_cache_build leaves.  work:
 * bo_gp_cache_extend_work(n, k) doubles.  info: device int the caller zeroes;
 * a non-positive pivot of S leaves its 1-based index there (no jitter ladder:
 * the caller then rebuilds with bo_gp_cache_build, and also when the old
 * caches were built with jitter).  Enqueue only.  L, Linv, their outputs,
 * U_out and work 16-B aligned, ld and ld_out even.  BO_ERR_ARG (nothing
 * launched) on k < 1, ld_out < np', a NULL or misaligned buffer, d > 8. */
int bo_gp_cache_extend_work(int64_t n, int k, int64_t* work_elems);
int bo_gp_cache_extend(int kind, const double* Xt_scaled, const double* L, const double* Linv,
                       const double* beta, const double* alpha, int64_t ld, int64_t n, int d,
                       const double* lengthscale, double outputscale, double constant,
                       const double* X_new, const double* y_new, int k, double noise,
                       const double* noise_vec, double* Xt_scaled_out, double* L_out,
                       double* Linv_out, double* U_out, double* beta_out, double* alpha_out,
                       int64_t ld_out, double* work, int* info, void* stream);

/* Geometry of the fused posterior kernels for B t-batches of q points (1 <= q
 * <= 16) over n training points: Qp = q rounded up to a power of two,
 * nrows_pad = roundup(B*Qp, 128) test rows, nC = ceil(n/128) column tiles.
 * Host pointers. */
int bo_post_geometry(int64_t B, int q, int64_t n, int* Qp, int* nrows_pad, int* nC);

/* Xq[(b*Qp + a)*8 + t] = X[b][a][t] / lengthscale[t] (X: B x q x d, d <= 8);
 * Xq: nrows_pad x 8. */
int bo_prepare_rows(const double* X, int B, int q, int d, const double* lengthscale,
                    double* Xq, void* stream);


/* K*x^T of the same call, np x nrows_pad (np = 128 nC): Kt[k][i] =
 * outputscale k(x_i, x_k), zero for k >= n and padding rows.  Passed to
 * bo_post_partials_v as Kt, the posterior kernel reads these values instead of
 * evaluating each one again for every column tile that covers it. */
int bo_post_kxt(int kind, const double* Xq, int B, int q, int d, const double* Xt_scaled,
                int64_t n, double outputscale, double* Kt, void* stream);

/* bo_prepare_rows and bo_post_kxt in one launch (ABI 11): Xq (nrows_pad x 8)
 * and Kt from X (B x q x d) and the lengthscale directly. */
int bo_post_kxt_rows(int kind, const double* X, int B, int q, int d, const double* lengthscale,
                     const double* Xt_scaled, int64_t n, double outputscale, double* Xq, double* Kt,
                     void* stream);

/* W^T = L^{-T} R^T = (K*x (K + s2 I)^{-1})^T for the posterior backward, np x
 * nrows_pad, from bo_post_partials_v's stored R^T (np x nrows_pad) and L^{-1}
 * (lower, ld ldl): the posterior kernel's MFMA tiles over the lower k-range
 * k >= c of each column (the second forward-size contraction of the gradient,
 * SURVEY.md 8(a) a14).  BO_ERR_ARG when the tile grid does not form 8 x 8
 * super-tiles (the caller then uses bo_gemm_f64). */
int bo_post_w(const double* Linv, int64_t ldl, const double* Rt, int B, int q, int64_t n,
              double* Wt, void* stream);
/* The same W^T under a stream-K plan (grids below four tiles per resident
 * slot, where the k-ranges [128 c, n) leave the one-pass grid imbalanced; no
 * super-tile condition).  bo_post_w_work: *kc_len = -1 and the workspace
 * doubles when the plan applies, else *kc_len = 0. */
int bo_post_w_work(int B, int q, int64_t n, int* kc_len, int64_t* work_elems);
int bo_post_w_split(const double* Linv, int64_t ldl, const double* Rt, int B, int q, int64_t n,
                    double* Wt, double* work, void* stream);
/* The same W^T of nm <= 8 models of one shape (a ModelListGP's members:
 * Linv[m], Rt[m], Wt[m]) in one stream-K launch + one reduction.
 * bo_post_w_members_work: the shared workspace in doubles, or -1 where the
 * one-model plan is not stream-K (then bo_post_w_split per model). */
int bo_post_w_members_work(int nm, int B, int q, int64_t n, int64_t* work_elems);
int bo_post_w_split_members(int nm, const double* const* Linv, int64_t ldl, const double* const* Rt,
                            int B, int q, int64_t n, double* const* Wt, double* work, void* stream);

/* The posterior backward without W: dX (B x q x d) of the posterior moments'
 * cotangents (dmean B x q, dcov B x q x q, standardised by ystd as in
 * bo_post_backward_v) from bo_post_partials_v's stored R^T and L^{-1}: the one-pass
 * W^T = L^{-T} R^T tiles of bo_post_w with the reduction dK*x = s dmean alpha^T
 * - G W (G_b = s^2 (dcov_b + dcov_b^T)) -> dX fused into their epilogue, W
 * never written; then the K** term and 1 / lengthscale (generation/gen.py:
 * 194-222 -> autograd through [G] exact prediction).
 * Rt in the BO_RT_BLOCKED layout (bo_post_partials_v with rt_layout =
 * BO_RT_BLOCKED).  work >= bo_post_w_dx_work doubles (nC x nrows_pad x 8 partials); a zero
 * size means the one-pass grid does not apply (stream-K plans: use
 * bo_post_w_split + bo_post_backward_v) and bo_post_w_dx returns BO_ERR_ARG. */
int bo_post_w_dx_work(int B, int q, int64_t n, int64_t* work_elems);
int bo_post_w_dx(int kind, const double* Linv, int64_t ldl, const double* Rt, int B, int q, int d,
                 int64_t n, const double* Xq, const double* Xt_scaled, const double* alpha,
                 const double* dmean, const double* dcov, const double* lengthscale,
                 double outputscale, double ystd, double* work, double* dX, void* stream);

/* Plan of bo_post_partials_v (host pointers): kc_len = 0 (one pass) or -1
 * (stream-K), whichever a k-step cost model of the triangular grid over
 * `slots` resident workgroups (slots <= 0: 512 = 256 CUs x 2) rates faster,
 * and the workspace size in doubles. */
int bo_post_split_plan(int64_t B, int q, int64_t n, int slots, int* kc_len,
                       int64_t* work_elems);
/* Workspace doubles of bo_post_partials_v under a given kc_len (0, -1 or a
 * chunk length). */
int bo_post_split_work(int64_t B, int q, int64_t n, int kc_len, int64_t* work_elems);
/* Route of the one-pass paired forward that reads K*x^T (kc_len = 0, Kt given,
 * no cross term, nC % 16 == 0 and nrows_pad / 128 % 8 == 0, BO_POST_PAIRED not
 * 0): 0 (default) the library's choice, -1 the 256-thread kernel, 1 the 8-wave
 * kernel (one 512-thread workgroup per 256 x 128 tile, U staged through LDS
 * two k-steps per barrier).  Every output is bit for bit the same on
 * both routes; every other shape and flag runs the 256-thread kernel.
 * bo_post_wide_applies: *out = 1 where a bo_post_partials_v call of that shape
 * would take the 8-wave kernel under the current mode (tests assert the route).
 * bo_post_wide_schedule (host): the 8-wave kernel's LDS schedule for one half
 * (0: waves 0-3, 1: waves 4-7) of a segment of nsteps k-steps walked ascending
 * (rev = 0) or descending, as rows of 6 ints (barrier interval, kind, step,
 * k-slice, LDS stage, first training row of the step) in program order; kind
 * 0 = a k-slice read, 1 = the U store of a step (slice -1), 2 = the slice's
 * MFMAs; interval -1 is the prologue in front of the first barrier.  Writes at
 * most `cap` rows; *n_events = the number of rows, *n_barriers = the barriers
 * every wave executes. */
int bo_post_set_wide(int mode);
int bo_post_wide_applies(int64_t B, int q, int64_t n, int kc_len, int has_cross, int has_kt,
                         int* out);
int bo_post_wide_schedule(int nsteps, int half, int rev, int cap, int* n_barriers, int* n_events,
                          int* events);

/* Small-grid forward posterior (round 5; replaces the stream-K split + split-k
 * reduction of small forward-only grids such as C2, the R R^T / R beta
 * contraction of [G] exact prediction, botorch/models/gpytorch.py:446 under
 * acquisition/monte_carlo.py:405-414): units of 32 test rows x a pair of
 * 32-column tiles of U = L^{-T} whose triangular k-ranges sum to a constant,
 * so every unit covers whole k-ranges and emits finished 16 x 16 partials.
 * bo_post_small_plan: *nparts = np / 64 partials per 16-row tile where the
 * library takes this route (BO_POST_SMALL: 0 never, 1 always, default where
 * the 128-tile plan would be stream-K), else 0.  bo_post_small: Kt = K*x^T
 * (np x nrows_pad, bo_post_kxt), U (ld ldu >= np), beta (n); writes Spart
 * (nparts x nrows_pad/16 x 16 x 16) and mpart (nparts x nrows_pad), the
 * bo_qmc_finalize_v inputs with nparts = *nparts, sym_parts = 0, and with Rt
 * non-null R^T row-major (np x nrows_pad) for the gradient's W^T routes. */
int bo_post_small_plan(int64_t B, int q, int64_t n, int* nparts);
int bo_post_small(const double* Kt, int64_t B, int q, int64_t n, const double* U, int64_t ldu,
                  const double* beta, double* Spart, double* mpart, double* Rt, void* stream);
/* nm <= 8 models of one shape (B, q, n, ldu) in ONE launch -- the members of
 * a ModelListGP (botorch/models/gpytorch.py:629-726: C4's three outputs), each
 * with its own K*x^T, U, beta and outputs (host arrays of device pointers; Rt
 * may be null, or hold nulls).  Rt[m]: R^T row-major (np x nrows_pad), the
 * gradient path's input to the W^T routes. */
int bo_post_small_batched(int nm, const double* const* Kt, const double* const* U,
                          const double* const* beta, double* const* Spart, double* const* mpart,
                          double* const* Rt, int64_t B, int q, int64_t n, int64_t ldu,
                          void* stream);
/* The same nm <= 8 models' partials where the one-model plan is stream-K
 * (C4: ModelListGP(3), n = 2048, q = 8, b = 128): ONE stream-K launch over
 * every member's 128 x 128 tiles plus one split-k reduction, replacing one
 * bo_post_partials_v per member (models/model_list_gp.py -> [G]
 * ModelListGP.posterior's per-model loop).  Spart[m] / mpart[m] hold nC
 * column-tile partials (bo_post_partials_v's layout); Rt[m] (optional) R^T
 * row-major; Xq0 any member's padded rows (bo_post_kxt_rows).
 * bo_post_members_work: the shared workspace in doubles, -1 where the
 * one-model plan is not stream-K (one launch per model then). */
int bo_post_members_work(int nm, int64_t B, int q, int64_t n, int64_t* work_elems);
/* bo_post_kxt_rows for nm <= 8 models of one shape and kernel kind sharing X
 * (lengthscale[m], Xt_scaled[m], outputscale[m] -> Xq[m], Kt[m]) in one
 * launch. */
int bo_post_kxt_rows_members(int nm, int kind, const double* X, int B, int q, int d,
                             const double* const* lengthscale, const double* const* Xt_scaled,
                             const double* outputscale, int64_t n, double* const* Xq,
                             double* const* Kt, void* stream);
int bo_post_partials_members(int nm, const double* const* Kt, const double* const* U,
                             const double* const* beta, double* const* Spart, double* const* mpart,
                             double* const* Rt, const double* Xq0, int64_t B, int q, int64_t n,
                             int64_t ldu, double* work, void* stream);
/* A^{-1} = L^{-T} L^{-1} for the MLL gradient (replaces the U U^T GEMM of
 * fit.py's closure, optim/closures/model_closures.py:171-184 -> [G]
 * ExactMarginalLogLikelihood backward): Linv np x np (ld = np = n rounded up
 * to 128, identity pad), Ainv np x np receives the lower tiles (tile row >=
 * tile column; diagonal tiles whole).  work >= bo_ainv_work doubles. */
int bo_ainv_work(int64_t n, int64_t* work_elems);
int bo_ainv(const double* Linv, int64_t ld, int64_t n, double* Ainv, double* work, void* stream);

/* A[r][c] = A[c][r] for r < c < n: the full symmetric A^{-1} from bo_ainv's
 * lower tiles (call with n = np so the identity pad is mirrored too). */
int bo_sym_lower(double* A, int64_t ld, int64_t n, void* stream);

/* Forward-only posterior partials of small grids through A^{-1} (the "quad"
 * plan, csrc/quad.hip): Sigma_b = K**_b - sum_{kb <= lb} (P + P^T) over 64 x 64
 * block pairs of the full symmetric A^{-1} = (K + s2 I)^{-1} (bo_ainv +
 * bo_sym_lower), mu_b = c + K*x alpha -- the same [G] exact_predictive_mean /
 * covar as bo_post_partials_v (models/gpytorch.py:405-466), linear in the blocks
 * of A^{-1}, so the units' partials are 16 x 16 blocks and no split-k
 * reduction runs; the pairs of one block row are taken in chunks of G (one
 * partial per chunk and row tile).  bo_post_quad_plan: *npairs = the partial
 * count (> 0) when the plan applies to (B, q, n) (opt-in: BO_POST_QUAD=auto
 * for stream-K geometries with n <= 2048 and <= 1024 pair units, =1 forces
 * it; unset / 0: the R route, measured as fast at C2; BO_QUAD_G sets the
 * chunk, default 1); the caller then sizes Spart as npairs x
 * nrows_pad/16 x 16 x 16 and mpart as npairs x nrows_pad and finalises with
 * BoQmcFinalizeArgs nparts = npairs, sym_parts = 1.  Kt: bo_post_kxt's K*x^T
 * (np x nrows_pad). */
int bo_post_quad_plan(int64_t B, int q, int64_t n, int* npairs);
int bo_post_quad(const double* Kt, const double* Ainv, int64_t lda, const double* alpha, int64_t B,
                 int q, int64_t n, double* Spart, double* mpart, void* stream);

/* The segment table of a split plan (host only; tests): up to cap segments as
 * 4 ints (ci | ii << 16, kbeg, kend, chunk or -1 = whole tile in place) and
 * up to wcap + 1 per-workgroup offsets; *nseg, *nwg receive the sizes. */
int bo_post_split_table(int64_t B, int q, int64_t n, int kc_len, int* segs, int cap, int* wg_off,
                        int wcap, int* nseg, int* nwg);


/* Kernel-matrix gradient for any d <= 128 (inputs in the original scale):
 *   dX[i][t] (+)= sum_k dK[i][k] d k(X_i, Y_k) / d X_it,
 * group > 0: row i pairs only with the `group` rows of its own block of Y
 * (dK row = group entries) -- the K** term of q-batches.  Generic-d path of
 * the posterior backward (SAAS, d = 50: models/fully_bayesian.py:509-546). */
int bo_kernel_grad(int kind, const double* X, int64_t rows, const double* Y, int64_t n, int d,
                   const double* lengthscale, double outputscale, const double* dK, int64_t ldk,
                   int group, int accumulate, double* dX, void* stream);

/* Exact-MLL terms for fit_gpytorch_mll (botorch/fit.py:75-258 ->
 * optim/closures/model_closures.py:171-184, [G] ExactMarginalLogLikelihood),
 * given bo_gp_cache_build's L, alpha, beta and Ainv = U U^T (lower triangle
 * read; ld = np).  partial: n x (d+5) per-row sums
 *   [0..d-1] sum_k w_ik W_ik outputscale g_ik (x_ij - x_kj)^2,   W = alpha alpha^T - Ainv
 *   [d]      W_ii        [d+1] sum_k w_ik W_ik kbar_ik   [d+2] log L_ii
 *   [d+3]    beta_i^2    [d+4] alpha_i          (w_ik = 2 for k < i, 1 for k = i)
 * from which the host forms the loss and its gradient in (ell, noise, constant,
 * outputscale) exactly. */
int bo_mll_terms(int kind, const double* X, int64_t n, int d, const double* lengthscale,
                 double outputscale, const double* L, const double* Ainv, int64_t ld,
                 const double* alpha, const double* beta, double* partial, void* stream);


/* Batched Cholesky backward (torch linalg.cholesky backward): L, dL (B x q x q,
 * lower) -> dA (B x q x q, symmetric), q <= 64. */
int bo_chol_backward(int B, int q, const double* L, const double* dL, double* dA, void* stream);

/* MC qEI / qNEI reduction of given samples (S x B x q):
 * acq[b] = mean_s max(max_a samples[s][b][a] - bf_s, 0), bf_s = best_f_s[s] or best_f. */
int bo_mc_reduce(int S, int B, int q, const double* samples, double best_f,
                 const double* best_f_s, double* acq, void* stream);

/* Scrambled Sobol N(0,1) samples, points skip..skip+n-1: out (n x dim).
 * state: dim x 30 int64 scrambled direction numbers, shift: dim int64
 * (torch.quasirandom.SobolEngine(dim, scramble=True, seed) state).
 * first_f32: the engine's first point was formed in float32 (torch's default
 * dtype at construction), so point 0 is rounded through float32 like it.
 * Replaces draw_sobol_normal_samples (botorch/utils/sampling.py:108-137). */
int bo_sobol_normal(const int64_t* state, const int64_t* shift, int dim, int64_t n,
                    int64_t skip, int first_f32, double* out, void* stream);

/* The scrambled engine state itself: state (dim x 30) and shift (dim) of
 * SobolEngine(dim, scramble=True, seed) from state0 (dim x 30, the unscrambled
 * direction numbers, torch._sobol_engine_initialize_state_) and bits (uint8,
 * 0/1): the engine's two draws from its seeded generator, in order -- dim x 30
 * shift bits, then dim x 30 x 30 matrix bits.  Replaces SobolEngine._scramble
 * (torch/quasirandom.py; torch._sobol_engine_scramble_), which the reference's
 * samplers run at every construction (sampling/qmc.py:56). */
int bo_sobol_scramble(int dim, const int64_t* state0, const uint8_t* bits, int64_t* state,
                      int64_t* shift, void* stream);


/* HOST: out[0..5] = V, IV, MAT, DS, IS, maximum m. */
int bo_lbfgsb_layout(int* out);
/* Profiling aid: subsequent bo_lbfgsb_step_v launches of at most `capacity`
 * restarts add each restart's phase times (wall-clock ticks: load, Cauchy
 * point, free set, formk, cmprlb, subsm, line search + update, store) into prof
 * (capacity x 8, device memory); larger launches are not profiled; NULL stops. */
int bo_lbfgsb_set_profile(unsigned long long* prof, int capacity);
/* Timing aid: 0 keeps every restart's working set in HBM; 1 (default) stages it
 * in LDS for each launch when it fits (8 (10 + 2m) n + 8 n bytes <= ~40 KB). */
int bo_lbfgsb_set_staging(int on);
/* Route of a single restart (B == 1, the joint problem of
 * gen_candidates_device(joint=True)): 0 (default) runs n >= 2048 on the
 * grid-wide kernel (one workgroup per 256 variables, the S / Y ring in LDS;
 * n <= 16384 and maxcor small enough for its LDS), 1 every single restart
 * that fits, -1 never (the one-workgroup kernel).  Same state layout. */
int bo_lbfgsb_set_grid(int mode);
/* Number of grid-wide L-BFGS-B launches this process has made (tests assert
 * the route). */
int64_t bo_lbfgsb_grid_launches(void);

/* HOST function (plain host pointers; no GPU involved): exact non-dominated
 * box decompositions of S point sets Y (S x n x m, maximisation) w.r.t. ref (m),
 * FastNondominatedPartitioning per set (botorch/utils/multi_objective/
 * box_decompositions/non_dominated.py:353-457, utils.py:103-288), padded with
 * empty all-zero cells to the common maximum K (box_decomposition_list.py:
 * 62-94).  *K_out receives K; with cell_lo / cell_hi NULL the call only sizes,
 * else they receive S x K_cap x m (BO_ERR_ARG if K > K_cap).  The per-sample
 * decompositions of qNEHVI (utils/multi_objective/hypervolume.py:680-700) run
 * on `nthreads` host threads. */
int bo_nd_partition_host(const double* Y, int64_t S, int64_t n, int m, const double* ref,
                         int64_t K_cap, int64_t* K_out, double* cell_lo, double* cell_hi,
                         int nthreads);

/* HOST function: bo_nd_partition_host's contract with NondominatedPartitioning's
 * binary partitioning instead (botorch/utils/multi_objective/box_decompositions/
 * non_dominated.py:81-192 + get_hypercell_bounds :248-335): cells that straddle
 * the front are halved until adjacent, and with alpha > 0 dropped once their
 * volume is at most alpha of the box around the front (the approximate
 * decomposition qNEHVI uses for alpha > 0, m > 2:
 * utils/multi_objective/hypervolume.py:606-612, 744-758). */
int bo_nd_partition_alpha_host(const double* Y, int64_t S, int64_t n, int m, const double* ref,
                               double alpha, int64_t K_cap, int64_t* K_out, double* cell_lo,
                               double* cell_hi, int nthreads);

/* HOST function (plain host pointers; no GPU involved): the hit-and-run chain
 * of sample_polytope (botorch/utils/sampling.py:219-309) over {y : A y <= b}
 * (A m x k row-major, b m), from y0 (k).  Step t moves along the unit direction
 * R[t] (n_tot x k) by lo + u[t] (hi - lo), [lo, hi] the feasible segment from
 * the slacks max(b - A y, 0) / AR[t] (AR = R A^T, n_tot x m, made by the caller
 * with torch as the reference makes it); after n0 burn-in steps every n_thin-th
 * point goes to out (n x k); n_tot must equal n0 + n * n_thin.  Replaces the
 * Python loop at sampling.py:278-308 that gen_batch_initial_conditions runs
 * under linear constraints (optim/initializers.py:365-375). */
int bo_hit_and_run_host(const double* A, const double* b, int64_t m, int64_t k, const double* y0,
                        const double* R, const double* AR, const double* u, int64_t n_tot,
                        int64_t n0, int64_t n_thin, double* out, int64_t n);

/* Scrambled Sobol raw designs in a box, points skip..skip+n-1: out (n x dim),
 * dim = q * d, out[i][j] = lower[j % d] + range[j % d] * u_i[j] (device
 * lower/range of length d).  Same engine state as bo_sobol_normal.
 * Replaces draw_sobol_samples (botorch/utils/sampling.py:66-105) in
 * gen_batch_initial_conditions (botorch/optim/initializers.py:350-362). */
int bo_sobol_box(const int64_t* state, const int64_t* shift, int dim, int64_t n, int64_t skip,
                 int first_f32, const double* lower, const double* range, int d, double* out,
                 void* stream);

/* ---- Parameter-struct entry points (ABI 9; ABI 10 adds rt_layout, ABI 11 the
 * quad-plan and fused-status fields of BoQmcFinalizeArgs; ABI 12 retires the
 * positional twins of the eight oldest launches) ------------------------------
 * The widest calls take one struct of named fields, so a binding declares a
 * record instead of a positional list of 20-33 arguments; the bo_<name>_v
 * function is the only entry point of such a launch.  Every struct opens with
 * struct_size = sizeof(struct) and abi_version = BO_ABI_VERSION; a mismatch
 * returns BO_ERR_ARG (never a misread field) before anything else runs.  The
 * comment on each record documents the launch and its fields. */
#define BO_STRUCT_HEADER \
  uint32_t struct_size;  \
  uint32_t abi_version

/* Fused K*x build + R^T = U^T K*x^T GEMM + R R^T / R beta epilogue
 * ([G] exact_predictive_mean / exact_predictive_covar under fast_pred_var,
 * botorch/models/gpytorch.py:446).  Xt_scaled: n x 8 lengthscale-scaled
 * training inputs; U: >= np x np with leading dim ldu; beta: n.
 * Spart: nC x (nrows_pad/16) x 16 x 16,  mpart: nC x nrows_pad.
 * Rt (nullable, gradient path): R^T, (nC*128) x nrows_pad.
 * kc_len = 0: one workgroup per (column tile, row tile), work unused;
 * kc_len > 0: split (every tile cut into chunks of kc_len training rows);
 * kc_len = -1: stream-K (the tiles' k-steps cut into one equal share per
 * resident slot).  Split plans reduce each cut tile's chunks in k order, with
 * `work` >= the work_elems of bo_post_split_plan / bo_post_split_work.
 * Qc (nullable, one-pass only): rq <= 16 rows (leading dim ldq >= n) whose
 * products with K*x are returned as nC column-tile partials
 * Cx[ci] (nC x rq x nrows_pad; sum over ci = Qc K*x^T) -- the
 * qNEI cross-covariance P_b R^T = Q_b K*x^T, Q_b = P_b U^T
 * (acquisition/cached_cholesky.py:94-120), without storing R.
 * Kt (nullable): K*x^T from bo_post_kxt (read instead of evaluated).
 *
 * The triangular operand (every entry point on the posterior kernel's 128 x
 * 128 tiles: bo_post_partials_v, bo_post_partials_members with U = L^{-T}
 * upper; bo_post_w*, bo_post_w_dx, bo_ainv with L^{-1} lower).  Column tile c
 * reads rows [0, 128 c + 128) of U (rows [128 c, n) of L^{-1}) and nothing
 * beyond.  Inside the tile's diagonal 128 x 128 block it multiplies only the
 * 16 x 16 blocks on or above the block diagonal (on or below, L^{-1}): the
 * 16 x 16 blocks on the zero side are loaded but never multiplied, so their
 * contents do not reach the result.  What the caller owes: the zero triangle
 * INSIDE the 16 x 16 diagonal blocks holds exact zeros, and rows / columns
 * >= n hold the identity pad.  bo_gp_cache_build*, bo_cholesky_inverse* and
 * bo_gp_cache_extend leave the whole opposite triangle zero. */
typedef struct BoPostPartialsArgs {
  BO_STRUCT_HEADER;
  int32_t kind, B, q, d;
  const double* Xq;
  const double* Xt_scaled;
  int64_t n;
  const double* U;
  int64_t ldu;
  const double* beta;
  double outputscale;
  double *Spart, *mpart, *Rt;
  int32_t kc_len, rq;
  double* work;
  const double* Qc;
  int64_t ldq;
  double* Cx;
  const double* Kt;
  int32_t rt_layout, _pad; /* ABI 10: BO_RT_ROWMAJOR or BO_RT_BLOCKED (the layout of Rt) */
} BoPostPartialsArgs;
int bo_post_partials_v(const BoPostPartialsArgs* a, void* stream);

/* Finalise the posterior of each t-batch and (mode != POSTERIOR) run the
 * fused q x q psd_safe_cholesky + reparameterised sampling + MC reduction:
 *   mean_out (B x q) = ymean + ystd (constant + R beta)
 *   cov_out (B x q x q) = ystd^2 (K** - R R^T)       [Standardize.untransform_posterior,
 *                                                     botorch/models/transforms/outcome.py:373-447]
 *   L_out (B x q x q), info_out (B), jitter_out (B)  [posteriors/gpytorch.py:85-126]
 *   acq (B): qEI  mean_s max_a relu(f - best_f)      [acquisition/monte_carlo.py:405-414]
 *            qNEI mean_s max_a relu(f - best_f_s[s])  [acquisition/monte_carlo.py:580-589]
 *            qLogEI / qLogNEI (best_f / best_f_s[s]):
 *              logmeanexp_s fatmax_a log_fatplus(f - best_f, tau_relu)   (fat != 0)
 *              logmeanexp_s smooth_amax_a log_softplus(f - best_f, tau_relu) (fat == 0)
 *              with the q-reduction at temperature tau_max
 *              [acquisition/logei.py:122, 219-234, 347-362, 509-534;
 *               utils/safe_math.py:209-352]; fat/tau_* are ignored by other modes
 *            qSR  mean_s max_a f                      [acquisition/monte_carlo.py:789-798]
 *            qPI  mean_s max_a sigmoid((f - best_f) / tau), tau in tau_relu   [:721-731]
 *            qUCB mean_s max_a (fbar_a + beta' |f_a - fbar_a|), fbar = mean_s f =
 *                 mean' + L_q zbar; beta' in best_f, zbar (q) in best_f_s       [:861-871]
 *            (the slots per mode: see BO_QMC_QSR above)
 * Z: S x q base samples (SobolQMCNormalSampler, sampling/normal.py:178-209).
 * Output pointers may be NULL when not needed (acq required for QEI/QNEI).
 * Cached-root qNEI (utils/low_rank.py:85-173, acquisition/cached_cholesky.py):
 * Tm (r x ldT) = L_rr^{-1} Sigma'(X_baseline, X) columns per padded test row,
 * F (S x ldF) = Z_baseline Tm; then Sigma'_qq <- Sigma'_qq - Tm^T Tm and
 * f = mean' + F + chol(.) Z (Z: the q new Sobol columns).  NULL otherwise. */
typedef struct BoQmcFinalizeArgs {
  BO_STRUCT_HEADER;
  int32_t kind, mode, B, q;
  const double *Xq, *Spart, *mpart;
  int64_t n;
  double outputscale, constant, ymean, ystd;
  const double* Z;
  int32_t S, max_tries;
  double best_f;
  const double* best_f_s;
  double jitter0;
  double *acq, *mean_out, *cov_out, *L_out;
  int* info_out;
  double* jitter_out;
  const double* Tm;
  int32_t r, fat;
  int64_t ldT;
  const double* F;
  int64_t ldF;
  double tau_relu, tau_max;
  /* ABI 11.  nparts: the number of partials in Spart / mpart (0: the column
   * tiles of bo_post_geometry); sym_parts = 1: the quad plan's partials
   * (bo_post_quad), summed as P + P^T.  status_out (2 doubles) + status_count
   * (one int, zero before the first call): the batch's [max info, max jitter]
   * of bo_ladder_status computed by the same launch (the last workgroup to
   * finish reduces them and re-zeroes the counter); null: not computed. */
  int32_t nparts, sym_parts;
  double* status_out;
  int32_t* status_count;
} BoQmcFinalizeArgs;
int bo_qmc_finalize_v(const BoQmcFinalizeArgs* a, void* stream);

/* Backward of the MC reduction + q x q Cholesky (gen_candidates_scipy's
 * autograd.grad, botorch/generation/gen.py:194-222):
 * dacq (B) -> dmean (B x q), dcov (B x q x q, symmetric) w.r.t. the outcome-
 * space posterior (mean', Sigma'), given mean' and L_q from bo_qmc_finalize_v.
 * mode: BO_QMC_QEI or BO_QMC_QNEI (best_f_s per sample).  torch semantics:
 * amax splits ties evenly, clamp_min(0) passes the gradient at >= 0.
 * qNEI (cached root, utils/low_rank.py:85-173): the forward samples include
 * F = Z_base T (S x ldF, rows b*Qp + a, as passed to bo_qmc_finalize_v); dF (same
 * layout) receives its cotangent, from which dT = Z_base^T dF.  F/dF may be
 * NULL for qEI.  Log modes (BO_QMC_QLOGEI / BO_QMC_QLOGNEI) also take the
 * forward values acq_fwd (B) and the forward's fat / tau_relu / tau_max; their
 * weights are dense over (sample, q) rather than one-hot.
 * BO_QMC_QSR / BO_QMC_QPI / BO_QMC_QUCB: one-hot weights as qEI (amax ties
 * split evenly; qPI's scaled by sigma (1 - sigma) / tau at the winning value,
 * ties taken among the sigmoid values as torch.amax sees them); qUCB also
 * carries the gradient through the sample mean,
 *   dL[a][j] = zbar[j] sum_s w + beta' sum_s w sgn(e) (Z[s][j] - zbar[j]),
 *   e = (L_q (z_s - zbar))[a], sgn(0) = 0.  Parameter slots as the forward's. */
typedef struct BoQmcBackwardArgs {
  BO_STRUCT_HEADER;
  int32_t mode, B, q, S;
  const double *mean, *Lq, *Z;
  double best_f;
  const double *best_f_s, *F;
  int64_t ldF;
  const double* dacq;
  double *dmean, *dcov, *dF;
  const double* acq_fwd;
  int32_t fat, _pad;
  double tau_relu, tau_max;
} BoQmcBackwardArgs;
int bo_qmc_backward_v(const BoQmcBackwardArgs* a, void* stream);

/* Backward of the batched exact posterior w.r.t. the candidates X (B x q x d):
 *   dK*x = ystd dmean alpha^T - G W,  G = ystd^2 (dcov + dcov^T),
 *   W = R L^{-1} (nrows_pad x ldw, rows b*Qp + a; w_kmajor != 0: W^T as
 *   bo_post_w writes it, np x ldw), dK** = ystd^2 dcov,
 *   + E (optional extra dK*x, nrows_pad x lde, same rows: the qNEI cross-
 *     covariance terms),
 * reduced through dk/dx.  Xq / Xt_scaled as for bo_post_partials_v.  W, alpha,
 * dmean, dcov and E may each be NULL (term absent); accumulate != 0 adds into
 * dX.  With Xt_scaled = the qNEI baseline points and only E, this is the
 * gradient through K(X_baseline, X).  Caches carry no gradient ([G]
 * detach_test_caches, botorch/models/utils/assorted.py:286-298). */
typedef struct BoPostBackwardArgs {
  BO_STRUCT_HEADER;
  int32_t kind, B, q, d;
  const double *Xq, *Xt_scaled;
  int64_t n;
  const double* W;
  int64_t ldw;
  const double *alpha, *dmean, *dcov, *E;
  int64_t lde;
  const double* lengthscale;
  double outputscale, ystd;
  int32_t accumulate, w_kmajor;
  double* dX;
} BoPostBackwardArgs;
int bo_post_backward_v(const BoPostBackwardArgs* a, void* stream);
/* njobs <= 16 posterior backward passes of one (B, q, d, kind) in one launch
 * (a ModelListGP's members, each with its training and baseline passes):
 * job j's dX (its dX / accumulate fields ignored) is written to dX_parts + j B q d;
 * the caller sums the slices. */
int bo_post_backward_jobs(int njobs, const BoPostBackwardArgs* const* jobs, double* dX_parts,
                          void* stream);

/* qEHVI over hypercells ([lo, hi] K x m from the non-dominated partitioning,
 * botorch/acquisition/multi_objective/monte_carlo.py:230-317) for B t-batches of
 * q points of an m-output independent model (ModelListGP):
 *   f[s][p][t] = mean[t][b][p] + sum_j L[t][b][p][j] Z[s][j m + t]
 *   acq[b] = mean_s sum_k inclusion-exclusion volume.
 * mean: m x B x q, L: m x B x q x q, Z: S x (q m).  2 <= m <= 4, q <= 12.
 * cell_stride 0: one set of K cells for every sample; > 0 (qNEHVI,
 * NoisyExpectedHypervolumeMixin, botorch/utils/multi_objective/hypervolume.py:
 * 507-835): sample s reads its own cells at cell_lo/hi + s * cell_stride (padded
 * with empty cells as BoxDecompositionList does).  F (nullable): the cached-root
 * baseline term added to f (m x S x ldF, output stride sF, row b * Qp + p).
 * The backward (autograd through _compute_qehvi,
 * multi_objective/monte_carlo.py:230-317): dacq (B) -> dmean (m x B x q) and
 * dL (m x B x q x q, lower) of the per-output posterior roots, and (with F)
 * dF (the cotangent of F, same layout) from which dT = Z_base^T dF. */
typedef struct BoQehviArgs { /* forward and backward (d* fields: backward only) */
  BO_STRUCT_HEADER;
  int32_t B, q, m, S;
  const double *mean, *L, *Z, *cell_lo, *cell_hi;
  int32_t K, Qp;
  int64_t cell_stride;
  const double* F;
  int64_t ldF, sF;
  double* acq;
  const double* dacq;
  double *dmean, *dL, *dF;
  /* ABI 11 (optional): a workspace lets the samples of each t-batch split
   * over several workgroups when B leaves CUs idle -- forward >= 2 B doubles,
   * backward >= 2 B m q (q + 3) / 2 */
  double* work;
  int64_t work_elems;
} BoQehviArgs;
int bo_qehvi_v(const BoQehviArgs* a, void* stream);
int bo_qehvi_backward_v(const BoQehviArgs* a, void* stream);

/* Feasibility-weighted qEHVI (outcome constraints: botorch/acquisition/
 * multi_objective/monte_carlo.py:245-251, 303-309; qNEHVI,
 * botorch/utils/multi_objective/hypervolume.py:725-767): every
 * inclusion-exclusion term of bo_qehvi_v is multiplied by prod_{p in T}
 * feas[s][b][p] (feas: S x B x q, the smoothed feasibility indicator of the
 * samples).  The model list has Mt >= m members, of which objective t is member
 * out_idx[t] (injective, any order): mean is Mt x B x q, L is Mt x B x q x q, F is
 * Mt x S x ldF, and objective t reads column j zm + out_idx[t] of a base-sample
 * row zld doubles wide (zm >= Mt, zld >= q zm), so no caller gathers anything.
 * The backward writes dmean / dL / dF at the objective members' slices only
 * (the rest is the caller's) and dfeas (S x B x q), the cotangent of feas,
 * formed without dividing by a weight. */
typedef struct BoQehviFeasArgs {
  BO_STRUCT_HEADER;
  int32_t B, q, m, S;
  const double *mean, *L, *Z, *cell_lo, *cell_hi;
  int32_t K, Qp;
  int64_t cell_stride;
  const double* F;
  int64_t ldF, sF;
  double* acq;
  const double* dacq;
  double *dmean, *dL, *dF;
  double* work; /* as BoQehviArgs: the sample split's workspace */
  int64_t work_elems;
  const double* feas;
  double* dfeas; /* backward only */
  int32_t Mt, zm;
  int64_t zld;
  int32_t out_idx[4];
} BoQehviFeasArgs;
int bo_qehvi_feas_v(const BoQehviFeasArgs* a, void* stream);
int bo_qehvi_feas_backward_v(const BoQehviFeasArgs* a, void* stream);

/* qLogEHVI / qLogNEHVI (botorch/acquisition/multi_objective/logei.py:147-310):
 * the log expected hypervolume improvement in log space.  Samples, cells, F and
 * the member map exactly as BoQehviFeasArgs (Mt >= m members, objective t is
 * member out_idx[t]; without constraint members Mt = m, out_idx = 0..m-1).  For
 * every sample, cell and non-empty subset T of the q <= 8 points,
 *   a_T = sum_t smin2(smin_{p in T} li[p][t], log(min(u_t, 1e10) - l_t))
 *         + sum_{p in T} logw[s][b][p],
 * li = log_fatplus (fat) or log_softplus of f - l at tau_relu, smin / smin2 =
 * fatmin (fat) or smooth_amin at tau_max; the odd and the even subsets are
 * summed in log space, differenced (logdiffexp), summed over the cells
 * (-> hvi[s][b]) and averaged over the samples (-> acq[b], a log value).  Cells
 * with a zero-length side are skipped.  logw (S x B x q, optional): the log
 * smoothed feasibility of the points.
 * Forward: writes acq (B) and hvi (S x B).  Backward: reads both, and dacq;
 * writes dmean / dL / dF at the objective members' slices only and, with logw,
 * dlogw (S x B x q).  work (optional, the sample split over workgroups):
 * forward >= 4 B doubles, backward >= 2 B m q (q + 3) / 2. */
typedef struct BoQlogehviArgs {
  BO_STRUCT_HEADER;
  int32_t B, q, m, S;
  const double *mean, *L, *Z, *cell_lo, *cell_hi;
  int32_t K, Qp;
  int64_t cell_stride;
  const double* F;
  int64_t ldF, sF;
  double* acq; /* forward: output; backward: the forward's value */
  double* hvi; /* S x B, likewise */
  const double* dacq;
  double *dmean, *dL, *dF;
  double* work;
  int64_t work_elems;
  const double* logw;
  double* dlogw; /* backward only, with logw */
  int32_t Mt, zm;
  int64_t zld;
  int32_t out_idx[4];
  int32_t fat, _pad;
  double tau_relu, tau_max;
} BoQlogehviArgs;
int bo_qlogehvi_v(const BoQlogehviArgs* a, void* stream);
int bo_qlogehvi_backward_v(const BoQlogehviArgs* a, void* stream);

/* Feasibility-weighted qEI / qLogEI / qNEI / qLogNEI over the Mt <= 8
 * single-output members of a model list (botorch/acquisition/monte_carlo.py:
 * 253-330, logei.py:219-234, utils/objective.py:134-180), q <= 16.  Layouts as
 * BoQehviFeasArgs with zm = Mt, zld = q Mt: mean Mt x B x q, L Mt x B x q x q
 * (lower triangle read), Z S x (q Mt) with column j Mt + t, F (optional)
 * Mt x S x ldF (member stride sF, rows b Qp + a).  Per sample and point
 *   f_t = mean + L z (+ F),  obj = sum_t c[t] f_t,
 *   con_i = sum_t A[i * 8 + t] f_t - rhs[i]   (i < k <= 8),
 *   l = sum_i logsig(-con_i / eta[i])  in this order; logsig = logexpit, or
 *       log_fatmoid with fat;
 *   plain: u_s = max_a relu(obj_a - bf_s) exp(l_a),            acq = mean_s u_s
 *   log:   u_s = q_reduce_a(log_soft_relu(obj_a - bf_s) + l_a), acq = logmeanexp_s u_s
 * (the smooth functions at tau_relu / tau_max, fat as for the constraints),
 * bf_s = best_f_s[s] if given, else best_f.  With feas (S x B x q; then k = 0)
 * the weights exp(l) (plain) or the log-weights l (log) are the caller's, and
 * the backward returns their cotangent dfeas.  Backward: from dacq (B), and in
 * log mode the forward's acq, writes dmean, dL (full q x q, upper zero), dF
 * (with F; entries of rows a < q) following torch autograd: amax shares the
 * cotangent evenly among all maximal entries (ties at 0 included), clamp_min
 * passes it where obj - bf >= 0.  No atomics; fixed summation order. */
typedef struct BoQmcFeasArgs {
  BO_STRUCT_HEADER;
  int32_t B, q, Mt, S;
  const double *mean, *L, *Z, *F;
  int64_t ldF, sF;
  int32_t Qp, k;
  double best_f;
  const double* best_f_s;
  double c[8], A[64], rhs[8], eta[8];
  const double* feas;
  double* dfeas; /* backward only, with feas */
  int32_t log, fat;
  double tau_relu, tau_max;
  double* acq; /* forward: output; backward (log): the forward's value */
  const double* dacq;
  double *dmean, *dL, *dF;
} BoQmcFeasArgs;
int bo_qmc_feas_v(const BoQmcFeasArgs* a, void* stream);
int bo_qmc_feas_backward_v(const BoQmcFeasArgs* a, void* stream);

/* One-shot knowledge gradient with the posterior mean as inner value
 * (botorch/acquisition/knowledge_gradient.py:151-207, models/model.py:328-407)
 * from packed posterior moments.  Restart b owns T tiles of q' = q_a + slots
 * rows: the q_a actual points, then `slots` fantasy solutions; fantasy i sits
 * in tile i / slots, row q_a + i % slots.  mean: B T q', cov: B T q' q'.
 *   A = cov[tile 0][:q_a, :q_a] + noise I,   L = psd_safe_cholesky(A)
 *   w_i = L^{-T} z_i                         (z_i: row i of Z, N_f x q_a)
 *   v_i = mean[row_i] + sum_j cov[row_i][j] w_ij   (j < q_a)
 *   values[b][i] = v_i,   acq[b] = mean_i v_i      (fixed summation order)
 * Only those entries of mean / cov are read.  The ladder is plain first, then
 * jitter0 10^k (k < max_tries) on the diagonal; info[b] (0: factored) and
 * jitter[b] (total added) are nullable; a failed restart's outputs are NaN.
 * L (B q_a q_a, upper zero) and W (B N_f q_a) are kept for the backward,
 * which from dacq (B) and optionally dvalues (B N_f) writes all of dmean and
 * dcov: with c_i = dacq[b] / N_f + dvalues[b][i], dmean[row_i] = c_i,
 * dcov[row_i][j] = c_i w_ij, the tile-0 q_a x q_a block the (symmetric)
 * Cholesky backward of dL = -tril(sum_i c_i w_i u_i^T), u_i = L^{-1} cov[row_i][:q_a],
 * and every other entry zero.  One workgroup per restart, one launch each way,
 * no atomics. */
typedef struct BoKgArgs {
  BO_STRUCT_HEADER;
  int32_t B, T, q_a, slots, N_f, max_tries;
  double noise, jitter0;
  const double *mean, *cov, *Z;
  double *acq, *values, *L, *W; /* forward: outputs; backward: L, W are inputs */
  int32_t* info;
  double* jitter;
  const double *dacq, *dvalues; /* backward only; dvalues nullable */
  double *dmean, *dcov;         /* backward only */
} BoKgArgs;
int bo_kg_v(const BoKgArgs* a, void* stream);
int bo_kg_backward_v(const BoKgArgs* a, void* stream);

/* Batched fantasy models (botorch/models/model.py:328-407 fantasize, then the
 * conditioned model's posterior) from packed posterior moments.  T-batch b owns
 * T tiles of q' = q_a + slots q rows: the q_a fantasised points, then `slots`
 * groups of q evaluation points; group g sits in tile g / slots at rows
 * q_a + (g % slots) q ... + q.  F = N_f groups (one per fantasy), or F = 1 with
 * `shared` (one group for all fantasies).  mean: B T q', cov: B T q' q'.
 *   A = cov[tile 0][:q_a, :q_a] + diag(noise_b),   L = psd_safe_cholesky(A)
 *   V_g = C_g L^{-T}            (C_g: the rows of group g, columns < q_a;  q x q_a)
 *   mean_out[b][f] = mean[rows of g_f] + V_{g_f} z_f   (g_f = f, or 0 when shared;
 *                                                       z_f: row f of Z, N_f x q_a)
 *   cov_out[b][g]  = D_g - V_g V_g^T                   (D_g: the group's own q x q
 *                                                       diagonal block, both triangles)
 * noise: q_a doubles per t-batch at stride noise_stride (0: one vector for all,
 * or q_a).  Only the lower triangle of tile 0's X x X block, each C_g and D_g
 * and the mean at the groups' rows are read.  The ladder is plain first, then
 * jitter0 10^k (k < max_tries) on the diagonal; info[b] (0: factored) and
 * jitter[b] (total added) are nullable; a failed t-batch's outputs are NaN.
 * mean_out: B N_f q, cov_out: B F q q; L (B q_a q_a, upper zero) and V (B F q
 * q_a) are kept for the backward, which from dmean_out and dcov_out (the
 * forward's shapes) writes every entry of dmean and dcov -- the groups' rows,
 * cross and diagonal blocks, the tile-0 X x X block the (symmetric) Cholesky
 * backward of dL = -tril(sum_rows dC_row^T V_row), dC = dV L^{-1}, dV_g =
 * sum_{f: g_f = g} dmean_out_f z_f^T - (dcov_out_g + dcov_out_g^T) V_g; zero
 * elsewhere -- and, when dZ is given, dZ[b][f] = V_{g_f}^T dmean_out[b][f] (B N_f
 * q_a; the caller sums over b).  One workgroup per t-batch, one launch each
 * way, sums in a fixed order, no atomics. */
typedef struct BoFantasyArgs {
  BO_STRUCT_HEADER;
  int32_t B, T, q_a, q, slots, N_f, shared, max_tries;
  double jitter0;
  int64_t noise_stride;
  const double *mean, *cov, *Z, *noise;
  double *mean_out, *cov_out, *L, *V; /* forward: outputs; backward: L, V are inputs */
  int32_t* info;
  double* jitter;
  const double *dmean_out, *dcov_out; /* backward only */
  double *dmean, *dcov, *dZ;          /* backward only; dZ nullable */
} BoFantasyArgs;
int bo_fantasy_posterior(const BoFantasyArgs* a, void* stream);
int bo_fantasy_posterior_backward(const BoFantasyArgs* a, void* stream);

/* Pathwise posterior samples (Matheron paths) of one single-output exact GP
 * (botorch/sampling/pathwise: features/generators.py:66-193, prior_samplers.py:
 * 52-106, update_strategies.py:72-135, posterior_samplers.py:198-224), S paths
 * evaluated at the R rows of X (R x d, original scale) in one launch.  With
 * theta_j(x) = sum_t Omega[j][t] x_t / lengthscale[t] and H = M / 2:
 *   g_s(x) = constant + sqrt(2 outputscale / M) sum_{j<H} (W[s][j] sin theta_j(x)
 *                                                        + W[s][H+j] cos theta_j(x))
 *            + sum_{i<n} V[s][i] outputscale k(x, Xt_i)
 *   f_s(x) = ymean + ystd g_s(x)
 * Omega: H x d frequencies, W: S x M prior weights, V: S x n update weights,
 * Xt_scaled: n x d training inputs divided by the lengthscale (row length d, no
 * padding); n = 0 switches the update term off (Xt_scaled, V may be null).
 *   inner = 0  (all):    out[s][r] = f_s(X_r),  out S x R, dout S x R
 *   inner >= 1 (mapped): out[r] = f_p(X_r), p = (r / inner) % S,  out R, dout R
 * Backward: dX[r][t] = sum_s dout[s][r] df_s/dx_t(X_r) over the paths of row r
 * (every entry of dX written); Omega, W and V get no gradient.
 * d <= 128 (a runtime loop), M even, fp64 throughout, sincos on the unreduced
 * phase.  The features and the kernel row of a 16-row tile live in registers:
 * no workspace, one launch each way, no atomics (repeated calls are bitwise
 * identical). */
typedef struct BoPathsArgs {
  BO_STRUCT_HEADER;
  int32_t kind, d, S, M;
  int64_t R, n, inner;
  const double *X, *lengthscale, *Xt_scaled, *Omega, *W, *V;
  double outputscale, constant, ymean, ystd;
  double* out;        /* forward */
  const double* dout; /* backward */
  double* dX;         /* backward */
} BoPathsArgs;
int bo_paths_eval_v(const BoPathsArgs* a, void* stream);
int bo_paths_eval_backward_v(const BoPathsArgs* a, void* stream);

/* qJointEntropySearch, lower bound (botorch/acquisition/joint_entropy_search.py:
 * 195-265): the mean over P optima (x*_j, f*_j) of the conditional entropies
 * of the R rows of X (R x d, original scale) in one launch.  The GP conditioned
 * on one pair is a rank-one correction of the current posterior, so with k the
 * kernel without its outputscale and V[j] = A^{-1} outputscale k(Xt, x*_j) (P x n):
 *   c_ij  = outputscale (k(x_i, x*_j) - sum_t k(x_i, Xt_t) V[j][t])
 *   mu_ji = mu[i] + c_ij g[j]       s2_ji = max(var[i] - c_ij^2 sinv[j], 1e-10)
 *   z     = (wf[j] - w mu_ji) / sqrt(s2_ji)
 *   r     = phi(z) / max(Phi(z), 1e-8),   Phi(z) = erfc(-z / sqrt 2) / 2
 *   vt_ji = s2_ji max(1 - (z + r) r, 1e-8) + tau2[j]
 *   out[i] = (1 / P) sum_j log(vt_ji) / 2
 * Xt_scaled (n x d) and Xopt_scaled (P x d) are divided by the lengthscale (row
 * length d, no padding); n = 0 switches the training term off (Xt_scaled, V may
 * be null).  g, sinv, wf, tau2: P per-optimum constants; mu, var: the current
 * posterior mean and variance of each row; w = +1 (maximize) or -1.
 * Backward, from dout (R): dX (R x d, through c_ij only), dmu (R), dvar (R);
 * every entry is written, the caller clears nothing.
 * d <= 128 (a runtime loop), P >= 1, R >= 1, fp64 throughout.  c_ij lives in
 * the MFMA accumulators: no R x P array, no workspace, one launch each way, no
 * atomics (repeated calls are bitwise identical). */
typedef struct BoJesArgs {
  BO_STRUCT_HEADER;
  int32_t kind, d, P, _pad;
  int64_t R, n;
  const double *X, *lengthscale, *Xt_scaled, *Xopt_scaled, *V;
  const double *g, *sinv, *wf, *tau2;
  const double *mu, *var;
  double outputscale, w;
  double* out;               /* forward */
  const double* dout;        /* backward */
  double *dX, *dmu, *dvar;   /* backward */
} BoJesArgs;
int bo_jes_v(const BoJesArgs* a, void* stream);
int bo_jes_backward_v(const BoJesArgs* a, void* stream);

/* Max-value entropy search (botorch/acquisition/max_value_entropy_search.py),
 * one t-batch of q = 1 per row, everything in outcome space.  mu, var: the
 * noiseless posterior mean and variance of each row (R); tau2 the observation
 * noise a noisy posterior adds; w = +1 (maximize) or -1; fstar (S_M) the
 * max-value samples in the w-signed space; CLAMP_LB = 1e-8;
 * Phi(x) = erfc(-x / sqrt 2) / 2.
 *
 * qMaxValueEntropy (lines 399-515 without fantasies or trace observations),
 * with z (S_m) the base samples shared by all rows:
 *   m = w mu   vM = max(var, 1e-8)   vm = var + tau2   t = vM / vm
 *   mean_new_k = m + t sqrt(vm) w z_k       s2n = max(vM - vM^2 / vm, 1e-8)
 *   Phin_jk = max(Phi((fstar_j - mean_new_k) / sqrt s2n), 1e-8)
 *   Phi0_j  = max(Phi((fstar_j - m) / sqrt vM), 1e-8)     Z_jk = Phin_jk / Phi0_j
 *   lp_k = -z_k^2 / 2 - log(2 pi vm) / 2    h1_jk = -Z_jk log Z_jk - Z_jk lp_k
 *   h0_k = -lp_k     H1bar = mean_jk h1     cov = mean_jk (h1 - H1bar)(h0_k - mean h0)
 *   beta = cov / sqrt(var_k(h0) var_jk(h1))   (both variances unbiased)
 *   out = H0 - H1bar + beta (mean_k h0 - H0),   H0 = log(2 pi e vm) / 2
 * The row-independent constants come from the host: kappa = mean_k h0 - H0 =
 * (mean z^2 - 1) / 2, var_h0 = var_k(z^2 / 2) and zsq_mean = mean z^2
 * (h0_k - mean h0 = (z_k^2 - zsq_mean) / 2).
 * Backward, from dout (R): dmu, dvar (R each), analytic; the clamps pass
 * gradient as torch.clamp_min does.  Every entry is written.
 * 1 <= S_M <= 1024, 2 <= S_m <= 4096, 1 <= R < 2^31.  One wave per row, the
 * pairs spread over its lanes; sums folded in a fixed order by lane exchanges:
 * no atomics, no workspace, no R x S_M x S_m array; repeated calls are bitwise
 * identical. */
typedef struct BoMesArgs {
  BO_STRUCT_HEADER;
  int32_t S_M, S_m;
  int64_t R;
  const double *mu, *var, *fstar, *z;
  double kappa, var_h0, zsq_mean, tau2, w;
  double* out;             /* forward */
  const double* dout;      /* backward */
  double *dmu, *dvar;      /* backward */
} BoMesArgs;
int bo_mes_v(const BoMesArgs* a, void* stream);
int bo_mes_backward_v(const BoMesArgs* a, void* stream);

/* qLowerBoundMaxValueEntropy, GIBBON (lines 537-664):
 *   vM = max(var, 1e-8)   vm = max(var + tau2, 1e-8)   rho2 = vM / vm
 *   gamma_j = (fstar_j - w mu) / sqrt vM    r_j = phi(gamma_j) / max(Phi(gamma_j), 1e-8)
 *   out = -mean_j log max(1 - rho2 r_j (gamma_j + r_j), 1e-8) / 2
 * and with m > 0 pending points, A (R x m) the noiseless posterior covariance of
 * each row with them and Binv (m x m) the inverse of their noisy covariance:
 *   qf = A Binv A^T    out += (log(max(vm, qf (1 + 1e-12)) - qf) - log vm) / 2
 * (on the clamped branch the gradient runs through qf, as torch.clamp with a
 * tensor bound does).  Backward, from dout (R): dmu, dvar (R) and dA (R x m),
 * every entry written; Binv is read as (Binv + Binv^T) / 2.
 * S_M >= 1, 0 <= m <= 15 (A, Binv, dA may be null at m = 0), 1 <= R < 2^34. */
typedef struct BoGibbonArgs {
  BO_STRUCT_HEADER;
  int32_t S_M, m;
  int64_t R;
  const double *mu, *var, *A, *Binv, *fstar;
  double tau2, w;
  double* out;                 /* forward */
  const double* dout;          /* backward */
  double *dmu, *dvar, *dA;     /* backward */
} BoGibbonArgs;
int bo_gibbon_v(const BoGibbonArgs* a, void* stream);
int bo_gibbon_backward_v(const BoGibbonArgs* a, void* stream);

/* The quantiles the Gumbel sampler of the max values fits (lines 983-1010):
 * out[q], q < 3, is the y with sum_i log Phi((y - mu_i) / sigma_i) = log p_q,
 * p = 0.25, 0.5, 0.75, for the N candidates' w-signed means and standard
 * deviations (sigma > 0).  One launch: a bisection on [min(mu - 3 sigma),
 * max(mu + 5 sigma)] (or on [lo, hi] when have_bounds is set) down to an
 * interval of four ulp, one workgroup per quantile.  status[q] (device int32) is
 * non-zero when the end points do not bracket the root; out[q] is then the
 * midpoint.  log Phi is evaluated tail-safe; a sum of -inf counts as below p. */
typedef struct BoMvQuantilesArgs {
  BO_STRUCT_HEADER;
  int32_t have_bounds, _pad;
  int64_t N;
  const double *mu, *sigma;
  double lo, hi;
  double* out;
  int32_t* status;
} BoMvQuantilesArgs;
int bo_mv_quantiles_v(const BoMvQuantilesArgs* a, void* stream);

/* qNegIntegratedPosteriorVariance (botorch/acquisition/active_learning.py:
 * 40-135): the Gram matrices of the posterior cross-covariance of every
 * t-batch of q rows of X (R x d, original scale, R = B q) with N integration
 * points, in one launch.  With k the kernel without its outputscale and
 * V[z] = A^{-1} outputscale k(Xt, z) (N x n):
 *   c(x_i, z) = outputscale (k(x_i, z) - sum_t k(x_i, Xt_t) V[z][t])
 *   G[b]      = C_b C_b^T  (q x q),  C_b = [c(x_i, z)]  (q x N), rows of t-batch b
 * The integrated posterior variance after observing X_b with noise tau2 is
 * mean_z var(z) - tr((Sigma(X_b, X_b) + tau2 I)^{-1} G[b]) / N.
 * Xt_scaled (n x d) and Z_scaled (N x d) are divided by the lengthscale (row
 * length d, no padding); n = 0 switches the training term off (Xt_scaled, V may
 * be null).  split: the number of slices of Z that separate workgroups take
 * (0: chosen by size; at most 1024, and never more than one slice per 16
 * points); their partial sums are added in slice order.
 * Backward, from dG (B x q x q, arbitrary, need not be symmetric): dX (R x d);
 * every entry is written, the caller clears nothing.
 * 1 <= q <= 16, q | R, d <= 128 (a runtime loop), N >= 1, fp64 throughout.
 * Neither C (R x N) nor the kernel rows (R x n) reach memory; with more than
 * one slice a stream-ordered workspace of split x B q q (forward) or split x
 * R d (backward) doubles is taken and returned.  No atomics (repeated calls
 * are bitwise identical). */
typedef struct BoNipvArgs {
  BO_STRUCT_HEADER;
  int32_t kind, d, q, split;
  int64_t R, n, N;
  const double *X, *lengthscale, *Xt_scaled, *Z_scaled, *V;
  double outputscale;
  double* G;          /* forward: (R / q) x q x q */
  const double* dG;   /* backward */
  double* dX;         /* backward: R x d */
} BoNipvArgs;
int bo_nipv_gram_v(const BoNipvArgs* a, void* stream);
int bo_nipv_gram_backward_v(const BoNipvArgs* a, void* stream);

/* qBayesianActiveLearningByDisagreement (botorch/acquisition/
 * bayesian_active_learning.py:52-126) over the Gaussian-mixture posterior of an
 * ensemble of M models at B t-batches of q points, in outcome space with the
 * observation noise in the covariances.  Row r = m B + b of mean (M B x q) and
 * L (M B x q x q, lower Cholesky roots, row-major; the upper triangle is not
 * read) is component m of t-batch b; Z (S x q) are the base samples all
 * components and t-batches share.  With y_ms = mu_m + L_m z_s and
 *   l_msm' = -|L_m'^{-1} (y_ms - mu_m')|^2 / 2 - sum_i log L_m',ii - (q / 2) log 2 pi
 *   H_b    = -(1 / (M S)) sum_{m,s} [logsumexp_m' l_msm' - log M]   (mixture entropy)
 *   C_bm   = mean_s |z_s|^2 / 2 + sum_i log L_m,ii + (q / 2) log 2 pi  (component entropy)
 *   out[b][m] = H_b - C_bm                                           (B x M)
 * The log-sum-exp runs online in registers (finite where exp underflows); the
 * means and roots of a t-batch sit in LDS, one workgroup per (b, m); nothing of
 * size M^2 S reaches memory.  Backward, from dout (B x M): dmean (M B x q) and dL
 * (M B x q x q; the lower triangle holds the gradient, the upper is zero), every
 * entry written, the caller clears nothing.
 * work: scratch of work_size doubles, at least B M (forward) or B M S
 * (backward: the per-sample log-sum-exp).
 * 1 <= M <= 64, 1 <= q <= 16, 1 <= S <= 2^20, B >= 1 with B M < 2^31, fp64.
 * Sums fold in a fixed order, no atomics: repeated calls are bitwise identical. */
typedef struct BoBaldArgs {
  BO_STRUCT_HEADER;
  int32_t M, q, S, _pad;
  int64_t B;
  const double *mean, *L, *Z;
  double* out;          /* forward: B x M */
  const double* dout;   /* backward: B x M */
  double *dmean, *dL;   /* backward: M B x q, M B x q x q */
  double* work;
  int64_t work_size;
} BoBaldArgs;
int bo_bald_v(const BoBaldArgs* a, void* stream);
int bo_bald_backward_v(const BoBaldArgs* a, void* stream);

/* The analytic q = 1 acquisition family (botorch/acquisition/analytic.py:
 * LogExpectedImprovement 357-420, LogConstrainedExpectedImprovement 528-608,
 * the helpers 960-1053 and 1182-1220) as one chain on the posterior moments,
 * one t-batch per row.  mean, var (Mt x R, row stride R, outcome space):
 * member j of row i at [j R + i].  With s2 = max(var[obj], min_var) (the floor
 * is taken where var <= min_var), sigma = sqrt(s2), bf = best_f[i best_f_stride]
 * and u = w (mean[obj] - bf) / sigma:
 *   BO_AN_LOG_EI  log_ei(u) + log sigma,  log_ei(u) = log(phi(u) + u Phi(u)):
 *                 u > -1: the logarithm of the sum; -1e6 < u <= -1:
 *                 log phi(u) + log1mexp(log(erfcx(-u / sqrt 2) |u|) + log sqrt(pi / 2));
 *                 u <= -1e6: log phi(u) - 2 log |u|
 *   BO_AN_EI      sigma (phi(u) + u Phi(u))
 *   BO_AN_LOG_PI  log Phi(u): log(erfc(-u / sqrt 2) / 2) for u >= 0,
 *                 log erfcx(-u / sqrt 2) - u^2 / 2 - log 2 below
 *   BO_AN_PI      Phi(u)
 *   BO_AN_UCB     w mean[obj] + sqrt(beta) sigma
 *   BO_AN_STD     w sigma
 * ncon <= BO_AN_CMAX constraints, each on its own member con_member[c] != obj
 * with standard deviation s_c (the same floor): kind BO_AN_CON_LOWER adds
 * log Phi((mean - lower) / s_c), BO_AN_CON_UPPER log Phi((upper - mean) / s_c),
 * BO_AN_CON_BOTH log(Phi(b) - Phi(a)), a = (lower - mean) / s_c, b = (upper -
 * mean) / s_c, taken on the left tail (a, b -> -b, -a when |b| > |a|), without
 * a difference of logarithms.  The sum of these log probabilities is added to the
 * two log modes; its exponential multiplies the other four.
 * Backward, from dacq (R): dmean, dvar (Mt x R), analytic; every element is
 * written (members no term reads get 0); on the floor dvar is 0.  With
 * r = Phi / phi = sqrt(pi / 2) erfcx(-u / sqrt 2): d log_ei / du = r / (1 + u r),
 * and for u < -5 the continued fraction -u + 2 / (-u + 3 / (-u + ...)) of the
 * same quantity, which has no cancellation; d log Phi / dx = 1 / r for x < 0.
 * Finite for |u| <= 1e100.
 * 1 <= Mt <= 16, 0 <= R < 2^38 (R = 0 returns at once), min_var > 0, w = +-1,
 * beta >= 0, best_f_stride 0 or 1, upper > lower on two-sided constraints.
 * One thread per row, 256-thread blocks, no LDS, no atomics, no workspace:
 * repeated calls are bitwise identical. */
#define BO_AN_CMAX 15
enum { BO_AN_LOG_EI = 0, BO_AN_EI = 1, BO_AN_LOG_PI = 2, BO_AN_PI = 3, BO_AN_UCB = 4,
       BO_AN_STD = 5 };
enum { BO_AN_CON_LOWER = 0, BO_AN_CON_UPPER = 1, BO_AN_CON_BOTH = 2 };
typedef struct BoAnalyticArgs {
  BO_STRUCT_HEADER;
  int32_t mode, Mt, obj, ncon;
  int32_t best_f_stride, _pad;
  int64_t R;
  const double *mean, *var, *best_f;
  double w, beta, min_var;
  int32_t con_member[BO_AN_CMAX + 1], con_kind[BO_AN_CMAX + 1];
  double con_lower[BO_AN_CMAX + 1], con_upper[BO_AN_CMAX + 1];
  double* acq;               /* forward: R */
  const double* dacq;        /* backward: R */
  double *dmean, *dvar;      /* backward: Mt x R */
} BoAnalyticArgs;
int bo_analytic_v(const BoAnalyticArgs* a, void* stream);
int bo_analytic_backward_v(const BoAnalyticArgs* a, void* stream);

/* The potential of the SAAS GP for NUTS (botorch/models/fully_bayesian.py:168-247,
 * SaasPyroModel.sample): U = -log p(z, Y) and dU/dz for C unconstrained vectors
 *   z = [log outputscale, mean, log g, log tau, log iota_1 .. log iota_d]   (C x (d + 4))
 * over the training data X (n x d, row-major) and y (n).  With os = e^z0, c = z1,
 * sigma^2 = 1e-4 + e^z2, w_j = e^z3 e^z(4+j) (inverse squared lengthscales),
 * r^2_ik = sum_j w_j (x_ij - x_kj)^2 and A = os Matern-5/2(r) + sigma^2 I:
 *   log p = log N(y | c 1, A) + Gamma(2, 0.15)(os) + N(0, 1)(c) + Gamma(0.9, 10)(e^z2)
 *           + HalfCauchy(0.1)(e^z3) + sum_j HalfCauchy(1)(e^z(4+j))
 *           + z0 + z2 + z3 + sum_j z(4+j)                     (the exp Jacobians)
 * n = 0 leaves the priors.  The gradient is closed-form: with alpha = A^{-1}(y - c),
 * W = alpha alpha^T - A^{-1}, Kbar the unit-outputscale kernel and
 * Kbar' = dKbar/dr^2 = -(5/6)(1 + sqrt5 r) e^{-sqrt5 r}:
 *   d ll/d z0 = os sum W Kbar / 2, d ll/d c = sum alpha, d ll/d z2 = e^z2 tr W / 2,
 *   d ll/d w_j = os sum_ik W_ik Kbar'_ik (x_ij - x_kj)^2 / 2, d/d z(4+j) = w_j times
 *   that and d/d z3 their sum; the priors' terms are added.
 * One workgroup per row of z: A, a blocked Cholesky (16 x 16 blocks, the
 * trailing updates on v_mfma_f64_16x16x4), L^{-1}, A^{-1} and the sums, in the
 * row's slice of work (bo_saas_potential_work doubles for the whole call).
 * status (C): 0 ok; 1 a non-finite input or a non-finite os, sigma^2, w_j or
 * result; 2 a non-positive or non-finite Cholesky pivot.  A row with status != 0
 * returns U = +inf and a zero gradient; the other rows are unaffected.
 * 0 <= n <= 1024, 1 <= d <= 256, C >= 1 with C n^2 < 2^31, fp64.  No atomics,
 * nothing shared between workgroups: repeated calls are bitwise identical and
 * row c of a C-row call equals the one-row call on that row. */
typedef struct BoSaasPotentialArgs {
  BO_STRUCT_HEADER;
  int32_t d, _pad;
  int64_t n, C;
  const double *X, *y, *z;
  double *U, *grad;      /* C, C x (d + 4) */
  int32_t* status;       /* C */
  double* work;
  int64_t work_size;
} BoSaasPotentialArgs;
int bo_saas_potential_v(const BoSaasPotentialArgs* a, void* stream);
/* HOST: doubles of work for a call of C rows. */
int bo_saas_potential_work(int64_t n, int d, int64_t C, int64_t* elems);

/* One function evaluation of the device-resident multi-start projected L-BFGS
 * (replaces scipy L-BFGS-B in gen_candidates_scipy, botorch/generation/gen.py:
 * 194-267).  B restarts of dimension n, history m (<= 32).  The caller fills
 * ft (B) / gt (B x n) with the objective (-acq) and its gradient at the trial
 * points xt; the step accepts (Armijo, c1) or backtracks, updates x / f / g
 * and the (S, Y, rho) ring, tests convergence (status: 1 projected gradient
 * <= pgtol, 2 relative decrease <= ftol, 3 step below min_alpha; -1 on the first
 * call = take xt as the start), and writes the next trial points to xt.
 * x, g, xt, gt, d: B x n; S, Y: B x m x n; f, alpha: B; rho: B x m;
 * hcount, hhead, status, nacc (accepted steps): B int32; lower, upper: n. */
typedef struct BoLbfgsStepArgs {
  BO_STRUCT_HEADER;
  int32_t B, n, m, _pad;
  double *x, *f, *g, *xt;
  const double *ft, *gt;
  double *d, *alpha, *S, *Y, *rho;
  int *hcount, *hhead, *status, *nacc;
  const double *lower, *upper;
  double c1, ftol, pgtol, min_alpha;
} BoLbfgsStepArgs;
int bo_lbfgs_step_v(const BoLbfgsStepArgs* a, void* stream);

/* One function evaluation of the device-resident multi-start L-BFGS-B: scipy
 * 1.15's L-BFGS-B (generalized Cauchy point, subspace minimisation with the
 * v3.0 projection, More-Thuente line search; the optimiser of
 * gen_candidates_scipy, botorch/generation/gen.py:252-267) as a reverse-
 * communication state machine, one 64-lane wave per restart.  The caller
 * writes ft (B) / gt (B x n) = objective and gradient at the trial points xt
 * (B x n); the call advances every restart to its next evaluation and
 * overwrites xt.  Zeroed state (v, iv, ws, wy, mat, ds, is) means "start at
 * xt".  ftol / pgtol / maxls / maxiter / maxfun are scipy's options of the same
 * names (m = maxcor <= 20).  Per restart: v = V x n doubles, iv = IV x n ints,
 * ws / wy = m x n, mat = MAT doubles, ds = DS doubles, is = IS ints, with
 * (V, IV, MAT, DS, IS) from bo_lbfgsb_layout; is[1] is the status (0 running,
 * 1 projected gradient <= pgtol, 2 relative reduction <= ftol, 3 abnormal line
 * search, 4 maxiter, 5 maxfun, 6 error), is[10] the iterations, ds[0] f and
 * v[0..n) x. */
typedef struct BoLbfgsbArgs {
  BO_STRUCT_HEADER;
  int32_t B, n, m, maxls, maxiter, maxfun;
  double ftol, pgtol;
  const double *lower, *upper;
  double* xt;
  const double *ft, *gt;
  double* v;
  int* iv;
  double *ws, *wy, *mat, *ds;
  int* is;
} BoLbfgsbArgs;
int bo_lbfgsb_step_v(const BoLbfgsbArgs* a, void* stream);

/* ---- Multi-task GP, intrinsic coregionalisation model (botorch/models/multitask.py:
 * 123-333): k((x, a), (x', b)) = outputscale kbar(x, x') B[a][b] over T tasks, B = F F^T +
 * diag(v) (T x T, row-major), task[i] in [0, T) the task of training point i (the
 * caller checks the range; the kernels clamp it, so a bad index reads no other
 * memory).  X: n x d WITHOUT the task column.  Added within ABI 12 (plain names, as
 * bo_fantasy_posterior).  1 <= T <= BO_ICM_MAX_TASKS, 1 <= d <= BO_ICM_MAX_DIM, kind
 * RBF or Matern-5/2; fp64; no atomics, sums in a fixed order. */
#define BO_ICM_MAX_TASKS 16
#define BO_ICM_MAX_DIM 64

/* A[i][k] = outputscale kbar(x_i, x_k) B[task_i][task_k] + (i == k)(noise + noise_vec[i])
 * for k <= i < n, zeros above the diagonal, the identity on rows / columns >= n:
 * the np x np input bo_cholesky_inverse / bo_cholesky_inverse_ainv factorise in
 * place (np = bo_padded_order(n)).  noise_vec (n) is nullable; `noise` carries the
 * homoskedastic noise and / or a ladder's jitter. */
typedef struct BoIcmCovarArgs {
  BO_STRUCT_HEADER;
  int32_t kind, d, T, _pad;
  int64_t n, np;
  const double *X, *lengthscale, *B;
  const int32_t* task;
  const double* noise_vec;
  double outputscale, noise;
  double* A;
} BoIcmCovarArgs;
int bo_icm_covar(const BoIcmCovarArgs* a, void* stream);

/* bo_mll_terms for the ICM covariance: one pass over the lower triangle, one
 * workgroup per row i, with W_ik = alpha_i alpha_k - A^{-1}_ik, w = 2 off the
 * diagonal, B_ik = B[task_i][task_k].  partial: n x (d + 5 + T),
 *   [0..d-1] sum_k w W_ik outputscale B_ik g_ik (x_ij - x_kj)^2   (d ll/d ls_j = 1/2 . / ls_j^3)
 *   [d] W_ii        [d+1] sum_k w W_ik kbar_ik B_ik        [d+2] log L_ii
 *   [d+3] beta_i^2  [d+4] alpha_i
 *   [d+5+b] sum_{k <= i, task_k = b} w W_ik outputscale kbar_ik   (row i's bins of d ll/d B)
 * The host folds the bins into Gl[task_i][b] and symmetrises: G = (Gl + Gl^T) / 2,
 * d ll/d B = G / 2.  L, Ainv (lower part read): leading dimension ld. */
typedef struct BoIcmMllArgs {
  BO_STRUCT_HEADER;
  int32_t kind, d, T, _pad;
  int64_t n, ld;
  const double *X, *lengthscale, *B;
  const int32_t* task;
  double outputscale;
  const double *L, *Ainv, *alpha, *beta;
  double* partial;
} BoIcmMllArgs;
int bo_icm_mll_terms(const BoIcmMllArgs* a, void* stream);

/* The prediction caches of output task t as a single-task model sees them: with
 * D = diag(B[t][task_j] / B[t][t]) (1 on the padding),
 *   U_out = D U,  Linv_out = U_out^T,  alpha_out = D alpha;
 * together with outputscale' = outputscale B[t][t] and the unchanged beta, constant
 * and scaled inputs, the posterior kernels compute task t's exact posterior.  D may
 * hold zeros and negative entries, so there is no factor L for this view.  U, U_out,
 * Linv_out: np x np (U_out apart from U); B[t][t] > 0 is the caller's to ensure. */
typedef struct BoIcmTaskViewArgs {
  BO_STRUCT_HEADER;
  int32_t T, t;
  int64_t n, np;
  const double* B;
  const int32_t* task;
  const double *U, *alpha;
  double *U_out, *Linv_out, *alpha_out;
} BoIcmTaskViewArgs;
int bo_icm_task_view(const BoIcmTaskViewArgs* a, void* stream);

/* HOST: sizeof the named record ("BoPostPartialsArgs", ...), -1 if unknown --
 * lets a binding check its declared layout once at load time. */
int64_t bo_struct_size(const char* name);

#ifdef __cplusplus
}
#endif

#endif /* BOTORCH_AMD_H */
