// Intrinsic coregionalisation model (ICM) multi-task GP: the long-format exact
// GP of botorch/models/multitask.py:123-333 whose kernel is
//   k((x, a), (x', b)) = outputscale kbar(x, x') B[a][b],   B = F F^T + diag(v)
// over T <= BO_ICM_MAX_TASKS tasks, tau_i the task of training point i.
//
//   icm_covar_kernel      A = outputscale kbar B[tau, tau] + diag(noise), straight
//                         into the padded lower workspace bo_cholesky_inverse*
//                         factorises in place (strict upper zero, identity pad)
//   icm_mll_terms_kernel  mll.hip's one pass over the lower triangle with B[tau_i,
//                         tau_k] as an extra factor per pair, plus T task bins per
//                         row for d ll / d B
//   icm_task_view_kernel  the caches of one output task t: U' = D U, L^{-1}' = U'^T,
//                         alpha' = D alpha with D = diag(B[t][tau_j] / B[t][t]); with
//                         outputscale' = outputscale B[t][t] the single-task posterior
//                         kernels then compute task t's posterior exactly
//
// No atomics, every sum in a fixed order: repeated calls are bitwise identical.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAXD = BO_ICM_MAX_DIM;
constexpr int MAXT = BO_ICM_MAX_TASKS;
constexpr int CV_ROWS = 8;  // rows of A per workgroup (x 256 columns)

__device__ __forceinline__ int clamp_task(int t, int T) { return t < 0 ? 0 : (t >= T ? T - 1 : t); }

// A workgroup takes CV_ROWS rows x 256 columns, as covar_matrix_kernel does: the
// rows' scaled inputs and tasks, the reciprocal lengthscales and B sit in LDS,
// each thread reuses its column's input for all rows.  Workgroups wholly above
// the diagonal only write zeros.
template <int KIND>
__global__ __launch_bounds__(THREADS) void icm_covar_kernel(
    const double* __restrict__ X, int64_t n, int d, const double* __restrict__ ls,
    const int32_t* __restrict__ task, const double* __restrict__ B, int T, double outputscale,
    double noise, const double* __restrict__ noise_vec, double* __restrict__ A, int64_t np) {
  __shared__ double invl[MAXD], xi[CV_ROWS][MAXD], Bs[MAXT * MAXT];
  __shared__ int ti[CV_ROWS];
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * THREADS + tid;
  const int64_t i0 = (int64_t)blockIdx.y * CV_ROWS;
  if (tid < d) invl[tid] = 1.0 / ls[tid];
  if (tid < T * T) Bs[tid] = B[tid];
  if (tid < CV_ROWS) ti[tid] = (i0 + tid < n) ? clamp_task(task[i0 + tid], T) : 0;
  __syncthreads();
  for (int e = tid; e < CV_ROWS * d; e += THREADS) {
    const int r = e / d, t = e - r * d;
    xi[r][t] = (i0 + r < n) ? X[(i0 + r) * d + t] * invl[t] : 0.0;
  }
  __syncthreads();
  if (j >= np) return;
  const bool jv = j < n;
  double d2[CV_ROWS];
#pragma unroll
  for (int r = 0; r < CV_ROWS; ++r) d2[r] = 0.0;
  int tj = 0;
  if (jv && i0 < n && j <= i0 + CV_ROWS - 1) {  // some row of this workgroup has j <= i
    tj = clamp_task(task[j], T);
    for (int t = 0; t < d; ++t) {
      const double v = X[j * d + t] * invl[t];
#pragma unroll
      for (int r = 0; r < CV_ROWS; ++r) {
        const double diff = xi[r][t] - v;
        d2[r] = fma(diff, diff, d2[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < CV_ROWS; ++r) {
    const int64_t i = i0 + r;
    if (i >= np) break;
    double val;
    if (i >= n || !jv) {
      val = (i == j) ? 1.0 : 0.0;
    } else if (j > i) {
      val = 0.0;
    } else {
      val = outputscale * kernel_from_d2<KIND>(d2[r]) * Bs[ti[r] * T + tj];
      if (i == j) val += noise_vec ? noise_vec[i] + noise : noise;
    }
    A[i * np + j] = val;
  }
}

// One workgroup per row i (its task fixed).  partial[i], d + 5 + T doubles:
//   [0..d-1] sum_k w W_ik os B_ik g_ik Delta_ikj^2    [d]   W_ii
//   [d+1]    sum_k w W_ik kbar_ik B_ik               [d+2] log L_ii
//   [d+3]    beta_i^2                                [d+4] alpha_i
//   [d+5+b]  sum_{k <= i, tau_k = b} w W_ik os kbar_ik            (w = 2 off-diagonal)
// DC: compile-time input dimension (0 = runtime d <= MAXD); NT: task bins held per
// thread (T <= NT), each in a register of its own: a pair adds to the bin of its
// task by a select per bin, never by a dynamic index.
template <int KIND, int DC, int NT>
__global__ __launch_bounds__(THREADS) void icm_mll_terms_kernel(
    const double* __restrict__ X, int n, int d_rt, const double* __restrict__ ls,
    const int32_t* __restrict__ task, const double* __restrict__ B, int T, double outputscale,
    const double* __restrict__ L, const double* __restrict__ Ainv, int64_t ld,
    const double* __restrict__ alpha, const double* __restrict__ beta,
    double* __restrict__ partial) {
  const int d = DC > 0 ? DC : d_rt;
  constexpr int NA = DC > 0 ? DC : MAXD;
  __shared__ double red[THREADS / 64][MAXD + 1 + MAXT];
  __shared__ double sl[MAXD], Bi[MAXT];
  const int i = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < d) sl[tid] = 1.0 / ls[tid];
  if (tid < T) Bi[tid] = B[clamp_task(task[i], T) * T + tid];
  __syncthreads();
  double acc[NA], bin[NT];
#pragma unroll
  for (int t = 0; t < NA; ++t) acc[t] = 0.0;
#pragma unroll
  for (int b = 0; b < NT; ++b) bin[b] = 0.0;
  double acc_os = 0.0;
  const double ai = alpha[i];
  const double* xi = X + (int64_t)i * d;
  for (int k = tid; k <= i; k += THREADS) {
    const double* xk = X + (int64_t)k * d;
    double r2 = 0.0;
    for (int t = 0; t < d; ++t) {
      const double df = (xi[t] - xk[t]) * sl[t];
      r2 = fma(df, df, r2);
    }
    const int tk = clamp_task(task[k], T);
    const double Bik = Bi[tk];
    const double W = ai * alpha[k] - Ainv[(int64_t)i * ld + k];
    const double w = (k == i) ? W : 2.0 * W;
    double kbar, g;  // unit-outputscale kernel value; dk/dell_j = outputscale g Delta_j^2 / ell_j^3
    if (KIND == BO_RBF) {
      kbar = exp(-0.5 * r2);
      g = kbar;
    } else {
      const double r = sqrt(r2);
      const double s5r = 2.23606797749978969641 * r;
      const double e = exp(-s5r);
      kbar = (1.0 + s5r + (5.0 / 3.0) * r2) * e;
      g = (5.0 / 3.0) * (1.0 + s5r) * e;
    }
    const double wg = w * g * outputscale * Bik;
    for (int t = 0; t < d; ++t) {
      const double df = xi[t] - xk[t];
      acc[t] = fma(wg, df * df, acc[t]);
    }
    const double wk = w * kbar;
    acc_os = fma(wk, Bik, acc_os);
    const double wb = wk * outputscale;
#pragma unroll
    for (int b = 0; b < NT; ++b) bin[b] += (tk == b) ? wb : 0.0;
  }
  // wave sums by shuffles, then the four waves in LDS: slots [0, d) lengthscales,
  // d the outputscale term, d + 1 + b the bins
  for (int t = 0; t < d; ++t) {
    const double v = wave_sum(acc[t]);
    if ((tid & 63) == 0) red[tid >> 6][t] = v;
  }
  {
    const double v = wave_sum(acc_os);
    if ((tid & 63) == 0) red[tid >> 6][d] = v;
  }
#pragma unroll
  for (int b = 0; b < NT; ++b) {
    if (b < T) {
      const double v = wave_sum(bin[b]);
      if ((tid & 63) == 0) red[tid >> 6][d + 1 + b] = v;
    }
  }
  __syncthreads();
  double* out = partial + (int64_t)i * (d + 5 + T);
  if (tid <= d + T) {
    double v = 0.0;
    for (int w = 0; w < THREADS / 64; ++w) v += red[w][tid];
    if (tid < d) out[tid] = v;
    else if (tid == d) out[d + 1] = v;
    else out[d + 5 + (tid - d - 1)] = v;
  }
  if (tid == 0) {
    out[d] = ai * ai - Ainv[(int64_t)i * ld + i];
    out[d + 2] = log(L[(int64_t)i * ld + i]);
    out[d + 3] = beta[i] * beta[i];
    out[d + 4] = ai;
  }
}

// One pass over U in 32 x 32 tiles: U'[j][c] = D_j U[j][c] to U_out and, through
// an LDS transpose, to Linv_out[c][j]; tiles strictly below U's diagonal are
// written as zeros without a read.  D_j = B[t][tau_j] / B[t][t] for j < n and 1
// on the padding, so the identity pad is copied as the cache build left it.
// The tiles of the first tile column also write alpha' = D alpha.
__global__ __launch_bounds__(256) void icm_task_view_kernel(
    const double* __restrict__ U, const double* __restrict__ alpha,
    const int32_t* __restrict__ task, const double* __restrict__ B, int T, int t, int64_t n,
    int64_t np, double* __restrict__ U_out, double* __restrict__ Linv_out,
    double* __restrict__ alpha_out) {
  __shared__ double tile[32][33];
  __shared__ double D[32];
  const int64_t bx = (int64_t)blockIdx.x * 32, by = (int64_t)blockIdx.y * 32;
  const int tx = threadIdx.x, ty = threadIdx.y;  // 32 x 8
  if (ty == 0) {
    const int64_t gi = by + tx;
    D[tx] = (gi < n) ? B[t * T + clamp_task(task[gi], T)] / B[t * T + t] : 1.0;
  }
  __syncthreads();
  const bool zero = by > bx;  // U is upper triangular
  for (int r = ty; r < 32; r += 8) {
    const int64_t gi = by + r, gj = bx + tx;  // np is a multiple of 32: always inside
    const double v = zero ? 0.0 : D[r] * U[gi * np + gj];
    U_out[gi * np + gj] = v;
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int64_t gi = bx + r, gj = by + tx;
    Linv_out[gi * np + gj] = tile[tx][r];
  }
  if (blockIdx.x == 0 && ty == 0) {
    const int64_t gi = by + tx;
    if (gi < n) alpha_out[gi] = D[tx] * alpha[gi];
  }
}

}  // namespace

#define BO_ICM_COMMON(who, a)                                                                  \
  BO_CHECK_ARG((a)->T >= 1 && (a)->T <= MAXT, who ": T = %d tasks (1..%d)", (a)->T, MAXT)

extern "C" int bo_icm_covar_impl(const BoIcmCovarArgs* a, void* stream) {
  BO_CHECK_ARG(a->kind == BO_RBF || a->kind == BO_MATERN52, "bo_icm_covar: bad kind %d", a->kind);
  BO_ICM_COMMON("bo_icm_covar", a);
  BO_CHECK_ARG(a->d >= 1 && a->d <= MAXD, "bo_icm_covar: d = %d (1..%d)", a->d, MAXD);
  BO_CHECK_ARG(a->n >= 0 && a->np >= a->n && a->np % 128 == 0,
               "bo_icm_covar: n = %lld, np = %lld (np >= n, a multiple of 128)", (long long)a->n,
               (long long)a->np);
  if (a->np == 0) return BO_OK;
  BO_CHECK_ARG(a->A && a->B && a->lengthscale && (a->n == 0 || (a->X && a->task)),
               "bo_icm_covar: X, lengthscale, task, B and A are required");
  BO_CHECK_ARG(ceil_div(a->np, CV_ROWS) <= 65535, "bo_icm_covar: np = %lld is too large",
               (long long)a->np);
  dim3 grid((unsigned)ceil_div(a->np, THREADS), (unsigned)ceil_div(a->np, CV_ROWS));
  hipStream_t st = as_stream(stream);
  if (a->kind == BO_RBF)
    icm_covar_kernel<BO_RBF><<<grid, THREADS, 0, st>>>(a->X, a->n, a->d, a->lengthscale, a->task,
                                                        a->B, a->T, a->outputscale, a->noise,
                                                        a->noise_vec, a->A, a->np);
  else
    icm_covar_kernel<BO_MATERN52><<<grid, THREADS, 0, st>>>(a->X, a->n, a->d, a->lengthscale,
                                                             a->task, a->B, a->T, a->outputscale,
                                                             a->noise, a->noise_vec, a->A, a->np);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_icm_mll_terms_impl(const BoIcmMllArgs* a, void* stream) {
  BO_CHECK_ARG(a->kind == BO_RBF || a->kind == BO_MATERN52, "bo_icm_mll_terms: bad kind %d",
               a->kind);
  BO_ICM_COMMON("bo_icm_mll_terms", a);
  BO_CHECK_ARG(a->d >= 1 && a->d <= MAXD, "bo_icm_mll_terms: d = %d (1..%d)", a->d, MAXD);
  BO_CHECK_ARG(a->n >= 0 && a->n < (int64_t(1) << 31) && a->ld >= a->n,
               "bo_icm_mll_terms: n = %lld, ld = %lld", (long long)a->n, (long long)a->ld);
  if (a->n == 0) return BO_OK;
  BO_CHECK_ARG(a->X && a->lengthscale && a->task && a->B && a->L && a->Ainv && a->alpha &&
                   a->beta && a->partial,
               "bo_icm_mll_terms: every pointer is required");
  hipStream_t st = as_stream(stream);
#define BO_ICM_MLL(KIND, DC, NT)                                                               \
  icm_mll_terms_kernel<KIND, DC, NT><<<(unsigned)a->n, THREADS, 0, st>>>(                      \
      a->X, (int)a->n, a->d, a->lengthscale, a->task, a->B, a->T, a->outputscale, a->L, a->Ainv, \
      a->ld, a->alpha, a->beta, a->partial)
#define BO_ICM_MLL_D(KIND, NT)                                                                 \
  do {                                                                                         \
    if (a->d == 6) BO_ICM_MLL(KIND, 6, NT);                                                    \
    else BO_ICM_MLL(KIND, 0, NT);                                                              \
  } while (0)
  if (a->kind == BO_RBF) {
    if (a->T <= 4) BO_ICM_MLL_D(BO_RBF, 4); else BO_ICM_MLL_D(BO_RBF, MAXT);
  } else {
    if (a->T <= 4) BO_ICM_MLL_D(BO_MATERN52, 4); else BO_ICM_MLL_D(BO_MATERN52, MAXT);
  }
#undef BO_ICM_MLL_D
#undef BO_ICM_MLL
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_icm_task_view_impl(const BoIcmTaskViewArgs* a, void* stream) {
  BO_ICM_COMMON("bo_icm_task_view", a);
  BO_CHECK_ARG(a->t >= 0 && a->t < a->T, "bo_icm_task_view: output task %d of %d", a->t, a->T);
  BO_CHECK_ARG(a->n >= 0 && a->np >= a->n && a->np % 128 == 0,
               "bo_icm_task_view: n = %lld, np = %lld (np >= n, a multiple of 128)",
               (long long)a->n, (long long)a->np);
  if (a->np == 0) return BO_OK;
  BO_CHECK_ARG(a->U && a->B && a->U_out && a->Linv_out && a->U_out != a->U &&
                   (a->n == 0 || (a->task && a->alpha && a->alpha_out)),
               "bo_icm_task_view: U, alpha, task, B and the three outputs are required "
               "(U_out apart from U)");
  BO_CHECK_ARG(a->np / 32 <= 65535, "bo_icm_task_view: np = %lld is too large", (long long)a->np);
  dim3 grid((unsigned)(a->np / 32), (unsigned)(a->np / 32));
  icm_task_view_kernel<<<grid, dim3(32, 8), 0, as_stream(stream)>>>(
      a->U, a->alpha, a->task, a->B, a->T, a->t, a->n, a->np, a->U_out, a->Linv_out, a->alpha_out);
  BO_LAUNCH_CHECK();
  return BO_OK;
}
