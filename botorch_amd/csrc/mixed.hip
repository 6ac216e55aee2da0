// Mixed continuous / categorical exact GP (botorch/models/gp_regression_mixed.py:
// 133-173, models/kernels/categorical.py): over rows z = (x, c) of d_c continuous
// and d_k categorical columns
//   K(z, z') = o_s (kbar(x, x'; l1) + o_c kap(c, c'; lam1)) + o_p kbar(x, x'; l2) kap(c, c'; lam2)
//   kap(c, c'; lam) = exp(-(1 / d_k) sum_j [c_j != c'_j] / lam_j)
// with 1 <= d_c, d_k <= 8.  Four kernels:
//
//   mixed_covar_kernel       A = K(Z, Z) + diag(noise) straight into the padded lower
//                            workspace bo_cholesky_inverse* factorises in place
//   mixed_mll_terms_kernel   one pass over the lower triangle with W = alpha alpha^T -
//                            A^{-1}: the 35 sums of the kernel hyperparameters' gradients
//   mixed_cross_kernel       K*x (R x n) and the B diagonal blocks K** (q x q), one launch
//   mixed_cross_grad_kernel  dX (R x d) from dK*x and the t-batch's own symmetric G
//
// What they share: both column groups are padded to 8 so that every loop over
// columns is unrolled and every accumulator is a named register (a padded
// continuous column has reciprocal lengthscale 0, a padded categorical column is
// masked out: both add exactly 0); both continuous terms come from one pass over
// the differences; kap is read from a table over the pair's 8-bit mismatch mask
// (2 x 256 doubles in LDS, built once per workgroup) -- mixed_cross_kernel also has
// a direct instance (two exp per pair) for the comparison in profiles/mixed/.
// Columns are gathered from the caller's n x d rows through the column lists of the
// argument record, so no packed copy of the inputs is made.  No atomics; wave
// shuffles then LDS in a fixed order: repeated calls are bitwise identical.
#include "common.h"
#include "launch_checks.h"

namespace {

constexpr int THREADS = 256;
constexpr int MD = BO_MIXED_MAX_DIM;  // 8: padded width of either column group
constexpr int CV_ROWS = 8;            // rows of A per workgroup (x 256 columns)
constexpr int CR_ROWS = 32;           // query rows per workgroup of the cross kernel
constexpr int NACC = 4 * MD + 3;      // 35 hyperparameter sums
constexpr int MLL_COLS = BO_MIXED_MLL_COLS;

// column lists by value: positions of the continuous / categorical columns in a row
// of d doubles, padded entries repeating a valid column (their result is zeroed)
struct Cols {
  int c[MD], k[MD];
  int d, dc, dk, kmask;
};

Cols make_cols(int d, int dc, int dk, const int32_t* cont, const int32_t* cat) {
  Cols s;
  for (int t = 0; t < MD; ++t) {
    s.c[t] = cont[t < dc ? t : 0];
    s.k[t] = cat[t < dk ? t : 0];
  }
  s.d = d, s.dc = dc, s.dk = dk, s.kmask = (1 << dk) - 1;
  return s;
}

// Hyperparameters and the two kap tables of a workgroup.
struct Shared {
  double il1[MD], il2[MD];  // 1 / l (0 on the padding)
  double a1[MD], a2[MD];    // 1 / (d_k lam) (0 on the padding)
  double k1[256], k2[256];  // kap[mask]
};

// hyper: [l1 (d_c), lam1 (d_k), l2 (d_c), lam2 (d_k)].  Ends with a barrier.
__device__ __forceinline__ void stage_hyper(Shared& s, const double* __restrict__ hyper,
                                            const Cols& cl) {
  const int tid = threadIdx.x;
  if (tid < MD) {
    s.il1[tid] = tid < cl.dc ? 1.0 / hyper[tid] : 0.0;
    s.il2[tid] = tid < cl.dc ? 1.0 / hyper[cl.dc + cl.dk + tid] : 0.0;
    s.a1[tid] = tid < cl.dk ? 1.0 / (cl.dk * hyper[cl.dc + tid]) : 0.0;
    s.a2[tid] = tid < cl.dk ? 1.0 / (cl.dk * hyper[2 * cl.dc + cl.dk + tid]) : 0.0;
  }
  __syncthreads();
  for (int m = tid; m < 256; m += blockDim.x) {
    double e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int j = 0; j < MD; ++j) {
      const double bit = (double)((m >> j) & 1);
      e1 = fma(bit, s.a1[j], e1);
      e2 = fma(bit, s.a2[j], e2);
    }
    s.k1[m] = exp(-e1);
    s.k2[m] = exp(-e2);
  }
  __syncthreads();
}

__device__ __forceinline__ void load_row(const double* __restrict__ X, int64_t row, const Cols& cl,
                                         double x[MD], double c[MD]) {
  const double* p = X + row * cl.d;
#pragma unroll
  for (int t = 0; t < MD; ++t) {
    x[t] = t < cl.dc ? p[cl.c[t]] : 0.0;  // padding: Delta = 0, so its sums are exactly 0
    c[t] = p[cl.k[t]];
  }
}

// unit-outputscale kernel value k and the radial factor g of its derivatives:
// dk/dl_j = g Delta_j^2 / l_j^3, dk/dx_j = -g Delta_j / l_j^2; finite at r = 0
template <int KIND>
__device__ __forceinline__ void kbar_g(double r2, double& k, double& g) {
  if (KIND == BO_RBF) {
    k = exp(-0.5 * r2);
    g = k;
  } else {
    const double s5r = 2.23606797749978969641 * sqrt(r2);
    const double e = exp(-s5r);
    k = (1.0 + s5r + (5.0 / 3.0) * r2) * e;
    g = (5.0 / 3.0) * (1.0 + s5r) * e;
  }
}

// One pair: differences, both scaled squared distances, the mismatch mask.
struct Pair {
  double df[MD];
  double r1, r2;
  int mask;
};

__device__ __forceinline__ Pair make_pair(const double xa[MD], const double ca[MD],
                                          const double xb[MD], const double cb[MD],
                                          const Shared& s, int kmask) {
  Pair p;
  p.r1 = 0.0, p.r2 = 0.0, p.mask = 0;
#pragma unroll
  for (int t = 0; t < MD; ++t) {
    p.df[t] = xa[t] - xb[t];
    const double u = p.df[t] * s.il1[t], v = p.df[t] * s.il2[t];
    p.r1 = fma(u, u, p.r1);
    p.r2 = fma(v, v, p.r2);
    p.mask |= (ca[t] != cb[t]) ? (1 << t) : 0;
  }
  p.mask &= kmask;
  return p;
}

// kap1, kap2 of a mask: the table, or (DIRECT) the sums and two exp
template <bool DIRECT>
__device__ __forceinline__ void kappa(const Shared& s, int mask, double& kp1, double& kp2) {
  if (!DIRECT) {
    kp1 = s.k1[mask];
    kp2 = s.k2[mask];
  } else {
    double e1 = 0.0, e2 = 0.0;
#pragma unroll
    for (int j = 0; j < MD; ++j) {
      const double bit = (double)((mask >> j) & 1);
      e1 = fma(bit, s.a1[j], e1);
      e2 = fma(bit, s.a2[j], e2);
    }
    kp1 = exp(-e1);
    kp2 = exp(-e2);
  }
}

template <int KIND, bool DIRECT>
__device__ __forceinline__ double pair_value(const Pair& p, const Shared& s, double os, double oc,
                                             double op) {
  double k1, g1, k2, g2, kp1, kp2;
  kbar_g<KIND>(p.r1, k1, g1);
  kbar_g<KIND>(p.r2, k2, g2);
  kappa<DIRECT>(s, p.mask, kp1, kp2);
  return os * fma(oc, kp1, k1) + op * (k2 * kp2);
}

// ---- training covariance --------------------------------------------------------------------
// CV_ROWS rows x 256 columns per workgroup, the rows' gathered inputs in LDS, each
// thread's column in registers for all rows.  Workgroups wholly above the diagonal
// write zeros only.
template <int KIND>
__global__ __launch_bounds__(THREADS) void mixed_covar_kernel(
    const double* __restrict__ X, int64_t n, Cols cl, const double* __restrict__ hyper, double os,
    double oc, double op, double noise, const double* __restrict__ noise_vec,
    double* __restrict__ A, int64_t np) {
  __shared__ Shared s;
  __shared__ double xi[CV_ROWS][MD], ci[CV_ROWS][MD];
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * THREADS + tid;
  const int64_t i0 = (int64_t)blockIdx.y * CV_ROWS;
  if (tid < CV_ROWS * MD) {
    const int r = tid / MD, t = tid - r * MD;
    const bool v = i0 + r < n;
    xi[r][t] = v ? X[(i0 + r) * cl.d + cl.c[t]] : 0.0;
    ci[r][t] = v ? X[(i0 + r) * cl.d + cl.k[t]] : 0.0;
  }
  stage_hyper(s, hyper, cl);
  if (j >= np) return;
  const bool jv = j < n;
  const bool work = jv && i0 < n && j <= i0 + CV_ROWS - 1;  // some row has j <= i
  double xj[MD], cj[MD];
  if (work) load_row(X, j, cl, xj, cj);
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
      const Pair p = make_pair(xi[r], ci[r], xj, cj, s, cl.kmask);
      val = pair_value<KIND, false>(p, s, os, oc, op);
      if (i == j) val += noise_vec ? noise_vec[i] + noise : noise;
    }
    A[i * np + j] = val;
  }
}

// ---- marginal log likelihood ------------------------------------------------------------------
// One workgroup per row i over k <= i, w = 2 off the diagonal.  partial[i], MLL_COLS:
//   [0..7]   sum w W o_s g1 Delta_j^2          (d ll/d l1_j   = 1/2 . / l1_j^3)
//   [8..15]  sum w W o_s o_c kap1 [c_j != c'_j] (d ll/d lam1_j = 1/2 . / (d_k lam1_j^2))
//   [16..23] sum w W o_p kap2 g2 Delta_j^2      (d ll/d l2_j)
//   [24..31] sum w W o_p k2 kap2 [c_j != c'_j]  (d ll/d lam2_j)
//   [32] sum w W (k1 + o_c kap1)   [33] sum w W o_s kap1   [34] sum w W k2 kap2
//   [35] W_ii   [36] log L_ii   [37] beta_i^2   [38] alpha_i   [39] 0
template <int KIND>
__global__ __launch_bounds__(THREADS) void mixed_mll_terms_kernel(
    const double* __restrict__ X, int n, Cols cl, const double* __restrict__ hyper, double os,
    double oc, double op, const double* __restrict__ L, const double* __restrict__ Ainv,
    int64_t ld, const double* __restrict__ alpha, const double* __restrict__ beta,
    double* __restrict__ partial) {
  __shared__ Shared s;
  __shared__ double red[THREADS / 64][NACC];
  const int i = blockIdx.x;
  const int tid = threadIdx.x;
  stage_hyper(s, hyper, cl);
  double xi[MD], ci[MD];
  load_row(X, i, cl, xi, ci);
  double a_l1[MD], a_m1[MD], a_l2[MD], a_m2[MD];
#pragma unroll
  for (int t = 0; t < MD; ++t) a_l1[t] = a_m1[t] = a_l2[t] = a_m2[t] = 0.0;
  double a_os = 0.0, a_oc = 0.0, a_op = 0.0;
  const double ai = alpha[i];
  for (int k = tid; k <= i; k += THREADS) {
    double xk[MD], ck[MD];
    load_row(X, k, cl, xk, ck);
    const Pair p = make_pair(xi, ci, xk, ck, s, cl.kmask);
    const double W = ai * alpha[k] - Ainv[(int64_t)i * ld + k];
    const double w = (k == i) ? W : 2.0 * W;
    double k1, g1, k2, g2, kp1, kp2;
    kbar_g<KIND>(p.r1, k1, g1);
    kbar_g<KIND>(p.r2, k2, g2);
    kappa<false>(s, p.mask, kp1, kp2);
    const double wl1 = w * os * g1, wl2 = w * op * kp2 * g2;
    const double wm1 = w * os * oc * kp1, wm2 = w * op * k2 * kp2;
#pragma unroll
    for (int t = 0; t < MD; ++t) {
      const double q2 = p.df[t] * p.df[t];
      a_l1[t] = fma(wl1, q2, a_l1[t]);
      a_l2[t] = fma(wl2, q2, a_l2[t]);
      const bool ne = (p.mask >> t) & 1;
      a_m1[t] += ne ? wm1 : 0.0;
      a_m2[t] += ne ? wm2 : 0.0;
    }
    a_os = fma(w, fma(oc, kp1, k1), a_os);
    a_oc = fma(w * os, kp1, a_oc);
    a_op = fma(w, k2 * kp2, a_op);
  }
  const int wv = tid >> 6;
  const bool lead = (tid & 63) == 0;
#pragma unroll
  for (int t = 0; t < MD; ++t) {
    const double v0 = wave_sum(a_l1[t]), v1 = wave_sum(a_m1[t]);
    const double v2 = wave_sum(a_l2[t]), v3 = wave_sum(a_m2[t]);
    if (lead) {
      red[wv][t] = v0;
      red[wv][MD + t] = v1;
      red[wv][2 * MD + t] = v2;
      red[wv][3 * MD + t] = v3;
    }
  }
  {
    const double v0 = wave_sum(a_os), v1 = wave_sum(a_oc), v2 = wave_sum(a_op);
    if (lead) {
      red[wv][4 * MD] = v0;
      red[wv][4 * MD + 1] = v1;
      red[wv][4 * MD + 2] = v2;
    }
  }
  __syncthreads();
  double* out = partial + (int64_t)i * MLL_COLS;
  if (tid < NACC) {
    double v = 0.0;
    for (int w = 0; w < THREADS / 64; ++w) v += red[w][tid];
    out[tid] = v;
  }
  if (tid == NACC) {
    out[NACC] = ai * ai - Ainv[(int64_t)i * ld + i];
    out[NACC + 1] = log(L[(int64_t)i * ld + i]);
    out[NACC + 2] = beta[i] * beta[i];
    out[NACC + 3] = ai;
    out[NACC + 4] = 0.0;
  }
}

// ---- cross covariance ---------------------------------------------------------------------------
// grid (column tiles of 256 training points + 1, chunks of CR_ROWS query rows).  A
// column-tile workgroup holds one training point per thread in registers and walks
// the chunk's query rows, staged in LDS (broadcast reads; the stores of a row are
// contiguous over the threads).  The last x index writes the chunk's rows of the
// K** blocks: row r against the q points of its own t-batch.  Every value goes
// through the same selects: no branch depends on a value.
template <int KIND, bool DIRECT>
__global__ __launch_bounds__(THREADS) void mixed_cross_kernel(
    const double* __restrict__ Xq, int64_t R, int q, const double* __restrict__ Xt, int64_t n,
    Cols cl, const double* __restrict__ hyper, double os, double oc, double op,
    double* __restrict__ Kx, double* __restrict__ Kxx) {
  __shared__ Shared s;
  __shared__ double xr[CR_ROWS][MD], cr[CR_ROWS][MD];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * CR_ROWS;
  const int rows = (int)((R - r0 < CR_ROWS) ? R - r0 : CR_ROWS);
  {
    const int r = tid / MD, t = tid - r * MD;  // 256 = CR_ROWS x MD
    const bool v = r < rows;
    xr[r][t] = v ? Xq[(r0 + r) * cl.d + cl.c[t]] : 0.0;
    cr[r][t] = v ? Xq[(r0 + r) * cl.d + cl.k[t]] : 0.0;
  }
  stage_hyper(s, hyper, cl);
  if (blockIdx.x + 1 < gridDim.x) {
    const int64_t k = (int64_t)blockIdx.x * THREADS + tid;
    if (k >= n) return;
    double xk[MD], ck[MD];
    load_row(Xt, k, cl, xk, ck);
    for (int r = 0; r < rows; ++r) {
      const Pair p = make_pair(xr[r], cr[r], xk, ck, s, cl.kmask);
      Kx[(r0 + r) * n + k] = pair_value<KIND, DIRECT>(p, s, os, oc, op);
    }
  } else {
    for (int e = tid; e < rows * q; e += THREADS) {
      const int r = e / q, c = e - r * q;
      const int64_t row = r0 + r;
      const int64_t other = (row / q) * q + c;
      double xo[MD], co[MD];
      load_row(Xq, other, cl, xo, co);
      const Pair p = make_pair(xr[r], cr[r], xo, co, s, cl.kmask);
      Kxx[row * q + c] = pair_value<KIND, DIRECT>(p, s, os, oc, op);
    }
  }
}

// ---- gradient of the cross covariance -----------------------------------------------------------
// One wave per query row r: dX_r = sum_k dKx[r][k] dK(z_r, zt_k)/dx_r
//                                + sum_c G[r][c] dK(z_r, z_(b q + c))/dx_r  (b = r / q),
// dK/dx_j = -(o_s g1 / l1_j^2 + o_p kap2 g2 / l2_j^2) Delta_j; lanes stride over k,
// then over c, eight register sums, one wave_sum each.  The row of d entries is
// written whole: categorical columns get an exact 0.
template <int KIND>
__global__ __launch_bounds__(THREADS) void mixed_cross_grad_kernel(
    const double* __restrict__ Xq, int64_t R, int q, const double* __restrict__ Xt, int64_t n,
    Cols cl, const double* __restrict__ hyper, double os, double op,
    const double* __restrict__ dKx, const double* __restrict__ G, double* __restrict__ dX) {
  __shared__ Shared s;
  stage_hyper(s, hyper, cl);
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  if (r >= R) return;
  double xq[MD], cq[MD], acc[MD], s1[MD], s2[MD];
  load_row(Xq, r, cl, xq, cq);
#pragma unroll
  for (int t = 0; t < MD; ++t) {
    acc[t] = 0.0;
    s1[t] = os * s.il1[t] * s.il1[t];
    s2[t] = op * s.il2[t] * s.il2[t];
  }
  const int64_t b0 = (r / q) * q;
  const int64_t total = n + q;
  for (int64_t e = lane; e < total; e += 64) {
    const bool tr = e < n;
    const double* src = tr ? Xt : Xq;
    const int64_t row = tr ? e : b0 + (e - n);
    const double wgt = tr ? dKx[r * n + e] : G[r * q + (e - n)];
    double xo[MD], co[MD];
    load_row(src, row, cl, xo, co);
    const Pair p = make_pair(xq, cq, xo, co, s, cl.kmask);
    double k1, g1, k2, g2;
    kbar_g<KIND>(p.r1, k1, g1);
    kbar_g<KIND>(p.r2, k2, g2);
    const double f1 = -wgt * g1, f2 = -wgt * g2 * s.k2[p.mask];
#pragma unroll
    for (int t = 0; t < MD; ++t) acc[t] = fma(fma(f1, s1[t], f2 * s2[t]), p.df[t], acc[t]);
  }
  double out = 0.0;
#pragma unroll
  for (int t = 0; t < MD; ++t) {
    const double v = wave_sum(acc[t]);
    out = (t < cl.dc && cl.c[t] == lane) ? v : out;
  }
  if (lane < cl.d) dX[r * cl.d + lane] = out;
}

int check_cols(const char* who, int kind, int d, int dc, int dk, const int32_t* cont,
               const int32_t* cat) {
  BO_CHECK_ARG(kind == BO_RBF || kind == BO_MATERN52, "%s: bad kind %d", who, kind);
  BO_CHECK_ARG(dc >= 1 && dc <= MD && dk >= 1 && dk <= MD && d == dc + dk,
               "%s: d_c = %d, d_k = %d, d = %d (1..%d each, d = d_c + d_k)", who, dc, dk, d, MD);
  return check_partition(who, d, dc, cont, dk, cat);
}

}  // namespace

#define BO_MIXED_COLS(who, a)                                                                    \
  do {                                                                                           \
    const int _st = check_cols(who, (a)->kind, (a)->d, (a)->d_c, (a)->d_k, (a)->cont_cols,       \
                               (a)->cat_cols);                                                   \
    if (_st != BO_OK) return _st;                                                                \
  } while (0)

extern "C" int bo_mixed_covar_impl(const BoMixedCovarArgs* a, void* stream) {
  BO_MIXED_COLS("bo_mixed_covar", a);
  BO_CHECK_ARG(a->n >= 0 && a->np >= a->n && a->np % 128 == 0,
               "bo_mixed_covar: n = %lld, np = %lld (np >= n, a multiple of 128)", (long long)a->n,
               (long long)a->np);
  if (a->np == 0) return BO_OK;
  BO_CHECK_ARG(a->A && a->hyper && (a->n == 0 || a->X), "bo_mixed_covar: X, hyper and A are required");
  BO_CHECK_ARG(ceil_div(a->np, CV_ROWS) <= 65535, "bo_mixed_covar: np = %lld is too large",
               (long long)a->np);
  const Cols cl = make_cols(a->d, a->d_c, a->d_k, a->cont_cols, a->cat_cols);
  dim3 grid((unsigned)ceil_div(a->np, THREADS), (unsigned)ceil_div(a->np, CV_ROWS));
  hipStream_t st = as_stream(stream);
#define BO_GO(KIND)                                                                              \
  mixed_covar_kernel<KIND><<<grid, THREADS, 0, st>>>(a->X, a->n, cl, a->hyper, a->o_s, a->o_c,   \
                                                     a->o_p, a->noise, a->noise_vec, a->A, a->np)
  if (a->kind == BO_RBF) BO_GO(BO_RBF); else BO_GO(BO_MATERN52);
#undef BO_GO
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_mixed_mll_terms_impl(const BoMixedMllArgs* a, void* stream) {
  BO_MIXED_COLS("bo_mixed_mll_terms", a);
  BO_CHECK_ARG(a->n >= 0 && a->n < (int64_t(1) << 31) && a->ld >= a->n,
               "bo_mixed_mll_terms: n = %lld, ld = %lld", (long long)a->n, (long long)a->ld);
  if (a->n == 0) return BO_OK;
  BO_CHECK_ARG(a->X && a->hyper && a->L && a->Ainv && a->alpha && a->beta && a->partial,
               "bo_mixed_mll_terms: every pointer is required");
  const Cols cl = make_cols(a->d, a->d_c, a->d_k, a->cont_cols, a->cat_cols);
  hipStream_t st = as_stream(stream);
#define BO_GO(KIND)                                                                              \
  mixed_mll_terms_kernel<KIND><<<(unsigned)a->n, THREADS, 0, st>>>(                              \
      a->X, (int)a->n, cl, a->hyper, a->o_s, a->o_c, a->o_p, a->L, a->Ainv, a->ld, a->alpha,     \
      a->beta, a->partial)
  if (a->kind == BO_RBF) BO_GO(BO_RBF); else BO_GO(BO_MATERN52);
#undef BO_GO
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_mixed_cross_impl(const BoMixedCrossArgs* a, void* stream) {
  BO_MIXED_COLS("bo_mixed_cross", a);
  if (int st = check_cross("bo_mixed_cross", a)) return st;
  const int64_t R = a->B * a->q;
  if (R == 0) return BO_OK;
  BO_CHECK_ARG(a->Kxx && (a->n == 0 || a->Kx), "bo_mixed_cross: Kx and Kxx are required");
  BO_CHECK_ARG(ceil_div(R, CR_ROWS) <= 65535, "bo_mixed_cross: %lld query rows are too many",
               (long long)R);
  const Cols cl = make_cols(a->d, a->d_c, a->d_k, a->cont_cols, a->cat_cols);
  dim3 grid((unsigned)ceil_div(a->n, THREADS) + 1, (unsigned)ceil_div(R, CR_ROWS));
  hipStream_t st = as_stream(stream);
#define BO_GO(KIND, DIRECT)                                                                      \
  mixed_cross_kernel<KIND, DIRECT><<<grid, THREADS, 0, st>>>(                                    \
      a->Xq, R, (int)a->q, a->Xt, a->n, cl, a->hyper, a->o_s, a->o_c, a->o_p, a->Kx, a->Kxx)
  if (a->kind == BO_RBF) {
    if (a->kappa_direct) BO_GO(BO_RBF, true); else BO_GO(BO_RBF, false);
  } else {
    if (a->kappa_direct) BO_GO(BO_MATERN52, true); else BO_GO(BO_MATERN52, false);
  }
#undef BO_GO
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_mixed_cross_grad_impl(const BoMixedCrossArgs* a, void* stream) {
  BO_MIXED_COLS("bo_mixed_cross_grad", a);
  if (int st = check_cross("bo_mixed_cross_grad", a)) return st;
  const int64_t R = a->B * a->q;
  if (R == 0) return BO_OK;
  BO_CHECK_ARG(a->G && a->dX && (a->n == 0 || a->dKx),
               "bo_mixed_cross_grad: dKx, G and dX are required");
  const Cols cl = make_cols(a->d, a->d_c, a->d_k, a->cont_cols, a->cat_cols);
  const unsigned grid = (unsigned)ceil_div(R, THREADS / 64);
  hipStream_t st = as_stream(stream);
#define BO_GO(KIND)                                                                              \
  mixed_cross_grad_kernel<KIND><<<grid, THREADS, 0, st>>>(a->Xq, R, (int)a->q, a->Xt, a->n, cl,  \
                                                          a->hyper, a->o_s, a->o_p, a->dKx, a->G, \
                                                          a->dX)
  if (a->kind == BO_RBF) BO_GO(BO_RBF); else BO_GO(BO_MATERN52);
#undef BO_GO
  BO_LAUNCH_CHECK();
  return BO_OK;
}
