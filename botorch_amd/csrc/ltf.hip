// Multi-fidelity exact GP with the linear truncated fidelity kernel
// (botorch/models/kernels/linear_truncated_fidelity.py:183-238,
// models/gp_regression_fidelity.py:218-308): over rows z = (x, s) of d_x ordinary
// columns and one or two fidelity columns, s clamped to [0, 1], u = 1 - s,
//   K(z, z') = o [k0(x, x'; l0) + c(s, s'; p) k1(x, x'; l1)]
//   c  = u1 u1' (1 + s1 s1')^p
//   c += u2 u2' (1 + s2 s2')^p + u1 u1' u2 u2' (1 + s1 s1' + s2 s2')^p   (two columns)
// k0, k1 Matern-5/2 ARD.  Four kernels:
//
//   ltf_covar_kernel       A = K(Z, Z) + diag(noise) straight into the padded lower
//                          workspace bo_cholesky_inverse* factorises in place
//   ltf_mll_terms_kernel   one pass over the lower triangle with W = alpha alpha^T -
//                          A^{-1}: the sums of d ll / d (l0, l1, p, o)
//   ltf_cross_kernel       K*x (R x n) and the B diagonal blocks K** (q x q), one launch
//   ltf_cross_grad_kernel  dX (R x d) from dK*x and the t-batch's own symmetric G,
//                          fidelity columns included (torch.clamp's gradient)
//
// What they share.  The padded width DXP of x is a template parameter (8, 16): every
// loop over columns is unrolled, every accumulator a named register, a padded column
// has reciprocal lengthscale 0 and adds exactly 0.  The fidelity terms of a row
// (clamped s, u, the clamp mask) are computed once where the row is staged.  The
// powers are exp(p log1p(t)), t in [0, 2].  Rows that every thread of a workgroup
// meets (a covariance tile's rows, a chunk of query rows, a tile of training rows in
// the gradient) are staged in LDS; the per-pair loops read x from LDS or registers.
// A row with every u = 0 (target fidelity) has c = 0 against every partner: where the
// row is uniform over a wave the kernels branch on its flag and evaluate k0 alone --
// the general path gives fma(0, k1, k0) there, the same bits.  Contraction is off in
// this file so that both paths round alike; every fused multiply-add is written out.
// Columns are gathered through the record's column lists.  No atomics: wave shuffles,
// then LDS, in a fixed order.
#include "common.h"
#include "launch_checks.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAXD = BO_LTF_MAX_DIM;  // 16: the widest padded x
constexpr int CV_ROWS = 8;            // rows of A per workgroup (x 256 columns)
constexpr int CR_ROWS = 16;           // query rows per workgroup of the cross kernel
constexpr int GT = 256;               // training rows per LDS tile of the gradient kernel
constexpr int NACC = 2 * MAXD + 2;    // 34 hyperparameter sums
constexpr int MLL_COLS = BO_LTF_MLL_COLS;

// column lists by value; padded entries repeat a valid column (their values are zeroed)
struct Cols {
  int x[MAXD], f[2];
  int d, dx, nf;
};

Cols make_cols(int d, int dx, int nf, const int32_t* xc, const int32_t* fc) {
  Cols s;
  for (int t = 0; t < MAXD; ++t) s.x[t] = xc[t < dx ? t : 0];
  for (int t = 0; t < 2; ++t) s.f[t] = fc[t < nf ? t : 0];
  s.d = d, s.dx = dx, s.nf = nf;
  return s;
}

// the fidelity terms of one row: clamped s, u = 1 - s, the clamp's pass mask
struct Fid {
  double s1, s2, u1, u2;
  int m1, m2;
};

__device__ __forceinline__ Fid fid_of(const double* __restrict__ row, const Cols& cl) {
  Fid f;
  const double a = row[cl.f[0]], b = row[cl.f[1]];
  f.s1 = fmin(fmax(a, 0.0), 1.0);
  f.u1 = 1.0 - f.s1;
  f.m1 = (a >= 0.0 && a <= 1.0) ? 1 : 0;
  const bool two = cl.nf == 2;
  f.s2 = two ? fmin(fmax(b, 0.0), 1.0) : 0.0;  // one column: u2 = 0 removes both extra terms
  f.u2 = two ? 1.0 - f.s2 : 0.0;
  f.m2 = (two && b >= 0.0 && b <= 1.0) ? 1 : 0;
  return f;
}

__device__ __forceinline__ Fid fid_zero() {
  Fid f;
  f.s1 = f.s2 = f.u1 = f.u2 = 0.0;
  f.m1 = f.m2 = 0;
  return f;
}

__device__ __forceinline__ bool at_target(const Fid& f, int nf) {
  return f.u1 == 0.0 && (nf == 1 || f.u2 == 0.0);
}

// reciprocal lengthscales (0 on the padding).  hyper: [l0 (d_x), l1 (d_x)].  Ends with a barrier.
struct Shared {
  double il0[MAXD], il1[MAXD];
};

__device__ __forceinline__ void stage_hyper(Shared& s, const double* __restrict__ hyper,
                                            const Cols& cl) {
  const int tid = threadIdx.x;
  if (tid < MAXD) {
    s.il0[tid] = tid < cl.dx ? 1.0 / hyper[tid] : 0.0;
    s.il1[tid] = tid < cl.dx ? 1.0 / hyper[cl.dx + tid] : 0.0;
  }
  __syncthreads();
}

template <int DXP>
__device__ __forceinline__ void load_x(const double* __restrict__ row, const Cols& cl,
                                       double x[DXP]) {
#pragma unroll
  for (int t = 0; t < DXP; ++t) x[t] = t < cl.dx ? row[cl.x[t]] : 0.0;
}

// Matern-5/2 value k and the radial factor g of its derivatives:
// dk/dl_j = g Delta_j^2 / l_j^3, dk/dx_j = -g Delta_j / l_j^2; finite at r = 0
__device__ __forceinline__ void matern_g(double r2, double& k, double& g) {
  const double s5r = 2.23606797749978969641 * sqrt(r2);
  const double e = exp(-s5r);
  k = (1.0 + s5r + (5.0 / 3.0) * r2) * e;
  g = (5.0 / 3.0) * (1.0 + s5r) * e;
}

// the differences and the l0 distance (every pair), and the l1 distance in the same
// pass (pairs off the target-fidelity shortcut); r0 takes the same operations in both
template <int DXP, bool BOTH>
__device__ __forceinline__ void distances(const double* xa, const double xb[DXP],
                                          const Shared& s, double df[DXP], double& r0,
                                          double& r1) {
  r0 = 0.0, r1 = 0.0;
#pragma unroll
  for (int t = 0; t < DXP; ++t) {
    df[t] = xa[t] - xb[t];
    const double a = df[t] * s.il0[t];
    r0 = fma(a, a, r0);
    if (BOTH) {
      const double b = df[t] * s.il1[t];
      r1 = fma(b, b, r1);
    }
  }
}

// c(a, b) and, LEVEL 1: dc/dp; LEVEL 2: dc/ds1, dc/ds2 in a's fidelities (masked)
template <int LEVEL>
__device__ __forceinline__ void cterms(const Fid& a, const Fid& b, double p, int nf, double& c,
                                       double& dp, double& d1, double& d2) {
  const double t1 = a.s1 * b.s1;
  const double L1 = log1p(t1), E1 = exp(p * L1), w1 = a.u1 * b.u1;
  c = w1 * E1;
  if (LEVEL == 1) dp = c * L1;
  if (LEVEL == 2) {
    d1 = fma(w1 * p * E1, b.s1 / (1.0 + t1), -(b.u1 * E1));
    d2 = 0.0;
  }
  if (nf == 2) {
    const double t2 = a.s2 * b.s2, t12 = t1 + t2;
    const double L2 = log1p(t2), E2 = exp(p * L2), w2 = a.u2 * b.u2;
    const double L12 = log1p(t12), E12 = exp(p * L12), w12 = w2 * w1;
    c += w2 * E2;
    c += w12 * E12;
    if (LEVEL == 1) {
      dp += w2 * E2 * L2;
      dp += w12 * E12 * L12;
    }
    if (LEVEL == 2) {
      const double h = w12 * p * E12 / (1.0 + t12);
      d1 += fma(h, b.s1, -(b.u1 * w2 * E12));
      d2 = fma(w2 * p * E2, b.s2 / (1.0 + t2), -(b.u2 * E2));
      d2 += fma(h, b.s2, -(b.u2 * w1 * E12));
    }
  }
  if (LEVEL == 2) {
    d1 = a.m1 ? d1 : 0.0;
    d2 = a.m2 ? d2 : 0.0;
  }
}

// One covariance value, row a (flag ``target``: uniform over the wave) against b.
template <int DXP>
__device__ __forceinline__ double pair_value(const double* xa, const Fid& fa, bool target,
                                             const double xb[DXP], const Fid& fb,
                                             const Shared& s, double p, int nf, double o) {
  double df[DXP], r0, r1, k0, g0;
  if (target) {
    distances<DXP, false>(xa, xb, s, df, r0, r1);
    matern_g(r0, k0, g0);
    return o * k0;
  }
  double k1, g1, c, dp, d1, d2;
  distances<DXP, true>(xa, xb, s, df, r0, r1);
  matern_g(r0, k0, g0);
  matern_g(r1, k1, g1);
  cterms<0>(fa, fb, p, nf, c, dp, d1, d2);
  return o * fma(c, k1, k0);
}

// ---- training covariance --------------------------------------------------------------------
// CV_ROWS rows x 256 columns per workgroup: the rows' gathered x and fidelity terms
// in LDS, each thread's column in registers for all rows.  The branch on a row's
// target flag is uniform over the workgroup.  Workgroups wholly above the diagonal
// write zeros only.
template <int DXP>
__global__ __launch_bounds__(THREADS) void ltf_covar_kernel(
    const double* __restrict__ X, int64_t n, Cols cl, const double* __restrict__ hyper, double p,
    double o, double noise, const double* __restrict__ noise_vec, double* __restrict__ A,
    int64_t np) {
  __shared__ Shared s;
  __shared__ double xi[CV_ROWS][DXP];
  __shared__ Fid fi[CV_ROWS];
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * THREADS + tid;
  const int64_t i0 = (int64_t)blockIdx.y * CV_ROWS;
  if (tid < CV_ROWS * DXP) {
    const int r = tid / DXP, t = tid - r * DXP;
    xi[r][t] = (i0 + r < n && t < cl.dx) ? X[(i0 + r) * cl.d + cl.x[t]] : 0.0;
  }
  if (tid < CV_ROWS) fi[tid] = i0 + tid < n ? fid_of(X + (i0 + tid) * cl.d, cl) : fid_zero();
  stage_hyper(s, hyper, cl);
  if (j >= np) return;
  const bool jv = j < n;
  const bool work = jv && i0 < n && j <= i0 + CV_ROWS - 1;  // some row has j <= i
  double xj[DXP];
  Fid fj = fid_zero();
#pragma unroll
  for (int t = 0; t < DXP; ++t) xj[t] = 0.0;
  if (work) {
    load_x<DXP>(X + j * cl.d, cl, xj);
    fj = fid_of(X + j * cl.d, cl);
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
      val = pair_value<DXP>(xi[r], fi[r], at_target(fi[r], cl.nf), xj, fj, s, p, cl.nf, o);
      if (i == j) val += noise_vec ? noise_vec[i] + noise : noise;
    }
    A[i * np + j] = val;
  }
}

// ---- marginal log likelihood ------------------------------------------------------------------
// One workgroup per row i over k <= i, w = 2 off the diagonal; row i and its fidelity
// terms staged in LDS once, each partner row read once by the one thread that owns it.
// A row at target fidelity (uniform over the workgroup) adds to the l0 and o sums
// only.  partial[i], MLL_COLS:
//   [0..15]  sum w W o g0 Delta_j^2      (d ll/d l0_j = 1/2 . / l0_j^3)
//   [16..31] sum w W o c g1 Delta_j^2    (d ll/d l1_j = 1/2 . / l1_j^3)
//   [32] sum w W o k1 dc/dp   [33] sum w W (k0 + c k1)
//   [34] W_ii   [35] log L_ii   [36] beta_i^2   [37] alpha_i   [38] 0   [39] 0
template <int DXP>
__global__ __launch_bounds__(THREADS) void ltf_mll_terms_kernel(
    const double* __restrict__ X, int n, Cols cl, const double* __restrict__ hyper, double p,
    double o, const double* __restrict__ L, const double* __restrict__ Ainv, int64_t ld,
    const double* __restrict__ alpha, const double* __restrict__ beta,
    double* __restrict__ partial) {
  __shared__ Shared s;
  __shared__ double xs[DXP];
  __shared__ Fid fs;
  __shared__ double red[THREADS / 64][NACC];
  const int i = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid < DXP) xs[tid] = tid < cl.dx ? X[(int64_t)i * cl.d + cl.x[tid]] : 0.0;
  if (tid == 0) fs = fid_of(X + (int64_t)i * cl.d, cl);
  stage_hyper(s, hyper, cl);
  double xi[DXP], a_l0[DXP], a_l1[DXP];
#pragma unroll
  for (int t = 0; t < DXP; ++t) {
    xi[t] = xs[t];
    a_l0[t] = a_l1[t] = 0.0;
  }
  const Fid fi = fs;
  const bool target = at_target(fi, cl.nf);
  double a_p = 0.0, a_o = 0.0;
  const double ai = alpha[i];
  for (int k = tid; k <= i; k += THREADS) {
    double xk[DXP], df[DXP], r0, r1, k0, g0;
    load_x<DXP>(X + (int64_t)k * cl.d, cl, xk);
    const double W = ai * alpha[k] - Ainv[(int64_t)i * ld + k];
    const double w = (k == i) ? W : 2.0 * W;
    if (target) {
      distances<DXP, false>(xi, xk, s, df, r0, r1);
      matern_g(r0, k0, g0);
      const double wl0 = w * o * g0;
#pragma unroll
      for (int t = 0; t < DXP; ++t) a_l0[t] = fma(wl0, df[t] * df[t], a_l0[t]);
      a_o = fma(w, k0, a_o);
    } else {
      double k1, g1, c, dp, d1, d2;
      const Fid fk = fid_of(X + (int64_t)k * cl.d, cl);
      distances<DXP, true>(xi, xk, s, df, r0, r1);
      matern_g(r0, k0, g0);
      matern_g(r1, k1, g1);
      cterms<1>(fi, fk, p, cl.nf, c, dp, d1, d2);
      const double wl0 = w * o * g0, wl1 = w * o * c * g1;
#pragma unroll
      for (int t = 0; t < DXP; ++t) {
        const double q2 = df[t] * df[t];
        a_l0[t] = fma(wl0, q2, a_l0[t]);
        a_l1[t] = fma(wl1, q2, a_l1[t]);
      }
      a_p = fma(w * o * k1, dp, a_p);
      a_o = fma(w, fma(c, k1, k0), a_o);
    }
  }
  const int wv = tid >> 6;
  const bool lead = (tid & 63) == 0;
#pragma unroll
  for (int t = 0; t < MAXD; ++t) {
    double v0 = 0.0, v1 = 0.0;
    if (t < DXP) {
      v0 = wave_sum(a_l0[t < DXP ? t : 0]);
      v1 = wave_sum(a_l1[t < DXP ? t : 0]);
    }
    if (lead) {
      red[wv][t] = v0;
      red[wv][MAXD + t] = v1;
    }
  }
  {
    const double v0 = wave_sum(a_p), v1 = wave_sum(a_o);
    if (lead) {
      red[wv][2 * MAXD] = v0;
      red[wv][2 * MAXD + 1] = v1;
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
    out[NACC + 5] = 0.0;
  }
}

// ---- cross covariance ---------------------------------------------------------------------------
// grid (column tiles of 256 training points + 1, chunks of CR_ROWS query rows).  The
// chunk's query rows, their fidelity terms and target flags are staged in LDS.  A
// column-tile workgroup holds one training point per thread in registers (x and
// fidelity terms) and walks the chunk's rows: the row, so its flag, is uniform over
// the workgroup, and the stores of a row are contiguous over the threads.  The last x
// index writes the chunk's rows of the K** blocks, one wave per row at a time, lanes
// over the q partners of the row's t-batch.  SKIP = false ignores the flags.
template <int DXP, bool SKIP>
__global__ __launch_bounds__(THREADS) void ltf_cross_kernel(
    const double* __restrict__ Xq, int64_t R, int q, const double* __restrict__ Xt, int64_t n,
    Cols cl, const double* __restrict__ hyper, double p, double o, double* __restrict__ Kx,
    double* __restrict__ Kxx) {
  __shared__ Shared s;
  __shared__ double xr[CR_ROWS][DXP];
  __shared__ Fid fr[CR_ROWS];
  __shared__ int tg[CR_ROWS];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * CR_ROWS;
  const int rows = (int)((R - r0 < CR_ROWS) ? R - r0 : CR_ROWS);
  if (tid < CR_ROWS * DXP) {
    const int r = tid / DXP, t = tid - r * DXP;
    xr[r][t] = (r < rows && t < cl.dx) ? Xq[(r0 + r) * cl.d + cl.x[t]] : 0.0;
  }
  if (tid < CR_ROWS) {
    const Fid f = tid < rows ? fid_of(Xq + (r0 + tid) * cl.d, cl) : fid_zero();
    fr[tid] = f;
    tg[tid] = SKIP && tid < rows && at_target(f, cl.nf);
  }
  stage_hyper(s, hyper, cl);
  if (blockIdx.x + 1 < gridDim.x) {
    const int64_t k = (int64_t)blockIdx.x * THREADS + tid;
    if (k >= n) return;
    double xk[DXP];
    load_x<DXP>(Xt + k * cl.d, cl, xk);
    const Fid fk = fid_of(Xt + k * cl.d, cl);
    for (int r = 0; r < rows; ++r)
      Kx[(r0 + r) * n + k] = pair_value<DXP>(xr[r], fr[r], tg[r] != 0, xk, fk, s, p, cl.nf, o);
  } else {
    const int lane = tid & 63;
    for (int r = tid >> 6; r < rows; r += THREADS / 64) {
      const int64_t row = r0 + r;
      const int64_t b0 = (row / q) * q;
      for (int c = lane; c < q; c += 64) {
        double xo[DXP];
        load_x<DXP>(Xq + (b0 + c) * cl.d, cl, xo);
        const Fid fo = fid_of(Xq + (b0 + c) * cl.d, cl);
        Kxx[row * q + c] = pair_value<DXP>(xr[r], fr[r], tg[r] != 0, xo, fo, s, p, cl.nf, o);
      }
    }
  }
}

// ---- gradient of the cross covariance -----------------------------------------------------------
// One wave per query row r, four rows per workgroup:
//   dX_r = sum_k dKx[r][k] dK(z_r, zt_k)/dz_r + sum_c G[r][c] dK(z_r, z_(b q + c))/dz_r
//   dK/dx_j = -o (g0 / l0_j^2 + c g1 / l1_j^2) Delta_j,  dK/ds_f = o k1 dc/ds_f
// The training rows pass through LDS in tiles of GT rows, gathered (x column-major,
// so the lanes of a wave read consecutive words) and their fidelity terms computed
// once per workgroup; lanes stride over a tile, then over the q partners.  A row whose
// every fidelity lies beyond 1 (u = 0 and the clamp closed) needs g0 alone; a row at
// exactly 1 has c = 0 but an open clamp, so it takes the general path.
template <int DXP>
struct GradAcc {
  double x[DXP], f1, f2;
};

template <int DXP, bool GENERAL>
__device__ __forceinline__ void grad_pair(GradAcc<DXP>& acc, const double xq[DXP], const Fid& fq,
                                          const double xo[DXP], const Fid& fo, double wgt,
                                          const Shared& s, const double s0[DXP],
                                          const double s1[DXP], double p, int nf) {
  double df[DXP], r0, r1, k0, g0;
  if (!GENERAL) {
    distances<DXP, false>(xq, xo, s, df, r0, r1);
    matern_g(r0, k0, g0);
    const double h0 = -wgt * g0;
#pragma unroll
    for (int t = 0; t < DXP; ++t) acc.x[t] = fma(h0 * s0[t], df[t], acc.x[t]);
  } else {
    double k1, g1, c, dp, d1, d2;
    distances<DXP, true>(xq, xo, s, df, r0, r1);
    matern_g(r0, k0, g0);
    matern_g(r1, k1, g1);
    cterms<2>(fq, fo, p, nf, c, dp, d1, d2);
    const double h0 = -wgt * g0, h1 = -wgt * c * g1;
#pragma unroll
    for (int t = 0; t < DXP; ++t) acc.x[t] = fma(fma(h1, s1[t], h0 * s0[t]), df[t], acc.x[t]);
    const double wk = wgt * k1;
    acc.f1 = fma(wk, d1, acc.f1);
    acc.f2 = fma(wk, d2, acc.f2);
  }
}

template <int DXP, bool SKIP>
__global__ __launch_bounds__(THREADS) void ltf_cross_grad_kernel(
    const double* __restrict__ Xq, int64_t R, int q, const double* __restrict__ Xt, int64_t n,
    Cols cl, const double* __restrict__ hyper, double p, double o,
    const double* __restrict__ dKx, const double* __restrict__ G, double* __restrict__ dX) {
  __shared__ Shared s;
  __shared__ double xt[DXP][GT];
  __shared__ double ts1[GT], ts2[GT], tu1[GT], tu2[GT];
  stage_hyper(s, hyper, cl);
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t r = (int64_t)blockIdx.x * (THREADS / 64) + (tid >> 6);
  const bool live = r < R;
  double xq[DXP], s0[DXP], s1[DXP];
  GradAcc<DXP> acc;
  Fid fq = fid_zero();
#pragma unroll
  for (int t = 0; t < DXP; ++t) {
    xq[t] = 0.0;
    acc.x[t] = 0.0;
    s0[t] = o * s.il0[t] * s.il0[t];
    s1[t] = o * s.il1[t] * s.il1[t];
  }
  acc.f1 = acc.f2 = 0.0;
  if (live) {
    load_x<DXP>(Xq + r * cl.d, cl, xq);
    fq = fid_of(Xq + r * cl.d, cl);
  }
  const bool shut = SKIP && at_target(fq, cl.nf) && !fq.m1 && !fq.m2;  // uniform over the wave
  for (int64_t k0 = 0; k0 < n; k0 += GT) {
    __syncthreads();
    {
      const int64_t k = k0 + tid;  // GT == THREADS: one training row per thread
      double xk[DXP];
      Fid fk = fid_zero();
#pragma unroll
      for (int t = 0; t < DXP; ++t) xk[t] = 0.0;
      if (k < n) {
        load_x<DXP>(Xt + k * cl.d, cl, xk);
        fk = fid_of(Xt + k * cl.d, cl);
      }
#pragma unroll
      for (int t = 0; t < DXP; ++t) xt[t][tid] = xk[t];
      ts1[tid] = fk.s1, ts2[tid] = fk.s2, tu1[tid] = fk.u1, tu2[tid] = fk.u2;
    }
    __syncthreads();
    if (!live) continue;
    const int cnt = (int)((n - k0 < GT) ? n - k0 : GT);
    for (int e = lane; e < cnt; e += 64) {
      double xo[DXP];
      Fid fo;
#pragma unroll
      for (int t = 0; t < DXP; ++t) xo[t] = xt[t][e];
      fo.s1 = ts1[e], fo.s2 = ts2[e], fo.u1 = tu1[e], fo.u2 = tu2[e];
      fo.m1 = fo.m2 = 0;
      const double wgt = dKx[r * n + k0 + e];
      if (shut) grad_pair<DXP, false>(acc, xq, fq, xo, fo, wgt, s, s0, s1, p, cl.nf);
      else grad_pair<DXP, true>(acc, xq, fq, xo, fo, wgt, s, s0, s1, p, cl.nf);
    }
  }
  if (!live) return;
  const int64_t b0 = (r / q) * q;
  for (int c = lane; c < q; c += 64) {
    double xo[DXP];
    load_x<DXP>(Xq + (b0 + c) * cl.d, cl, xo);
    const Fid fo = fid_of(Xq + (b0 + c) * cl.d, cl);
    const double wgt = G[r * q + c];
    if (shut) grad_pair<DXP, false>(acc, xq, fq, xo, fo, wgt, s, s0, s1, p, cl.nf);
    else grad_pair<DXP, true>(acc, xq, fq, xo, fo, wgt, s, s0, s1, p, cl.nf);
  }
  double out = 0.0;
#pragma unroll
  for (int t = 0; t < DXP; ++t) {
    const double v = wave_sum(acc.x[t]);
    out = (t < cl.dx && cl.x[t] == lane) ? v : out;
  }
  {
    const double v1 = o * wave_sum(acc.f1), v2 = o * wave_sum(acc.f2);
    out = (cl.f[0] == lane) ? v1 : out;
    out = (cl.nf == 2 && cl.f[1] == lane) ? v2 : out;
  }
  if (lane < cl.d) dX[r * cl.d + lane] = out;
}

int check_cols(const char* who, int d, int dx, int nf, const int32_t* xc, const int32_t* fc) {
  BO_CHECK_ARG(dx >= 1 && dx <= MAXD && nf >= 1 && nf <= 2 && d == dx + nf,
               "%s: d_x = %d, n_f = %d, d = %d (d_x 1..%d, n_f 1..2, d = d_x + n_f)", who, dx, nf,
               d, MAXD);
  return check_partition(who, d, dx, xc, nf, fc);
}

}  // namespace

#define BO_LTF_COLS(who, a)                                                                \
  do {                                                                                     \
    const int _st = check_cols(who, (a)->d, (a)->d_x, (a)->n_f, (a)->x_cols, (a)->f_cols); \
    if (_st != BO_OK) return _st;                                                          \
  } while (0)

extern "C" int bo_ltf_covar_impl(const BoLtfCovarArgs* a, void* stream) {
  BO_LTF_COLS("bo_ltf_covar", a);
  BO_CHECK_ARG(a->n >= 0 && a->np >= a->n && a->np % 128 == 0,
               "bo_ltf_covar: n = %lld, np = %lld (np >= n, a multiple of 128)", (long long)a->n,
               (long long)a->np);
  if (a->np == 0) return BO_OK;
  BO_CHECK_ARG(a->A && a->hyper && (a->n == 0 || a->X), "bo_ltf_covar: X, hyper and A are required");
  BO_CHECK_ARG(ceil_div(a->np, CV_ROWS) <= 65535, "bo_ltf_covar: np = %lld is too large",
               (long long)a->np);
  const Cols cl = make_cols(a->d, a->d_x, a->n_f, a->x_cols, a->f_cols);
  dim3 grid((unsigned)ceil_div(a->np, THREADS), (unsigned)ceil_div(a->np, CV_ROWS));
  hipStream_t st = as_stream(stream);
#define BO_GO(DXP)                                                                            \
  ltf_covar_kernel<DXP><<<grid, THREADS, 0, st>>>(a->X, a->n, cl, a->hyper, a->power, a->o,   \
                                                  a->noise, a->noise_vec, a->A, a->np)
  if (a->d_x <= 8) BO_GO(8); else BO_GO(16);
#undef BO_GO
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_ltf_mll_terms_impl(const BoLtfMllArgs* a, void* stream) {
  BO_LTF_COLS("bo_ltf_mll_terms", a);
  BO_CHECK_ARG(a->n >= 0 && a->n < (int64_t(1) << 31) && a->ld >= a->n,
               "bo_ltf_mll_terms: n = %lld, ld = %lld", (long long)a->n, (long long)a->ld);
  if (a->n == 0) return BO_OK;
  BO_CHECK_ARG(a->X && a->hyper && a->L && a->Ainv && a->alpha && a->beta && a->partial,
               "bo_ltf_mll_terms: every pointer is required");
  const Cols cl = make_cols(a->d, a->d_x, a->n_f, a->x_cols, a->f_cols);
  hipStream_t st = as_stream(stream);
#define BO_GO(DXP)                                                                              \
  ltf_mll_terms_kernel<DXP><<<(unsigned)a->n, THREADS, 0, st>>>(                                \
      a->X, (int)a->n, cl, a->hyper, a->power, a->o, a->L, a->Ainv, a->ld, a->alpha, a->beta,   \
      a->partial)
  if (a->d_x <= 8) BO_GO(8); else BO_GO(16);
#undef BO_GO
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_ltf_cross_impl(const BoLtfCrossArgs* a, void* stream) {
  BO_LTF_COLS("bo_ltf_cross", a);
  if (int st = check_cross("bo_ltf_cross", a)) return st;
  const int64_t R = a->B * a->q;
  if (R == 0) return BO_OK;
  BO_CHECK_ARG(a->Kxx && (a->n == 0 || a->Kx), "bo_ltf_cross: Kx and Kxx are required");
  BO_CHECK_ARG(ceil_div(R, CR_ROWS) <= 65535, "bo_ltf_cross: %lld query rows are too many",
               (long long)R);
  const Cols cl = make_cols(a->d, a->d_x, a->n_f, a->x_cols, a->f_cols);
  dim3 grid((unsigned)ceil_div(a->n, THREADS) + 1, (unsigned)ceil_div(R, CR_ROWS));
  hipStream_t st = as_stream(stream);
#define BO_GO(DXP, SKIP)                                                                     \
  ltf_cross_kernel<DXP, SKIP><<<grid, THREADS, 0, st>>>(a->Xq, R, (int)a->q, a->Xt, a->n, cl, \
                                                        a->hyper, a->power, a->o, a->Kx, a->Kxx)
  if (a->d_x <= 8) {
    if (a->no_skip) BO_GO(8, false); else BO_GO(8, true);
  } else {
    if (a->no_skip) BO_GO(16, false); else BO_GO(16, true);
  }
#undef BO_GO
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_ltf_cross_grad_impl(const BoLtfCrossArgs* a, void* stream) {
  BO_LTF_COLS("bo_ltf_cross_grad", a);
  if (int st = check_cross("bo_ltf_cross_grad", a)) return st;
  const int64_t R = a->B * a->q;
  if (R == 0) return BO_OK;
  BO_CHECK_ARG(a->G && a->dX && (a->n == 0 || a->dKx),
               "bo_ltf_cross_grad: dKx, G and dX are required");
  const Cols cl = make_cols(a->d, a->d_x, a->n_f, a->x_cols, a->f_cols);
  const unsigned grid = (unsigned)ceil_div(R, THREADS / 64);
  hipStream_t st = as_stream(stream);
#define BO_GO(DXP, SKIP)                                                                        \
  ltf_cross_grad_kernel<DXP, SKIP><<<grid, THREADS, 0, st>>>(a->Xq, R, (int)a->q, a->Xt, a->n,  \
                                                             cl, a->hyper, a->power, a->o,      \
                                                             a->dKx, a->G, a->dX)
  if (a->d_x <= 8) {
    if (a->no_skip) BO_GO(8, false); else BO_GO(8, true);
  } else {
    if (a->no_skip) BO_GO(16, false); else BO_GO(16, true);
  }
#undef BO_GO
  BO_LAUNCH_CHECK();
  return BO_OK;
}
