// The 16-row tile of X shared by the kernels that contract kernel rows on the
// fp64 matrix cores (paths.hip, jes.hip, nipv.hip).
//
// Lane layout.  The tile's 16 rows of X, divided by the lengthscale, sit in LDS
// with the odd row stride ldx = d | 1.  Lane l works for row l & 15 on slot
// l >> 4: per step it takes four points (training points, optima, features),
// forms its number for each from the squared distance to its row (a runtime
// loop over d) and hands it to v_mfma_f64_16x16x4 as its own operand element,
// so kernel rows never leave the registers.  The points of a lane are either
// ib + m (ib = i0 + 4 (l >> 4): the lane's A / V elements are contiguous) or
// i0 + (l >> 4) + 4 m (the rows in which an accumulator leaves the lane).
// Points past the end are clamped to point 0 for the loads and masked to zero
// by the caller; coordinates past d are zero operands.
//
// dX of the tile is accumulated in scaled coordinates as dX[row][:] -= q point[:]
// per (row, point) pair with dk = q (x_row - point), accd[tt] holding
// dX[row = (l >> 4) + 4 r][t = 16 tt + (l & 15)]; x_row sum q is added at the end.
#pragma once

#include "common.h"

constexpr int ROWTILE = 16;

// rows r0 .. r0 + 15 of X divided by the lengthscale -> xs, by nthreads threads;
// rows from rows_valid on, or past R, are zeros
__device__ __forceinline__ void rowtile_load(const double* X, const double* ls, int64_t r0,
                                             int rows_valid, int64_t R, int d, int ldx, double* xs,
                                             int tid, int nthreads) {
  for (int e = tid; e < ROWTILE * d; e += nthreads) {
    const int rr = e / d, t = e - rr * d;
    const int64_t r = r0 + rr;
    xs[rr * ldx + t] = rr < rows_valid && r < R ? X[r * d + t] / ls[t] : 0.0;
  }
}

// squared distance of the lane's row to one point (scaled coordinates)
__device__ __forceinline__ double rowtile_dist2(const double* xr, const double* xo, int d) {
  double d2 = 0.0;
  for (int t = 0; t < d; ++t) {
    const double df = xr[t] - xo[t];
    d2 = fma(df, df, d2);
  }
  return d2;
}

// xt[m], d2[m]: point ib + STEP m of Xts (point 0 past n) and its squared
// distance to the lane's row
template <int STEP>
__device__ __forceinline__ void rowtile_dist2x4(const double* xr, const double* Xts, int64_t ib,
                                                int64_t n, int d, const double* (&xt)[4],
                                                double (&d2)[4]) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int64_t i = ib + STEP * m;
    xt[m] = Xts + (i < n ? i : 0) * d;
    d2[m] = 0.0;
  }
  for (int t = 0; t < d; ++t) {
    const double x = xr[t];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const double df = x - xt[m][t];
      d2[m] = fma(df, df, d2[m]);
    }
  }
}

// dX[row][:] -= q src[:] over the NDT column tiles (d <= 16 NDT): q is the lane's
// A element, src its own point (B[k = l >> 4][t = l & 15]), row = l & 15
template <int NDT>
__device__ __forceinline__ void rowtile_dx_acc(double q, bool ok, const double* src, int d, int row,
                                               v4d (&accd)[NDT]) {
#pragma unroll
  for (int tt = 0; tt < NDT; ++tt) {
    const int t = 16 * tt + row;
    const double b = ok && t < d ? src[t] : 0.0;
    accd[tt] = mfma_f64(-q, b, accd[tt]);
  }
}

// the sum of v over a row's four slots, in every lane of the row, in a fixed order
__device__ __forceinline__ double rowtile_fold4(double v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// dX[r0 + row][t] = scale (accd + x_row sumq) / ls[t]; sumq is the row's folded
// sum of q, held by the lanes l & 15 = row.  All lanes of the wave take part.
template <int NDT>
__device__ __forceinline__ void rowtile_dx_store(double* dX, const v4d (&accd)[NDT],
                                                 const double* xs, int ldx, double sumq,
                                                 double scale, const double* ls, int64_t r0,
                                                 int64_t R, int d, int lane) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ro = mfma_row(lane, r);
    const double sq = __shfl(sumq, ro);
#pragma unroll
    for (int tt = 0; tt < NDT; ++tt) {
      const int t = 16 * tt + (lane & 15);
      if (t < d && r0 + ro < R)
        dX[(r0 + ro) * d + t] = scale * (accd[tt][r] + xs[ro * ldx + t] * sq) / ls[t];
    }
  }
}

// LAUNCH(KIND, NDT) for the kernel kind and the column tiles that cover d <= 128
#define ROWTILE_DISPATCH_KIND(kind, NDT, LAUNCH) \
  do {                                           \
    if ((kind) == BO_RBF) LAUNCH(BO_RBF, NDT);   \
    else LAUNCH(BO_MATERN52, NDT);               \
  } while (0)
#define ROWTILE_DISPATCH(kind, d, LAUNCH)                        \
  do {                                                           \
    if ((d) <= 16) ROWTILE_DISPATCH_KIND(kind, 1, LAUNCH);       \
    else if ((d) <= 32) ROWTILE_DISPATCH_KIND(kind, 2, LAUNCH);  \
    else if ((d) <= 64) ROWTILE_DISPATCH_KIND(kind, 4, LAUNCH);  \
    else ROWTILE_DISPATCH_KIND(kind, 8, LAUNCH);                 \
  } while (0)

// the argument checks that every caller of the tile shares
static inline int rowtile_check_common(int kind, int d, int64_t n, const double* Xt_scaled,
                                       const double* V, double outputscale, const char* who) {
  BO_CHECK_ARG(kind == BO_RBF || kind == BO_MATERN52, "%s: unknown kernel kind %d", who, kind);
  BO_CHECK_ARG(d >= 1 && d <= 128, "%s: 1 <= d <= 128 (got %d)", who, d);
  BO_CHECK_ARG(n == 0 || (Xt_scaled && V), "%s: Xt_scaled and V are required when n > 0", who);
  BO_CHECK_ARG(outputscale >= 0.0, "%s: outputscale >= 0", who);
  return BO_OK;
}
