// Bordered update of the exact-GP prediction caches on gfx950: the caches of
// the n + k point model from those of the n point model, without refactoring.
//
// Replaces, for Model.condition_on_observations (botorch/models/gpytorch.py:
// 468-531 -> [G] ExactGP.get_fantasy_model), the rebuild of
//   L' = chol(K' + s2 I),  Linv' = L'^{-1},  U' = L'^{-T},  beta', alpha'
// on the concatenated data.  With A = L L^T the old matrix and X2 the k new
// points, the new factor is the old one with a k-row border (the last block
// row of a blocked Cholesky):
//   B    = K(X2, X1) L^{-T}                      (k x n)
//   S    = K(X2, X2) + s2 - B B^T,  L22 = chol(S)
//   C    = -L22^{-1} B L^{-1}                    (k x n)
//   L'    = [[L, 0], [B, L22]],  Linv' = [[Linv, 0], [C, L22^{-1}]],  U' = Linv'^T
//   beta' = [beta; b2],  b2 = L22^{-1} (y2 - c - B beta)
//   alpha' = [alpha + C^T b2; L22^{-T} b2]
// O(n^2 k) flops and a few streaming passes over L^{-1} instead of the
// O(n^3) factorisation.
//
// The border is applied in blocks of <= 16 rows (one v_mfma_f64_16x16x4f64
// tile); each later block sees the rows the earlier ones wrote.  Every launch
// is a plain stream-ordered launch; no workgroup waits on another.
//   copy    L, Linv -> L', Linv', Linv^T -> U' at the new padded order, with the
//           identity pad and zero opposite triangle a fresh build leaves
//   per block of kb rows at current order m:
//     kx      Kx = K(X1', X2) (m x 16) from the scaled inputs
//     rows<0> Bt = Linv' Kx: 16-row tiles stream their rows of Linv' once
//             (columns <= row); B -> rows m.. of L'; per-tile partials of
//             B B^T and B beta
//     reduce  the tiles' partials summed in a fixed order
//     border  one workgroup: S, its Cholesky (status, no retry), L22^{-1},
//             b2, the trailing blocks and the tails of beta', alpha'
//     rows<1> Dt = U' Bt (columns >= row; the second read of L^{-1}),
//             C^T = -Dt L22^{-T} -> columns m.. of U' and rows m.. of Linv',
//             alpha'[:m] += C^T b2
#include "common.h"

namespace {

constexpr int CE_T = 16;       // border rows per block = the MFMA tile
constexpr int CE_DP = 8;       // width of Xt_scaled
constexpr int CE_PART = 272;   // per row tile: 16 x 16 of B B^T + 16 of B beta
constexpr int CE_TILE = 64;    // copy kernel's tile
constexpr int CE_WAVES = 8;    // waves of a row tile's workgroup (loads in flight per CU)

__device__ __forceinline__ double ce_kernel(int kind, double d2) {
  return kind == BO_RBF ? kernel_from_d2<BO_RBF>(d2) : kernel_from_d2<BO_MATERN52>(d2);
}

__device__ __forceinline__ double ce_d2(const double* __restrict__ a,
                                        const double* __restrict__ b) {
  double d2 = 0.0;
#pragma unroll
  for (int t = 0; t < CE_DP; ++t) {
    const double diff = a[t] - b[t];
    d2 = fma(diff, diff, d2);
  }
  return d2;
}

// L, Linv (order n, leading dimension ld) -> Lo, Linvo, Uo = Linv^T (order
// npo, leading dimension ldo): 64 x 64 tiles, 16-B accesses.  128-blocks
// strictly above the diagonal are zero in a built cache and are not read;
// rows / columns >= n get the identity pad.
__global__ __launch_bounds__(256) void ce_copy_kernel(
    const double* __restrict__ L, const double* __restrict__ Linv, int64_t ld, int64_t n,
    double* __restrict__ Lo, double* __restrict__ Linvo, double* __restrict__ Uo, int64_t ldo,
    int64_t npo) {
  __shared__ double tile[CE_TILE][CE_TILE + 1];
  const int64_t by = (int64_t)blockIdx.y * CE_TILE, bx = (int64_t)blockIdx.x * CE_TILE;
  const int c2 = threadIdx.x & 31, rr = threadIdx.x >> 5;
  const bool upper = (bx / 128) > (by / 128);
  for (int r = rr; r < CE_TILE; r += 8) {
    const int64_t gi = by + r, gj = bx + 2 * c2;
    double2 vl, vi;
    vl.x = vi.x = (gi == gj) ? 1.0 : 0.0;
    vl.y = vi.y = (gi == gj + 1) ? 1.0 : 0.0;
    if (!upper && gi < n && gj < n) {
      const double2 a = *reinterpret_cast<const double2*>(&L[gi * ld + gj]);
      const double2 b = *reinterpret_cast<const double2*>(&Linv[gi * ld + gj]);
      vl.x = a.x;
      vi.x = b.x;
      if (gj + 1 < n) {
        vl.y = a.y;
        vi.y = b.y;
      }
    }
    *reinterpret_cast<double2*>(&Lo[gi * ldo + gj]) = vl;
    *reinterpret_cast<double2*>(&Linvo[gi * ldo + gj]) = vi;
    tile[r][2 * c2] = vi.x;
    tile[r][2 * c2 + 1] = vi.y;
  }
  __syncthreads();
  for (int r = rr; r < CE_TILE; r += 8) {
    double2 v;
    v.x = tile[2 * c2][r];
    v.y = tile[2 * c2 + 1][r];
    *reinterpret_cast<double2*>(&Uo[(bx + r) * ldo + by + 2 * c2]) = v;
  }
}

// Kx[i][c] = outputscale k(x_i, x_{m+c}), i < m, c < kb; zero elsewhere over
// mp16 x 16 (Xs: the scaled inputs, old rows then new ones).
__global__ __launch_bounds__(256) void ce_kx_kernel(int kind, const double* __restrict__ Xs,
                                                    int64_t m, int kb, int64_t mp16,
                                                    double outputscale, double* __restrict__ Kx) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= mp16 * CE_T) return;
  const int64_t i = idx / CE_T;
  const int c = (int)(idx % CE_T);
  double v = 0.0;
  if (i < m && c < kb)
    v = outputscale * ce_kernel(kind, ce_d2(Xs + i * CE_DP, Xs + (m + c) * CE_DP));
  Kx[idx] = v;
}

// One 16-row tile of A (order m, rows streamed once with 16-B loads) times the
// m x 16 operand Bop on the fp64 matrix cores; the CE_WAVES waves split the
// columns in chunks of 8 and are summed in wave order through LDS (the first
// 256 threads run the epilogue).
//   MODE 0: A = Linv' (columns <= row), Bop = Kx.  Writes Bt (mp16 x 16, zero
//           rows >= m), B into rows m.. of L', and the tile's partials of
//           B B^T and B beta.
//   MODE 1: A = U' (columns >= row), Bop = Bt.  Writes C^T = -(U' Bt) L22^{-T}
//           into columns m.. of U' and rows m.. of Linv', and adds C^T b2 to
//           alpha'.
template <int MODE>
__global__ __launch_bounds__(64 * CE_WAVES) void ce_rows_kernel(
    const double* A, int64_t ld, int64_t m, int kb, int64_t mp16, const double* Bop, double* Bt,
    double* Lo, double* Linvo, double* Uo, const double* __restrict__ beta,
    double* __restrict__ alpha, double* __restrict__ part, const double* __restrict__ small) {
  __shared__ double red[CE_WAVES][CE_T][CE_T + 1];
  __shared__ double tl[CE_T][CE_T + 1];
  __shared__ double ct[CE_T][CE_T + 1];
  __shared__ double li[CE_T][CE_T + 1];
  __shared__ double b2[CE_T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the longest rows first
  const int64_t rt = MODE == 0 ? (int64_t)gridDim.x - 1 - blockIdx.x : (int64_t)blockIdx.x;
  const int64_t r0 = rt * CE_T;
  const int64_t k0 = MODE == 0 ? 0 : r0;
  const int64_t k1 = MODE == 0 ? r0 + CE_T : mp16;
  const bool ep = threadIdx.x < 256;  // the epilogue's threads
  if (MODE == 1 && ep) {
    li[threadIdx.x >> 4][threadIdx.x & 15] = small[threadIdx.x];
    if (threadIdx.x < CE_T) b2[threadIdx.x] = small[256 + threadIdx.x];
  }
  const int64_t row = r0 + (lane & 15);
  const int kq = lane >> 4;
  const double* arow = A + row * ld;
  v4d acc = v4d_zero();
  constexpr int KSTEP = 8 * CE_WAVES;
  const int nit = (int)((k1 - k0 - 8 * wave + KSTEP - 1) / KSTEP);
  // 4 chunks in flight per wave; a chunk past the end rereads chunk `it` as zeros
  for (int it = 0; it < nit; it += 4) {
    double2 a[4];
    double b0[4], b1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool on = it + u < nit;
      const int64_t kk = k0 + 8 * wave + KSTEP * (int64_t)(on ? it + u : it) + 2 * kq;
      a[u] = *reinterpret_cast<const double2*>(&arow[kk]);
      // only the triangle: whatever the opposite one holds inside a diagonal tile
      if (!on || (MODE == 0 ? kk > row : kk < row)) a[u].x = 0.0;
      if (!on || (MODE == 0 ? kk + 1 > row : kk + 1 < row)) a[u].y = 0.0;
      b0[u] = Bop[kk * CE_T + (lane & 15)];
      b1[u] = Bop[(kk + 1) * CE_T + (lane & 15)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc = mfma_f64(a[u].x, b0[u], acc);
      acc = mfma_f64(a[u].y, b1[u], acc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][mfma_row(lane, r)][mfma_col(lane)] = acc[r];
  __syncthreads();
  const int ti = (threadIdx.x >> 4) & 15, tj = threadIdx.x & 15;
  if (ep) {
    double v = red[0][ti][tj];
#pragma unroll
    for (int w = 1; w < CE_WAVES; ++w) v += red[w][ti][tj];
    tl[ti][tj] = (r0 + ti < m) ? v : 0.0;
  }
  __syncthreads();
  if (MODE == 0) {
    if (!ep) return;  // no barrier below
    Bt[(r0 + ti) * CE_T + tj] = tl[ti][tj];
    // B[c = ti][row r0 + tj]: 128-B row segments of L'
    if (r0 + tj < m && ti < kb) Lo[(m + ti) * ld + r0 + tj] = tl[tj][ti];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < CE_T; ++i) s = fma(tl[i][ti], tl[i][tj], s);
    part[rt * CE_PART + threadIdx.x] = s;
    if (threadIdx.x < CE_T) {
      double mb = 0.0;
      for (int i = 0; i < CE_T; ++i)
        if (r0 + i < m) mb = fma(tl[i][threadIdx.x], beta[r0 + i], mb);
      part[rt * CE_PART + 256 + threadIdx.x] = mb;
    }
  } else {
    // C^T[j = ti][a = tj] = -sum_c Dt[j][c] L22inv[a][c]
    if (ep) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < CE_T; ++c) s = fma(tl[ti][c], li[tj][c], s);
      s = -s;
      ct[ti][tj] = s;
      if (r0 + ti < m && tj < kb) Uo[(r0 + ti) * ld + m + tj] = s;
    }
    __syncthreads();
    if (!ep) return;
    if (r0 + tj < m && ti < kb) Linvo[(m + ti) * ld + r0 + tj] = ct[tj][ti];
    if (threadIdx.x < CE_T && r0 + threadIdx.x < m) {
      double da = 0.0;
      for (int a = 0; a < kb; ++a) da = fma(ct[threadIdx.x][a], b2[a], da);
      alpha[r0 + threadIdx.x] += da;
    }
  }
}

// sums[o] = sum over the row tiles w of part[w][o], o < CE_PART: workgroup j
// takes outputs 16 j .. 16 j + 15 (128-B segments), its 16 thread rows the
// tiles w = g mod 16, added in g order through LDS.
__global__ __launch_bounds__(256) void ce_reduce_kernel(const double* __restrict__ part,
                                                        int ntiles, double* __restrict__ sums) {
  __shared__ double red[CE_T][CE_T + 1];
  const int g = threadIdx.x >> 4, o = blockIdx.x * CE_T + (threadIdx.x & 15);
  double s = 0.0;
#pragma unroll 4
  for (int w = g; w < ntiles; w += CE_T) s += part[(int64_t)w * CE_PART + o];
  red[g][threadIdx.x & 15] = s;
  __syncthreads();
  if (threadIdx.x < CE_T) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < CE_T; ++i) t += red[i][threadIdx.x];
    sums[o] = t;
  }
}

// The k x k border of one block (one workgroup): S = K22 + noise - B B^T from
// the row tiles' summed partials, its Cholesky (a non-positive pivot is reported in
// *info as its 1-based global index and replaced by 1: no retry, the caller
// rebuilds), L22^{-1}, b2 = L22^{-1}(y2 - c - B beta), and the trailing
// blocks of L', Linv', U', beta', alpha'.  small: L22^{-1} (16 x 16, identity
// beyond kb) then b2 (16), for rows<1>.
__global__ __launch_bounds__(256) void ce_border_kernel(
    int kind, const double* __restrict__ Xs, int64_t m, int kb, double outputscale,
    double noise, const double* __restrict__ noise_vec, double constant,
    const double* __restrict__ y2, const double* __restrict__ sums, double* __restrict__ Lo,
    double* __restrict__ Linvo, double* __restrict__ Uo, int64_t ld, double* __restrict__ beta,
    double* __restrict__ alpha, double* __restrict__ small, int* __restrict__ info) {
  __shared__ double S[CE_T][CE_T + 1];
  __shared__ double Li[CE_T][CE_T + 1];
  __shared__ double rhs[CE_T], bb[CE_T];
  __shared__ int bad;
  const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
  if (threadIdx.x == 0) bad = 0;
  {
    const double s = sums[threadIdx.x];
    double v = (a == b) ? 1.0 : 0.0;
    if (a < kb && b < kb) {
      v = outputscale * ce_kernel(kind, ce_d2(Xs + (m + a) * CE_DP, Xs + (m + b) * CE_DP));
      if (a == b) v += noise_vec ? noise_vec[a] : noise;
      v -= s;
    }
    S[a][b] = v;
  }
  if (threadIdx.x < CE_T) {
    const double s = sums[256 + threadIdx.x];
    rhs[threadIdx.x] = threadIdx.x < kb ? (y2[threadIdx.x] - constant) - s : 0.0;
  }
  __syncthreads();
  for (int j = 0; j < CE_T; ++j) {
    double piv = S[j][j];
    const bool ok = piv > 0.0;  // false for NaN too
    if (!ok) piv = 1.0;
    const double dj = sqrt(piv);
    __syncthreads();
    if (threadIdx.x == 0 && !ok && bad == 0) bad = j + 1;
    if (b == j && a >= j) S[a][j] = (a == j) ? dj : S[a][j] / dj;
    __syncthreads();
    if (a > j && b > j && b <= a) S[a][b] -= S[a][j] * S[b][j];
    __syncthreads();
  }
  if (b > a) S[a][b] = 0.0;
  __syncthreads();
  // L22^{-1} by forward substitution, one column per thread
  if (threadIdx.x < CE_T) {
    const int c = threadIdx.x;
    for (int i = 0; i < CE_T; ++i) {
      double x = 0.0;
      if (i >= c) {
        double s = (i == c) ? 1.0 : 0.0;
        for (int p = c; p < i; ++p) s -= S[i][p] * Li[p][c];
        x = s / S[i][i];
      }
      Li[i][c] = x;
    }
  }
  __syncthreads();
  if (threadIdx.x < CE_T) {
    double s = 0.0;
    for (int c = 0; c <= threadIdx.x; ++c) s = fma(Li[threadIdx.x][c], rhs[c], s);
    bb[threadIdx.x] = s;  // b2
  }
  __syncthreads();
  small[threadIdx.x] = Li[a][b];
  if (threadIdx.x < CE_T) {
    small[256 + threadIdx.x] = bb[threadIdx.x];
    if (threadIdx.x < kb) {
      double s = 0.0;
      for (int c = threadIdx.x; c < kb; ++c) s = fma(Li[c][threadIdx.x], bb[c], s);
      beta[m + threadIdx.x] = bb[threadIdx.x];
      alpha[m + threadIdx.x] = s;
    }
  }
  if (a < kb && b < kb) {
    Lo[(m + a) * ld + m + b] = S[a][b];
    Linvo[(m + a) * ld + m + b] = Li[a][b];
    Uo[(m + b) * ld + m + a] = Li[a][b];
  }
  if (threadIdx.x == 0 && bad != 0 && *info == 0) *info = (int)(m + bad);
}

}  // namespace

extern "C" {

int bo_gp_cache_extend_work(int64_t n, int k, int64_t* work_elems) {
  BO_CHECK_ARG(work_elems != nullptr, "bo_gp_cache_extend_work: work_elems is NULL");
  BO_CHECK_ARG(n >= 1 && k >= 1, "bo_gp_cache_extend_work: n = %lld, k = %d (both >= 1)",
               (long long)n, k);
  const int64_t mp16 = ceil_div(n + k, CE_T) * CE_T;
  // Kx, Bt (mp16 x 16 each), the row tiles' partials, their sums, L22^{-1} and b2
  *work_elems = 2 * mp16 * CE_T + (mp16 / CE_T) * CE_PART + 2 * CE_PART;
  return BO_OK;
}

int bo_gp_cache_extend(int kind, const double* Xt_scaled, const double* L, const double* Linv,
                       const double* beta, const double* alpha, int64_t ld, int64_t n, int d,
                       const double* lengthscale, double outputscale, double constant,
                       const double* X_new, const double* y_new, int k, double noise,
                       const double* noise_vec, double* Xt_scaled_out, double* L_out,
                       double* Linv_out, double* U_out, double* beta_out, double* alpha_out,
                       int64_t ld_out, double* work, int* info, void* stream) {
  BO_CHECK_ARG(kind == BO_RBF || kind == BO_MATERN52, "bo_gp_cache_extend: bad kind %d", kind);
  BO_CHECK_ARG(k >= 1, "bo_gp_cache_extend: k = %d new points (at least 1)", k);
  BO_CHECK_ARG(n >= 1, "bo_gp_cache_extend: n = %lld (at least 1)", (long long)n);
  BO_CHECK_ARG(d >= 1 && d <= CE_DP, "bo_gp_cache_extend: d = %d (1..%d, the width of Xt_scaled)",
               d, CE_DP);
  const int64_t npo = bo_padded_order(n + k);
  BO_CHECK_ARG(ld >= n && ld % 2 == 0 && ld >= ceil_div(n, 2) * 2,
               "bo_gp_cache_extend: leading dimension %lld of the old caches (even, >= n = %lld)",
               (long long)ld, (long long)n);
  BO_CHECK_ARG(ld_out >= npo && ld_out % 2 == 0,
               "bo_gp_cache_extend: leading dimension %lld of the new caches (even, >= "
               "bo_padded_order(n + k) = %lld)", (long long)ld_out, (long long)npo);
  BO_CHECK_ARG(Xt_scaled && L && Linv && beta && alpha && lengthscale && X_new && y_new &&
                   Xt_scaled_out && L_out && Linv_out && U_out && beta_out && alpha_out && work &&
                   info,
               "bo_gp_cache_extend: NULL buffer");
  BO_CHECK_ARG((((uintptr_t)L | (uintptr_t)Linv | (uintptr_t)L_out | (uintptr_t)Linv_out |
                 (uintptr_t)U_out | (uintptr_t)work) & 15) == 0,
               "bo_gp_cache_extend: L, Linv, their outputs, U' and work must be 16-B aligned");
  hipStream_t st = as_stream(stream);

  BO_HIP(hipMemcpyAsync(Xt_scaled_out, Xt_scaled, sizeof(double) * n * CE_DP,
                        hipMemcpyDeviceToDevice, st));
  BO_HIP(hipMemcpyAsync(beta_out, beta, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  BO_HIP(hipMemcpyAsync(alpha_out, alpha, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
  int s = bo_scale_inputs(X_new, k, d, lengthscale, nullptr, CE_DP, Xt_scaled_out + n * CE_DP,
                          stream);
  if (s) return s;
  {
    dim3 grid((unsigned)(npo / CE_TILE), (unsigned)(npo / CE_TILE));
    ce_copy_kernel<<<grid, 256, 0, st>>>(L, Linv, ld, n, L_out, Linv_out, U_out, ld_out, npo);
    BO_LAUNCH_CHECK();
  }
  const int64_t mp16max = ceil_div(n + k, CE_T) * CE_T;
  double* Kx = work;
  double* Bt = Kx + mp16max * CE_T;
  double* part = Bt + mp16max * CE_T;
  double* sums = part + (mp16max / CE_T) * CE_PART;
  double* small = sums + CE_PART;
  for (int done = 0; done < k; done += CE_T) {
    const int kb = k - done < CE_T ? k - done : CE_T;
    const int64_t m = n + done;
    const int64_t mp16 = ceil_div(m, CE_T) * CE_T;
    const unsigned ntiles = (unsigned)(mp16 / CE_T);
    ce_kx_kernel<<<(unsigned)ceil_div(mp16 * CE_T, 256), 256, 0, st>>>(kind, Xt_scaled_out, m, kb,
                                                                      mp16, outputscale, Kx);
    BO_LAUNCH_CHECK();
    ce_rows_kernel<0><<<ntiles, 64 * CE_WAVES, 0, st>>>(Linv_out, ld_out, m, kb, mp16, Kx, Bt, L_out,
                                              Linv_out, U_out, beta_out, alpha_out, part, small);
    BO_LAUNCH_CHECK();
    ce_reduce_kernel<<<CE_PART / CE_T, 256, 0, st>>>(part, (int)ntiles, sums);
    BO_LAUNCH_CHECK();
    ce_border_kernel<<<1, 256, 0, st>>>(kind, Xt_scaled_out, m, kb, outputscale, noise,
                                        noise_vec ? noise_vec + done : nullptr, constant,
                                        y_new + done, sums, L_out, Linv_out, U_out, ld_out,
                                        beta_out, alpha_out, small, info);
    BO_LAUNCH_CHECK();
    ce_rows_kernel<1><<<ntiles, 64 * CE_WAVES, 0, st>>>(U_out, ld_out, m, kb, mp16, Bt, Bt, L_out, Linv_out,
                                              U_out, beta_out, alpha_out, part, small);
    BO_LAUNCH_CHECK();
  }
  return BO_OK;
}

}  // extern "C"
