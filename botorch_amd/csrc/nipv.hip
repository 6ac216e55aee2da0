// qNegIntegratedPosteriorVariance (botorch/acquisition/active_learning.py:40-135):
// the Gram matrices of the posterior cross-covariance of every t-batch with N
// integration points, in one launch.  Observing q points X_b with noise tau2
// lowers the posterior variance at z by c(X_b, z)^T M_b^{-1} c(X_b, z), M_b =
// Sigma(X_b, X_b) + tau2 I, so the integrated variance needs only
//
//   c(x_i, z) = o k(x_i, z) - o sum_t k(x_i, Xt_t) V[z][t],  V[z] = A^{-1} o k(Xt, z)
//   G_b       = C_b C_b^T  (q x q),  C_b = [c(x_i, z)]  (q x N)
//
// with k the kernel without its outputscale o.  Neither C (R x N) nor the
// kernel rows (R x n) reach memory.
//
// Tile plan (the row tile and its lane layout: rowtile.h; here the tile belongs
// to the workgroup).  A workgroup of four waves owns one tile of 16 rows of X -- the
// floor(16 / q) t-batches that fit, so no t-batch straddles a tile -- and one
// slice of Z (blockIdx.y).  The slice is walked in passes of 128 points: wave w
// owns the 16-point tiles w and w + 4 of the pass (four tiles per wave would
// not fit two workgroups' registers on a CU without scratch).  The training
// points are walked in chunks of 64: wave w builds k(Xt_t, x_row) for the
// chunk's points 16 w .. 16 w + 15 (lane l: row l & 15, points (l >> 4) + 4 m)
// into LDS, once for the four waves, and every wave contracts the chunk against
// its own rows of V on v_mfma_f64_16x16x4: D[z][row] += V[z][t] k[t][row], the
// lane's A elements 16 consecutive doubles of one row of V.  The accumulator
// leaves lane l, register r, with C[z = (l >> 4) + 4 r][row = l & 15], which is
// at once the A element C^T[row][z-step] and the B element C[z-step][row] of
// G += C^T C: four MFMAs per 16-point tile with the register in both operand
// slots, no data movement.  Only the q x q diagonal blocks of the 16 x 16 tile
// are t-batches; the rest is dropped.  The four waves' tiles are summed through
// LDS in a fixed order; with more than one slice the partial Grams go to a
// workspace and a second kernel sums them in slice order.  No atomics: repeated
// calls are bitwise identical.
//
// Backward, from dG (B x q x q, arbitrary): per pass C is recomputed as above
// and written to LDS, dC[z][i] = sum_j C[z][j] (dG + dG^T)[j][i] is four more
// MFMAs per tile (A from LDS, the block-diagonal S = dG + dG^T in registers),
// the dk(x_i, z) term goes from the registers into dX, and dC of the whole pass
// (128 x 16) stays in LDS for the sweep over the training points, which is
// jes.hip's with dC in the place of its G_ij and the 16-point tiles of Xt dealt
// to the waves: coef[t][row] = sum_z V[z][t] dC[z][row], times dk / dd2, is the
// A element of dX[row][:] -= q[row][t] Xt[t][:].  The waves' dX tiles are added
// through LDS in wave order, the slices' through the workspace in slice order.
#include <algorithm>

#include "rowtile.h"

namespace {

constexpr int THREADS = 256;
constexpr int NW = THREADS / BO_WAVE;  // waves per workgroup
constexpr int TR = ROWTILE;            // rows of X per workgroup
constexpr int NT = 2;                  // 16-point tiles of Z per wave and pass
constexpr int PZ = 16 * NT * NW;       // integration points per pass
constexpr int TC = 16 * NW;            // training points per shared chunk
constexpr int KSLOT = 16 * TR + 16;    // a wave's 16 x 16 part of the chunk (+16: the four
                                       // slots of one ds_read_b64 fall on both bank halves)
constexpr int KS = NW * KSLOT;
constexpr int LDG = TR + 1;            // row stride of the pass's C / dC in LDS
constexpr int MAX_SPLIT = 1024;

struct Dev {
  int kind, d, q, tb, split;  // tb: t-batches per tile
  int64_t R, n, N, B, zlen;   // zlen: points per slice, a multiple of 16
  const double *X, *ls, *Xts, *Zs, *V;
  double o;
  double* G;
  const double* dG;
  double* dX;
  double* part;  // split > 1: the slices' partial outputs
};

// number of the wave's tiles 16 (wave + NW qq) of the pass at zp that begin
// before zend (wave-uniform)
__device__ __forceinline__ int wave_tiles(int64_t zp, int64_t zend, int wave) {
  int nt = 0;
#pragma unroll
  for (int qq = 0; qq < NT; ++qq) nt += zp + 16 * (wave + NW * qq) < zend;
  return nt;
}

// acc[qq][r] = sum_t V[zp + 16 (wave + NW qq) + (l >> 4) + 4 r][t] k(x_row, Xt_t)
// for the wave's ntw tiles; the kernel chunk goes through ks, built once for
// the workgroup.  Every wave of the workgroup calls it (barriers inside).
template <int KIND>
__device__ __forceinline__ void contract_v(const Dev& a, const double* xr, double* ks, int64_t zp,
                                           int64_t zend, int ntw, int lane, int wave, v4d* acc) {
  const int row = lane & 15, kk = lane >> 4;
  const double* vp[NT];  // the A operand's row of V, or null
#pragma unroll
  for (int qq = 0; qq < NT; ++qq) {
    const int64_t z = zp + 16 * (wave + NW * qq) + row;
    vp[qq] = qq < ntw && z < zend ? a.V + z * a.n : nullptr;
    acc[qq] = v4d_zero();
  }
  for (int64_t c0 = 0; c0 < a.n; c0 += TC) {
    {
      const int64_t ib = c0 + 16 * wave + kk;
      const double* xt[4];
      double d2[4];
      rowtile_dist2x4<4>(xr, a.Xts, ib, a.n, a.d, xt, d2);
#pragma unroll
      for (int m = 0; m < 4; ++m)
        ks[wave * KSLOT + (kk + 4 * m) * TR + row] =
            ib + 4 * m < a.n ? kernel_from_d2<KIND>(d2[m]) : 0.0;
    }
    __syncthreads();
    const int64_t tb0 = c0 + 16 * kk;  // the lane's 16 consecutive training points
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const bool tok = tb0 + s < a.n;
      const double b = ks[kk * KSLOT + s * TR + row];
#pragma unroll
      for (int qq = 0; qq < NT; ++qq) {
        if (qq < ntw) {
          const double v = tok && vp[qq] ? vp[qq][tb0 + s] : 0.0;
          acc[qq] = mfma_f64(v, b, acc[qq]);
        }
      }
    }
    __syncthreads();  // ks is rewritten by the next chunk
  }
}

template <int KIND>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(2))) void
nipv_gram_kernel(const Dev a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = a.d, ldx = d | 1, nr = a.tb * a.q;
  double* xs = smem;
  double* ks = xs + TR * ldx;
  const int64_t tile = blockIdx.x, r0 = tile * nr;
  const int64_t z0 = (int64_t)blockIdx.y * a.zlen, zend = min(a.N, z0 + a.zlen);
  rowtile_load(a.X, a.ls, r0, nr, a.R, d, ldx, xs, threadIdx.x, THREADS);
  __syncthreads();
  const int row = lane & 15;
  const double* xr = xs + row * ldx;
  v4d g = v4d_zero();  // G[(l >> 4) + 4 r][l & 15], the wave's tiles of Z
  for (int64_t zp = z0; zp < zend; zp += PZ) {
    const int ntw = wave_tiles(zp, zend, wave);
    v4d acc[NT];
    contract_v<KIND>(a, xr, ks, zp, zend, ntw, lane, wave, acc);
#pragma unroll
    for (int qq = 0; qq < NT; ++qq) {
      if (qq < ntw) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t z = zp + 16 * (wave + NW * qq) + mfma_row(lane, r);
          double c = 0.0;
          if (z < zend)
            c = a.o * (kernel_from_d2<KIND>(rowtile_dist2(xr, a.Zs + z * d, d)) - acc[qq][r]);
          g = mfma_f64(c, c, g);
        }
      }
    }
  }
  // the four waves' Grams in wave order; ks is free after contract_v's last barrier
  double* red = ks;
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave * 256 + mfma_row(lane, r) * 16 + row] = g[r];
  __syncthreads();
  const int e = threadIdx.x, i = e >> 4, j = e & 15;
  const double sum = ((red[e] + red[256 + e]) + red[512 + e]) + red[768 + e];
  const int64_t b = tile * a.tb + i / a.q;
  if (i < nr && j < nr && i / a.q == j / a.q && b < a.B) {
    double* dst = a.split > 1 ? a.part + (int64_t)blockIdx.y * a.B * a.q * a.q : a.G;
    dst[(b * a.q + i % a.q) * a.q + j % a.q] = sum;
  }
}

// out[e] = sum_s part[s][e], in slice order
__global__ __launch_bounds__(256) void nipv_sum_kernel(int split, int64_t total,
                                                       const double* part, double* out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  double s = part[e];
  for (int k = 1; k < split; ++k) s += part[k * total + e];
  out[e] = s;
}

// NDT: 16-column tiles of dX (d <= 16 NDT); two workgroups per CU up to NDT = 4
template <int KIND, int NDT>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(NDT <= 4 ? 2 : 1))) void
nipv_gram_backward_kernel(const Dev a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = a.d, ldx = d | 1, nr = a.tb * a.q;
  double* xs = smem;
  double* ks = xs + TR * ldx;
  double* gs = ks + KS;  // C, then dC, of the pass: [z of the pass][row], stride LDG
  const int64_t tile = blockIdx.x, r0 = tile * nr;
  const int64_t z0 = (int64_t)blockIdx.y * a.zlen, zend = min(a.N, z0 + a.zlen);
  rowtile_load(a.X, a.ls, r0, nr, a.R, d, ldx, xs, threadIdx.x, THREADS);
  __syncthreads();
  const int row = lane & 15, kk = lane >> 4;
  const double* xr = xs + row * ldx;

  // S[j = (l >> 4) + 4 step][i = l & 15] of the block-diagonal S = dG + dG^T
  double sreg[4];
#pragma unroll
  for (int step = 0; step < 4; ++step) {
    const int i = row, j = kk + 4 * step;
    const int64_t b = tile * a.tb + i / a.q;
    sreg[step] = 0.0;
    if (i < nr && j < nr && i / a.q == j / a.q && b < a.B) {
      const double* dg = a.dG + b * a.q * a.q;
      sreg[step] = dg[(i % a.q) * a.q + j % a.q] + dg[(j % a.q) * a.q + i % a.q];
    }
  }

  v4d accd[NDT];  // dX[row = (l >> 4) + 4 r][t = 16 tt + (l & 15)], scaled coordinates
#pragma unroll
  for (int tt = 0; tt < NDT; ++tt) accd[tt] = v4d_zero();
  double sumq = 0.0;

  for (int64_t zp = z0; zp < zend; zp += PZ) {
    const int ntw = wave_tiles(zp, zend, wave);
    const int plen = (int)min((int64_t)PZ, zend - zp);
    double d2v[NT][4];
    {
      v4d acc[NT];
      contract_v<KIND>(a, xr, ks, zp, zend, ntw, lane, wave, acc);
#pragma unroll
      for (int qq = 0; qq < NT; ++qq) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int zl = 16 * (wave + NW * qq) + mfma_row(lane, r);
          const bool ok = qq < ntw && zp + zl < zend;
          double c = 0.0;
          d2v[qq][r] = 0.0;
          if (ok) {
            d2v[qq][r] = rowtile_dist2(xr, a.Zs + (zp + zl) * d, d);
            c = a.o * (kernel_from_d2<KIND>(d2v[qq][r]) - acc[qq][r]);
          }
          gs[zl * LDG + row] = c;
        }
      }
    }
    __syncthreads();
    // dC[z][i] = sum_j C[z][j] S[j][i]: A[z = l & 15][j = (l >> 4) + 4 step] from LDS
    v4d dc[NT];
#pragma unroll
    for (int qq = 0; qq < NT; ++qq) {
      dc[qq] = v4d_zero();
      if (qq < ntw) {
#pragma unroll
        for (int step = 0; step < 4; ++step)
          dc[qq] = mfma_f64(gs[(16 * (wave + NW * qq) + row) * LDG + kk + 4 * step], sreg[step],
                            dc[qq]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int qq = 0; qq < NT; ++qq) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int zl = 16 * (wave + NW * qq) + mfma_row(lane, r);
        const bool ok = qq < ntw && zp + zl < zend;
        const double G = ok ? dc[qq][r] : 0.0;
        gs[zl * LDG + row] = G;
        if (qq < ntw) {
          // the direct term: dX[row] += dC dk(x_row, z)
          const double* zo = a.Zs + (ok ? zp + zl : 0) * d;
          const double qd = G * dkernel_factor<KIND>(d2v[qq][r], a.o);
          sumq += qd;
          rowtile_dx_acc<NDT>(qd, ok, zo, d, row, accd);
        }
      }
    }
    __syncthreads();
    // ---- the training points: coef[t][row] = -sum_z V[z][t] dC[z][row] -----------
    for (int64_t i0 = 16 * wave; i0 < a.n; i0 += 16 * NW) {
      v4d cf = v4d_zero();
      const int64_t ia = i0 + row;  // A[t = l & 15][k = l >> 4] = V[z][i0 + t]
      for (int zs = 0; zs < plen; zs += 4) {
        const int zl = zs + kk;
        const double v = zl < plen && ia < a.n ? a.V[(zp + zl) * a.n + ia] : 0.0;
        cf = mfma_f64(v, gs[zl * LDG + row], cf);
      }
      const double* xt[4];
      double d2[4];
      rowtile_dist2x4<4>(xr, a.Xts, i0 + kk, a.n, d, xt, d2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = i0 + kk + 4 * r < a.n;
        const double q = ok ? -cf[r] * dkernel_factor<KIND>(d2[r], a.o) : 0.0;
        sumq += q;
        rowtile_dx_acc<NDT>(q, ok, xt[r], d, row, accd);
      }
    }
    __syncthreads();  // gs is rewritten by the next pass
  }
  sumq = rowtile_fold4(sumq);  // the wave's sum for the row
  // the four waves' tiles in wave order (same lane layout in every wave)
  double* red = gs;             // NDT x 4 x 64
  double* rs = gs + NDT * 256;  // 16 row sums
  for (int w = 0; w < NW; ++w) {
    if (wave == w) {
#pragma unroll
      for (int tt = 0; tt < NDT; ++tt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int idx = (tt * 4 + r) * 64 + lane;
          red[idx] = w ? red[idx] + accd[tt][r] : accd[tt][r];
        }
      }
      if (kk == 0) rs[row] = w ? rs[row] + sumq : sumq;
    }
    __syncthreads();
  }
  if (wave != 0) return;
  double* dst = a.split > 1 ? a.part + (int64_t)blockIdx.y * a.R * d : a.dX;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ro = mfma_row(lane, r);
    const double sq = rs[ro];
#pragma unroll
    for (int tt = 0; tt < NDT; ++tt) {
      const int t = 16 * tt + row;
      if (t < d && ro < nr && r0 + ro < a.R)
        dst[(r0 + ro) * d + t] = (red[(tt * 4 + r) * 64 + lane] + xs[ro * ldx + t] * sq) / a.ls[t];
    }
  }
}

int fill(const BoNipvArgs* a, const char* who, Dev* v) {
  if (int st = rowtile_check_common(a->kind, a->d, a->n, a->Xt_scaled, a->V, a->outputscale, who);
      st != BO_OK)
    return st;
  BO_CHECK_ARG(a->N >= 1, "%s: N >= 1 (got %lld)", who, (long long)a->N);
  BO_CHECK_ARG(a->R >= 1 && a->n >= 0, "%s: R >= 1, n >= 0", who);
  BO_CHECK_ARG(a->q >= 1 && a->q <= 16, "%s: 1 <= q <= 16 (got %d)", who, a->q);
  BO_CHECK_ARG(a->R % a->q == 0, "%s: q must divide R (got R = %lld, q = %d)", who,
               (long long)a->R, a->q);
  BO_CHECK_ARG(a->R < (int64_t(1) << 31) && a->N < (int64_t(1) << 31) &&
                   a->n < (int64_t(1) << 31),
               "%s: R, N or n too large", who);
  BO_CHECK_ARG(a->split >= 0 && a->split <= MAX_SPLIT, "%s: 0 <= split <= %d (got %d)", who,
               MAX_SPLIT, a->split);
  BO_CHECK_ARG(a->X && a->lengthscale && a->Z_scaled, "%s: X, lengthscale and Z_scaled are "
               "required", who);
  v->kind = a->kind;
  v->d = a->d;
  v->q = a->q;
  v->tb = 16 / a->q;
  v->R = a->R;
  v->n = a->n;
  v->N = a->N;
  v->B = a->R / a->q;
  v->X = a->X;
  v->ls = a->lengthscale;
  v->Xts = a->Xt_scaled;
  v->Zs = a->Z_scaled;
  v->V = a->V;
  v->o = a->outputscale;
  v->G = a->G;
  v->dG = a->dG;
  v->dX = a->dX;
  v->part = nullptr;
  // slices of Z: by size, until tiles x slices reaches ~256 workgroups with at
  // least one 16-point tile per wave; a request is honoured down to one tile
  const int64_t tiles = ceil_div(v->B, v->tb);
  int64_t split = a->split;
  if (split == 0) split = std::min(ceil_div(256, tiles), ceil_div(v->N, 16 * NW));
  split = std::max<int64_t>(1, std::min(split, ceil_div(v->N, 16)));
  v->zlen = 16 * ceil_div(ceil_div(v->N, split), 16);
  v->split = (int)ceil_div(v->N, v->zlen);
  return BO_OK;
}

}  // namespace

// bo_nipv_gram_v / bo_nipv_gram_backward_v behind their header checks (abi_structs.cpp).
extern "C" int bo_nipv_gram_impl(const BoNipvArgs* a, void* stream) {
  Dev v;
  if (int st = fill(a, "bo_nipv_gram", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->G, "bo_nipv_gram: G is required");
  hipStream_t st = as_stream(stream);
  const int64_t total = v.B * v.q * v.q;
  if (v.split > 1) {
    keep_pool_warm();
    BO_HIP(hipMallocAsync(reinterpret_cast<void**>(&v.part),
                          sizeof(double) * (size_t)v.split * total, st));
  }
  const dim3 grid((unsigned)ceil_div(v.B, v.tb), (unsigned)v.split);
  const size_t lds = sizeof(double) * (size_t)(TR * (v.d | 1) + KS);
  if (v.kind == BO_RBF)
    nipv_gram_kernel<BO_RBF><<<grid, THREADS, lds, st>>>(v);
  else
    nipv_gram_kernel<BO_MATERN52><<<grid, THREADS, lds, st>>>(v);
  BO_LAUNCH_CHECK();
  if (v.part) {
    nipv_sum_kernel<<<(unsigned)ceil_div(total, 256), 256, 0, st>>>(v.split, total, v.part, v.G);
    BO_LAUNCH_CHECK();
    BO_HIP(hipFreeAsync(v.part, st));
  }
  return BO_OK;
}

extern "C" int bo_nipv_gram_backward_impl(const BoNipvArgs* a, void* stream) {
  Dev v;
  if (int st = fill(a, "bo_nipv_gram_backward", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->dG && a->dX, "bo_nipv_gram_backward: dG and dX are required");
  hipStream_t st = as_stream(stream);
  const int64_t total = v.R * v.d;
  if (v.split > 1) {
    keep_pool_warm();
    BO_HIP(hipMallocAsync(reinterpret_cast<void**>(&v.part),
                          sizeof(double) * (size_t)v.split * total, st));
  }
  const dim3 grid((unsigned)ceil_div(v.B, v.tb), (unsigned)v.split);
  // rows + kernel chunk + the pass's dC: at most 41.6 KiB of LDS
  const size_t lds = sizeof(double) * (size_t)(TR * (v.d | 1) + KS + PZ * LDG);
#define BO_NIPV(KIND, NDT) nipv_gram_backward_kernel<KIND, NDT><<<grid, THREADS, lds, st>>>(v)
  ROWTILE_DISPATCH(v.kind, v.d, BO_NIPV);
#undef BO_NIPV
  BO_LAUNCH_CHECK();
  if (v.part) {
    nipv_sum_kernel<<<(unsigned)ceil_div(total, 256), 256, 0, st>>>(v.split, total, v.part, v.dX);
    BO_LAUNCH_CHECK();
    BO_HIP(hipFreeAsync(v.part, st));
  }
  return BO_OK;
}
