// The Laplace approximation of the preference GP (botorch/models/pairwise_gp.py:503-620,
// 653-702, 1169-1217; likelihoods/pairwise.py:102-169): the MAP utility by Newton's
// method in whitened variables, the Laplace evidence Psi, its exact gradient in the
// kernel hyperparameters and the posterior's matrix R, for a batch of hyperparameter
// rows over shared data, one workgroup per row.  The formulas stand in
// include/botorch_amd.h (BoPairwiseLaplaceArgs) and DESIGN.md section 27.
//
// Layout.  A row's slice of the caller's workspace holds six NP x NP matrices (NP = n
// rounded up to 16; the padding of K is an identity block), the transposed inputs,
// eight vectors and four per-comparison arrays.  A workgroup of 512 threads walks
//   1  scalars, finiteness, lengthscales into LDS, X transposed into the slice
//   2  K's lower triangle (B0)
//   3  blocked right-looking Cholesky K = L L^T in place: 16 x 16 diagonal blocks in
//      one wave's registers, the panel in LDS, the trailing update on
//      v_mfma_f64_16x16x4
//   4  a = L^{-1} f_init by a blocked substitution (the vector in LDS)
//   5  Newton: f = L a, the probit terms per comparison, b and C by one thread per
//      datapoint over its incidence list (list order, no atomics), T = C L and
//      M = I + L^T T as block products that skip L's zero blocks, M's Cholesky as
//      in 3, two substitutions, step halving on ||a + L^T b||_2
//   6  M at the root, Psi, alpha = L^{-T} a, L^{-1} and L_m^{-1} as in
//      saas_nuts.hip, R = L^{-T} L_m^{-T} L_m^{-1} L^T C as three block products;
//      for the gradient s_k from Q^T = L L_m^{-T}, u, v (M over C_iota when a
//      comparison is clamped), W, the outputscale sum and V = W dKbar/dr^2, then the
//      lengthscale sums with one accumulator per (dimension, row slice)
// Only workgroup barriers, every sum in a fixed order, nothing shared between
// workgroups: a row does not depend on its neighbours and a second call is
// bit-identical.
#include "normal.h"

namespace {

constexpr int PW_T = 512, PW_NW = PW_T / 64, PW_NMAX = 1024, PW_DMAX = 256;
constexpr int PW_RB = 4;   // rows a pair loop takes at a time
constexpr int PW_PS = 17;  // row stride of the LDS blocks (doubles)
constexpr int PW_HALVINGS = 8;
constexpr double PW_SQRT5 = 2.23606797749978969641, PW_LOG_SQRT_2PI = 0.91893853320467274178;
constexpr double PW_ZLIM = 3.0;

// which blocks of a product's operands are zero: a(i, p) = 0 for p > i (A_LO) or
// p < i (A_UP); b(p, j) = 0 for p < j (B_LO) or p > j (B_UP); OUT_LO: only j <= i
enum : int { PW_A_LO = 1, PW_A_UP = 2, PW_B_LO = 4, PW_B_UP = 8, PW_OUT_LO = 16 };

struct PwDev {
  int n, d, NP, kind, maxfev, want_grad;
  int m;
  int64_t ldr, stride;
  const double* X;
  const int32_t *comp, *inc_ptr, *inc;
  const double *hyper, *f_init;
  double jitter, tol;
  double *f, *alpha, *psi, *grad, *R;
  int32_t *iters, *status;
  double* work;
};

__host__ __device__ inline int64_t pw_slice(int64_t NP, int64_t d, int64_t m) {
  return 6 * NP * NP + d * NP + 8 * NP + 4 * m;
}

__host__ inline size_t pw_lds_bytes(int NP) {
  return sizeof(double) * ((size_t)NP * PW_PS + 2 * 16 * PW_PS + 16 + PW_T + PW_DMAX + NP);
}

struct PwLds {
  double *P, *Db, *Di, *rd, *red, *w, *xs;
  int* flag;
};

template <bool NEG>
__device__ __forceinline__ v4d blk_mma(v4d acc, const double* A, int64_t sai, int64_t sak,
                                       const double* B, int64_t sbk, int64_t sbj) {
  const int lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = 4 * s + kq;
    const double a = A[m * sai + k * sak], b = B[k * sbk + m * sbj];
    acc = mfma_f64(NEG ? -a : a, b, acc);
  }
  return acc;
}

__device__ __forceinline__ v4d blk_load(const double* Cp, int64_t ld) {
  const int lane = threadIdx.x & 63;
  v4d c;
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] = Cp[(int64_t)mfma_row(lane, r) * ld + mfma_col(lane)];
  return c;
}

__device__ __forceinline__ void blk_store(double* Cp, int64_t ld, v4d c) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < 4; ++r) Cp[(int64_t)mfma_row(lane, r) * ld + mfma_col(lane)] = c[r];
}

__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = PW_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double block_max(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = PW_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ bool pw_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// r2[q] = sum_j w_j (x_{i0+q,j} - x_kj)^2 for PW_RB rows against a lane's column k
__device__ __forceinline__ void pair_r2(const double* X, const double* XT, const double* w, int n,
                                        int d, int NP, int i0, int k, double (&r2)[PW_RB]) {
  const double* xr[PW_RB];
#pragma unroll
  for (int q = 0; q < PW_RB; ++q) {
    r2[q] = 0.0;
    xr[q] = X + (int64_t)(i0 + q < n ? i0 + q : n - 1) * d;
  }
  if (k >= n) return;
#pragma unroll 8
  for (int j = 0; j < d; ++j) {
    const double xk = XT[(int64_t)j * NP + k], wj = w[j];
#pragma unroll
    for (int q = 0; q < PW_RB; ++q) {
      const double dl = xk - xr[q][j];
      r2[q] += wj * dl * dl;
    }
  }
}

__device__ __forceinline__ double pw_kernel(int kind, double r2) {
  return kind == BO_RBF ? kernel_from_d2<BO_RBF>(r2) : kernel_from_d2<BO_MATERN52>(r2);
}

// dKbar / dr^2
__device__ __forceinline__ double pw_dkernel(int kind, double r2) {
  if (kind == BO_RBF) return -0.5 * exp(-0.5 * r2);
  const double s5r = PW_SQRT5 * sqrt(fmax(r2, 1e-30));
  return -(5.0 / 6.0) * (1.0 + s5r) * exp(-s5r);
}

// Blocked right-looking Cholesky of the lower triangle of A (NP x NP) in place; the
// strict upper triangle of the diagonal blocks is left zero.  A non-positive or
// non-finite pivot sets *flag = 2.  Ends on a barrier.
__device__ void pw_chol(double* A, int NP, const PwLds& s) {
  const int tid = threadIdx.x, lane = tid & 63, nb = NP / 16;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int kb = 0; kb < nb; ++kb) {
    const int k0 = kb * 16;
    if (wv == 0) {
      const int r = lane & 15;
      double row[16];
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) row[cc] = cc <= r ? A[(int64_t)(k0 + r) * NP + k0 + cc] : 0.0;
      bool badp = false;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        double piv = __shfl(row[j], j);
        if (!(piv > 0.0) || !pw_finite(piv)) {
          badp = true;
          piv = 1.0;
        }
        const double sq = sqrt(piv), rp = 1.0 / sq;
        const double lj = (r == j) ? sq : row[j] * rp;
        row[j] = lj;
        if (lane == j) s.rd[j] = rp;
#pragma unroll
        for (int cc = j + 1; cc < 16; ++cc) row[cc] -= lj * __shfl(lj, cc);
      }
      if (lane < 16) {
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) {
          const double v = cc <= r ? row[cc] : 0.0;
          s.Db[r * PW_PS + cc] = v;
          A[(int64_t)(k0 + r) * NP + k0 + cc] = v;
        }
      }
      if (badp) *s.flag = 2;
    }
    __syncthreads();
    if (*s.flag) return;
    for (int i = k0 + 16 + tid; i < NP; i += PW_T) {
      double x[16];
      double* row = A + (int64_t)i * NP + k0;
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) x[cc] = row[cc];
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) {
        double t = x[cc];
#pragma unroll
        for (int p = 0; p < cc; ++p) t -= x[p] * s.Db[cc * PW_PS + p];
        x[cc] = t * s.rd[cc];
      }
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) {
        row[cc] = x[cc];
        s.P[(size_t)i * PW_PS + cc] = x[cc];
      }
    }
    __syncthreads();
    int cnt = 0;
    for (int bi = kb + 1; bi < nb; ++bi) {
      for (int bj = kb + 1; bj <= bi; ++bj, ++cnt) {
        if (cnt % PW_NW != wv) continue;
        double* Cp = A + (int64_t)bi * 16 * NP + bj * 16;
        v4d acc = blk_load(Cp, NP);
        acc = blk_mma<true>(acc, s.P + (size_t)bi * 16 * PW_PS, PW_PS, 1,
                            s.P + (size_t)bj * 16 * PW_PS, 1, PW_PS);
        blk_store(Cp, NP, acc);
      }
    }
    __syncthreads();
  }
}

// Z = L^{-1} (lower blocks; the diagonal blocks whole), block row by block row
__device__ void pw_trinv(const double* L, double* Z, int NP, const PwLds& s) {
  const int tid = threadIdx.x, nb = NP / 16;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int ib = 0; ib < nb; ++ib) {
    const int i0 = ib * 16;
    if (tid < 256) {
      const int r = tid >> 4, cc = tid & 15;
      s.Db[r * PW_PS + cc] = cc <= r ? L[(int64_t)(i0 + r) * NP + i0 + cc] : 0.0;
    }
    __syncthreads();
    if (tid < 16) {
      double x[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        double t = (r == tid) ? 1.0 : 0.0;
#pragma unroll
        for (int p = 0; p < r; ++p) t -= s.Db[r * PW_PS + p] * x[p];
        x[r] = (r < tid) ? 0.0 : t / s.Db[r * PW_PS + r];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) s.Di[r * PW_PS + tid] = x[r];
    }
    for (int j = wv; j < ib; j += PW_NW) {
      v4d acc = v4d_zero();
      for (int p = j; p < ib; ++p)
        acc = blk_mma<false>(acc, L + (int64_t)i0 * NP + p * 16, NP, 1,
                             Z + (int64_t)p * 16 * NP + j * 16, NP, 1);
      blk_store(s.P + (size_t)j * 16 * PW_PS, PW_PS, acc);
    }
    __syncthreads();
    for (int j = wv; j <= ib; j += PW_NW) {
      double* Zp = Z + (int64_t)i0 * NP + j * 16;
      if (j == ib) {
        blk_store(Zp, NP, blk_load(s.Di, PW_PS));
      } else {
        const v4d acc =
            blk_mma<true>(v4d_zero(), s.Di, PW_PS, 1, s.P + (size_t)j * 16 * PW_PS, PW_PS, 1);
        blk_store(Zp, NP, acc);
      }
    }
    __syncthreads();
  }
}

// D (NP x NP, row-major) = A B by 16 x 16 blocks dealt to the waves in turn; a(i, k) at
// A[i sai + k sak], b(k, j) at B[k sbk + j sbj]; flags name the operands' zero blocks,
// which are neither read nor multiplied.  Ends on a barrier.
__device__ void pw_gemm(double* D, const double* A, int64_t sai, int64_t sak, const double* B,
                        int64_t sbk, int64_t sbj, int NP, int flags) {
  const int nb = NP / 16;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  int cnt = 0;
  for (int bi = 0; bi < nb; ++bi) {
    const int jend = (flags & PW_OUT_LO) ? bi + 1 : nb;
    for (int bj = 0; bj < jend; ++bj, ++cnt) {
      if (cnt % PW_NW != wv) continue;
      int plo = 0, phi = nb - 1;
      if (flags & PW_A_UP) plo = bi;
      if ((flags & PW_B_LO) && bj > plo) plo = bj;
      if (flags & PW_A_LO) phi = bi;
      if ((flags & PW_B_UP) && bj < phi) phi = bj;
      v4d acc = v4d_zero();
      for (int p = plo; p <= phi; ++p)
        acc = blk_mma<false>(acc, A + (int64_t)bi * 16 * sai + (int64_t)p * 16 * sak, sai, sak,
                             B + (int64_t)p * 16 * sbk + (int64_t)bj * 16 * sbj, sbk, sbj);
      blk_store(D + (int64_t)bi * 16 * NP + bj * 16, NP, acc);
    }
  }
  __syncthreads();
}

// xs <- L^{-1} xs: the diagonal block in wave 0 (a row per lane, shuffles), then one
// row per thread takes the block's 16 columns.  Ends on a barrier.
__device__ void pw_fwd(const double* L, int NP, double* xs) {
  const int tid = threadIdx.x, lane = tid & 63, nb = NP / 16;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int kb = 0; kb < nb; ++kb) {
    const int k0 = kb * 16;
    if (wv == 0) {
      const int r = lane & 15;
      double row[16];
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) row[cc] = L[(int64_t)(k0 + r) * NP + k0 + cc];
      double x = xs[k0 + r];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double xj = __shfl(x, j) / __shfl(row[j], j);
        if (r == j) x = xj;
        if (r > j) x -= row[j] * xj;
      }
      if (lane < 16) xs[k0 + r] = x;
    }
    __syncthreads();
    for (int i = k0 + 16 + tid; i < NP; i += PW_T) {
      const double* row = L + (int64_t)i * NP + k0;
      double t = xs[i];
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) t -= row[cc] * xs[k0 + cc];
      xs[i] = t;
    }
    __syncthreads();
  }
}

// xs <- L^{-T} xs
__device__ void pw_bwd(const double* L, int NP, double* xs) {
  const int tid = threadIdx.x, lane = tid & 63, nb = NP / 16;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int kb = nb - 1; kb >= 0; --kb) {
    const int k0 = kb * 16;
    if (wv == 0) {
      const int r = lane & 15;
      double col[16];  // column r of the block: (L^T)[r][j] = L[j][r]
#pragma unroll
      for (int j = 0; j < 16; ++j) col[j] = L[(int64_t)(k0 + j) * NP + k0 + r];
      double x = xs[k0 + r];
#pragma unroll
      for (int j = 15; j >= 0; --j) {
        const double xj = __shfl(x, j) / __shfl(col[j], j);
        if (r == j) x = xj;
        if (r < j) x -= col[j] * xj;
      }
      if (lane < 16) xs[k0 + r] = x;
    }
    __syncthreads();
    for (int i = tid; i < k0; i += PW_T) {
      double t = xs[i];
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) t -= L[(int64_t)(k0 + cc) * NP + i] * xs[k0 + cc];
      xs[i] = t;
    }
    __syncthreads();
  }
}

// a row's vectors and per-comparison arrays
struct PwVec {
  double *av, *at, *dl, *gv, *fv, *bv, *uv, *vv;  // NP each
  double *zr, *hh, *cc, *ss;                      // m each
};

// f = L avec, the probit terms, b and g_a = avec + L^T b; returns ||g_a||^2 and the sum
// of log Phi(z) in sumlog
__device__ double pw_eval(const PwDev& a, const double* L, const PwVec& v, const double* avec,
                          double* red, double& sumlog) {
  const int n = a.n, NP = a.NP, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  __syncthreads();
  for (int i = wv; i < n; i += PW_NW) {
    double t = 0.0;
    for (int k = lane; k <= i; k += 64) t += L[(int64_t)i * NP + k] * avec[k];
    t = wave_sum(t);
    if (lane == 0) v.fv[i] = t;
  }
  __syncthreads();
  double sl = 0.0;
  for (int k = tid; k < a.m; k += PW_T) {
    const double zr = (v.fv[a.comp[2 * k]] - v.fv[a.comp[2 * k + 1]]) * INV_SQRT2;
    const double z = fmin(fmax(zr, -PW_ZLIM), PW_ZLIM);
    const double lp = log(0.5 * erfc(-z * INV_SQRT2));
    const double h = exp(-0.5 * z * z - PW_LOG_SQRT_2PI - lp);  // phi / Phi in log space
    v.zr[k] = zr;
    v.hh[k] = h;
    v.cc[k] = 0.5 * h * (h + z);
    sl += lp;
  }
  __syncthreads();
  for (int i = tid; i < n; i += PW_T) {
    double b = 0.0;
    for (int e = a.inc_ptr[i]; e < a.inc_ptr[i + 1]; ++e) {
      const int code = a.inc[e];
      const double t = v.hh[code >> 1] * INV_SQRT2;
      b += (code & 1) ? t : -t;
    }
    v.bv[i] = b;
  }
  __syncthreads();
  double g2 = 0.0;
  for (int k = tid; k < n; k += PW_T) {
    double t = 0.0;
    for (int i = k; i < n; ++i) t += L[(int64_t)i * NP + k] * v.bv[i];
    const double g = avec[k] + t;
    v.gv[k] = g;
    g2 += g * g;
  }
  g2 = block_sum(g2, red);
  sumlog = block_sum(sl, red);
  return g2;
}

// C = sum_k w_k d_k d_k^T into Cm (NP x NP, whole), w_k = c_k, or iota_k c_k when
// unclamped_only; T = C L; Cm <- M = I + L^T T (lower blocks); its Cholesky in place
__device__ void pw_newton_matrix(const PwDev& a, const double* L, double* Cm, double* T,
                                 const PwVec& v, const PwLds& s, bool unclamped_only) {
  const int n = a.n, NP = a.NP, tid = threadIdx.x;
  __syncthreads();
  for (int64_t e = tid; e < (int64_t)NP * NP; e += PW_T) Cm[e] = 0.0;
  __syncthreads();
  for (int i = tid; i < n; i += PW_T) {
    double* row = Cm + (int64_t)i * NP;
    for (int e = a.inc_ptr[i]; e < a.inc_ptr[i + 1]; ++e) {
      const int code = a.inc[e], k = code >> 1;
      const int other = a.comp[2 * k + ((code & 1) ^ 1)];
      const double wk = (unclamped_only && fabs(v.zr[k]) > PW_ZLIM) ? 0.0 : v.cc[k];
      row[i] += wk;
      row[other] -= wk;
    }
  }
  __syncthreads();
  pw_gemm(T, Cm, NP, 1, L, NP, 1, NP, PW_B_LO);
  pw_gemm(Cm, L, 1, NP, T, NP, 1, NP, PW_A_UP | PW_OUT_LO);
  for (int i = tid; i < NP; i += PW_T) Cm[(int64_t)i * NP + i] += 1.0;
  __syncthreads();
  pw_chol(Cm, NP, s);
}

// status != 0 without values: Psi = -inf, zeros elsewhere
__device__ void pw_fail(const PwDev& a, int c, int code, int iters) {
  const int D = a.d + 1;
  if (a.grad)
    for (int e = threadIdx.x; e < D; e += PW_T) a.grad[(int64_t)c * D + e] = 0.0;
  for (int i = threadIdx.x; i < a.n; i += PW_T) {
    a.f[(int64_t)c * a.n + i] = 0.0;
    a.alpha[(int64_t)c * a.n + i] = 0.0;
  }
  if (threadIdx.x == 0) {
    a.psi[c] = -INFINITY;
    a.status[c] = code;
    a.iters[c] = iters;
  }
}

__global__ __launch_bounds__(PW_T) void pairwise_laplace_kernel(const PwDev a) {
  extern __shared__ double pw_smem[];
  __shared__ int flag;
  const int n = a.n, d = a.d, NP = a.NP, D = d + 1, m = a.m;
  PwLds s;
  s.P = pw_smem;
  s.Db = s.P + (size_t)NP * PW_PS;
  s.Di = s.Db + 16 * PW_PS;
  s.rd = s.Di + 16 * PW_PS;
  s.red = s.rd + 16;
  s.w = s.red + PW_T;
  s.xs = s.w + PW_DMAX;
  s.flag = &flag;
  double* red = s.red;
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const double* hy = a.hyper + (int64_t)c * D;
  const int64_t N2 = (int64_t)NP * NP;
  double* B0 = a.work + (int64_t)c * a.stride;  // K, then L
  double* B1 = B0 + N2;                         // C, M, then L_m
  double* B2 = B1 + N2;                         // T; L_m^{-T} (..); C_iota's T; V
  double* B3 = B2 + N2;                         // L^{-1}
  double* B4 = B3 + N2;                         // L_m^{-1}
  double* B5 = B4 + N2;                         // L_m^{-1} T^T; R; Q^T
  double* XT = B5 + N2;                         // d x NP
  PwVec v;
  v.av = XT + (int64_t)d * NP;
  v.at = v.av + NP;
  v.dl = v.at + NP;
  v.gv = v.dl + NP;
  v.fv = v.gv + NP;
  v.bv = v.fv + NP;
  v.uv = v.bv + NP;
  v.vv = v.uv + NP;
  v.zr = v.vv + NP;
  v.hh = v.zr + m;
  v.cc = v.hh + m;
  v.ss = v.cc + m;

  // ---- 1: scalars, lengthscales, finiteness, X^T --------------------------------------------
  if (tid == 0) flag = 0;
  __syncthreads();
  const double os = hy[0];
  bool bad = !(pw_finite(os) && os > 0.0 && pw_finite(a.jitter));
  for (int j = tid; j < d; j += PW_T) {
    const double l = hy[1 + j], wj = 1.0 / (l * l);
    s.w[j] = wj;
    bad = bad || !pw_finite(l) || !(l > 0.0) || !pw_finite(wj);
  }
  for (int64_t e = tid; e < (int64_t)n * d; e += PW_T) {
    const double x = a.X[e];
    bad = bad || !pw_finite(x);
    XT[(e % d) * NP + e / d] = x;
  }
  if (a.f_init)
    for (int i = tid; i < n; i += PW_T) bad = bad || !pw_finite(a.f_init[(int64_t)c * n + i]);
  if (bad) flag = 1;
  __syncthreads();
  if (flag) {
    pw_fail(a, c, 1, 0);
    return;
  }

  // ---- 2: K's lower triangle, identity on the padding, zeros above the diagonal of the
  // diagonal blocks ----------------------------------------------------------------------------
  for (int i0 = PW_RB * wv; i0 < NP; i0 += PW_RB * PW_NW) {
    for (int k = lane; k < i0 + PW_RB; k += 64) {
      double r2[PW_RB];
      pair_r2(a.X, XT, s.w, n, d, NP, i0, k, r2);
#pragma unroll
      for (int q = 0; q < PW_RB; ++q) {
        const int i = i0 + q;
        if (k > i) continue;
        double val;
        if (i >= n)
          val = (i == k) ? 1.0 : 0.0;
        else if (i == k)
          val = os * (1.0 + a.jitter);
        else
          val = os * pw_kernel(a.kind, r2[q]);
        B0[(int64_t)i * NP + k] = val;
      }
    }
  }
  for (int e = tid; e < NP * 16; e += PW_T) {
    const int i = e >> 4, k = (i & ~15) + (e & 15);
    if (k > i) B0[(int64_t)i * NP + k] = 0.0;
  }
  __syncthreads();

  // ---- 3: K = L L^T ----------------------------------------------------------------------------
  pw_chol(B0, NP, s);
  if (flag) {
    pw_fail(a, c, 2, 0);
    return;
  }

  // ---- 4: a = L^{-1} f_init --------------------------------------------------------------------
  if (a.f_init) {
    for (int i = tid; i < NP; i += PW_T) s.xs[i] = i < n ? a.f_init[(int64_t)c * n + i] : 0.0;
  } else {
    // (wins - mean) / std sqrt(os) over the datapoints, wins_i = #won - #lost
    double sw = 0.0;
    for (int i = tid; i < n; i += PW_T) {
      double wc = 0.0;
      for (int e = a.inc_ptr[i]; e < a.inc_ptr[i + 1]; ++e) wc += (a.inc[e] & 1) ? -1.0 : 1.0;
      v.bv[i] = wc;
      sw += wc;
    }
    const double mean = block_sum(sw, red) / n;
    double sq = 0.0;
    for (int i = tid; i < n; i += PW_T) sq += (v.bv[i] - mean) * (v.bv[i] - mean);
    const double sd = fmax(sqrt(block_sum(sq, red) / n), 1e-6);
    const double sc = sqrt(os) / sd;
    for (int i = tid; i < NP; i += PW_T) s.xs[i] = i < n ? (v.bv[i] - mean) * sc : 0.0;
  }
  __syncthreads();
  pw_fwd(B0, NP, s.xs);
  for (int i = tid; i < NP; i += PW_T) v.av[i] = s.xs[i];

  // ---- 5: Newton --------------------------------------------------------------------------------
  double sumlog = 0.0;
  double g2 = pw_eval(a, B0, v, v.av, red, sumlog);
  int it = 0, status = 3;
  while (it < a.maxfev) {
    ++it;
    pw_newton_matrix(a, B0, B1, B2, v, s, false);
    if (flag) break;
    for (int i = tid; i < NP; i += PW_T) s.xs[i] = i < n ? v.gv[i] : 0.0;
    __syncthreads();
    pw_fwd(B1, NP, s.xs);
    pw_bwd(B1, NP, s.xs);
    double dmax = 0.0, amax = 0.0;
    for (int i = tid; i < n; i += PW_T) {
      v.dl[i] = s.xs[i];
      dmax = fmax(dmax, fabs(s.xs[i]));
      amax = fmax(amax, fabs(v.av[i]));
    }
    dmax = block_max(dmax, red);
    amax = block_max(amax, red);
    if (!pw_finite(dmax)) {
      if (tid == 0) flag = 1;
      __syncthreads();
      break;
    }
    const bool small = dmax <= a.tol * fmax(1.0, amax);
    double t = 1.0, gn = 0.0;
    bool stalled = false;
    for (int hv = 0;; ++hv) {
      for (int i = tid; i < NP; i += PW_T) v.at[i] = i < n ? v.av[i] - t * v.dl[i] : 0.0;
      gn = pw_eval(a, B0, v, v.at, red, sumlog);
      if (small || gn < g2) break;
      if (hv == PW_HALVINGS) {
        stalled = true;
        break;
      }
      t *= 0.5;
    }
    for (int i = tid; i < NP; i += PW_T) v.av[i] = v.at[i];
    g2 = gn;
    if (!pw_finite(gn)) {
      if (tid == 0) flag = 1;
      __syncthreads();
      break;
    }
    // (a step that no halving improves is rounding noise once it is this short)
    if (small || (stalled && dmax <= 1e-9 * fmax(1.0, amax))) {
      status = 0;
      break;
    }
  }
  if (flag) {
    pw_fail(a, c, 1, it);
    return;
  }

  // ---- 6: outputs -------------------------------------------------------------------------------
  pw_newton_matrix(a, B0, B1, B2, v, s, false);  // M at the root; T = C L stays in B2
  if (flag) {
    pw_fail(a, c, 1, it);
    return;
  }
  double logdet = 0.0, quad = 0.0, nclamp = 0.0;
  for (int i = tid; i < n; i += PW_T) {
    logdet += log(B1[(int64_t)i * NP + i]);
    quad += v.av[i] * v.av[i];
  }
  for (int k = tid; k < m; k += PW_T) nclamp += fabs(v.zr[k]) > PW_ZLIM ? 1.0 : 0.0;
  logdet = block_sum(logdet, red);
  quad = block_sum(quad, red);
  nclamp = block_sum(nclamp, red);
  const double psi = sumlog - 0.5 * quad - logdet;

  for (int i = tid; i < NP; i += PW_T) s.xs[i] = v.av[i];
  __syncthreads();
  pw_bwd(B0, NP, s.xs);
  for (int i = tid; i < NP; i += PW_T) v.bv[i] = s.xs[i];  // alpha (b is dead)
  double* alpha = v.bv;

  pw_trinv(B0, B3, NP, s);
  pw_trinv(B1, B4, NP, s);
  pw_gemm(B5, B4, NP, 1, B2, 1, NP, NP, PW_A_LO);  // L_m^{-1} T^T
  pw_gemm(B2, B4, 1, NP, B5, NP, 1, NP, PW_A_UP);  // L_m^{-T} ..
  pw_gemm(B5, B3, 1, NP, B2, NP, 1, NP, PW_A_UP);  // R = L^{-T} ..
  double* Rc = a.R + (int64_t)c * n * a.ldr;
  bool nonfinite = false;
  for (int64_t e = tid; e < (int64_t)n * n; e += PW_T) {
    const int i = (int)(e / n), k = (int)(e % n);
    const double r = 0.5 * (B5[(int64_t)i * NP + k] + B5[(int64_t)k * NP + i]);
    nonfinite = nonfinite || !pw_finite(r);
    Rc[(int64_t)i * a.ldr + k] = r;
  }
  __syncthreads();

  double g_os = 0.0, gj = 0.0;
  if (a.want_grad) {
    // s_k = || L_m^{-1} L^T d_k ||^2 from the rows of Q^T = L L_m^{-T} (over B2)
    pw_gemm(B2, B0, NP, 1, B4, 1, NP, NP, PW_A_LO | PW_B_UP);
    for (int k = wv; k < m; k += PW_NW) {
      const double *qi = B2 + (int64_t)a.comp[2 * k] * NP, *qj = B2 + (int64_t)a.comp[2 * k + 1] * NP;
      double t = 0.0;
      for (int r = lane; r < n; r += 64) t += (qi[r] - qj[r]) * (qi[r] - qj[r]);
      t = wave_sum(t);
      if (lane == 0) v.ss[k] = t;
    }
    __syncthreads();
    for (int i = tid; i < NP; i += PW_T) {
      double u = 0.0;
      if (i < n)
        for (int e = a.inc_ptr[i]; e < a.inc_ptr[i + 1]; ++e) {
          const int code = a.inc[e], k = code >> 1;
          const double h = v.hh[k];
          double t;
          if (fabs(v.zr[k]) > PW_ZLIM) {
            t = -h * INV_SQRT2;
          } else {
            const double z = v.zr[k], hp = -h * (h + z);
            t = -0.5 * (0.5 * (hp * (2.0 * h + z) + h)) * v.ss[k] * INV_SQRT2;
          }
          u += (code & 1) ? -t : t;
        }
      v.uv[i] = u;
    }
    if (nclamp > 0.0) {
      pw_newton_matrix(a, B0, B1, B2, v, s, true);  // (B4, B2's Q^T and L_m are dead)
      if (flag) {
        pw_fail(a, c, 1, it);
        return;
      }
    }
    __syncthreads();
    // v = L^{-T} M_iota^{-1} L^T u
    for (int k = tid; k < NP; k += PW_T) {
      double t = 0.0;
      for (int i = k; i < n; ++i) t += B0[(int64_t)i * NP + k] * v.uv[i];
      s.xs[k] = k < n ? t : 0.0;
    }
    __syncthreads();
    pw_fwd(B1, NP, s.xs);
    pw_bwd(B1, NP, s.xs);
    pw_bwd(B0, NP, s.xs);
    for (int i = tid; i < NP; i += PW_T) v.vv[i] = s.xs[i];
    __syncthreads();

    // W against the kernel; V = W dKbar/dr^2 over B2's lower triangle
    double sK = 0.0;
    for (int i0 = PW_RB * wv; i0 < n; i0 += PW_RB * PW_NW) {
      for (int k = lane; k < i0 + PW_RB && k < n; k += 64) {
        double r2[PW_RB];
        pair_r2(a.X, XT, s.w, n, d, NP, i0, k, r2);
        const double ak = alpha[k], vk = v.vv[k];
#pragma unroll
        for (int q = 0; q < PW_RB; ++q) {
          const int i = i0 + q;
          if (i >= n || k > i) continue;
          const double W = 0.5 * (alpha[i] * ak - Rc[(int64_t)i * a.ldr + k] + alpha[i] * vk +
                                  v.vv[i] * ak);
          if (k == i) {
            sK += W * (1.0 + a.jitter);
          } else {
            sK += 2.0 * W * pw_kernel(a.kind, r2[q]);
            B2[(int64_t)i * NP + k] = W * pw_dkernel(a.kind, r2[q]);
          }
        }
      }
    }
    g_os = block_sum(sK, red);  // (its barriers also publish V)

    // the lengthscale sums sum_{i>k} V_ik (x_ij - x_kj)^2, one accumulator per thread
    {
      const int S = PW_T / d, j = tid % d, sl = tid / d;
      double acc = 0.0;
      if (sl < S) {
        for (int ib = sl; ib < n; ib += PW_RB * S) {
          double xi[PW_RB], part[PW_RB];
          const double* Vr[PW_RB];
          int iq[PW_RB];
#pragma unroll
          for (int q = 0; q < PW_RB; ++q) {
            const int i = ib + q * S;
            iq[q] = i < n ? i : 0;
            xi[q] = a.X[(int64_t)iq[q] * d + j];
            Vr[q] = B2 + (int64_t)iq[q] * NP;
            part[q] = 0.0;
          }
          int kend = 0;
#pragma unroll
          for (int q = 0; q < PW_RB; ++q) kend = iq[q] > kend ? iq[q] : kend;
#pragma unroll 4
          for (int k = 0; k < kend; ++k) {
            const double xk = a.X[(int64_t)k * d + j];
#pragma unroll
            for (int q = 0; q < PW_RB; ++q) {
              const double val = Vr[q][k], dl = xi[q] - xk;
              part[q] += k < iq[q] ? val * dl * dl : 0.0;
            }
          }
#pragma unroll
          for (int q = 0; q < PW_RB; ++q) acc += part[q];
        }
      }
      __syncthreads();
      red[tid] = acc;
      __syncthreads();
      if (tid < d) {
        for (int q = 0; q < S; ++q) gj += red[q * d + tid];
        const double l = hy[1 + tid];
        gj *= -4.0 * os / (l * l * l);
        nonfinite = nonfinite || !pw_finite(gj);
      }
    }
    nonfinite = nonfinite || !pw_finite(g_os);
  }

  for (int i = tid; i < n; i += PW_T) nonfinite = nonfinite || !pw_finite(v.fv[i]) || !pw_finite(alpha[i]);
  nonfinite = nonfinite || !pw_finite(psi);
  __syncthreads();
  if (nonfinite) flag = 1;
  __syncthreads();
  if (flag) {
    pw_fail(a, c, 1, it);
    return;
  }
  for (int i = tid; i < n; i += PW_T) {
    a.f[(int64_t)c * n + i] = v.fv[i];
    a.alpha[(int64_t)c * n + i] = alpha[i];
  }
  if (a.want_grad && tid < d) a.grad[(int64_t)c * D + 1 + tid] = gj;
  if (tid == 0) {
    if (a.want_grad) a.grad[(int64_t)c * D] = g_os;
    a.psi[c] = psi;
    a.status[c] = status;
    a.iters[c] = it;
  }
}

int pw_limits(const char* who, int64_t n, int64_t m, int64_t d, int64_t C) {
  BO_CHECK_ARG(n >= 2 && n <= PW_NMAX, "%s: 2 <= n <= %d (got %lld)", who, PW_NMAX, (long long)n);
  BO_CHECK_ARG(m >= 1 && 2 * m < ((int64_t)1 << 31), "%s: 1 <= m with 2 m < 2^31 (got %lld)", who,
               (long long)m);
  BO_CHECK_ARG(d >= 1 && d <= PW_DMAX, "%s: 1 <= d <= %d (got %lld)", who, PW_DMAX, (long long)d);
  BO_CHECK_ARG(C >= 1 && C * n * n < ((int64_t)1 << 31), "%s: C >= 1 and C n^2 < 2^31 (got C = %lld)",
               who, (long long)C);
  return BO_OK;
}

}  // namespace

extern "C" int bo_pairwise_laplace_work(int64_t n, int64_t m, int d, int64_t C, int64_t* elems) {
  if (int st = pw_limits("bo_pairwise_laplace_work", n, m, d, C); st != BO_OK) return st;
  BO_CHECK_ARG(elems, "bo_pairwise_laplace_work: elems is required");
  *elems = C * pw_slice(ceil_div(n, 16) * 16, d, m);
  return BO_OK;
}

extern "C" int bo_pairwise_laplace_impl(const BoPairwiseLaplaceArgs* a, void* stream) {
  const char* who = "bo_pairwise_laplace";
  if (int st = pw_limits(who, a->n, a->m, a->d, a->C); st != BO_OK) return st;
  BO_CHECK_ARG(a->kind == BO_RBF || a->kind == BO_MATERN52, "%s: kind must be RBF or Matern-5/2", who);
  BO_CHECK_ARG(a->X && a->comp && a->inc_ptr && a->inc && a->hyper,
               "%s: X, comp, inc_ptr, inc and hyper are required", who);
  BO_CHECK_ARG(a->f && a->alpha && a->psi && a->R && a->iters && a->status,
               "%s: f, alpha, psi, R, iters and status are required", who);
  BO_CHECK_ARG(!a->want_grad || a->grad, "%s: grad is required when want_grad is set", who);
  BO_CHECK_ARG(a->ldr >= a->n, "%s: ldr >= n (got %lld)", who, (long long)a->ldr);
  BO_CHECK_ARG(a->maxfev >= 1, "%s: maxfev >= 1 (got %d)", who, a->maxfev);
  BO_CHECK_ARG(a->tol >= 0.0 && a->jitter >= 0.0, "%s: tol and jitter must be >= 0", who);
  PwDev v;
  v.n = (int)a->n;
  v.m = (int)a->m;
  v.d = a->d;
  v.NP = (int)(ceil_div(a->n, 16) * 16);
  v.kind = a->kind;
  v.maxfev = a->maxfev;
  v.want_grad = a->want_grad;
  v.ldr = a->ldr;
  v.stride = pw_slice(v.NP, v.d, v.m);
  const int64_t need = a->C * v.stride;
  BO_CHECK_ARG(a->work && a->work_size >= need,
               "%s: work of at least %lld doubles is required (work_size %lld)", who,
               (long long)need, (long long)a->work_size);
  v.X = a->X;
  v.comp = a->comp;
  v.inc_ptr = a->inc_ptr;
  v.inc = a->inc;
  v.hyper = a->hyper;
  v.f_init = a->f_init;
  v.jitter = a->jitter;
  v.tol = a->tol;
  v.f = a->f;
  v.alpha = a->alpha;
  v.psi = a->psi;
  v.grad = a->grad;
  v.R = a->R;
  v.iters = a->iters;
  v.status = a->status;
  v.work = a->work;
  const size_t lds = pw_lds_bytes(v.NP);
  if (lds > 48 * 1024)
    BO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pairwise_laplace_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  pairwise_laplace_kernel<<<(unsigned)a->C, PW_T, lds, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}
