// The potential of the SAAS GP for NUTS (botorch/models/fully_bayesian.py:168-247,
// SaasPyroModel.sample): U(z) = -log p(z, Y) and its closed-form gradient for a
// batch of unconstrained vectors z, one workgroup per row of z.  The density and
// the gradient formulas stand in include/botorch_amd.h (BoSaasPotentialArgs) and
// DESIGN.md section 22.
//
// Layout.  A row's matrices live in its slice of the caller's workspace: two
// NP x NP matrices (NP = n rounded up to 16; the padding is an identity block,
// which adds nothing to a determinant, a solve or a sum that stops at n), the
// transposed inputs (d x NP) and two vectors.  A workgroup of 512 threads walks
// these phases, separated by workgroup barriers only:
//   1  scalars and the inverse squared lengthscales into LDS; X transposed into
//      the slice (so that the pair loops read it along the lanes)
//   2  A = os Matern-5/2 + sigma^2 I, lower triangle, four rows per wave at a
//      time (a lane's column is loaded once for the four pairs)
//   3  right-looking blocked Cholesky in place, 16 x 16 blocks: the diagonal
//      block is factored in the registers of one wave (a row per lane, the
//      column read across the lanes by shuffles), the panel below it is solved
//      one row per thread and kept in LDS, the trailing blocks take
//      A_ij -= P_i P_j^T on v_mfma_f64_16x16x4 from that LDS panel
//   4  Z = L^{-1} block row by block row (T_j = sum_p L_ip Z_pj on the matrix
//      cores, staged in the LDS panel, then Z_ij = -L_ii^{-1} T_j)
//   5  beta = Z (y - c), alpha = Z^T beta
//   6  A^{-1} = Z^T Z over L's storage (L is dead by then)
//   7  W = alpha alpha^T - A^{-1}; the sums against the kernel and the trace;
//      V = W dKbar/dr^2 over A^{-1}'s storage
//   8  the d lengthscale sums sum_{i>k} V_ik (x_ij - x_kj)^2: a thread owns one
//      dimension j and one slice of the rows, so it keeps ONE accumulator
//      whatever d is; the slices are added in slice order
// Every sum folds in a fixed order and there are no atomics, no spin-waits and
// nothing shared between workgroups: a row's result does not depend on the
// other rows of the call, and a second call is bit-identical.
#include "common.h"

namespace {

constexpr int SN_T = 512, SN_NW = SN_T / 64, SN_NMAX = 1024, SN_DMAX = 256;
constexpr int SN_RB = 4;   // rows a pair loop takes at a time
constexpr int SN_PS = 17;  // row stride of the LDS blocks (doubles): 16 + 1 against bank conflicts
constexpr double SN_SQRT5 = 2.23606797749978969641, SN_LOG_2PI = 1.83787706640934548356;
constexpr double SN_PI = 3.14159265358979323846;

struct SaasDev {
  int n, d, NP;
  const double *X, *y, *z;
  double* work;
  int64_t stride;  // doubles of a row's slice
  double *U, *grad;
  int* status;
  double lgamma09;
};

__host__ __device__ inline int64_t sn_slice(int64_t NP, int64_t d) {
  return 2 * NP * NP + d * NP + 2 * NP;
}

__host__ inline size_t sn_lds_bytes(int NP) {
  return sizeof(double) * ((size_t)NP * SN_PS + 2 * 16 * SN_PS + 16 + SN_T + SN_DMAX);
}

// acc (+/-)= A B for 16 x 16 blocks: a(i, k) at A[i sai + k sak], b(k, j) at
// B[k sbk + j sbj] (either may be LDS or the workspace)
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

// the sum of v over the workgroup in every thread: a tree over red[SN_T] in a
// fixed order
__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = SN_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// r2[q] = sum_j w_j (x_{i0+q,j} - x_kj)^2 for SN_RB rows against one column k (a
// lane's): the column's coordinates are loaded once for the SN_RB rows, the
// rows' are wave-uniform.  Rows past n repeat row n - 1 (their result is unused).
__device__ __forceinline__ void pair_r2(const double* X, const double* XT, const double* w, int n,
                                        int d, int NP, int i0, int k, double (&r2)[SN_RB]) {
  const double* xr[SN_RB];
#pragma unroll
  for (int q = 0; q < SN_RB; ++q) {
    r2[q] = 0.0;
    xr[q] = X + (int64_t)(i0 + q < n ? i0 + q : n - 1) * d;
  }
  if (k >= n) return;
#pragma unroll 8
  for (int j = 0; j < d; ++j) {
    const double xk = XT[(int64_t)j * NP + k], wj = w[j];
#pragma unroll
    for (int q = 0; q < SN_RB; ++q) {
      const double dl = xk - xr[q][j];
      r2[q] += wj * dl * dl;
    }
  }
}

__device__ __forceinline__ bool sn_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

// status != 0: U = +inf and a zero gradient
__device__ __forceinline__ void sn_fail(const SaasDev& a, int c, int code) {
  const int D = a.d + 4;
  for (int e = threadIdx.x; e < D; e += SN_T) a.grad[(int64_t)c * D + e] = 0.0;
  if (threadIdx.x == 0) {
    a.U[c] = INFINITY;
    a.status[c] = code;
  }
}

__global__ __launch_bounds__(SN_T) void saas_potential_kernel(const SaasDev a) {
  extern __shared__ double sn_smem[];
  __shared__ int flag;
  const int n = a.n, d = a.d, NP = a.NP, D = d + 4, nb = NP / 16;
  double* P = sn_smem;                       // NP x 17: the panel / the staged T blocks
  double* Db = P + (size_t)NP * SN_PS;       // 16 x 17: a diagonal block
  double* Di = Db + 16 * SN_PS;              // 16 x 17: its inverse
  double* rd = Di + 16 * SN_PS;              // 16: reciprocal pivots
  double* red = rd + 16;                     // SN_T
  double* w = red + SN_T;                    // d: tau iota_j
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const double* z = a.z + (int64_t)c * D;
  double* Lm = a.work + (int64_t)c * a.stride;  // A, then L, then A^{-1}, then V
  double* Z = Lm + (int64_t)NP * NP;            // L^{-1}
  double* XT = Z + (int64_t)NP * NP;            // d x NP
  double* beta = XT + (int64_t)d * NP;
  double* alpha = beta + NP;

  // ---- 1: scalars, lengthscales, finiteness, X^T -----------------------------------------
  if (tid == 0) flag = 0;
  __syncthreads();
  const double os = exp(z[0]), cm = z[1], g = exp(z[2]), tau = exp(z[3]);
  const double s2 = 1e-4 + g;
  bool bad = !(sn_finite(os) && sn_finite(cm) && sn_finite(s2) && sn_finite(tau));
  for (int j = tid; j < d; j += SN_T) {
    const double wj = tau * exp(z[4 + j]);
    w[j] = wj;
    bad = bad || !sn_finite(wj) || !sn_finite(z[4 + j]);
  }
  for (int64_t e = tid; e < (int64_t)n * d; e += SN_T) {
    const double v = a.X[e];
    bad = bad || !sn_finite(v);
    XT[(e % d) * NP + e / d] = v;
  }
  for (int i = tid; i < n; i += SN_T) bad = bad || !sn_finite(a.y[i]);
  if (bad) flag = 1;
  __syncthreads();
  if (flag) {
    sn_fail(a, c, 1);
    return;
  }

  double quad = 0.0, logdet_half = 0.0, sum_alpha = 0.0, sK = 0.0, trW = 0.0, gj = 0.0;
  if (n > 0) {
    // ---- 2: A's lower triangle, identity on the padding ---------------------------------
    for (int i0 = SN_RB * wv; i0 < NP; i0 += SN_RB * SN_NW) {
      for (int k = lane; k < i0 + SN_RB; k += 64) {
        double r2[SN_RB];
        pair_r2(a.X, XT, w, n, d, NP, i0, k, r2);
#pragma unroll
        for (int q = 0; q < SN_RB; ++q) {
          const int i = i0 + q;
          if (k > i) continue;
          double v;
          if (i >= n)
            v = (i == k) ? 1.0 : 0.0;
          else if (i == k)
            v = os + s2;
          else
            v = os * kernel_from_d2<BO_MATERN52>(r2[q]);
          Lm[(int64_t)i * NP + k] = v;
        }
      }
    }
    __syncthreads();

    // ---- 3: blocked right-looking Cholesky ----------------------------------------------
    for (int kb = 0; kb < nb; ++kb) {
      const int k0 = kb * 16;
      // the diagonal block, in the registers of wave 0: lane r (and its three
      // copies r + 16, ...) holds row r; column j is scaled by its pivot and the
      // trailing columns take the rank-one update, the column read across the
      // lanes by shuffles.  No LDS round trip sits on the dependent chain.
      if (wv == 0) {
        const int r = lane & 15;
        double row[16];
#pragma unroll
        for (int cc = 0; cc < 16; ++cc)
          row[cc] = cc <= r ? Lm[(int64_t)(k0 + r) * NP + k0 + cc] : 0.0;
        bool badp = false;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          double piv = __shfl(row[j], j);
          if (!(piv > 0.0) || !sn_finite(piv)) {
            badp = true;
            piv = 1.0;
          }
          const double sq = sqrt(piv), rp = 1.0 / sq;
          const double lj = (r == j) ? sq : row[j] * rp;  // L[r][j] (0 above the diagonal)
          row[j] = lj;
          if (lane == j) rd[j] = rp;
#pragma unroll
          for (int cc = j + 1; cc < 16; ++cc) row[cc] -= lj * __shfl(lj, cc);
        }
        if (lane < 16) {
#pragma unroll
          for (int cc = 0; cc < 16; ++cc) {
            Db[r * SN_PS + cc] = cc <= r ? row[cc] : 0.0;
            if (cc <= r) Lm[(int64_t)(k0 + r) * NP + k0 + cc] = row[cc];
          }
        }
        if (badp) flag = 2;
      }
      __syncthreads();
      if (flag) {
        sn_fail(a, c, 2);
        return;
      }
      // the panel: row i of the block column solves x L_kk^T = a
      for (int i = k0 + 16 + tid; i < NP; i += SN_T) {
        double x[16];
        double* row = Lm + (int64_t)i * NP + k0;
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) x[cc] = row[cc];
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) {
          double s = x[cc];
#pragma unroll
          for (int p = 0; p < cc; ++p) s -= x[p] * Db[cc * SN_PS + p];
          x[cc] = s * rd[cc];
        }
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) {
          row[cc] = x[cc];
          P[(size_t)i * SN_PS + cc] = x[cc];
        }
      }
      __syncthreads();
      // the trailing blocks (bi >= bj > kb), dealt to the waves in turn
      int cnt = 0;
      for (int bi = kb + 1; bi < nb; ++bi) {
        for (int bj = kb + 1; bj <= bi; ++bj, ++cnt) {
          if (cnt % SN_NW != wv) continue;
          double* Cp = Lm + (int64_t)bi * 16 * NP + bj * 16;
          v4d acc = blk_load(Cp, NP);
          acc = blk_mma<true>(acc, P + (size_t)bi * 16 * SN_PS, SN_PS, 1,
                              P + (size_t)bj * 16 * SN_PS, 1, SN_PS);
          blk_store(Cp, NP, acc);
        }
      }
      __syncthreads();
    }

    // log det L
    for (int i = tid; i < n; i += SN_T) logdet_half += log(Lm[(int64_t)i * NP + i]);
    logdet_half = block_sum(logdet_half, red);

    // ---- 4: Z = L^{-1}, block row by block row -----------------------------------------
    for (int ib = 0; ib < nb; ++ib) {
      const int i0 = ib * 16;
      if (tid < 256) {
        const int r = tid >> 4, cc = tid & 15;
        Db[r * SN_PS + cc] = cc <= r ? Lm[(int64_t)(i0 + r) * NP + i0 + cc] : 0.0;
      }
      __syncthreads();
      if (tid < 16) {  // column tid of L_ii^{-1} by forward substitution
        double x[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          double s = (r == tid) ? 1.0 : 0.0;
#pragma unroll
          for (int p = 0; p < r; ++p) s -= Db[r * SN_PS + p] * x[p];
          x[r] = (r < tid) ? 0.0 : s / Db[r * SN_PS + r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) Di[r * SN_PS + tid] = x[r];
      }
      for (int j = wv; j < ib; j += SN_NW) {  // T_j = sum_p L_ip Z_pj
        v4d acc = v4d_zero();

        for (int p = j; p < ib; ++p)
          acc = blk_mma<false>(acc, Lm + (int64_t)i0 * NP + p * 16, NP, 1,
                               Z + (int64_t)p * 16 * NP + j * 16, NP, 1);
        blk_store(P + (size_t)j * 16 * SN_PS, SN_PS, acc);
      }
      __syncthreads();
      for (int j = wv; j <= ib; j += SN_NW) {
        double* Zp = Z + (int64_t)i0 * NP + j * 16;
        if (j == ib) {
          blk_store(Zp, NP, blk_load(Di, SN_PS));
        } else {
          const v4d acc = blk_mma<true>(v4d_zero(), Di, SN_PS, 1, P + (size_t)j * 16 * SN_PS,
                                        SN_PS, 1);
          blk_store(Zp, NP, acc);
        }
      }
      __syncthreads();
    }

    // ---- 5: beta = Z (y - c), alpha = Z^T beta -------------------------------------------
    for (int i = wv; i < n; i += SN_NW) {
      double s = 0.0;
      for (int k = lane; k <= i; k += 64) s += Z[(int64_t)i * NP + k] * (a.y[k] - cm);
      s = wave_sum(s);
      if (lane == 0) beta[i] = s;
    }
    __syncthreads();
    for (int k = tid; k < n; k += SN_T) {
      double s = 0.0;
      for (int i = k; i < n; ++i) s += Z[(int64_t)i * NP + k] * beta[i];
      alpha[k] = s;
      sum_alpha += s;
      quad += beta[k] * beta[k];
    }
    quad = block_sum(quad, red);
    sum_alpha = block_sum(sum_alpha, red);

    // ---- 6: A^{-1} = Z^T Z, lower blocks, over L's storage -------------------------------
    {
      int cnt = 0;
      for (int bi = 0; bi < nb; ++bi) {
        for (int bj = 0; bj <= bi; ++bj, ++cnt) {
          if (cnt % SN_NW != wv) continue;
          v4d acc = v4d_zero();

          for (int p = bi; p < nb; ++p)
            acc = blk_mma<false>(acc, Z + (int64_t)p * 16 * NP + bi * 16, 1, NP,
                                 Z + (int64_t)p * 16 * NP + bj * 16, NP, 1);
          blk_store(Lm + (int64_t)bi * 16 * NP + bj * 16, NP, acc);
        }
      }
    }
    __syncthreads();

    // ---- 7: W against the kernel; V = W dKbar / dr^2 -------------------------------------
    for (int i0 = SN_RB * wv; i0 < n; i0 += SN_RB * SN_NW) {
      for (int k = lane; k < i0 + SN_RB && k < n; k += 64) {
        double r2[SN_RB];
        pair_r2(a.X, XT, w, n, d, NP, i0, k, r2);
        const double ak = alpha[k];
#pragma unroll
        for (int q = 0; q < SN_RB; ++q) {
          const int i = i0 + q;
          if (i >= n || k > i) continue;
          const double W = alpha[i] * ak - Lm[(int64_t)i * NP + k];
          if (k == i) {
            trW += W;
            sK += W;
          } else {
            const double s5r = SN_SQRT5 * sqrt(fmax(r2[q], 1e-30));
            const double ex = exp(-s5r);
            sK += 2.0 * W * (1.0 + s5r + (5.0 / 3.0) * r2[q]) * ex;
            Lm[(int64_t)i * NP + k] = W * (-(5.0 / 6.0) * (1.0 + s5r) * ex);
          }
        }
      }
    }
    sK = block_sum(sK, red);
    trW = block_sum(trW, red);  // (its barriers also publish V)

    // ---- 8: the lengthscale sums, one accumulator per thread -----------------------------
    {
      const int S = SN_T / d, j = tid % d, s = tid / d;
      double acc = 0.0;
      if (s < S) {
        // SN_RB rows at a time share the loads of x_kj
        for (int ib = s; ib < n; ib += SN_RB * S) {
          double xi[SN_RB], part[SN_RB];
          const double* Vr[SN_RB];
          int iq[SN_RB];
#pragma unroll
          for (int q = 0; q < SN_RB; ++q) {
            const int i = ib + q * S;
            iq[q] = i < n ? i : 0;  // (a row past n takes no k)
            xi[q] = a.X[(int64_t)iq[q] * d + j];
            Vr[q] = Lm + (int64_t)iq[q] * NP;
            part[q] = 0.0;
          }
          int kend = 0;
#pragma unroll
          for (int q = 0; q < SN_RB; ++q) kend = iq[q] > kend ? iq[q] : kend;
#pragma unroll 4
          for (int k = 0; k < kend; ++k) {
            const double xk = a.X[(int64_t)k * d + j];
#pragma unroll
            for (int q = 0; q < SN_RB; ++q) {
              // (loaded whatever k is, so that the loads of several k go out
              // together; past the diagonal the row holds other data: selected away)
              const double v = Vr[q][k], dl = xi[q] - xk;
              part[q] += k < iq[q] ? v * dl * dl : 0.0;
            }
          }
#pragma unroll
          for (int q = 0; q < SN_RB; ++q) acc += part[q];
        }
      }
      __syncthreads();
      red[tid] = acc;
      __syncthreads();
      if (tid < d) {
        for (int q = 0; q < S; ++q) gj += red[q * d + tid];
        gj *= os * w[tid];  // d ll / d z_{4+j}
      }
    }
  }

  // ---- the priors, the Jacobians and the outputs -------------------------------------------
  const double sum_gj = block_sum(tid < d ? gj : 0.0, red);
  double lp = 0.0;
  if (tid < d) {
    const double io = exp(z[4 + tid]);
    lp = log(2.0 / SN_PI) - log1p(io * io) + z[4 + tid];
    const double dprior = 1.0 - 2.0 / (1.0 + 1.0 / (io * io));
    gj = -(gj + dprior);
  }
  lp = block_sum(lp, red);
  bool nonfinite = tid < d && !sn_finite(gj);
  double U = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
  {
    const double t = tau / 0.1;
    const double ll = n > 0 ? -0.5 * quad - logdet_half - 0.5 * n * SN_LOG_2PI : 0.0;
    lp += 2.0 * log(0.15) + 2.0 * z[0] - 0.15 * os;
    lp += -0.5 * cm * cm - 0.5 * SN_LOG_2PI;
    lp += 0.9 * log(10.0) - a.lgamma09 + 0.9 * z[2] - 10.0 * g;
    lp += log(2.0 / (SN_PI * 0.1)) - log1p(t * t) + z[3];
    U = -(ll + lp);
    g0 = -(0.5 * os * sK + 2.0 - 0.15 * os);
    g1 = -(sum_alpha - cm);
    g2 = -(0.5 * g * trW + 0.9 - 10.0 * g);
    g3 = -(sum_gj + 1.0 - 2.0 / (1.0 + 1.0 / (t * t)));
    nonfinite = nonfinite || !(sn_finite(U) && sn_finite(g0) && sn_finite(g1) && sn_finite(g2) &&
                               sn_finite(g3));
  }
  if (nonfinite) flag = 1;
  __syncthreads();
  if (flag) {
    sn_fail(a, c, 1);
    return;
  }
  if (tid < d) a.grad[(int64_t)c * D + 4 + tid] = gj;
  if (tid == 0) {
    a.U[c] = U;
    a.grad[(int64_t)c * D + 0] = g0;
    a.grad[(int64_t)c * D + 1] = g1;
    a.grad[(int64_t)c * D + 2] = g2;
    a.grad[(int64_t)c * D + 3] = g3;
    a.status[c] = 0;
  }
}

int sn_limits(const char* who, int64_t n, int64_t d, int64_t C) {
  BO_CHECK_ARG(n >= 0 && n <= SN_NMAX, "%s: 0 <= n <= %d (got %lld)", who, SN_NMAX, (long long)n);
  BO_CHECK_ARG(d >= 1 && d <= SN_DMAX, "%s: 1 <= d <= %d (got %lld)", who, SN_DMAX, (long long)d);
  BO_CHECK_ARG(C >= 1 && C * n * n < ((int64_t)1 << 31), "%s: C >= 1 and C n^2 < 2^31 (got C = %lld)",
               who, (long long)C);
  return BO_OK;
}

}  // namespace

extern "C" int bo_saas_potential_work(int64_t n, int d, int64_t C, int64_t* elems) {
  if (int st = sn_limits("bo_saas_potential_work", n, d, C); st != BO_OK) return st;
  BO_CHECK_ARG(elems, "bo_saas_potential_work: elems is required");
  *elems = C * sn_slice(ceil_div(n, 16) * 16, d);
  return BO_OK;
}

extern "C" int bo_saas_potential_impl(const BoSaasPotentialArgs* a, void* stream) {
  const char* who = "bo_saas_potential";
  if (int st = sn_limits(who, a->n, a->d, a->C); st != BO_OK) return st;
  BO_CHECK_ARG(a->z && a->U && a->grad && a->status, "%s: z, U, grad and status are required", who);
  BO_CHECK_ARG(a->n == 0 || (a->X && a->y), "%s: X and y are required", who);
  SaasDev v;
  v.n = (int)a->n;
  v.d = a->d;
  v.NP = (int)(ceil_div(a->n, 16) * 16);
  v.stride = sn_slice(v.NP, v.d);
  const int64_t need = a->C * v.stride;
  BO_CHECK_ARG(need == 0 || (a->work && a->work_size >= need),
               "%s: work of at least %lld doubles is required (work_size %lld)", who,
               (long long)need, (long long)a->work_size);
  v.X = a->X;
  v.y = a->y;
  v.z = a->z;
  v.work = a->work;
  v.U = a->U;
  v.grad = a->grad;
  v.status = a->status;
  v.lgamma09 = std::lgamma(0.9);
  const size_t lds = sn_lds_bytes(v.NP);
  if (lds > 48 * 1024)
    BO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(saas_potential_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  saas_potential_kernel<<<(unsigned)a->C, SN_T, lds, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}
