// Risk-averse Monte-Carlo acquisition under input perturbations: the sample,
// risk-measure and acquisition reduction over a wide t-batch of Q = q n_w
// jointly distributed points (botorch/acquisition/risk_measures.py: CVaR, VaR,
// WorstCase, Expectation behind models/transforms/input.py InputPerturbation),
// and its gradient.  The definitions stand in include/botorch_amd.h
// (BoQmcRiskArgs) and DESIGN.md section 29.
//
//   f[s][j] = mean_j + sum_{i <= j} L[j][i] Z[s][i]          (S x Q)
//   r[s][a] = risk of the block f[s][a n_w .. (a + 1) n_w)   (S x q)
//   acq     = the mode's reduction of r over a and s, as qmc.hip reduces f
//
// Layout.  One workgroup of 256 threads (4 waves) owns one t-batch.  Q reaches
// 128, so no lane can hold a row of L as qmc.hip's do: the root's lower 16 x 16
// tiles are staged once in LDS, transposed ([k][j], the B operand's order) and
// zero-padded to QT = ceil(Q / 16) tile rows: QT (QT + 1) / 2 tiles, 72 KB at
// Q = 128.  Samples go through in passes of 64, 16 per wave:
//
//   1. F = mean + Z L^T on v_mfma_f64_16x16x4.  A wave's A operand is its 16
//      rows of Z (read from memory: S x Q is shared by every workgroup and stays
//      in L2), the B operand an LDS tile; column tile tj accumulates over the
//      k-tiles tk <= tj only, from an accumulator initialised with mean.  One Z
//      element feeds every column tile tj >= tk.  The pass's F (64 x QP, row
//      pitch QP + 2) goes to LDS: an n_w-block straddles MFMA tiles whenever
//      n_w is no multiple of 16.
//   2. Ranks.  Element (s, j) counts the entries of its block that precede it
//      (smaller, or equal with a lower index): 64 Q independent counts over the
//      256 threads, n_w LDS reads each, which a wave mostly shares (a broadcast).
//      The count is the element's 0-based rank, a byte in LDS.  No sort, no
//      data-dependent exchange: equal values never flip.
//   3. r[s][a]: one thread per (s, a) walks its block in index order and sums
//      the entries of rank < k (kind 0), or picks rank k - 1 (kind 1).
//   4. One lane per sample (wave 0) reduces r[s][.] by the mode and folds the
//      result into its own running sum (or online log-sum-exp pair) in pass
//      order; a xor butterfly over the wave ends the call.
//
// Backward: the same passes; step 4 turns into the q-level weights
// w[s][a] = dacq d acq / d r[s][a], then G[s][j] = w[s][a] (1 / k on the
// selected entries | 1 on the k-th) overwrites F in place.
// dL = tril(G^T Z) accumulates on the matrix cores across all passes, each wave
// owning the lower tiles w, w + 4, ... (9 at Q = 128) in registers; the A operand
// is G from LDS, the B operand Z from memory.  dmean_j = sum_s G[s][j], thread j
// in sample order.  LDS at Q = 128: 72 KB of L, 65 KB of F / G, 8 KB of r / w and
// 8 KB of ranks: 153 KB of gfx950's 160, so one workgroup per CU.
//
// No atomics, every sum in a fixed order: repeated calls are bitwise identical
// and row b of a B-row call equals the one-row call.
#include "common.h"

#include "logred.h"

namespace {

constexpr int RISK_T = 256, RISK_PASS = 64, RISK_QMAX = 16, RISK_NWMAX = 128, RISK_QQMAX = 128;
constexpr int RISK_TMAX = RISK_QQMAX / 16;               // tile rows
constexpr int RISK_WTILES = (RISK_TMAX * (RISK_TMAX + 1) / 2 + 3) / 4;  // dL tiles per wave

struct RiskDev {
  int q, n_w, k, kind, mode, Q, QT;
  int64_t B, S;
  const double *mean, *L, *Z;
  double best_f;
  LogRedParams lp;
  double* acq;
  const double* dacq;
  double *dmean, *dL;
};

__host__ __device__ constexpr int tri(int i) { return i * (i + 1) / 2; }
__host__ __device__ constexpr int risk_fs(int QP) { return QP + 2; }

size_t risk_lds_bytes(int QT) {
  const int QP = QT * 16;
  return (size_t)(tri(QT) * 256 + RISK_PASS * risk_fs(QP) + RISK_PASS * RISK_QMAX) * sizeof(double) +
         (size_t)RISK_PASS * QP;
}

template <bool GRAD>
__global__ __launch_bounds__(RISK_T) void risk_kernel(const RiskDev a) {
  extern __shared__ double risk_smem[];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, col = lane & 15, quad = lane >> 4;
  const int Q = a.Q, QT = a.QT, QP = QT * 16, FS = risk_fs(QP), nw = a.n_w, q = a.q, k = a.k;
  const int ntiles = tri(QT);
  const int64_t b = blockIdx.x, S = a.S;
  double* Lt = risk_smem;                  // ntiles x [k][j]
  double* F = Lt + ntiles * 256;           // 64 x FS: f, then G (backward)
  double* R = F + RISK_PASS * FS;          // 64 x 16: r, then w (backward)
  unsigned char* Rk = reinterpret_cast<unsigned char*>(R + RISK_PASS * RISK_QMAX);  // 64 x QP

  const double* Lb = a.L + b * Q * Q;
  for (int e = t; e < ntiles * 256; e += RISK_T) {
    const int tile = e >> 8, jj = (e >> 4) & 15, kk = e & 15;
    int tj = 0;
    while (tri(tj + 1) <= tile) ++tj;
    const int j = tj * 16 + jj, i = (tile - tri(tj)) * 16 + kk;
    Lt[tile * 256 + kk * 16 + jj] = (j < Q && i <= j) ? Lb[(int64_t)j * Q + i] : 0.0;
  }
  double meanv[RISK_TMAX];
#pragma unroll
  for (int tj = 0; tj < RISK_TMAX; ++tj)
    meanv[tj] = (tj < QT && tj * 16 + col < Q) ? a.mean[b * Q + tj * 16 + col] : 0.0;

  // backward: this wave's lower tiles (tj, ti) of dL and their accumulators
  int tjv[RISK_WTILES], tiv[RISK_WTILES];
  v4d dacc[RISK_WTILES];
  double dm = 0.0;
  if (GRAD) {
#pragma unroll
    for (int m = 0; m < RISK_WTILES; ++m) {
      const int tile = w + 4 * m;
      int tj = 0;
      while (tri(tj + 1) <= tile) ++tj;
      tjv[m] = tj;
      tiv[m] = tile - tri(tj);
      dacc[m] = v4d_zero();
    }
  }
  const double inv_k = 1.0 / (double)k, inv_S = 1.0 / (double)S;
  const bool log_mode = a.mode == BO_QMC_QLOGEI;
  double dacq = 0.0, acq_in = 0.0;
  if (GRAD) {
    dacq = a.dacq[b];
    if (log_mode) acq_in = a.acq[b];
  }
  double vsum = 0.0;               // wave 0: lane's share of sum_s u_s
  LseAcc lse{-INFINITY, 0.0};      // or of the log-sum-exp
  __syncthreads();

  for (int64_t s0 = 0; s0 < S; s0 += RISK_PASS) {
    {  // 1. F = mean + Z L^T
      v4d acc[RISK_TMAX];
#pragma unroll
      for (int tj = 0; tj < RISK_TMAX; ++tj) {
        const v4d m4 = {meanv[tj], meanv[tj], meanv[tj], meanv[tj]};
        acc[tj] = m4;
      }
      const int64_t srow = s0 + 16 * w + col;
      const bool sok = srow < S;
      const double* zrow = a.Z + (sok ? srow : 0) * Q;
      for (int tk = 0; tk < QT; ++tk) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int c = tk * 16 + kk * 4 + quad;
          const double av = (sok && c < Q) ? zrow[c] : 0.0;
          const double* lt = Lt + (kk * 4 + quad) * 16 + col;
#pragma unroll
          for (int tj = 0; tj < RISK_TMAX; ++tj)
            if (tj >= tk && tj < QT) acc[tj] = mfma_f64(av, lt[(tri(tj) + tk) * 256], acc[tj]);
        }
      }
#pragma unroll
      for (int tj = 0; tj < RISK_TMAX; ++tj)
        if (tj < QT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) F[(16 * w + mfma_row(lane, r)) * FS + tj * 16 + col] = acc[tj][r];
        }
    }
    __syncthreads();
    // 2. the rank of every element in its block
    for (int e = t; e < RISK_PASS * Q; e += RISK_T) {
      const int s = e / Q, j = e - s * Q;
      const int base = (j / nw) * nw, jo = j - base;
      const double* fb = F + s * FS + base;
      const double v = fb[jo];
      int cnt = 0;
#pragma unroll 4
      for (int i = 0; i < nw; ++i) {
        const double fi = fb[i];
        cnt += (fi < v) || (fi == v && i < jo);
      }
      Rk[s * QP + j] = (unsigned char)cnt;
    }
    __syncthreads();
    // 3. r[s][a], its block in index order
    for (int it = t; it < RISK_PASS * q; it += RISK_T) {
      const int s = it / q, ai = it - s * q;
      const double* fb = F + s * FS + ai * nw;
      const unsigned char* rb = Rk + s * QP + ai * nw;
      double r = 0.0;
      if (a.kind == 0) {
        for (int i = 0; i < nw; ++i)
          if (rb[i] < k) r += fb[i];
        r *= inv_k;
      } else {
        for (int i = 0; i < nw; ++i)
          if (rb[i] == k - 1) r = fb[i];
      }
      R[s * RISK_QMAX + ai] = r;
    }
    __syncthreads();
    // 4. the mode's reduction over a; one lane of wave 0 per sample
    if (t < RISK_PASS) {
      const bool ok = s0 + t < S;
      double r[RISK_QMAX], wv[RISK_QMAX];
#pragma unroll
      for (int ai = 0; ai < RISK_QMAX; ++ai) {
        r[ai] = ai < q ? R[t * RISK_QMAX + ai] : 0.0;
        wv[ai] = 0.0;
      }
      if (log_mode) {
        double li[RISK_QMAX], dz[RISK_QMAX], g[RISK_QMAX];
#pragma unroll
        for (int ai = 0; ai < RISK_QMAX; ++ai) {
          dz[ai] = 0.0;
          li[ai] = ai < q ? log_soft_relu(r[ai] - a.best_f, a.lp, GRAD ? &dz[ai] : nullptr) : 0.0;
        }
        const double u = log_q_reduce<RISK_QMAX>(li, q, a.lp, GRAD ? &g : nullptr);
        if (GRAD) {
          const double coef = ok ? dacq * exp(u - acq_in) * inv_S : 0.0;
#pragma unroll
          for (int ai = 0; ai < RISK_QMAX; ++ai)
            if (ai < q) wv[ai] = coef * g[ai] * dz[ai];
        } else if (ok) {
          lse = lse_push(lse, u);
        }
      } else {
        double M = r[0];
        int arg = 0;
#pragma unroll
        for (int ai = 1; ai < RISK_QMAX; ++ai)
          if (ai < q && r[ai] > M) {
            M = r[ai];
            arg = ai;
          }
        const bool relu = a.mode == BO_QMC_QEI;
        if (GRAD) {
          const double coef = (ok && (!relu || M > a.best_f)) ? dacq * inv_S : 0.0;
#pragma unroll
          for (int ai = 0; ai < RISK_QMAX; ++ai)
            if (ai == arg) wv[ai] = coef;
        } else if (ok) {
          vsum += relu ? fmax(M - a.best_f, 0.0) : M;
        }
      }
      if (GRAD) {
#pragma unroll
        for (int ai = 0; ai < RISK_QMAX; ++ai) R[t * RISK_QMAX + ai] = wv[ai];
      }
    }
    if (GRAD) {
      __syncthreads();
      // G over F, in place
      for (int e = t; e < RISK_PASS * Q; e += RISK_T) {
        const int s = e / Q, j = e - s * Q;
        const int rk = Rk[s * QP + j];
        const double sel = a.kind == 0 ? (rk < k ? inv_k : 0.0) : (rk == k - 1 ? 1.0 : 0.0);
        F[s * FS + j] = R[s * RISK_QMAX + j / nw] * sel;
      }
      __syncthreads();
      // dL += tril(G^T Z): D[j][i], A = G[s][j] (LDS), B = Z[s][i] (memory)
#pragma unroll
      for (int m = 0; m < RISK_WTILES; ++m) {
        if (w + 4 * m < ntiles) {
          const int c = tiv[m] * 16 + col;
          const double* gp = F + tjv[m] * 16 + col;
#pragma unroll 4
          for (int ks = 0; ks < RISK_PASS / 4; ++ks) {
            const int sl = ks * 4 + quad;
            const int64_t sg = s0 + sl;
            const double bv = (sg < S && c < Q) ? a.Z[sg * Q + c] : 0.0;
            dacc[m] = mfma_f64(gp[sl * FS], bv, dacc[m]);
          }
        }
      }
      if (t < Q) {
        for (int sl = 0; sl < RISK_PASS; ++sl) dm += F[sl * FS + t];
      }
      __syncthreads();  // (G is read before the next pass's F lands)
    }
  }

  if (GRAD) {
    double* dLb = a.dL + b * Q * Q;
#pragma unroll
    for (int m = 0; m < RISK_WTILES; ++m) {
      if (w + 4 * m < ntiles) {
        const int i = tiv[m] * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = tjv[m] * 16 + mfma_row(lane, r);
          if (j < Q && i < Q) dLb[(int64_t)j * Q + i] = i <= j ? dacc[m][r] : 0.0;
        }
      }
    }
    for (int e = t; e < Q * Q; e += RISK_T) {  // the tiles above the diagonal
      const int j = e / Q, i = e - j * Q;
      if ((i >> 4) > (j >> 4)) dLb[e] = 0.0;
    }
    if (t < Q) a.dmean[b * Q + t] = dm;
  } else if (t < RISK_PASS) {
    if (log_mode) {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const LseAcc other{__shfl_xor(lse.m, o), __shfl_xor(lse.s, o)};
        lse = lse_merge(lse, other);
      }
      if (t == 0) a.acq[b] = lse.m + log(lse.s) - log((double)S);
    } else {
      vsum = wave_sum(vsum);
      if (t == 0) a.acq[b] = vsum * inv_S;
    }
  }
}

int risk_fill(const BoQmcRiskArgs* a, const char* who, RiskDev* v) {
  BO_CHECK_ARG(a->n_w >= 2 && a->n_w <= RISK_NWMAX, "%s: 2 <= n_w <= %d (got %d)", who, RISK_NWMAX,
               a->n_w);
  BO_CHECK_ARG(a->q >= 1 && a->q <= RISK_QMAX, "%s: 1 <= q <= %d (got %d)", who, RISK_QMAX, a->q);
  BO_CHECK_ARG(a->q * a->n_w <= RISK_QQMAX, "%s: Q = q n_w <= %d (got %d)", who, RISK_QQMAX,
               a->q * a->n_w);
  BO_CHECK_ARG(a->k >= 1 && a->k <= a->n_w, "%s: 1 <= k <= n_w (got k = %d, n_w = %d)", who, a->k,
               a->n_w);
  BO_CHECK_ARG(a->kind == 0 || a->kind == 1, "%s: kind 0 (CVaR) or 1 (VaR) (got %d)", who, a->kind);
  BO_CHECK_ARG(a->mode == BO_QMC_QSR || a->mode == BO_QMC_QEI || a->mode == BO_QMC_QLOGEI,
               "%s: mode BO_QMC_QSR, BO_QMC_QEI or BO_QMC_QLOGEI (got %d)", who, a->mode);
  BO_CHECK_ARG(a->S >= 1 && a->S <= (int64_t)1 << 24, "%s: 1 <= S <= 2^24 (got %lld)", who,
               (long long)a->S);
  BO_CHECK_ARG(a->B >= 1 && a->B <= 0x7fffffff, "%s: 1 <= B < 2^31 (got %lld)", who,
               (long long)a->B);
  BO_CHECK_ARG(a->mean && a->L && a->Z, "%s: mean, L and Z are required", who);
  if (a->mode == BO_QMC_QLOGEI)
    BO_CHECK_ARG(a->tau_relu > 0.0 && a->tau_max > 0.0, "%s: tau_relu and tau_max must be positive",
                 who);
  v->q = a->q;
  v->n_w = a->n_w;
  v->k = a->k;
  v->kind = a->kind;
  v->mode = a->mode;
  v->Q = a->q * a->n_w;
  v->QT = (v->Q + 15) / 16;
  v->B = a->B;
  v->S = a->S;
  v->mean = a->mean;
  v->L = a->L;
  v->Z = a->Z;
  v->best_f = a->best_f;
  v->lp = LogRedParams{a->tau_relu, a->tau_max, a->fat};
  v->acq = a->acq;
  v->dacq = a->dacq;
  v->dmean = a->dmean;
  v->dL = a->dL;
  return BO_OK;
}

template <typename K>
int risk_launch(K kernel, const RiskDev& v, void* stream) {
  const size_t lds = risk_lds_bytes(v.QT);
  if (lds > 48 * 1024)
    BO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kernel<<<(unsigned)v.B, RISK_T, lds, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

}  // namespace

// The C ABI entry points (include/botorch_amd.h): bo_qmc_risk and
// bo_qmc_risk_backward behind their header checks (abi_structs.cpp).
extern "C" int bo_qmc_risk_impl(const BoQmcRiskArgs* a, void* stream) {
  RiskDev v;
  if (int st = risk_fill(a, "bo_qmc_risk", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->acq, "bo_qmc_risk: acq is required");
  return risk_launch(risk_kernel<false>, v, stream);
}

extern "C" int bo_qmc_risk_backward_impl(const BoQmcRiskArgs* a, void* stream) {
  RiskDev v;
  if (int st = risk_fill(a, "bo_qmc_risk_backward", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->dacq && a->dmean && a->dL,
               "bo_qmc_risk_backward: dacq, dmean and dL are required");
  BO_CHECK_ARG(a->mode != BO_QMC_QLOGEI || a->acq,
               "bo_qmc_risk_backward: the log mode reads the forward's acq");
  return risk_launch(risk_kernel<true>, v, stream);
}
