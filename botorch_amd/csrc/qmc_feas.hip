// Feasibility-weighted single-objective MC reductions over the members of a
// model list: qEI / qLogEI (scalar best_f) and qNEI / qLogNEI (per-sample best_f,
// cached-root term F) with outcome constraints (botorch/acquisition/
// monte_carlo.py:253-330, logei.py:219-234, utils/objective.py:134-180).
//
//   f[s][b][a][t] = mean[t][b][a] + sum_{j<=a} L[t][b][a][j] Z[s][j Mt + t] (+ F[t][s][b Qp + a])
//   obj   = sum_t c_t f_t                    con_i = sum_t A[i][t] f_t - rhs_i
//   l     = sum_i logsig(-con_i / eta_i)     (logexpit | log_fatmoid; or the caller's tensor)
//   plain: u_s = max_a relu(obj_a - bf_s) exp(l_a),                 acq_b = mean_s u_s
//   log:   u_s = q_reduce_a(log_soft_relu(obj_a - bf_s) + l_a),     acq_b = logmeanexp_s u_s
//
// One workgroup per t-batch.  The members' roots and means live in LDS for the
// whole kernel; the samples go through in chunks: the chunk's base-sample rows
// (q Mt doubles each) are staged in LDS, a lane evaluates one sample (phase 1),
// and in the backward leaves, per (sample, point), the cotangent of obj and of
// every con_i in LDS -- the cotangent of f_t is gobj c_t + sum_i gcon_i A[i][t],
// rank 1 + k in t, so no S x q x Mt tensor exists anywhere.  Phase 2 gives each
// thread fixed entries (t, a, j <= a) of dL (and dmean at j = 0), summed over the
// chunk's samples in order: no atomics, bitwise reproducible.  The chunk length
// is chosen by the host from the LDS budget (qmc_feas_chunk below).
#include "common.h"

#include <algorithm>

#include "logred.h"

namespace {

constexpr int QMAX = 16;
constexpr int MTMAX = 8;
constexpr int KMAX = 8;
constexpr int THREADS = 256;
constexpr int EPT = MTMAX * QMAX * QMAX / THREADS;  // dL entries per thread (phase 2)
constexpr int LDS_DOUBLES = 8000;                   // 62.5 KiB: two workgroups per CU
constexpr int TAB_DOUBLES = MTMAX + KMAX * MTMAX + 2 * KMAX;
constexpr int RED_DOUBLES = 2 * THREADS;

// The objective weights and the in-kernel (linear) constraints, by value.
struct FeasTab {
  double c[MTMAX];
  double A[KMAX][MTMAX];
  double rhs[KMAX];
  double eta[KMAX];
  int k;
  int fat;
};

// utils/safe_math.py:84-99: logexpit(x) = -log1pexp(-x), log1pexp(y) =
// log1p(e^y) up to y = 18 and y + e^-y above; d receives the derivative that
// autograd takes through the selected branch.
__device__ __forceinline__ double logexpit_d(double x, double* d) {
  const double y = -x;
  if (y <= 18.0) {
    const double e = exp(y);
    if (d) *d = e / (1.0 + e);
    return -log1p(e);
  }
  const double e = exp(-y);
  if (d) *d = 1.0 - e;
  return -(y + e);
}

// utils/safe_math.py:422-451: log of the two Cauchy halves joined at 0.
__device__ __forceinline__ double log_fatmoid_d(double x, double* d) {
  const double s = 0.57735026918962576451;  // 1 / sqrt(3)
  if (x < 0.0) {
    const double z = x - s;
    const double den = 1.0 + z * z;
    if (d) *d = -2.0 * z / den;
    return log((2.0 / 3.0) / den);
  }
  const double z = x + s;
  const double den = 1.0 + z * z;
  const double f = 1.0 - (2.0 / 3.0) / den;
  if (d) *d = (4.0 / 3.0) * z / (den * den) / f;
  return log(f);
}

struct Carve {
  double *Ls, *mu, *tab, *red, *Zs, *gs;
  int ZS, GS;
};

__device__ __forceinline__ Carve carve(double* sm, int q, int Mt, int kk, int chunk) {
  Carve c;
  c.Ls = sm;
  c.mu = c.Ls + Mt * q * q;
  c.tab = c.mu + Mt * q;
  c.red = c.tab + TAB_DOUBLES;
  c.Zs = c.red + RED_DOUBLES;
  c.ZS = (q * Mt) | 1;        // odd row strides: a lane per sample, no bank conflicts
  c.GS = (q * (kk + 1)) | 1;
  c.gs = c.Zs + chunk * c.ZS;
  return c;
}

// QB: the q bucket li[] is sized for.  LOG: the LogEI reductions.  EXT: the
// weights (plain) / log-weights (LOG) come from wext (S x B x q) and the
// backward returns their cotangent dfeas.  BWD: the backward (acq is then the
// forward's value, read in LOG mode).
template <int QB, bool LOG, bool EXT, bool BWD>
__global__ __launch_bounds__(THREADS) void qmc_feas_kernel(
    int B, int q, int Mt, int S, const double* __restrict__ mean, const double* __restrict__ Lg,
    const double* __restrict__ Z, const double* __restrict__ F, int64_t ldF, int64_t sF, int Qp,
    double best_f, const double* __restrict__ best_f_s, FeasTab tb, const double* __restrict__ wext,
    LogRedParams lp, int chunk, double* __restrict__ acq, const double* __restrict__ dacq,
    double* __restrict__ dmean, double* __restrict__ dL, double* __restrict__ dF,
    double* __restrict__ dfeas) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int kk = EXT ? 0 : tb.k;
  const Carve cv = carve(smem, q, Mt, kk, chunk);
  double* const tc = cv.tab;                    // c[t]
  double* const tA = tc + MTMAX;                // A[i][t]
  double* const trhs = tA + KMAX * MTMAX;
  double* const tie = trhs + KMAX;

  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int zw = q * Mt;
  for (int e = tid; e < Mt * q * q; e += THREADS) {
    const int t = e / (q * q), r = e % (q * q);
    cv.Ls[e] = Lg[((int64_t)t * B + b) * q * q + r];
  }
  for (int e = tid; e < Mt * q; e += THREADS)
    cv.mu[e] = mean[((int64_t)(e / q) * B + b) * q + e % q];
  if (tid < MTMAX) tc[tid] = tb.c[tid];
  if (tid < KMAX * MTMAX) tA[tid] = tb.A[tid / MTMAX][tid % MTMAX];
  if (tid < KMAX) {
    trhs[tid] = tb.rhs[tid];
    tie[tid] = tb.eta[tid];
  }

  double g = 0.0, a_fwd = 0.0;
  if (BWD) {
    g = dacq[b] / (double)S;
    if (LOG) a_fwd = acq[b];
  }
  double usum = 0.0;                 // forward, plain: this thread's samples in order
  LseAcc lse{-INFINITY, 0.0};        // forward, log
  double dl_acc[EPT], dm_acc[EPT];   // backward: this thread's entries
#pragma unroll
  for (int r = 0; r < EPT; ++r) dl_acc[r] = dm_acc[r] = 0.0;

  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int ns = min(chunk, S - s0);
    __syncthreads();  // the tables (first pass); the previous chunk's phase 2
    for (int e = tid; e < ns * zw; e += THREADS)
      cv.Zs[(e / zw) * cv.ZS + e % zw] = Z[(int64_t)s0 * zw + e];
    __syncthreads();
    // Phase 1: a lane per sample.
    for (int s = tid; s < ns; s += THREADS) {
      const double* z = cv.Zs + s * cv.ZS;
      double* gsm = cv.gs + s * cv.GS;
      const double bf = best_f_s ? best_f_s[s0 + s] : best_f;
      const int64_t wrow = ((int64_t)(s0 + s) * B + b) * q;
      double li[QB];  // plain: relu * w;  log: log_soft_relu + l
#pragma unroll
      for (int a = 0; a < QB; ++a) {
        li[a] = LOG ? -INFINITY : 0.0;
        if (a < q) {
          double obj = 0.0, con[KMAX];
#pragma unroll
          for (int i = 0; i < KMAX; ++i) con[i] = 0.0;
          for (int t = 0; t < Mt; ++t) {
            const double* Lr = cv.Ls + (t * q + a) * q;
            double f = cv.mu[t * q + a];
            if (F) f += F[t * sF + (int64_t)(s0 + s) * ldF + (int64_t)b * Qp + a];
            for (int j = 0; j <= a; ++j) f = fma(Lr[j], z[j * Mt + t], f);
            obj = fma(tc[t], f, obj);
            if (!EXT) {
#pragma unroll
              for (int i = 0; i < KMAX; ++i)
                if (i < kk) con[i] = fma(tA[i * MTMAX + t], f, con[i]);
            }
          }
          double l = 0.0;
          if (EXT) {
            l = wext[wrow + a];  // plain: the weight itself
          } else {
#pragma unroll
            for (int i = 0; i < KMAX; ++i) {
              if (i < kk) {
                const double x = -(con[i] - trhs[i]) / tie[i];
                l += tb.fat ? log_fatmoid_d(x, nullptr) : logexpit_d(x, nullptr);
                if (BWD) gsm[a * (kk + 1) + 1 + i] = x;
              }
            }
          }
          const double zi = obj - bf;
          if (BWD) gsm[a * (kk + 1)] = zi;
          if (LOG) {
            li[a] = log_soft_relu(zi, lp, nullptr) + l;
          } else {
            const double w = EXT ? l : exp(l);
            li[a] = fmax(zi, 0.0) * w;
          }
        }
      }
      if (LOG) {
        double gq[QB];
        const double u = log_q_reduce<QB>(li, q, lp, BWD ? &gq : nullptr);
        if (!BWD) {
          lse = lse_push(lse, u);
        } else {
          const double ws = g * exp(u - a_fwd);
#pragma unroll
          for (int a = 0; a < QB; ++a) {
            if (a < q) {
              const double gl = ws * gq[a];  // cotangent of li_a, hence of l_a
              double dz;
              (void)log_soft_relu(gsm[a * (kk + 1)], lp, &dz);
              gsm[a * (kk + 1)] = gl * dz;
              if (EXT) {
                dfeas[wrow + a] = gl;
              } else {
#pragma unroll
                for (int i = 0; i < KMAX; ++i) {
                  if (i < kk) {
                    double dx;
                    const double x = gsm[a * (kk + 1) + 1 + i];
                    if (tb.fat) (void)log_fatmoid_d(x, &dx);
                    else (void)logexpit_d(x, &dx);
                    gsm[a * (kk + 1) + 1 + i] = -gl * dx / tie[i];
                  }
                }
              }
            }
          }
        }
      } else {
        double m = 0.0;
#pragma unroll
        for (int a = 0; a < QB; ++a)
          if (a < q) m = fmax(m, li[a]);
        if (!BWD) {
          usum += m;
        } else {
          // torch: amax splits the cotangent evenly among all maximal entries
          // (ties at 0 included); clamp_min(0) passes it where obj - bf >= 0
          int cnt = 0;
#pragma unroll
          for (int a = 0; a < QB; ++a) cnt += (a < q && li[a] == m);
          const double share = cnt ? g / (double)cnt : 0.0;
#pragma unroll
          for (int a = 0; a < QB; ++a) {
            if (a < q) {
              const bool win = li[a] == m;
              const double zi = gsm[a * (kk + 1)];
              const double relu = fmax(zi, 0.0);
              // w from relu * w is not recoverable at relu = 0: take it again
              double w;
              if (EXT) {
                w = wext[wrow + a];
              } else {
                double l = 0.0;
#pragma unroll
                for (int i = 0; i < KMAX; ++i) {
                  if (i < kk) {
                    const double x = gsm[a * (kk + 1) + 1 + i];
                    l += tb.fat ? log_fatmoid_d(x, nullptr) : logexpit_d(x, nullptr);
                  }
                }
                w = exp(l);
              }
              gsm[a * (kk + 1)] = (win && zi >= 0.0) ? share * w : 0.0;
              const double gw = win ? share * relu : 0.0;  // cotangent of w
              if (EXT) {
                dfeas[wrow + a] = gw;
              } else {
                const double gl = gw * w;  // w = exp(l)
#pragma unroll
                for (int i = 0; i < KMAX; ++i) {
                  if (i < kk) {
                    double dx;
                    const double x = gsm[a * (kk + 1) + 1 + i];
                    if (tb.fat) (void)log_fatmoid_d(x, &dx);
                    else (void)logexpit_d(x, &dx);
                    gsm[a * (kk + 1) + 1 + i] = -gl * dx / tie[i];
                  }
                }
              }
            }
          }
        }
      }
    }
    if (BWD) {
      __syncthreads();
      // Phase 2: fixed entries per thread, the chunk's samples in order.
#pragma unroll
      for (int r = 0; r < EPT; ++r) {
        const int e = tid + r * THREADS;
        if (e < Mt * q * q) {
          const int t = e / (q * q), a = (e / q) % q, j = e % q;
          if (j <= a) {
            const double ct = tc[t];
            double dl = dl_acc[r], dm = dm_acc[r];
            for (int s = 0; s < ns; ++s) {
              const double* gp = cv.gs + s * cv.GS + a * (kk + 1);
              double cot = gp[0] * ct;
              for (int i = 0; i < kk; ++i) cot = fma(gp[1 + i], tA[i * MTMAX + t], cot);
              dl = fma(cot, cv.Zs[s * cv.ZS + j * Mt + t], dl);
              dm += cot;
            }
            dl_acc[r] = dl;
            dm_acc[r] = dm;
          }
        }
      }
      if (dF) {
        for (int e = tid; e < ns * q * Mt; e += THREADS) {
          const int s = e / (q * Mt), a = (e / Mt) % q, t = e % Mt;
          const double* gp = cv.gs + s * cv.GS + a * (kk + 1);
          double cot = gp[0] * tc[t];
          for (int i = 0; i < kk; ++i) cot = fma(gp[1 + i], tA[i * MTMAX + t], cot);
          dF[t * sF + (int64_t)(s0 + s) * ldF + (int64_t)b * Qp + a] = cot;
        }
      }
    }
  }

  if (BWD) {
#pragma unroll
    for (int r = 0; r < EPT; ++r) {
      const int e = tid + r * THREADS;
      if (e < Mt * q * q) {
        const int t = e / (q * q), a = (e / q) % q, j = e % q;
        dL[((int64_t)t * B + b) * q * q + a * q + j] = (j <= a) ? dl_acc[r] : 0.0;
        if (j == 0) dmean[((int64_t)t * B + b) * q + a] = dm_acc[r];
      }
    }
    return;
  }
  // forward: the threads' partial results in a fixed tree
  __syncthreads();
  double* red = cv.red;
  if (LOG) {
    red[tid] = lse.m;
    red[THREADS + tid] = lse.s;
  } else {
    red[tid] = usum;
  }
  __syncthreads();
  for (int off = THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) {
      if (LOG) {
        const LseAcc r = lse_merge(LseAcc{red[tid], red[THREADS + tid]},
                                   LseAcc{red[tid + off], red[THREADS + tid + off]});
        red[tid] = r.m;
        red[THREADS + tid] = r.s;
      } else {
        red[tid] += red[tid + off];
      }
    }
    __syncthreads();
  }
  if (tid == 0) acq[b] = LOG ? red[0] + log(red[THREADS]) - log((double)S) : red[0] / (double)S;
}

// Samples per LDS chunk: what the budget leaves after the members' roots,
// means, tables and the reduction scratch, over a sample's base-sample row and
// (backward) its 1 + k cotangents per point; at most one sample per lane.
int qmc_feas_chunk(int q, int Mt, int kk, int S, bool bwd) {
  const int fixed = Mt * q * q + Mt * q + TAB_DOUBLES + RED_DOUBLES;
  const int per = ((q * Mt) | 1) + (bwd ? ((q * (kk + 1)) | 1) : 0);
  return std::max(1, std::min(std::min(THREADS, S), (LDS_DOUBLES - fixed) / per));
}

int check_args(const BoQmcFeasArgs* a, const char* who, FeasTab* tb) {
  BO_CHECK_ARG(a->B >= 0 && a->S > 0, "%s: bad B / S", who);
  BO_CHECK_ARG(a->q >= 1 && a->q <= QMAX, "%s: 1 <= q <= %d (got %d)", who, QMAX, a->q);
  BO_CHECK_ARG(a->Mt >= 1 && a->Mt <= MTMAX, "%s: 1 <= Mt <= %d (got %d)", who, MTMAX, a->Mt);
  BO_CHECK_ARG(a->k >= 0 && a->k <= KMAX, "%s: 0 <= k <= %d (got %d)", who, KMAX, a->k);
  BO_CHECK_ARG(a->feas == nullptr || a->k == 0,
               "%s: the weight tensor and the constraint table exclude each other", who);
  BO_CHECK_ARG(a->mean && a->L && a->Z, "%s: mean, L and Z are required", who);
  BO_CHECK_ARG(a->F == nullptr || (a->Qp >= a->q && a->ldF >= (int64_t)a->B * a->Qp && a->sF >= 0),
               "%s: bad F layout", who);
  BO_CHECK_ARG(!a->log || (a->tau_relu > 0.0 && a->tau_max > 0.0), "%s: tau must be positive", who);
  tb->k = a->k;
  tb->fat = a->fat;
  for (int t = 0; t < MTMAX; ++t) tb->c[t] = t < a->Mt ? a->c[t] : 0.0;
  for (int i = 0; i < KMAX; ++i) {
    const bool on = i < a->k;
    BO_CHECK_ARG(!on || a->eta[i] > 0.0, "%s: eta[%d] must be positive", who, i);
    tb->rhs[i] = on ? a->rhs[i] : 0.0;
    tb->eta[i] = on ? a->eta[i] : 1.0;
    for (int t = 0; t < MTMAX; ++t) tb->A[i][t] = (on && t < a->Mt) ? a->A[i * MTMAX + t] : 0.0;
  }
  return BO_OK;
}

template <bool BWD>
int launch(const BoQmcFeasArgs* a, const FeasTab& tb, hipStream_t st) {
  const bool ext = a->feas != nullptr;
  const int kk = ext ? 0 : a->k;
  const int chunk = qmc_feas_chunk(a->q, a->Mt, kk, a->S, BWD);
  const int fixed = a->Mt * a->q * a->q + a->Mt * a->q + TAB_DOUBLES + RED_DOUBLES;
  const int per = ((a->q * a->Mt) | 1) + (BWD ? ((a->q * (kk + 1)) | 1) : 0);
  const size_t lds = sizeof(double) * (size_t)(fixed + chunk * per);
  const LogRedParams lp{a->tau_relu, a->tau_max, a->fat};
#define BO_SF(QQ, LG, EX)                                                                         \
  qmc_feas_kernel<QQ, LG, EX, BWD><<<(unsigned)a->B, THREADS, lds, st>>>(                         \
      a->B, a->q, a->Mt, a->S, a->mean, a->L, a->Z, a->F, a->ldF, a->sF, a->Qp, a->best_f,        \
      a->best_f_s, tb, a->feas, lp, chunk, a->acq, a->dacq, a->dmean, a->dL, a->dF, a->dfeas)
#define BO_SFQ(LG, EX)        \
  if (a->q <= 4) {            \
    BO_SF(4, LG, EX);         \
  } else if (a->q <= 8) {     \
    BO_SF(8, LG, EX);         \
  } else {                    \
    BO_SF(QMAX, LG, EX);      \
  }
  if (a->log) {
    if (ext) {
      BO_SFQ(true, true);
    } else {
      BO_SFQ(true, false);
    }
  } else {
    if (ext) {
      BO_SFQ(false, true);
    } else {
      BO_SFQ(false, false);
    }
  }
#undef BO_SFQ
#undef BO_SF
  BO_LAUNCH_CHECK();
  return BO_OK;
}

}  // namespace

// bo_qmc_feas_v / bo_qmc_feas_backward_v behind their header checks (abi_structs.cpp).
extern "C" int bo_qmc_feas_impl(const BoQmcFeasArgs* a, void* stream) {
  FeasTab tb;
  if (int st = check_args(a, "bo_qmc_feas", &tb); st != BO_OK) return st;
  BO_CHECK_ARG(a->acq != nullptr, "bo_qmc_feas: acq is required");
  if (a->B == 0) return BO_OK;
  return launch<false>(a, tb, as_stream(stream));
}

extern "C" int bo_qmc_feas_backward_impl(const BoQmcFeasArgs* a, void* stream) {
  FeasTab tb;
  if (int st = check_args(a, "bo_qmc_feas_backward", &tb); st != BO_OK) return st;
  BO_CHECK_ARG(a->dacq && a->dmean && a->dL, "bo_qmc_feas_backward: dacq, dmean and dL are required");
  BO_CHECK_ARG(!a->log || a->acq != nullptr, "bo_qmc_feas_backward: log mode reads the forward's acq");
  BO_CHECK_ARG((a->F == nullptr) == (a->dF == nullptr), "bo_qmc_feas_backward: F and dF go together");
  BO_CHECK_ARG((a->feas == nullptr) == (a->dfeas == nullptr),
               "bo_qmc_feas_backward: feas and dfeas go together");
  if (a->B == 0) return BO_OK;
  return launch<true>(a, tb, as_stream(stream));
}
