// qLogEHVI: Monte-Carlo log expected hypervolume improvement in log space.
//
// Reference: qLogExpectedHypervolumeImprovement._compute_log_qehvi
// (botorch/acquisition/multi_objective/logei.py:147-310).  For every sample s,
// cell k and objective t
//   li[p][t]  = log_fatplus(f[s][p][t] - l_kt; tau_relu)   (fat; else log_softplus)
//   loglen[t] = log(min(u_kt, 1e10) - l_kt)
// and for every non-empty subset T of the q points
//   a_T = sum_t smin2(smin_{p in T} li[p][t], loglen[t]) + sum_{p in T} logw[s][b][p]
// with smin = fatmin (fat) or smooth_amin at temperature tau_max
// (botorch/utils/safe_math.py:276-283, 355-378), anchored at the subset's own
// minimum as safe_math anchors it (a global anchor underflows at tau_max =
// 1e-3), and smin2 the same function of two values (fatminimum, :404-419).
// Then
//   odd = LSE_{|T| odd} a_T,  even = LSE_{|T| even} a_T,
//   cell = logdiffexp(even, odd)   (safe_math.py:108-121; no clamp when
//                                   even >= odd, as the reference),
//   hvi_s = LSE_k cell,  acq_b = LSE_s hvi_s - log S.
//
// Reordering.  The reference takes one logsumexp per subset size and folds
// the sizes into the odd / even totals with logplusexp (logei.py:203-267);
// here all subsets of one parity go through one online (max, sum) pair in
// mask order.  The two are the same sum in a different order, not term for
// term: permuting points and subsets moved the fp64 torch composition by
// <= 1e-14 on the log value and 5e-14 relative on the gradient.
//
// Unlike qehvi.hip no term is ever zero: all 2^q - 1 subsets of every
// (sample, cell) pair contribute, so the fused route stops at q = 8 (255
// subsets).  Only cells with a zero-length side are skipped, before any
// logarithm (the padding cells lo = hi = 0 of qNEHVI's per-sample
// decompositions; the reference's value and gradient ignore them too).
//
// Layout: one workgroup per t-batch (or per 1 / H of its samples when B leaves
// CUs idle); GROUP consecutive lanes share one sample and stride over its
// cells, their (max, sum) pairs merge in a fixed butterfly, the group leaders'
// sample pairs merge in order.  The sample split writes pairs, not sums;
// qlogehvi_part_reduce_kernel finishes the logmeanexp.  The forward also
// writes hvi_s (S x B) for the backward.
//
// Samples as qehvi.hip's weighted variant: the model list has Mt >= M members,
// objective t is member oi(t), f = mean + L z (+ F).
#include "common.h"
#include "logred.h"

#include <algorithm>

namespace {

constexpr int NT = 256;      // threads per workgroup, forward and backward
constexpr int GROUP = 16;    // lanes per sample
constexpr int SPP = NT / GROUP;  // samples per pass
constexpr int QLMAX = 8;
constexpr int MMAX = 4;
constexpr int LDS_CELL_DOUBLES = 2048;  // K * M <= 1024 staged in LDS

struct QlogParams {
  int B, q, S, K, H, Qp, zm, zld;
  unsigned oi;  // member of objective t in bits [8 t, 8 t + 8)
  int64_t cstride, ldF, sF;
  const double *mean, *L, *Z, *lo, *hi, *F, *logw;
  double *acq, *hvi, *part;                 // forward outputs
  const double *dacq, *acq_in, *hvi_in;     // backward inputs
  double *dmean, *dL, *dF, *dlogw;          // backward outputs
  LogRedParams lp;
};

__device__ __forceinline__ int member_of(const QlogParams& a, int t) {
  return (int)((a.oi >> (8 * t)) & 0xffu);
}

// lse_push that leaves the pair alone on -inf (an empty parity, a skipped cell)
__device__ __forceinline__ LseAcc lse_add(LseAcc a, double v) {
  if (v == -INFINITY) return a;
  return lse_push(a, v);
}
__device__ __forceinline__ double lse_value(LseAcc a) {
  return a.m == -INFINITY ? -INFINITY : a.m + log(a.s);
}

// log(1 - e^x), x < 0 (safe_math.py:72-82)
__device__ __forceinline__ double log1mexp_d(double x) {
  return x > -0.6931471805599453 ? log(-expm1(x)) : log1p(-exp(x));
}

// _pareto(z, alpha = 2) = 2 / (2 + 2 z + z^2) and its derivative -p^2 (1 + z)
__device__ __forceinline__ double pareto2(double z) { return 2.0 / (2.0 + 2.0 * z + z * z); }

// Smooth minimum over the subset's points of li[.][t]; GRAD: g[p] = d / d li[p][t]
// (torch autograd through -fatmax(-x): the anchor's share 1 + sum p' / P goes to
// the minimal entries, split evenly among ties).
template <int M, int QB, bool GRAD>
__device__ __forceinline__ double subset_min(const double (&li)[QB][M], int t, unsigned sub,
                                             const LogRedParams& lp, double inv_tau,
                                             double (&g)[QB]) {
  double mn = INFINITY;
#pragma unroll
  for (int p = 0; p < QB; ++p)
    if (sub & (1u << p)) mn = fmin(mn, li[p][t]);
  if (lp.fat) {
    double P = 0.0, dP = 0.0;
    int cnt = 0;
#pragma unroll
    for (int p = 0; p < QB; ++p)
      if (sub & (1u << p)) {
        const double z = (li[p][t] - mn) * inv_tau;
        const double pz = pareto2(z);
        P += pz;
        if constexpr (GRAD) {
          const double d = -pz * pz * (1.0 + z);
          dP += d;
          g[p] = -d;
          cnt += (li[p][t] == mn);
        }
      }
    if constexpr (GRAD) {
      const double anchor = (1.0 + dP / P) / (double)cnt;
#pragma unroll
      for (int p = 0; p < QB; ++p)
        if (sub & (1u << p)) g[p] = g[p] / P + ((li[p][t] == mn) ? anchor : 0.0);
    }
    return mn - lp.tau_max * log(P);
  }
  double ssum = 0.0;
#pragma unroll
  for (int p = 0; p < QB; ++p)
    if (sub & (1u << p)) {
      const double e = exp((mn - li[p][t]) * inv_tau);
      ssum += e;
      if constexpr (GRAD) g[p] = e;
    }
  if constexpr (GRAD) {
#pragma unroll
    for (int p = 0; p < QB; ++p)
      if (sub & (1u << p)) g[p] /= ssum;
  }
  return mn - lp.tau_max * log(ssum);
}

// The same smooth minimum of (v, ll); w (GRAD) = d / d v.
template <bool GRAD>
__device__ __forceinline__ double smooth_min2(double v, double ll, const LogRedParams& lp,
                                              double inv_tau, double* w) {
  const double mn = fmin(v, ll);
  if (lp.fat) {
    const double z0 = (v - mn) * inv_tau, z1 = (ll - mn) * inv_tau;
    const double p0 = pareto2(z0), p1 = pareto2(z1);
    const double P = p0 + p1;
    if constexpr (GRAD) {
      const double d0 = -p0 * p0 * (1.0 + z0), d1 = -p1 * p1 * (1.0 + z1);
      const int cnt = (v == mn) + (ll == mn);
      *w = -d0 / P + ((v == mn) ? (1.0 + (d0 + d1) / P) / (double)cnt : 0.0);
    }
    return mn - lp.tau_max * log(P);
  }
  const double e0 = exp((mn - v) * inv_tau), e1 = exp((mn - ll) * inv_tau);
  if constexpr (GRAD) *w = e0 / (e0 + e1);
  return mn - lp.tau_max * log(e0 + e1);
}

// The cell's lower corner and log side lengths; false for an empty cell
// (a zero-length side: skipped before any logarithm).
template <int M, bool CELLS_LDS>
__device__ __forceinline__ bool load_cell(const QlogParams& a, const double* cells, int s, int k,
                                          double (&l)[M], double (&ll)[M]) {
  const int64_t co = (int64_t)s * a.cstride + (int64_t)k * M;
  bool ok = true;
  double len[M];
#pragma unroll
  for (int t = 0; t < M; ++t) {
    l[t] = CELLS_LDS ? cells[k * M + t] : a.lo[co + t];
    const double u = CELLS_LDS ? cells[LDS_CELL_DOUBLES / 2 + k * M + t] : a.hi[co + t];
    len[t] = fmin(u, 1e10) - l[t];
    ok = ok && (len[t] > 0.0);
  }
  if (!ok) return false;
#pragma unroll
  for (int t = 0; t < M; ++t) ll[t] = log(len[t]);
  return true;
}

// f[s][p][t] of the pass's samples into LDS (row stride QB * M), base samples
// from global memory
template <int M, int QB>
__device__ __forceinline__ void stage_samples(const QlogParams& a, int b, int s0, int ns, double* f,
                                              double* w) {
  const int q = a.q;
  for (int e = threadIdx.x; e < ns * q * M; e += NT) {
    const int s = e / (q * M), p = (e / M) % q, t = e % M;
    const int mt = member_of(a, t);
    const double* Lt = a.L + (((int64_t)mt * a.B + b) * q + p) * q;
    const double* zs = a.Z + (int64_t)(s0 + s) * a.zld + mt;
    double v = a.mean[((int64_t)mt * a.B + b) * q + p];
    if (a.F) v += a.F[mt * a.sF + (int64_t)(s0 + s) * a.ldF + (int64_t)b * a.Qp + p];
    for (int j = 0; j <= p; ++j) v = fma(Lt[j], zs[j * a.zm], v);
    f[s * QB * M + p * M + t] = v;
  }
  if (a.logw) {
    for (int e = threadIdx.x; e < ns * q; e += NT)
      w[(e / q) * QB + e % q] = a.logw[((int64_t)(s0 + e / q) * a.B + b) * q + e % q];
  }
}

template <int M, int QB, bool CELLS_LDS>
__global__ __launch_bounds__(NT) void qlogehvi_kernel(QlogParams a) {
  __shared__ double f[SPP * QB * M];
  __shared__ double w[SPP * QB];
  __shared__ double cells[CELLS_LDS ? LDS_CELL_DOUBLES : 1];
  __shared__ LseAcc red[SPP];
  const int H = a.H, q = a.q, K = a.K;
  const int b = blockIdx.x / H;
  const int h = blockIdx.x - b * H;
  const int sbeg = (int)((int64_t)a.S * h / H), send = (int)((int64_t)a.S * (h + 1) / H);
  const int tid = threadIdx.x;
  const int sl = tid / GROUP, gl = tid % GROUP;
  const double inv_tau = 1.0 / a.lp.tau_max;
  const unsigned full = (1u << q) - 1u;
  if constexpr (CELLS_LDS) {
    for (int e = tid; e < K * M; e += NT) {
      cells[e] = a.lo[e];
      cells[LDS_CELL_DOUBLES / 2 + e] = a.hi[e];
    }
  }
  LseAcc tot{-INFINITY, 0.0};  // the group leader's samples
  for (int s0 = sbeg; s0 < send; s0 += SPP) {
    const int ns = min(SPP, send - s0);
    __syncthreads();
    stage_samples<M, QB>(a, b, s0, ns, f, w);
    __syncthreads();
    LseAcc hv{-INFINITY, 0.0};
    if (sl < ns) {
      const double* fs = f + sl * QB * M;
      const double* ws = w + sl * QB;
      for (int k = gl; k < K; k += GROUP) {
        double l[M], ll[M];
        if (!load_cell<M, CELLS_LDS>(a, cells, s0 + sl, k, l, ll)) continue;
        double li[QB][M];
#pragma unroll
        for (int p = 0; p < QB; ++p)
#pragma unroll
          for (int t = 0; t < M; ++t)
            li[p][t] = p < q ? log_soft_relu(fs[p * M + t] - l[t], a.lp, nullptr) : 0.0;
        LseAcc par[2] = {{-INFINITY, 0.0}, {-INFINITY, 0.0}};  // even, odd
        for (unsigned sub = 1; sub <= full; ++sub) {
          double at = 0.0;
          double g[QB];
#pragma unroll
          for (int t = 0; t < M; ++t) {
            const double v = subset_min<M, QB, false>(li, t, sub, a.lp, inv_tau, g);
            at += smooth_min2<false>(v, ll[t], a.lp, inv_tau, nullptr);
          }
          if (a.logw) {
#pragma unroll
            for (int p = 0; p < QB; ++p)
              if (sub & (1u << p)) at += ws[p];
          }
          if (__popc(sub) & 1) par[1] = lse_add(par[1], at);
          else par[0] = lse_add(par[0], at);
        }
        const double odd = lse_value(par[1]), even = lse_value(par[0]);
        // logdiffexp(even, odd): odd is finite or -inf with even
        const double cell = odd == -INFINITY ? -INFINITY : odd + log1mexp_d(even - odd);
        hv = lse_add(hv, cell);
      }
    }
#pragma unroll
    for (int o = GROUP / 2; o > 0; o >>= 1) {
      const LseAcc other{__shfl_xor(hv.m, o, GROUP), __shfl_xor(hv.s, o, GROUP)};
      hv = lse_merge(hv, other);
    }
    if (gl == 0 && sl < ns) {
      const double v = lse_value(hv);
      a.hvi[(int64_t)(s0 + sl) * a.B + b] = v;
      tot = lse_add(tot, v);
    }
  }
  if (gl == 0) red[sl] = tot;
  __syncthreads();
  if (tid == 0) {
    LseAcc t = red[0];
    for (int i = 1; i < SPP; ++i) t = lse_merge(t, red[i]);
    if (H == 1) {
      a.acq[b] = lse_value(t) - log((double)a.S);
    } else {
      a.part[2 * (int64_t)blockIdx.x] = t.m;
      a.part[2 * (int64_t)blockIdx.x + 1] = t.s;
    }
  }
}

// The H sample-split pairs of a t-batch merged in order, then the logmeanexp.
__global__ __launch_bounds__(64) void qlogehvi_part_reduce_kernel(const double* __restrict__ part,
                                                                  int B, int H, int S,
                                                                  double* __restrict__ acq) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  LseAcc t{-INFINITY, 0.0};
  for (int h = 0; h < H; ++h) {
    const int64_t i = 2 * ((int64_t)b * H + h);
    t = lse_merge(t, LseAcc{part[i], part[i + 1]});
  }
  acq[b] = lse_value(t) - log((double)S);
}

// (t, p, j) of entry ent: j <= p -> dL[p][j], j == p + 1 -> dmean[p] (as qehvi.hip)
__device__ __forceinline__ void entry_of(int ent, int q, int* t, int* p, int* j) {
  const int per_t = q * (q + 3) / 2;
  *t = ent / per_t;
  int r = ent % per_t, pp = 0;
  while (r >= pp + 2) {
    r -= pp + 2;
    ++pp;
  }
  *p = pp;
  *j = r;
}

// Backward.  d acq_b / d a_T = +- exp(a_T - cell) exp(cell - hvi_s) exp(hvi_s -
// acq_b - log S) (sign by the subset's parity; the middle pair is the
// logdiffexp and cell-sum Jacobian and collapses to exp(a_T - hvi_s), so no
// per-cell quantity is stored or formed twice).  It reaches li[p][t] through
// the smooth-minimum weights and f through the derivative of the smooth ReLU;
// dlogw[s][b][p] is its sum over the subsets containing p.  One GROUP of lanes
// per sample, cells in a fixed order, a fixed butterfly: no atomics.
// dmean_t[p] = sum_s df, dL_t[p][j] = sum_s df Z[s][j] (j <= p), as
// qehvi_backward_kernel; H > 1 writes the entries to part for
// qlogehvi_backward_reduce_kernel.
template <int M, int QB, bool CELLS_LDS>
__global__ __launch_bounds__(NT) void qlogehvi_backward_kernel(QlogParams a) {
  __shared__ double f[SPP * QB * M];
  __shared__ double df[SPP * QB * M];
  __shared__ double zc[SPP * QB * M];  // the pass's base samples, objective members' columns
  __shared__ double w[SPP * QB];
  __shared__ double cells[CELLS_LDS ? LDS_CELL_DOUBLES : 1];
  const int H = a.H, q = a.q, K = a.K, B = a.B;
  const int b = blockIdx.x / H;
  const int h = blockIdx.x - b * H;
  const int sbeg = (int)((int64_t)a.S * h / H), send = (int)((int64_t)a.S * (h + 1) / H);
  const int tid = threadIdx.x;
  const int sl = tid / GROUP, gl = tid % GROUP;
  const double inv_tau = 1.0 / a.lp.tau_max;
  const unsigned full = (1u << q) - 1u;
  const int nent = M * q * (q + 3) / 2;  // <= NT (host-checked)
  const double shift = a.acq_in[b] + log((double)a.S);
  const double gb = a.dacq[b];
  double acc = 0.0;
  int et = 0, ep = 0, ej = 0;
  if (tid < nent) entry_of(tid, q, &et, &ep, &ej);
  if constexpr (CELLS_LDS) {
    for (int e = tid; e < K * M; e += NT) {
      cells[e] = a.lo[e];
      cells[LDS_CELL_DOUBLES / 2 + e] = a.hi[e];
    }
  }
  for (int s0 = sbeg; s0 < send; s0 += SPP) {
    const int ns = min(SPP, send - s0);
    __syncthreads();
    stage_samples<M, QB>(a, b, s0, ns, f, w);
    for (int e = tid; e < ns * q * M; e += NT) {
      const int s = e / (q * M), r = e % (q * M);
      zc[s * QB * M + r] = a.Z[(int64_t)(s0 + s) * a.zld + (r / M) * a.zm + member_of(a, r % M)];
    }
    __syncthreads();
    double gacc[QB][M];
    double gw[QB];
#pragma unroll
    for (int p = 0; p < QB; ++p) {
      gw[p] = 0.0;
#pragma unroll
      for (int t = 0; t < M; ++t) gacc[p][t] = 0.0;
    }
    if (sl < ns) {
      const double* fs = f + sl * QB * M;
      const double* ws = w + sl * QB;
      const double hvs = a.hvi_in[(int64_t)(s0 + sl) * B + b];
      const double gs = exp(hvs - shift) * gb;
      for (int k = gl; k < K; k += GROUP) {
        double l[M], ll[M];
        if (!load_cell<M, CELLS_LDS>(a, cells, s0 + sl, k, l, ll)) continue;
        double li[QB][M], gli[QB][M];
#pragma unroll
        for (int p = 0; p < QB; ++p)
#pragma unroll
          for (int t = 0; t < M; ++t) {
            li[p][t] = p < q ? log_soft_relu(fs[p * M + t] - l[t], a.lp, nullptr) : 0.0;
            gli[p][t] = 0.0;
          }
        for (unsigned sub = 1; sub <= full; ++sub) {
          double at = 0.0;
          double g[M][QB];
#pragma unroll
          for (int t = 0; t < M; ++t) {
            double w2;
            const double v = subset_min<M, QB, true>(li, t, sub, a.lp, inv_tau, g[t]);
            at += smooth_min2<true>(v, ll[t], a.lp, inv_tau, &w2);
#pragma unroll
            for (int p = 0; p < QB; ++p)
              if (sub & (1u << p)) g[t][p] *= w2;
          }
          if (a.logw) {
#pragma unroll
            for (int p = 0; p < QB; ++p)
              if (sub & (1u << p)) at += ws[p];
          }
          double c = exp(at - hvs) * gs;
          if (!(__popc(sub) & 1)) c = -c;
#pragma unroll
          for (int p = 0; p < QB; ++p)
            if (sub & (1u << p)) {
              gw[p] += c;
#pragma unroll
              for (int t = 0; t < M; ++t) gli[p][t] = fma(c, g[t][p], gli[p][t]);
            }
        }
#pragma unroll
        for (int p = 0; p < QB; ++p)
#pragma unroll
          for (int t = 0; t < M; ++t)
            if (p < q) {
              double d;
              log_soft_relu(fs[p * M + t] - l[t], a.lp, &d);
              gacc[p][t] = fma(gli[p][t], d, gacc[p][t]);
            }
      }
    }
#pragma unroll
    for (int p = 0; p < QB; ++p) {
      if (p >= q) break;
#pragma unroll
      for (int t = 0; t < M; ++t) {
        double v = gacc[p][t];
#pragma unroll
        for (int o = GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GROUP);
        if (gl == 0 && sl < ns) df[sl * QB * M + p * M + t] = v;
      }
      if (a.dlogw) {
        double v = gw[p];
#pragma unroll
        for (int o = GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, GROUP);
        if (gl == 0 && sl < ns) a.dlogw[((int64_t)(s0 + sl) * B + b) * q + p] = v;
      }
    }
    __syncthreads();
    if (a.dF) {  // cotangent of the cached-root baseline term (rows b * Qp + p)
      for (int e = tid; e < ns * q * M; e += NT) {
        const int s = e / (q * M), p = (e / M) % q, t = e % M;
        a.dF[member_of(a, t) * a.sF + (int64_t)(s0 + s) * a.ldF + (int64_t)b * a.Qp + p] =
            df[s * QB * M + p * M + t];
      }
    }
    if (tid < nent) {
      double v = 0.0;
      for (int s = 0; s < ns; ++s) {
        const double d = df[s * QB * M + ep * M + et];
        v = fma(d, (ej <= ep) ? zc[s * QB * M + ej * M + et] : 1.0, v);
      }
      acc += v;
    }
  }
  if (H > 1) {
    if (tid < nent) a.part[(int64_t)blockIdx.x * nent + tid] = acc;
    return;
  }
  if (tid < nent) {
    const int mt = member_of(a, et);
    if (ej <= ep) a.dL[(((int64_t)mt * B + b) * q + ep) * q + ej] = acc;
    else a.dmean[((int64_t)mt * B + b) * q + ep] = acc;
  }
  for (int e = tid; e < M * q * q; e += NT) {  // strict upper triangle of dL
    const int t = e / (q * q), p = (e / q) % q, j = e % q;
    if (j > p) a.dL[(((int64_t)member_of(a, t) * B + b) * q + p) * q + j] = 0.0;
  }
}

// Sum of the H sample-split partials (in order), then the backward's layout.
__global__ __launch_bounds__(NT) void qlogehvi_backward_reduce_kernel(
    const double* __restrict__ part, int B, int q, int M, int H, unsigned oi,
    double* __restrict__ dmean, double* __restrict__ dL) {
  const int b = blockIdx.x;
  const int nent = M * q * (q + 3) / 2;
  for (int ent = threadIdx.x; ent < nent; ent += NT) {
    double v = 0.0;
    for (int h = 0; h < H; ++h) v += part[((int64_t)b * H + h) * nent + ent];
    int t, p, j;
    entry_of(ent, q, &t, &p, &j);
    const int mt = (int)((oi >> (8 * t)) & 0xffu);
    if (j <= p) dL[(((int64_t)mt * B + b) * q + p) * q + j] = v;
    else dmean[((int64_t)mt * B + b) * q + p] = v;
  }
  for (int e = threadIdx.x; e < M * q * q; e += NT) {
    const int t = e / (q * q), p = (e / q) % q, j = e % q;
    if (j > p) dL[(((int64_t)((oi >> (8 * t)) & 0xffu) * B + b) * q + p) * q + j] = 0.0;
  }
}

// The record's checks shared by the forward and the backward -> the kernels'
// parameters, or BO_ERR_ARG.
int params_of(const BoQlogehviArgs* a, const char* who, QlogParams* p) {
  BO_CHECK_ARG(a->q >= 1 && a->q <= QLMAX, "%s: 1 <= q <= %d (got %d)", who, QLMAX, a->q);
  BO_CHECK_ARG(a->m >= 2 && a->m <= MMAX, "%s: 2 <= m <= %d (got %d)", who, MMAX, a->m);
  BO_CHECK_ARG(a->B >= 0 && a->S > 0 && a->K >= 0 && a->cell_stride >= 0, "%s: bad B/S/K/cell_stride",
               who);
  BO_CHECK_ARG(a->cell_stride == 0 || a->cell_stride >= (int64_t)a->K * a->m,
               "%s: per-sample cells need cell_stride >= K m", who);
  BO_CHECK_ARG(a->mean && a->L && a->Z && (a->K == 0 || (a->cell_lo && a->cell_hi)),
               "%s: mean, L, Z and the cells are required", who);
  BO_CHECK_ARG(a->F == nullptr || (a->Qp >= a->q && a->ldF >= (int64_t)a->B * a->Qp),
               "%s: bad F layout", who);
  BO_CHECK_ARG(a->Mt >= a->m && a->Mt <= 255, "%s: m <= Mt <= 255 (got %d)", who, a->Mt);
  BO_CHECK_ARG(a->zm >= a->Mt && a->zld >= (int64_t)a->q * a->zm && a->zld <= INT32_MAX,
               "%s: base samples need zm >= Mt and q zm <= zld < 2^31", who);
  BO_CHECK_ARG(a->tau_relu > 0.0 && a->tau_max > 0.0, "%s: temperatures must be positive", who);
  BO_CHECK_ARG(a->hvi != nullptr && a->acq != nullptr, "%s: acq and hvi are required", who);
  unsigned oi = 0;
  for (int t = 0; t < a->m; ++t) {
    BO_CHECK_ARG(a->out_idx[t] >= 0 && a->out_idx[t] < a->Mt, "%s: out_idx[%d] = %d outside [0, %d)",
                 who, t, a->out_idx[t], a->Mt);
    for (int u = 0; u < t; ++u)
      BO_CHECK_ARG(a->out_idx[u] != a->out_idx[t], "%s: out_idx must be injective", who);
    oi |= (unsigned)a->out_idx[t] << (8 * t);
  }
  *p = QlogParams{};
  p->B = a->B, p->q = a->q, p->S = a->S, p->K = a->K, p->H = 1, p->Qp = a->Qp;
  p->zm = a->zm, p->zld = (int)a->zld, p->oi = oi;
  p->cstride = a->cell_stride, p->ldF = a->ldF, p->sF = a->sF;
  p->mean = a->mean, p->L = a->L, p->Z = a->Z, p->lo = a->cell_lo, p->hi = a->cell_hi;
  p->F = a->F, p->logw = a->logw;
  p->lp = LogRedParams{a->tau_relu, a->tau_max, a->fat ? 1 : 0};
  return BO_OK;
}

}  // namespace

#define BO_QL_DISPATCH(KERNEL, GRID)                                                     \
  do {                                                                                   \
    const bool cl_ = a->cell_stride == 0 && (int64_t)a->K * a->m <= LDS_CELL_DOUBLES / 2; \
    const int qb_ = a->q <= 4 ? 4 : 8;                                                   \
    if (a->m == 2 && qb_ == 4 && cl_) KERNEL<2, 4, true><<<GRID, NT, 0, st>>>(p);        \
    else if (a->m == 2 && qb_ == 4) KERNEL<2, 4, false><<<GRID, NT, 0, st>>>(p);         \
    else if (a->m == 2 && cl_) KERNEL<2, 8, true><<<GRID, NT, 0, st>>>(p);               \
    else if (a->m == 2) KERNEL<2, 8, false><<<GRID, NT, 0, st>>>(p);                     \
    else if (a->m == 3 && qb_ == 4 && cl_) KERNEL<3, 4, true><<<GRID, NT, 0, st>>>(p);   \
    else if (a->m == 3 && qb_ == 4) KERNEL<3, 4, false><<<GRID, NT, 0, st>>>(p);         \
    else if (a->m == 3 && cl_) KERNEL<3, 8, true><<<GRID, NT, 0, st>>>(p);               \
    else if (a->m == 3) KERNEL<3, 8, false><<<GRID, NT, 0, st>>>(p);                     \
    else if (qb_ == 4 && cl_) KERNEL<4, 4, true><<<GRID, NT, 0, st>>>(p);                \
    else if (qb_ == 4) KERNEL<4, 4, false><<<GRID, NT, 0, st>>>(p);                      \
    else if (cl_) KERNEL<4, 8, true><<<GRID, NT, 0, st>>>(p);                            \
    else KERNEL<4, 8, false><<<GRID, NT, 0, st>>>(p);                                    \
  } while (0)

// bo_qlogehvi_v / bo_qlogehvi_backward_v behind their header checks
// (abi_structs.cpp).  work (optional): the samples of each t-batch split over
// H = min(8, 1024 / B (forward) | 256 / B (backward)) workgroups when B leaves
// CUs idle -- forward >= 4 B doubles (a pair per workgroup), backward
// >= 2 B m q (q + 3) / 2.
extern "C" int bo_qlogehvi_impl(const BoQlogehviArgs* a, void* stream) {
  QlogParams p;
  if (int rc = params_of(a, "bo_qlogehvi", &p); rc != BO_OK) return rc;
  if (a->B == 0) return BO_OK;
  hipStream_t st = as_stream(stream);
  const int B = a->B;
  int H = 1;
  if (a->work != nullptr && a->work_elems >= 4 * (int64_t)B) {
    H = (int)std::min<int64_t>(std::min(8, std::max(1, 1024 / B)), a->work_elems / (2 * (int64_t)B));
    H = std::max(1, std::min(H, a->S));
  }
  p.H = H;
  p.acq = a->acq, p.hvi = a->hvi, p.part = a->work;
  const unsigned grid = (unsigned)((int64_t)B * H);
  BO_QL_DISPATCH(qlogehvi_kernel, grid);
  BO_LAUNCH_CHECK();
  if (H > 1) {
    qlogehvi_part_reduce_kernel<<<(unsigned)ceil_div(B, 64), 64, 0, st>>>(a->work, B, H, a->S,
                                                                         a->acq);
    BO_LAUNCH_CHECK();
  }
  return BO_OK;
}

extern "C" int bo_qlogehvi_backward_impl(const BoQlogehviArgs* a, void* stream) {
  QlogParams p;
  if (int rc = params_of(a, "bo_qlogehvi_backward", &p); rc != BO_OK) return rc;
  BO_CHECK_ARG(a->dacq != nullptr && a->dmean != nullptr && a->dL != nullptr,
               "bo_qlogehvi_backward: dacq, dmean and dL are required");
  BO_CHECK_ARG((a->F == nullptr) == (a->dF == nullptr), "bo_qlogehvi_backward: F and dF go together");
  BO_CHECK_ARG((a->logw == nullptr) == (a->dlogw == nullptr),
               "bo_qlogehvi_backward: logw and dlogw go together");
  if (a->B == 0) return BO_OK;
  hipStream_t st = as_stream(stream);
  const int B = a->B;
  const int64_t nent = (int64_t)a->m * a->q * (a->q + 3) / 2;  // <= 4 * 8 * 11 / 2 = 176 <= NT
  int H = 1;
  if (a->work != nullptr && a->work_elems >= 2 * (int64_t)B * nent) {
    H = (int)std::min<int64_t>(std::min(8, std::max(1, 256 / B)), a->work_elems / ((int64_t)B * nent));
    H = std::max(1, std::min(H, a->S));
  }
  p.H = H;
  p.dacq = a->dacq, p.acq_in = a->acq, p.hvi_in = a->hvi, p.part = a->work;
  p.dmean = a->dmean, p.dL = a->dL, p.dF = a->dF, p.dlogw = a->dlogw;
  const unsigned grid = (unsigned)((int64_t)B * H);
  BO_QL_DISPATCH(qlogehvi_backward_kernel, grid);
  BO_LAUNCH_CHECK();
  if (H > 1) {
    qlogehvi_backward_reduce_kernel<<<(unsigned)B, NT, 0, st>>>(a->work, B, a->q, a->m, H, p.oi,
                                                                a->dmean, a->dL);
    BO_LAUNCH_CHECK();
  }
  return BO_OK;
}
#undef BO_QL_DISPATCH
