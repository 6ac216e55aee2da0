// Augmented Chebyshev scalarization (ParEGO) of a model list's members under the
// qEI / qLogEI / qNEI / qLogNEI reductions, with outcome constraints
// (botorch/utils/multi_objective/scalarization.py, acquisition/multi_objective/
// parego.py, logei.py:219-234, utils/objective.py:134-180).
//
//   f[t]  = mean[t][b][a] + sum_{j<=a} L[t][b][a][j] Z[s][j Mt + t] (+ F[t][s][b Qp + a])
//   p[t]  = ca[t] f[t] + cb[t]                       t in the objective set O
//   obj   = -(max_{t in O} p[t] + alpha sum_{t in O} p[t])
//   con_i = sum_t A[i][t] f[t] - rhs_i,   l = sum_i logsig(-con_i / eta_i)  (or the caller's tensor)
//   plain: u_s = max_a relu(obj_a - bf_s) exp(l_a),               acq_b = mean_s u_s
//   log:   u_s = q_reduce_a(log_soft_relu(obj_a - bf_s) + l_a),   acq_b = logmeanexp_s u_s
//
// Work split: grid B x G.  Workgroup (b, g) takes the samples [g Sg, (g + 1) Sg) of
// t-batch b (Sg a multiple of 16) and writes its partial result to a workspace; a second
// small kernel folds the G partials of a t-batch in index order.  No atomics; the result
// is a function of (G, chunk) and of nothing else.
//
// Samples on the fp64 matrix cores: a wave takes 16 samples at a time.  Per member t,
// D_t (16 points x 16 samples) = L_t (16 x q, zero above the diagonal and beyond q, in LDS
// for the whole kernel) x Z_t^T (q x 16 samples, from the staged chunk), in ceil(q / 4)
// k-steps of v_mfma_f64_16x16x4_f64 with the accumulator started at mean (+ F).  In the D
// fragment map a lane holds the points (l >> 4) + 4 r, r < 4, of sample l & 15, so the max
// / sum over members, the constraints and the soft-ReLU are elementwise in registers and
// the reduction over points is in-lane plus two cross-lane steps (xor 16, xor 32).
// No f, and no S x q x Mt tensor, reaches LDS or memory.
//
// Backward: the same pass leaves, per (sample, point) in registers, the cotangent of obj,
// the index t* of the max and the cotangent of l, hence
//   G_t = -gobj ca[t] ([t = t*] + alpha) [t in O] + sum_i gcon_i A[i][t]
// in the D fragment map.  dL_t = tril(G_t^T Z_t) summed over samples runs on the matrix
// cores with k over samples: G_t goes through a per-wave LDS tile into the A fragment map,
// the chunk's Z rows are the B operand.  dmean_t[a] = sum_s G_t[s][a] accumulates in-lane
// and is reduced once at the end; dF = G_t is written from the fragment.
#include "common.h"

#include <algorithm>

#include "logred.h"

namespace {

constexpr int QMAX = 16;
constexpr int MTMAX = 8;
constexpr int KMAX = 8;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / BO_WAVE;
constexpr int TILE = 16;            // samples of one MFMA tile
constexpr int LROW = QMAX + 1;      // row stride of a 16 x 16 tile in LDS
constexpr int LTILE = QMAX * LROW;
constexpr int LDS_DOUBLES = 8000;   // 62.5 KiB: two workgroups per CU
constexpr int RED_DOUBLES = 2 * THREADS;

// The scalarization and the in-kernel (linear) constraints, by value.
struct ChebTab {
  double ca[MTMAX];
  double cb[MTMAX];
  double A[KMAX][MTMAX];
  double rhs[KMAX];
  double eta[KMAX];
  double alpha;
  int omask;
  int k;
  int fat;
};

// utils/safe_math.py:84-99 (as qmc_feas.hip)
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

// utils/safe_math.py:422-451 (as qmc_feas.hip)
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

// v over the four lanes that hold one sample's points (l, l ^ 16, l ^ 32, l ^ 48)
__device__ __forceinline__ double quad_sum(double v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}
__device__ __forceinline__ double quad_max(double v) {
  v = fmax(v, __shfl_xor(v, 16));
  return fmax(v, __shfl_xor(v, 32));
}

// log_q_reduce of logred.h with the q entries spread over a lane quad: li[r] is the entry
// of point (l >> 4) + 4 r where on[r].  g receives d u / d li.
__device__ __forceinline__ double quad_log_q_reduce(const double (&li)[4], const bool (&on)[4],
                                                    const LogRedParams& p, double (*g)[4]) {
  const double tau = p.tau_max;
  double M = -INFINITY;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (on[r]) M = fmax(M, li[r]);
  M = quad_max(M);
  if (p.fat) {
    double P = 0.0, dP = 0.0, cnt = 0.0, pd[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pd[r] = 0.0;
      if (on[r]) {
        const double x = (M - li[r]) / tau;
        const double den = 2.0 + 2.0 * x + x * x;
        P += 2.0 / den;
        pd[r] = -2.0 * (2.0 + 2.0 * x) / (den * den);
        dP += pd[r];
        cnt += (li[r] == M) ? 1.0 : 0.0;
      }
    }
    P = quad_sum(P);
    dP = quad_sum(dP);
    cnt = quad_sum(cnt);
    if (g) {
      const double anchor = (1.0 + dP / P) / cnt;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        (*g)[r] = on[r] ? -pd[r] / P + ((li[r] == M) ? anchor : 0.0) : 0.0;
    }
    return M + tau * log(P);
  }
  const double Ms = M / tau;
  double e[4], ssum = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    e[r] = on[r] ? exp(li[r] / tau - Ms) : 0.0;
    ssum += e[r];
  }
  ssum = quad_sum(ssum);
  if (g) {
#pragma unroll
    for (int r = 0; r < 4; ++r) (*g)[r] = e[r] / ssum;
  }
  return tau * (Ms + log(ssum));
}

struct Carve {
  double *Ls, *mu, *tw, *red, *Zs;
  int ZS;
};

__device__ __forceinline__ Carve carve(double* sm, int q, int Mt) {
  Carve c;
  c.Ls = sm;                          // Mt tiles, [a][j], zero above the diagonal and beyond q
  c.mu = c.Ls + Mt * LTILE;           // Mt x 16, zero beyond q
  c.tw = c.mu + Mt * QMAX;            // a transposition tile per wave; the epilogue's scratch
  c.red = c.tw + WAVES * LTILE;
  c.Zs = c.red + RED_DOUBLES;
  c.ZS = (q * Mt) | 1;
  return c;
}

int fixed_doubles(int Mt) { return Mt * LTILE + Mt * QMAX + WAVES * LTILE + RED_DOUBLES; }

// LOG: the LogEI reductions.  EXT: the weights (plain) / log-weights (LOG) come from wext
// (S x B x q) and the backward returns their cotangent dfeas.  BWD: the backward (acq is
// then the forward's value, read in LOG mode).  work: per (b, g), forward 2 doubles (plain:
// the sum; LOG: max, scaled sum), backward Mt (q q + q) doubles (dL, then dmean).
template <bool LOG, bool EXT, bool BWD>
__global__ __launch_bounds__(THREADS) void cheb_kernel(
    int B, int q, int Mt, int S, int G, int Sg, const double* __restrict__ mean,
    const double* __restrict__ Lg, const double* __restrict__ Z, const double* __restrict__ F,
    int64_t ldF, int64_t sF, int Qp, double best_f, const double* __restrict__ best_f_s, ChebTab tb,
    const double* __restrict__ wext, LogRedParams lp, int chunk, const double* __restrict__ acq,
    const double* __restrict__ dacq, double* __restrict__ work, double* __restrict__ dF,
    double* __restrict__ dfeas) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const Carve cv = carve(smem, q, Mt);
  const int kk = EXT ? 0 : tb.k;
  const int b = blockIdx.x, grp = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, rg = lane >> 4;  // fragment column; first row of the lane
  const int zw = q * Mt;
  const int nks = (q + 3) >> 2;               // k-steps up to the diagonal block of the last row group

  for (int e = tid; e < Mt * LTILE; e += THREADS) {
    const int t = e / LTILE, a = (e % LTILE) / LROW, j = e % LROW;
    cv.Ls[e] = (a < q && j <= a) ? Lg[((int64_t)t * B + b) * q * q + a * q + j] : 0.0;
  }
  for (int e = tid; e < Mt * QMAX; e += THREADS) {
    const int t = e / QMAX, a = e % QMAX;
    cv.mu[e] = a < q ? mean[((int64_t)t * B + b) * q + a] : 0.0;
  }

  double g = 0.0, a_fwd = 0.0;
  if (BWD) {
    g = dacq[b] / (double)S;
    if (LOG) a_fwd = acq[b];
  }
  double usum = 0.0;            // forward, plain: this lane's samples in order
  LseAcc lse{-INFINITY, 0.0};   // forward, log
  v4d dl_acc[MTMAX], dm_acc[MTMAX];
#pragma unroll
  for (int t = 0; t < MTMAX; ++t) dl_acc[t] = dm_acc[t] = v4d_zero();
  double* const tw = cv.tw + wave * LTILE;

  const int s_lo = min(S, grp * Sg), s_hi = min(S, s_lo + Sg);
  for (int s0 = s_lo; s0 < s_hi; s0 += chunk) {
    const int ns = min(chunk, s_hi - s0);
    __syncthreads();  // the tables (first pass); the previous chunk's readers
    for (int e = tid; e < ns * zw; e += THREADS)
      cv.Zs[(e / zw) * cv.ZS + e % zw] = Z[(int64_t)s0 * zw + e];
    __syncthreads();
    const int ntiles = (ns + TILE - 1) / TILE;
    for (int tile = wave; tile < ntiles; tile += WAVES) {
      const int sl = tile * TILE + col;   // this lane's sample within the chunk
      const bool valid = sl < ns;
      const int s = s0 + sl;
      const double* zrow = cv.Zs + (valid ? sl : 0) * cv.ZS;
      // f_t of the lane's four points: the accumulator fragments
      v4d f[MTMAX];
#pragma unroll
      for (int t = 0; t < MTMAX; ++t) {
        f[t] = v4d_zero();
        if (t < Mt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = rg + 4 * r;
            double m = cv.mu[t * QMAX + a];
            if (F && valid && a < q) m += F[t * sF + (int64_t)s * ldF + (int64_t)b * Qp + a];
            f[t][r] = m;
          }
        }
      }
      for (int ks = 0; ks < nks; ++ks) {
        const int j = 4 * ks + rg;
        const bool zon = valid && j < q;
#pragma unroll
        for (int t = 0; t < MTMAX; ++t) {
          if (t < Mt) {
            const double av = cv.Ls[t * LTILE + col * LROW + j];   // A[i = point][k = j]
            const double bv = zon ? zrow[j * Mt + t] : 0.0;        // B[k = j][sample]
            f[t] = mfma_f64(av, bv, f[t]);
          }
        }
      }

      // elementwise over the fragments: the scalarization, the constraints, the soft-ReLU
      const double bf = best_f_s ? (valid ? best_f_s[s] : 0.0) : best_f;
      const int64_t wrow = ((int64_t)s * B + b) * q;
      double li[4], zi[4], wl[4];  // wl: l (or the caller's weight / log-weight)
      int ts[4];
      bool on[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int a = rg + 4 * r;
        on[r] = a < q;
        double mx = -INFINITY, sm = 0.0;
        int tsr = 0;
#pragma unroll
        for (int t = 0; t < MTMAX; ++t) {
          if (t < Mt && ((tb.omask >> t) & 1)) {
            const double p = fma(tb.ca[t], f[t][r], tb.cb[t]);
            if (p > mx) {  // ties keep the lowest t
              mx = p;
              tsr = t;
            }
            sm += p;
          }
        }
        ts[r] = tsr;
        zi[r] = -(mx + tb.alpha * sm) - bf;
        double l = 0.0;
        if (EXT) {
          l = (valid && on[r]) ? wext[wrow + a] : 0.0;
        } else {
#pragma unroll
          for (int i = 0; i < KMAX; ++i) {
            if (i < kk) {
              double con = 0.0;
#pragma unroll
              for (int t = 0; t < MTMAX; ++t)
                if (t < Mt) con = fma(tb.A[i][t], f[t][r], con);
              const double x = -(con - tb.rhs[i]) / tb.eta[i];
              l += tb.fat ? log_fatmoid_d(x, nullptr) : logexpit_d(x, nullptr);
            }
          }
        }
        wl[r] = l;
        if (LOG) {
          li[r] = log_soft_relu(zi[r], lp, nullptr) + l;
        } else {
          if (!EXT) wl[r] = exp(l);
          li[r] = on[r] ? fmax(zi[r], 0.0) * wl[r] : 0.0;
        }
      }

      double gz[4], gl[4];  // cotangents of obj and of l (EXT: of the caller's tensor)
      if (LOG) {
        double gq[4];
        const double u = quad_log_q_reduce(li, on, lp, BWD ? &gq : nullptr);
        if (!BWD) {
          if (valid && rg == 0) lse = lse_push(lse, u);
        } else {
          const double wsm = valid ? g * exp(u - a_fwd) : 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double dz;
            (void)log_soft_relu(zi[r], lp, &dz);
            gl[r] = on[r] ? wsm * gq[r] : 0.0;
            gz[r] = on[r] ? gl[r] * dz : 0.0;
          }
        }
      } else {
        double m = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmax(m, li[r]);
        m = quad_max(m);
        if (!BWD) {
          if (valid && rg == 0) usum += m;
        } else {
          // as qmc_feas.hip: amax shares the cotangent among all maximal entries,
          // clamp_min(0) passes it where obj - bf >= 0
          double cnt = 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) cnt += (on[r] && li[r] == m) ? 1.0 : 0.0;
          cnt = quad_sum(cnt);
          const double share = (valid && cnt > 0.0) ? g / cnt : 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool win = on[r] && li[r] == m;
            gz[r] = (win && zi[r] >= 0.0) ? share * wl[r] : 0.0;
            const double gw = win ? share * fmax(zi[r], 0.0) : 0.0;  // cotangent of w
            gl[r] = EXT ? gw : gw * wl[r];                             // w = exp(l)
          }
        }
      }

      if (BWD) {
        if (EXT) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (valid && on[r]) dfeas[wrow + rg + 4 * r] = gl[r];
        }
        // G_t in place of f_t
        v4d Gt[MTMAX];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double gc[KMAX];
          if (!EXT) {
#pragma unroll
            for (int i = 0; i < KMAX; ++i) {
              gc[i] = 0.0;
              if (i < kk) {
                double con = 0.0;
#pragma unroll
                for (int t = 0; t < MTMAX; ++t)
                  if (t < Mt) con = fma(tb.A[i][t], f[t][r], con);
                const double x = -(con - tb.rhs[i]) / tb.eta[i];
                double dx;
                if (tb.fat) (void)log_fatmoid_d(x, &dx);
                else (void)logexpit_d(x, &dx);
                gc[i] = -gl[r] * dx / tb.eta[i];
              }
            }
          }
#pragma unroll
          for (int t = 0; t < MTMAX; ++t) {
            double v = 0.0;
            if (t < Mt) {
              if ((tb.omask >> t) & 1)
                v = -gz[r] * tb.ca[t] * ((t == ts[r] ? 1.0 : 0.0) + tb.alpha);
              if (!EXT) {
#pragma unroll
                for (int i = 0; i < KMAX; ++i)
                  if (i < kk) v = fma(gc[i], tb.A[i][t], v);
              }
            }
            Gt[t][r] = v;
          }
        }
#pragma unroll
        for (int t = 0; t < MTMAX; ++t) {
          if (t < Mt) {
            dm_acc[t] += Gt[t];
            if (dF) {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (valid && on[r])
                  dF[t * sF + (int64_t)s * ldF + (int64_t)b * Qp + rg + 4 * r] = Gt[t][r];
            }
            // D fragment (point, sample) -> A fragment A[i = point][k = sample]
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 4; ++r) tw[col * LROW + rg + 4 * r] = Gt[t][r];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) {
              const int sk = tile * TILE + 4 * kq + rg;  // B[k = sample][j = col]
              const double av = tw[(4 * kq + rg) * LROW + col];
              const double bv = (sk < ns && col < q) ? cv.Zs[sk * cv.ZS + col * Mt + t] : 0.0;
              dl_acc[t] = mfma_f64(av, bv, dl_acc[t]);
            }
          }
        }
      }
    }
  }

  if (BWD) {
    // the waves' fragments, member by member, through the tiles: fixed order
    double* const part = work + ((int64_t)b * G + grp) * (Mt * (q * q + q));
#pragma unroll
    for (int t = 0; t < MTMAX; ++t) {
      if (t >= Mt) break;  // uniform; the fragments keep static indices
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) tw[(rg + 4 * r) * LROW + col] = dl_acc[t][r];
      __syncthreads();
      {
        const int a = tid >> 4, j = tid & 15;
        if (a < q && j < q) {
          double v = 0.0;
          for (int w = 0; w < WAVES; ++w) v += cv.tw[w * LTILE + a * LROW + j];
          part[t * q * q + a * q + j] = (j <= a) ? v : 0.0;
        }
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 4; ++r) tw[(rg + 4 * r) * LROW + col] = dm_acc[t][r];
      __syncthreads();
      if (tid < q) {
        double v = 0.0;
        for (int w = 0; w < WAVES; ++w)
          for (int c = 0; c < TILE; ++c) v += cv.tw[w * LTILE + tid * LROW + c];
        part[Mt * q * q + t * q + tid] = v;
      }
    }
    return;
  }
  // forward: the lanes' partial results in a fixed tree
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
  if (tid == 0) {
    double* const part = work + ((int64_t)b * G + grp) * 2;
    part[0] = red[0];
    part[1] = LOG ? red[THREADS] : 0.0;
  }
}

// acq_b from the G partials of t-batch b, in index order.
template <bool LOG>
__global__ void cheb_fold_fwd(int B, int G, int S, const double* __restrict__ work,
                              double* __restrict__ acq) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* part = work + (int64_t)b * G * 2;
  if (LOG) {
    LseAcc r{-INFINITY, 0.0};
    for (int gi = 0; gi < G; ++gi) r = lse_merge(r, LseAcc{part[2 * gi], part[2 * gi + 1]});
    acq[b] = r.m + log(r.s) - log((double)S);
  } else {
    double v = 0.0;
    for (int gi = 0; gi < G; ++gi) v += part[2 * gi];
    acq[b] = v / (double)S;
  }
}

// dL (Mt x B x q x q, upper zero) and dmean (Mt x B x q) from the G partials, in index order.
__global__ void cheb_fold_bwd(int B, int G, int q, int Mt, const double* __restrict__ work,
                              double* __restrict__ dmean, double* __restrict__ dL) {
  const int P = Mt * (q * q + q);
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)B * P) return;
  const int b = (int)(e / P), o = (int)(e % P);
  const double* part = work + (int64_t)b * G * P + o;
  double v = 0.0;
  for (int gi = 0; gi < G; ++gi) v += part[(int64_t)gi * P];
  if (o < Mt * q * q) {
    const int t = o / (q * q), r = o % (q * q);
    dL[((int64_t)t * B + b) * q * q + r] = v;
  } else {
    const int t = (o - Mt * q * q) / q, a = (o - Mt * q * q) % q;
    dmean[((int64_t)t * B + b) * q + a] = v;
  }
}

// Samples per LDS chunk: whole tiles of 16, what the budget leaves after the members'
// roots, means, the waves' tiles and the reduction scratch; no more than a group's samples.
int cheb_chunk(int q, int Mt, int Sg, int forced) {
  const int per = (q * Mt) | 1;
  int rows = (LDS_DOUBLES - fixed_doubles(Mt)) / per;
  rows = std::min(rows, (Sg + TILE - 1) / TILE * TILE);
  if (forced > 0) rows = std::min(rows, forced);
  return std::max(TILE, rows / TILE * TILE);
}

int check_args(const BoQmcChebArgs* a, const char* who, ChebTab* tb) {
  BO_CHECK_ARG(a->B >= 0 && a->S > 0, "%s: bad B / S", who);
  BO_CHECK_ARG(a->q >= 1 && a->q <= QMAX, "%s: 1 <= q <= %d (got %d)", who, QMAX, a->q);
  BO_CHECK_ARG(a->Mt >= 2 && a->Mt <= MTMAX, "%s: 2 <= Mt <= %d (got %d)", who, MTMAX, a->Mt);
  BO_CHECK_ARG(a->k >= 0 && a->k <= KMAX, "%s: 0 <= k <= %d (got %d)", who, KMAX, a->k);
  BO_CHECK_ARG(a->G >= 1 && (int64_t)(a->G - 1) * TILE < a->S,
               "%s: 1 <= G <= ceil(S / 16) (got G = %d, S = %d)", who, a->G, a->S);
  BO_CHECK_ARG(a->G <= 65535, "%s: G beyond the grid (got %d)", who, a->G);
  BO_CHECK_ARG(a->chunk >= 0 && a->chunk % TILE == 0, "%s: chunk must be a multiple of 16", who);
  const int no = __builtin_popcount((unsigned)a->omask);
  BO_CHECK_ARG(a->omask > 0 && a->omask < (1 << a->Mt) && no >= 2,
               "%s: the objective set needs 2 to Mt of the members (mask %d)", who, a->omask);
  BO_CHECK_ARG(a->feas == nullptr || a->k == 0,
               "%s: the weight tensor and the constraint table exclude each other", who);
  BO_CHECK_ARG(a->mean && a->L && a->Z, "%s: mean, L and Z are required", who);
  BO_CHECK_ARG(a->F == nullptr || (a->Qp >= a->q && a->ldF >= (int64_t)a->B * a->Qp && a->sF >= 0),
               "%s: bad F layout", who);
  BO_CHECK_ARG(!a->log || (a->tau_relu > 0.0 && a->tau_max > 0.0), "%s: tau must be positive", who);
  tb->k = a->k;
  tb->fat = a->fat;
  tb->alpha = a->alpha;
  tb->omask = a->omask;
  for (int t = 0; t < MTMAX; ++t) {
    const bool on = t < a->Mt && ((a->omask >> t) & 1);
    tb->ca[t] = on ? a->ca[t] : 0.0;
    tb->cb[t] = on ? a->cb[t] : 0.0;
  }
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
int launch(const BoQmcChebArgs* a, const ChebTab& tb, const char* who, hipStream_t st) {
  const bool ext = a->feas != nullptr;
  const int G = a->G;
  const int Sg = (int)(ceil_div(ceil_div(a->S, G), TILE) * TILE);
  BO_CHECK_ARG((int64_t)(G - 1) * Sg < a->S, "%s: G = %d leaves a group without samples (S = %d)",
               who, G, a->S);
  const int chunk = cheb_chunk(a->q, a->Mt, Sg, a->chunk);
  const size_t lds = sizeof(double) * (size_t)(fixed_doubles(a->Mt) + chunk * ((a->q * a->Mt) | 1));
  BO_CHECK_ARG(lds <= 65536, "%s: %zu bytes of LDS", who, lds);
  const int64_t P = BWD ? (int64_t)a->Mt * (a->q * a->q + a->q) : 2;
  const int64_t need = (int64_t)a->B * G * P;
  BO_CHECK_ARG(a->work && a->work_size >= need,
               "%s: work of at least %lld doubles is required (work_size %lld)", who,
               (long long)need, (long long)a->work_size);
  const LogRedParams lp{a->tau_relu, a->tau_max, a->fat};
  const dim3 grid((unsigned)a->B, (unsigned)G);
#define BO_CH(LG, EX)                                                                            \
  cheb_kernel<LG, EX, BWD><<<grid, THREADS, lds, st>>>(                                          \
      a->B, a->q, a->Mt, a->S, G, Sg, a->mean, a->L, a->Z, a->F, a->ldF, a->sF, a->Qp, a->best_f, \
      a->best_f_s, tb, a->feas, lp, chunk, a->acq, a->dacq, a->work, a->dF, a->dfeas)
  if (a->log) {
    if (ext) BO_CH(true, true);
    else BO_CH(true, false);
  } else {
    if (ext) BO_CH(false, true);
    else BO_CH(false, false);
  }
#undef BO_CH
  BO_LAUNCH_CHECK();
  if (BWD) {
    const int64_t n = (int64_t)a->B * P;
    cheb_fold_bwd<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(a->B, G, a->q, a->Mt, a->work,
                                                             a->dmean, a->dL);
  } else if (a->log) {
    cheb_fold_fwd<true><<<(unsigned)ceil_div(a->B, 64), 64, 0, st>>>(a->B, G, a->S, a->work, a->acq);
  } else {
    cheb_fold_fwd<false><<<(unsigned)ceil_div(a->B, 64), 64, 0, st>>>(a->B, G, a->S, a->work, a->acq);
  }
  BO_LAUNCH_CHECK();
  return BO_OK;
}

}  // namespace

// bo_qmc_cheb / bo_qmc_cheb_backward behind their header checks (abi_structs.cpp).
extern "C" int bo_qmc_cheb_impl(const BoQmcChebArgs* a, void* stream) {
  ChebTab tb;
  if (int st = check_args(a, "bo_qmc_cheb", &tb); st != BO_OK) return st;
  BO_CHECK_ARG(a->acq != nullptr, "bo_qmc_cheb: acq is required");
  if (a->B == 0) return BO_OK;
  return launch<false>(a, tb, "bo_qmc_cheb", as_stream(stream));
}

extern "C" int bo_qmc_cheb_backward_impl(const BoQmcChebArgs* a, void* stream) {
  ChebTab tb;
  if (int st = check_args(a, "bo_qmc_cheb_backward", &tb); st != BO_OK) return st;
  BO_CHECK_ARG(a->dacq && a->dmean && a->dL, "bo_qmc_cheb_backward: dacq, dmean and dL are required");
  BO_CHECK_ARG(!a->log || a->acq != nullptr, "bo_qmc_cheb_backward: log mode reads the forward's acq");
  BO_CHECK_ARG((a->F == nullptr) == (a->dF == nullptr), "bo_qmc_cheb_backward: F and dF go together");
  BO_CHECK_ARG((a->feas == nullptr) == (a->dfeas == nullptr),
               "bo_qmc_cheb_backward: feas and dfeas go together");
  if (a->B == 0) return BO_OK;
  return launch<true>(a, tb, "bo_qmc_cheb_backward", as_stream(stream));
}
