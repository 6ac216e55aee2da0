// One-shot qKnowledgeGradient with the posterior mean as inner value
// (botorch/acquisition/knowledge_gradient.py:151-207, models/model.py:328-407),
// from the packed posterior moments of bo::gp_posterior.
//
// Restart b owns T tiles of q' = q_a + slots rows: the q_a actual points, then
// `slots` fantasy solutions; fantasy i sits in tile i / slots, row q_a + i % slots.
//
//   A   = cov[tile 0][:q_a, :q_a] + noise I        L = psd_safe_cholesky(A)
//   w_i = L^{-T} z_i                               (z_i: row i of Z, N_f x q_a)
//   v_i = mean[row_i] + sum_{j < q_a} cov[row_i][j] w_ij
//   acq = mean_i v_i
//
// which is the fantasy model's posterior mean at x'_i after conditioning on
// (X, mu(X) + L z_i) with the same noise: mu(X) cancels, so nothing of the mean
// at the actual rows, of the fantasy x fantasy block or of the X x X blocks of
// the tiles t > 0 is read.
//
// One workgroup per restart.  Forward: A and L live in LDS, wave 0 factors
// (lane i owns row i, the [G] jitter ladder around it), then a lane per
// fantasy back-substitutes and takes the dot product, looping when N_f exceeds
// the workgroup; the lanes' partial sums meet in a fixed tree.  Backward: a
// lane per fantasy of a chunk leaves u_i = L^{-1} c_i and c_i w_i in LDS, a
// thread per entry of dL sums the chunk in order, the Cholesky backward runs in
// LDS and one last pass writes every entry of dmean and dcov.  No atomics:
// bitwise reproducible run to run.
#include "common.h"

#include <algorithm>

namespace {

constexpr int QMAX = 16;           // q_a + slots <= QMAX, hence q_a <= 15
constexpr int QS = QMAX + 1;       // odd row stride of the q_a x q_a planes
constexpr int PLANE = QMAX * QS;   // 272 doubles: every carve offset is a multiple of 16 B
constexpr int THREADS = 256;
constexpr int CHUNK = 128;         // fantasies per LDS chunk of the backward

// QB: the q_a bucket the register arrays are sized for.
template <int QB>
__global__ __launch_bounds__(THREADS) void kg_forward_kernel(
    int T, int qa, int slots, int Nf, double noise, double jitter0, int max_tries,
    const double* __restrict__ mean, const double* __restrict__ cov, const double* __restrict__ Z,
    double* __restrict__ acq, double* __restrict__ values, double* __restrict__ Lout,
    double* __restrict__ Wout, int* __restrict__ info_out, double* __restrict__ jitter_out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* const M = smem;                                  // QMAX x QS: A, then L (lower)
  double* const red = M + PLANE;                           // THREADS
  int* const fail = reinterpret_cast<int*>(red + THREADS);

  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int qp = qa + slots;
  const double* cov0 = cov + b * T * qp * qp;  // tile 0: its X x X block is A - noise I

  // psd_safe_cholesky: plain, then jitter0 10^k; the increments are added to the
  // diagonal and to the reported total one by one, as the reference adds them
  double dii = 0.0, added = 0.0, prev = 0.0, p10 = 1.0;
  if (tid < qa) dii = cov0[tid * qp + tid] + noise;
  int info = 0;
  for (int attempt = 0; attempt <= max_tries; ++attempt) {
    if (attempt > 0) {
// (no fused multiply-add: the reported total is the reference's to the last bit)
#pragma clang fp contract(off)
      const double jn = jitter0 * p10;
      p10 *= 10.0;
      const double inc = jn - prev;
      dii += inc;
      added += inc;
      prev = jn;
    }
    if (tid < qa)
      for (int c = 0; c <= tid; ++c) M[tid * QS + c] = (c == tid) ? dii : cov0[tid * qp + c];
    if (tid == 0) *fail = 0;
    __syncthreads();
    for (int j = 0; j < qa; ++j) {
      const double ajj = M[j * QS + j];
      if (tid == 0 && !(ajj > 0.0) && *fail == 0) *fail = j + 1;
      const double djj = sqrt(ajj);
      __syncthreads();
      if (tid == j) M[j * QS + j] = djj;
      if (tid > j && tid < qa) M[tid * QS + j] = M[tid * QS + j] / djj;
      __syncthreads();
      if (tid > j && tid < qa) {
        const double lij = M[tid * QS + j];
        for (int l = j + 1; l <= tid; ++l) M[tid * QS + l] = fma(-lij, M[l * QS + j], M[tid * QS + l]);
      }
      __syncthreads();
    }
    info = *fail;
    __syncthreads();
    if (info == 0) break;
  }
  if (tid < qa * qa) {
    const int i = tid / qa, c = tid % qa;
    Lout[b * qa * qa + tid] = info ? NAN : ((c <= i) ? M[i * QS + c] : 0.0);
  }
  if (tid == 0) {
    if (info_out) info_out[b] = info;
    if (jitter_out) jitter_out[b] = added;
  }

  // a lane per fantasy: w = L^{-T} z, then the dot product with the cross row
  double part = 0.0;
  for (int i = tid; i < Nf; i += THREADS) {
    const double* z = Z + (int64_t)i * qa;
    double w[QB];
#pragma unroll
    for (int j = QB - 1; j >= 0; --j) {
      w[j] = 0.0;
      if (j < qa) {
        double s = z[j];
#pragma unroll
        for (int k = j + 1; k < QB; ++k)
          if (k < qa) s = fma(-M[k * QS + j], w[k], s);
        w[j] = s / M[j * QS + j];
      }
    }
    const int64_t row = (b * T + i / slots) * qp + qa + i % slots;
    const double* cr = cov + row * qp;
    double* wo = Wout + (b * Nf + i) * qa;
    double v = mean[row];
#pragma unroll
    for (int j = 0; j < QB; ++j) {
      if (j < qa) {
        v = fma(cr[j], w[j], v);
        wo[j] = info ? NAN : w[j];
      }
    }
    if (info) v = NAN;
    values[b * Nf + i] = v;
    part += v;
  }
  red[tid] = part;
  __syncthreads();
  for (int off = THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) acq[b] = red[0] / (double)Nf;
}

template <int QB>
__global__ __launch_bounds__(THREADS) void kg_backward_kernel(
    int T, int qa, int slots, int Nf, const double* __restrict__ cov, const double* __restrict__ Lg,
    const double* __restrict__ Wg, const double* __restrict__ dacq,
    const double* __restrict__ dvalues, double* __restrict__ dmean, double* __restrict__ dcov) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* const L = smem;            // five QMAX x QS planes
  double* const dL = L + PLANE;      // dL, at the end dA
  double* const Li = dL + PLANE;     // L^{-1}
  double* const Pm = Li + PLANE;
  double* const Tm = Pm + PLANE;
  double* const Us = Tm + PLANE;     // chunk x US: u_i = L^{-1} c_i
  const int US = qa | 1;             // odd row stride: a lane per fantasy, no bank conflicts
  const int chunk = min(Nf, CHUNK);
  double* const Gs = Us + chunk * US;  // chunk x US: c_i w_i

  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int qp = qa + slots;
  const double g = dacq[b] / (double)Nf;
  const double* dvb = dvalues ? dvalues + b * Nf : nullptr;
  const double* Wb = Wg + b * Nf * qa;

  if (tid < qa * qa) L[(tid / qa) * QS + tid % qa] = Lg[b * qa * qa + tid];
  __syncthreads();

  // dL[a][j] = -sum_i c_i w_ia u_ij (j <= a): this thread's entry, the fantasies in order
  const int ea = tid / qa, ej = tid % qa;
  double acc = 0.0;
  for (int i0 = 0; i0 < Nf; i0 += chunk) {
    const int ns = min(chunk, Nf - i0);
    if (tid < ns) {
      const int i = i0 + tid;
      const double ci = g + (dvb ? dvb[i] : 0.0);
      const int64_t row = (b * T + i / slots) * qp + qa + i % slots;
      const double* cr = cov + row * qp;
      double u[QB];
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        u[j] = 0.0;
        if (j < qa) {
          double s = cr[j];
#pragma unroll
          for (int k = 0; k < j; ++k) s = fma(-L[j * QS + k], u[k], s);
          u[j] = s / L[j * QS + j];
          Us[tid * US + j] = u[j];
          Gs[tid * US + j] = ci * Wb[(int64_t)i * qa + j];
        }
      }
    }
    __syncthreads();
    if (tid < qa * qa && ej <= ea)
      for (int s = 0; s < ns; ++s) acc = fma(-Gs[s * US + ea], Us[s * US + ej], acc);
    __syncthreads();
  }
  if (tid < qa * qa) dL[ea * QS + ej] = (ej <= ea) ? acc : 0.0;
  // L^{-1}: a column per thread (forward substitution)
  if (tid < qa) {
    const int c = tid;
    for (int r = 0; r < qa; ++r) {
      double s = (r == c) ? 1.0 : 0.0;
      for (int k = c; k < r; ++k) s = fma(-L[r * QS + k], Li[k * QS + c], s);
      Li[r * QS + c] = (r >= c) ? s / L[r * QS + r] : 0.0;
    }
  }
  __syncthreads();
  // torch's cholesky backward: X = tril(L^T dL), P = (X + tril(X, -1)^T) / 2,
  // dA = L^{-T} P L^{-1}
  const bool on = tid < qa * qa;
  if (on && ea >= ej) {
    double x = 0.0;
    for (int k = ea; k < qa; ++k) x = fma(L[k * QS + ea], dL[k * QS + ej], x);
    Tm[ea * QS + ej] = x;
  }
  __syncthreads();
  if (on) Pm[ea * QS + ej] = 0.5 * ((ea >= ej) ? Tm[ea * QS + ej] : Tm[ej * QS + ea]);
  __syncthreads();
  if (on) {
    double x = 0.0;
    for (int k = ej; k < qa; ++k) x = fma(Pm[ea * QS + k], Li[k * QS + ej], x);
    Tm[ea * QS + ej] = x;  // T = P L^{-1}
  }
  __syncthreads();
  if (on) {
    double x = 0.0;
    for (int k = ea; k < qa; ++k) x = fma(Li[k * QS + ea], Tm[k * QS + ej], x);
    dL[ea * QS + ej] = x;  // dA (nobody reads dL any more)
  }
  __syncthreads();

  // every entry of this restart's dmean and dcov, each written once
  double* dmb = dmean + b * T * qp;
  for (int e = tid; e < T * qp; e += THREADS) {
    const int t = e / qp, r = e % qp;
    const int i = t * slots + r - qa;
    dmb[e] = (r >= qa && i < Nf) ? g + (dvb ? dvb[i] : 0.0) : 0.0;
  }
  double* dcb = dcov + b * T * qp * qp;
  for (int e = tid; e < T * qp * qp; e += THREADS) {
    const int t = e / (qp * qp), r = (e / qp) % qp, c = e % qp;
    double v = 0.0;
    if (c < qa) {
      if (r < qa) {
        if (t == 0) v = dL[r * QS + c];
      } else {
        const int i = t * slots + r - qa;
        if (i < Nf) v = (g + (dvb ? dvb[i] : 0.0)) * Wb[(int64_t)i * qa + c];
      }
    }
    dcb[e] = v;
  }
}

int check_args(const BoKgArgs* a, const char* who) {
  BO_CHECK_ARG(a->B >= 0 && a->N_f >= 1 && a->T >= 1, "%s: bad B / N_f / T", who);
  BO_CHECK_ARG(a->q_a >= 1, "%s: q_a >= 1 (got %d)", who, a->q_a);
  BO_CHECK_ARG(a->slots >= 1 && a->q_a + a->slots <= QMAX,
               "%s: slots >= 1 and q_a + slots <= %d (got %d + %d)", who, QMAX, a->q_a, a->slots);
  BO_CHECK_ARG((int64_t)a->T * a->slots >= a->N_f, "%s: T slots = %d x %d holds fewer than N_f = %d",
               who, a->T, a->slots, a->N_f);
  BO_CHECK_ARG((int64_t)a->T * (a->q_a + a->slots) * (a->q_a + a->slots) < (int64_t(1) << 31),
               "%s: a restart's tiles exceed 2^31 entries", who);
  BO_CHECK_ARG(a->cov && a->L && a->W, "%s: cov, L and W are required", who);
  return BO_OK;
}

size_t forward_lds() { return sizeof(double) * (PLANE + THREADS + 2); }

size_t backward_lds(const BoKgArgs* a) {
  const int chunk = std::min((int)a->N_f, CHUNK);
  return sizeof(double) * (size_t)(5 * PLANE + 2 * chunk * (a->q_a | 1));
}

}  // namespace

// bo_kg_v / bo_kg_backward_v behind their header checks (abi_structs.cpp).
extern "C" int bo_kg_impl(const BoKgArgs* a, void* stream) {
  if (int st = check_args(a, "bo_kg"); st != BO_OK) return st;
  BO_CHECK_ARG(a->max_tries >= 0 && a->noise >= 0.0, "bo_kg: bad max_tries / noise");
  BO_CHECK_ARG(a->mean && a->Z, "bo_kg: mean and Z are required");
  BO_CHECK_ARG(a->acq && a->values, "bo_kg: acq and values are required");
  if (a->B == 0) return BO_OK;
#define BO_KG(QQ)                                                                              \
  kg_forward_kernel<QQ><<<(unsigned)a->B, THREADS, forward_lds(), as_stream(stream)>>>(        \
      a->T, a->q_a, a->slots, a->N_f, a->noise, a->jitter0, a->max_tries, a->mean, a->cov,     \
      a->Z, a->acq, a->values, a->L, a->W, a->info, a->jitter)
  if (a->q_a <= 4) {
    BO_KG(4);
  } else if (a->q_a <= 8) {
    BO_KG(8);
  } else {
    BO_KG(QMAX);
  }
#undef BO_KG
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_kg_backward_impl(const BoKgArgs* a, void* stream) {
  if (int st = check_args(a, "bo_kg_backward"); st != BO_OK) return st;
  BO_CHECK_ARG(a->dacq && a->dmean && a->dcov, "bo_kg_backward: dacq, dmean and dcov are required");
  if (a->B == 0) return BO_OK;
#define BO_KG(QQ)                                                                              \
  kg_backward_kernel<QQ><<<(unsigned)a->B, THREADS, backward_lds(a), as_stream(stream)>>>(     \
      a->T, a->q_a, a->slots, a->N_f, a->cov, a->L, a->W, a->dacq, a->dvalues, a->dmean, a->dcov)
  if (a->q_a <= 4) {
    BO_KG(4);
  } else if (a->q_a <= 8) {
    BO_KG(8);
  } else {
    BO_KG(QMAX);
  }
#undef BO_KG
  BO_LAUNCH_CHECK();
  return BO_OK;
}
