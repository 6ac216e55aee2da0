// Batched fantasy models (botorch/models/model.py:328-407 fantasize, then
// models/gpytorch.py:405-466 posterior of the conditioned model) from the packed
// posterior moments of bo::gp_posterior.
//
// T-batch b owns T tiles of q' = q_a + slots q rows: the q_a fantasised points
// X_b, then `slots` groups of q evaluation points; group g sits in tile g / slots
// at rows q_a + (g % slots) q ... + q.  There are F groups: F = N_f (one set of
// evaluation points per fantasy) or F = 1 (`shared`: one set for all fantasies).
//
//   A     = cov[tile 0][:q_a, :q_a] + diag(noise)      L = psd_safe_cholesky(A)
//   V_g   = C_g L^{-T}                                 (C_g: group g's rows, columns < q_a)
//   mu'_f = mean[rows of g_f] + V_{g_f} z_f            (g_f = f, or 0 when shared)
//   S'_g  = D_g - V_g V_g^T                            (D_g: group g's own diagonal block)
//
// which are the moments of the model conditioned on (X_b, mu(X_b) + L z_f) under
// the same noise: mu(X_b) cancels.  Nothing but tile 0's X x X block (its lower
// triangle), each group's C_g and D_g and the mean at the groups' rows is read.
//
// One workgroup per t-batch.  Forward: A and L live in LDS, the [G] jitter
// ladder exactly as kg.hip runs it; then, a chunk of groups at a time, a lane per
// row forward-substitutes its row of V into LDS and the workgroup writes the
// chunk's means and covariances from there.  Backward: a lane per row forms its
// row of dV, back-substitutes dC = dV L^{-1} and leaves it in LDS beside V, a
// thread per entry of dL sums the rows in order, the Cholesky backward runs in
// LDS and one last pass writes every entry of dmean and dcov not written yet.
// No atomics: bitwise reproducible run to run.
#include "common.h"

#include <algorithm>

namespace {

constexpr int QMAX = 16;           // q_a + slots q <= QMAX, hence q_a, q <= 15
constexpr int QS = QMAX + 1;       // odd row stride of the q_a x q_a planes
constexpr int PLANE = QMAX * QS;   // 272 doubles: every carve offset is a multiple of 16 B
constexpr int THREADS = 256;
constexpr int CHUNK = 128;         // rows of V per LDS chunk (whole groups: at least 8)

// global row (of mean, and of cov's leading two dims) of row r of group g
__device__ __forceinline__ int64_t group_row(int64_t b, int T, int qp, int qa, int q, int slots,
                                             int g, int r) {
  return (b * T + g / slots) * qp + qa + (g % slots) * q + r;
}

// QB: the q_a bucket the register arrays are sized for.
template <int QB>
__global__ __launch_bounds__(THREADS) void fantasy_forward_kernel(
    int T, int qa, int q, int slots, int Nf, int shared, int64_t noise_stride, double jitter0,
    int max_tries, const double* __restrict__ mean, const double* __restrict__ cov,
    const double* __restrict__ Z, const double* __restrict__ noise, double* __restrict__ mean_out,
    double* __restrict__ cov_out, double* __restrict__ Lout, double* __restrict__ Vout,
    int* __restrict__ info_out, double* __restrict__ jitter_out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* const M = smem;                 // QMAX x QS: A, then L (lower)
  double* const Vs = M + PLANE;           // CHUNK x US: the chunk's rows of V
  int* const fail = reinterpret_cast<int*>(Vs + CHUNK * QMAX);
  const int US = qa | 1;                  // odd row stride: a lane per row, no bank conflicts

  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int qp = qa + slots * q;
  const int F = shared ? 1 : Nf;
  const double* cov0 = cov + b * T * qp * qp;  // tile 0: its X x X block is A - diag(noise)

  // psd_safe_cholesky: plain, then jitter0 10^k; the increments are added to the
  // diagonal and to the reported total one by one, as the reference adds them
  double dii = 0.0, added = 0.0, prev = 0.0, p10 = 1.0;
  if (tid < qa) dii = cov0[tid * qp + tid] + noise[b * noise_stride + tid];
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

  const int cg = CHUNK / q;  // groups per chunk
  for (int g0 = 0; g0 < F; g0 += cg) {
    const int ng = min(cg, F - g0);
    // a lane per row: v = L^{-1} c (row of V = C L^{-T}); its mean when the group is a fantasy's own
    if (tid < ng * q) {
      const int g = g0 + tid / q, r = tid % q;
      const int64_t row = group_row(b, T, qp, qa, q, slots, g, r);
      const double* cr = cov + row * qp;
      double* vo = Vout + ((b * F + g) * q + r) * qa;
      double v[QB];
      double m = shared ? 0.0 : mean[row];
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        v[j] = 0.0;
        if (j < qa) {
          double s = cr[j];
#pragma unroll
          for (int k = 0; k < j; ++k) s = fma(-M[j * QS + k], v[k], s);
          v[j] = s / M[j * QS + j];
          Vs[tid * US + j] = v[j];
          vo[j] = info ? NAN : v[j];
          if (!shared) m = fma(v[j], Z[(int64_t)g * qa + j], m);
        }
      }
      if (!shared) mean_out[(b * Nf + g) * q + r] = info ? NAN : m;
    }
    __syncthreads();
    if (shared) {  // one group (F = 1): every fantasy's mean from the same V
      for (int e = tid; e < Nf * q; e += THREADS) {
        const int f = e / q, r = e % q;
        double m = mean[group_row(b, T, qp, qa, q, slots, 0, r)];
        for (int j = 0; j < qa; ++j) m = fma(Vs[r * US + j], Z[(int64_t)f * qa + j], m);
        mean_out[(b * Nf + f) * q + r] = info ? NAN : m;
      }
    }
    // S' = D - V V^T, both triangles
    for (int e = tid; e < ng * q * q; e += THREADS) {
      const int gl = e / (q * q), r = (e / q) % q, c = e % q;
      const int g = g0 + gl;
      const int64_t row = group_row(b, T, qp, qa, q, slots, g, r);
      double s = cov[row * qp + qa + (g % slots) * q + c];
      const double* vr = Vs + (gl * q + r) * US;
      const double* vc = Vs + (gl * q + c) * US;
      for (int j = 0; j < qa; ++j) s = fma(-vr[j], vc[j], s);
      cov_out[((b * F + g) * q + r) * q + c] = info ? NAN : s;
    }
    __syncthreads();
  }
}

template <int QB>
__global__ __launch_bounds__(THREADS) void fantasy_backward_kernel(
    int T, int qa, int q, int slots, int Nf, int shared, const double* __restrict__ Z,
    const double* __restrict__ Lg, const double* __restrict__ Vg,
    const double* __restrict__ dmean_out, const double* __restrict__ dcov_out,
    double* __restrict__ dmean, double* __restrict__ dcov, double* __restrict__ dZ) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* const L = smem;            // five QMAX x QS planes
  double* const dL = L + PLANE;      // dL, at the end dA
  double* const Li = dL + PLANE;     // L^{-1}
  double* const Pm = Li + PLANE;
  double* const Tm = Pm + PLANE;
  double* const Us = Tm + PLANE;          // CHUNK x US: the chunk's rows of V
  double* const Gs = Us + CHUNK * QMAX;   // CHUNK x US: the chunk's rows of dC
  double* const Sm = Gs + CHUNK * QMAX;   // shared: sum_f dmu'_f z_f^T (q <= 15 rows of QS)
  double* const Ms = Sm + (QMAX - 1) * QS;  // shared: sum_f dmu'_f (q), the plane's last row
  const int US = qa | 1;             // odd row stride: a lane per row, no bank conflicts

  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int qp = qa + slots * q;
  const int F = shared ? 1 : Nf;
  const double* dmo = dmean_out + b * Nf * q;
  const double* dco = dcov_out + b * F * q * q;
  const double* Vb = Vg + b * F * q * qa;
  double* dmb = dmean + b * T * qp;
  double* dcb = dcov + b * T * qp * qp;

  if (tid < qa * qa) L[(tid / qa) * QS + tid % qa] = Lg[b * qa * qa + tid];
  if (shared) {  // the fantasies in order: the one group collects every fantasy's cotangent
    if (tid < q * qa) {
      const int r = tid / qa, k = tid % qa;
      double s = 0.0;
      for (int f = 0; f < Nf; ++f) s = fma(dmo[f * q + r], Z[(int64_t)f * qa + k], s);
      Sm[r * QS + k] = s;
    } else if (tid < q * qa + q) {
      const int r = tid - q * qa;
      double s = 0.0;
      for (int f = 0; f < Nf; ++f) s += dmo[f * q + r];
      Ms[r] = s;
    }
  }
  __syncthreads();

  // dL[a][j] = -sum_rows dC[row][a] V[row][j] (j <= a): this thread's entry, the rows in order
  const int ea = tid / qa, ej = tid % qa;
  double acc = 0.0;
  const int cg = CHUNK / q;
  for (int g0 = 0; g0 < F; g0 += cg) {
    const int ng = min(cg, F - g0);
    for (int e = tid; e < ng * q * qa; e += THREADS)
      Us[(e / qa) * US + e % qa] = Vb[(int64_t)g0 * q * qa + e];
    __syncthreads();
    if (tid < ng * q) {
      const int gl = tid / q, r = tid % q, g = g0 + gl;
      // dV = dmu' z^T - (dS' + dS'^T) V, this row of it
      const double* ds = dco + (int64_t)g * q * q;
      double w[QB];
#pragma unroll
      for (int j = 0; j < QB; ++j) {
        w[j] = 0.0;
        if (j < qa) w[j] = shared ? Sm[r * QS + j] : dmo[g * q + r] * Z[(int64_t)g * qa + j];
      }
      for (int c = 0; c < q; ++c) {
        const double sy = ds[r * q + c] + ds[c * q + r];
        const double* vc = Us + (gl * q + c) * US;
#pragma unroll
        for (int j = 0; j < QB; ++j)
          if (j < qa) w[j] = fma(-sy, vc[j], w[j]);
      }
      // dC = dV L^{-1}: L^T dC^T = dV^T, back substitution
      const int64_t row = group_row(b, T, qp, qa, q, slots, g, r);
#pragma unroll
      for (int j = QB - 1; j >= 0; --j) {
        if (j < qa) {
          double s = w[j];
#pragma unroll
          for (int k = j + 1; k < QB; ++k)
            if (k < qa) s = fma(-L[k * QS + j], w[k], s);
          w[j] = s / L[j * QS + j];
          Gs[tid * US + j] = w[j];
          dcb[(row - b * T * qp) * qp + j] = w[j];
        }
      }
    }
    if (dZ && !shared) {  // dz_f = V_f^T dmu'_f
      for (int e = tid; e < ng * qa; e += THREADS) {
        const int gl = e / qa, k = e % qa, g = g0 + gl;
        double s = 0.0;
        for (int r = 0; r < q; ++r) s = fma(Us[(gl * q + r) * US + k], dmo[g * q + r], s);
        dZ[(b * Nf + g) * qa + k] = s;
      }
    }
    if (dZ && shared) {
      for (int e = tid; e < Nf * qa; e += THREADS) {
        const int f = e / qa, k = e % qa;
        double s = 0.0;
        for (int r = 0; r < q; ++r) s = fma(Us[r * US + k], dmo[f * q + r], s);
        dZ[(b * Nf + f) * qa + k] = s;
      }
    }
    __syncthreads();
    if (tid < qa * qa && ej <= ea)
      for (int s = 0; s < ng * q; ++s) acc = fma(-Gs[s * US + ea], Us[s * US + ej], acc);
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

  // every entry of this t-batch's dmean, and every entry of its dcov but the
  // groups' cross blocks (written above), each once
  for (int e = tid; e < T * qp; e += THREADS) {
    const int t = e / qp, r = e % qp;
    double v = 0.0;
    if (r >= qa) {
      const int g = t * slots + (r - qa) / q, rr = (r - qa) % q;
      if (g < F) v = shared ? Ms[rr] : dmo[g * q + rr];
    }
    dmb[e] = v;
  }
  for (int e = tid; e < T * qp * qp; e += THREADS) {
    const int t = e / (qp * qp), r = (e / qp) % qp, c = e % qp;
    double v = 0.0;
    if (r < qa) {
      if (c < qa && t == 0) v = dL[r * QS + c];
    } else {
      const int s = (r - qa) / q, g = t * slots + s, rr = (r - qa) % q;
      if (g < F) {
        if (c < qa) continue;  // the cross block: dC
        const int cc = c - qa - s * q;
        if (cc >= 0 && cc < q) v = dco[((int64_t)g * q + rr) * q + cc];
      }
    }
    dcb[e] = v;
  }
}

int check_args(const BoFantasyArgs* a, const char* who) {
  BO_CHECK_ARG(a->B >= 0 && a->N_f >= 1 && a->T >= 1, "%s: bad B / N_f / T", who);
  BO_CHECK_ARG(a->q_a >= 1 && a->q >= 1, "%s: q_a >= 1 and q >= 1 (got %d, %d)", who, a->q_a, a->q);
  BO_CHECK_ARG(a->slots >= 1 && (int64_t)a->q_a + (int64_t)a->slots * a->q <= QMAX,
               "%s: slots >= 1 and q_a + slots q <= %d (got %d + %d x %d)", who, QMAX, a->q_a,
               a->slots, a->q);
  BO_CHECK_ARG(a->shared == 0 || a->shared == 1, "%s: shared is 0 or 1", who);
  const int64_t F = a->shared ? 1 : a->N_f;
  BO_CHECK_ARG((int64_t)a->T * a->slots >= F, "%s: T slots = %d x %d holds fewer than F = %lld groups",
               who, a->T, a->slots, (long long)F);
  const int64_t qp = a->q_a + a->slots * a->q;
  BO_CHECK_ARG((int64_t)a->T * qp * qp < (int64_t(1) << 31) &&
                   (int64_t)a->N_f * a->q * a->q * a->q_a < (int64_t(1) << 31),
               "%s: a t-batch's tiles or outputs exceed 2^31 entries", who);
  BO_CHECK_ARG(a->Z && a->L && a->V, "%s: Z, L and V are required", who);
  return BO_OK;
}

size_t forward_lds() { return sizeof(double) * (PLANE + CHUNK * QMAX + 2); }
size_t backward_lds() { return sizeof(double) * (5 * PLANE + 2 * CHUNK * QMAX + PLANE); }

}  // namespace

// bo_fantasy_posterior / bo_fantasy_posterior_backward behind their header checks (abi_structs.cpp).
extern "C" int bo_fantasy_posterior_impl(const BoFantasyArgs* a, void* stream) {
  if (int st = check_args(a, "bo_fantasy_posterior"); st != BO_OK) return st;
  BO_CHECK_ARG(a->max_tries >= 0, "bo_fantasy_posterior: bad max_tries");
  BO_CHECK_ARG(a->noise_stride == 0 || a->noise_stride == a->q_a,
               "bo_fantasy_posterior: noise_stride is 0 or q_a");
  BO_CHECK_ARG(a->mean && a->cov && a->noise, "bo_fantasy_posterior: mean, cov and noise are required");
  BO_CHECK_ARG(a->mean_out && a->cov_out, "bo_fantasy_posterior: mean_out and cov_out are required");
  if (a->B == 0) return BO_OK;
#define BO_FANTASY(QQ)                                                                          \
  fantasy_forward_kernel<QQ><<<(unsigned)a->B, THREADS, forward_lds(), as_stream(stream)>>>(    \
      a->T, a->q_a, a->q, a->slots, a->N_f, a->shared, a->noise_stride, a->jitter0,             \
      a->max_tries, a->mean, a->cov, a->Z, a->noise, a->mean_out, a->cov_out, a->L, a->V,       \
      a->info, a->jitter)
  if (a->q_a <= 4) {
    BO_FANTASY(4);
  } else if (a->q_a <= 8) {
    BO_FANTASY(8);
  } else {
    BO_FANTASY(QMAX);
  }
#undef BO_FANTASY
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_fantasy_posterior_backward_impl(const BoFantasyArgs* a, void* stream) {
  if (int st = check_args(a, "bo_fantasy_posterior_backward"); st != BO_OK) return st;
  BO_CHECK_ARG(a->dmean_out && a->dcov_out, "bo_fantasy_posterior_backward: dmean_out and dcov_out are required");
  BO_CHECK_ARG(a->dmean && a->dcov, "bo_fantasy_posterior_backward: dmean and dcov are required");
  if (a->B == 0) return BO_OK;
#define BO_FANTASY(QQ)                                                                          \
  fantasy_backward_kernel<QQ><<<(unsigned)a->B, THREADS, backward_lds(), as_stream(stream)>>>(  \
      a->T, a->q_a, a->q, a->slots, a->N_f, a->shared, a->Z, a->L, a->V, a->dmean_out,          \
      a->dcov_out, a->dmean, a->dcov, a->dZ)
  if (a->q_a <= 4) {
    BO_FANTASY(4);
  } else if (a->q_a <= 8) {
    BO_FANTASY(8);
  } else {
    BO_FANTASY(QMAX);
  }
#undef BO_FANTASY
  BO_LAUNCH_CHECK();
  return BO_OK;
}
