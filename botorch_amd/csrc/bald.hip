// qBayesianActiveLearningByDisagreement (botorch/acquisition/
// bayesian_active_learning.py:52-126): the entropy of the Gaussian-mixture
// posterior of an MCMC ensemble minus the entropy of each component, by Monte
// Carlo over base samples shared by all components.  The definitions stand in
// include/botorch_amd.h (BoBaldArgs) and DESIGN.md section 20.
//
// Layout.  One workgroup of 256 threads owns one (t-batch b, component m)
// pair, so the M components of a t-batch spread over M workgroups and B = 16
// already fills the chip at M = 16.  Every workgroup stages the t-batch's M
// means and M roots (lower triangle, packed, with the reciprocal diagonal
// beside it) into LDS, padded to QP = 1, 2, 4, 8 or 16 columns by identity rows
// (which add nothing to a residual or a log-determinant), so every loop over
// the q coordinates has a compile-time bound and its vectors stay in
// registers.  A thread takes the samples s = t, t + 256, ...: it forms
// y = mu_m + L_m z_s, then for every component m' solves L_m' w = y - mu_m' by
// forward substitution against the LDS copy (all lanes read the same address: a
// broadcast) and folds l = -|w|^2 / 2 - log det L_m' - (q / 2) log 2 pi into an
// online log-sum-exp.  The triangular solve costs what a product with the
// inverse root would (QP (QP + 1) / 2 fused multiply-adds) without forming an
// inverse.  This is VALU work: per pair of components the q x q by q x S
// product is 16 x 16 x 4 matrix-core tiles at best a quarter full for q = 4,
// and the exponentials and the running maximum sit on the vector unit anyway.
//
// Forward: the workgroup's sum over s (per thread in sample order, then a xor
// butterfly over the wave and the four waves in order) gives the component's
// share of the mixture entropy, which goes to work[b][m], and -C_bm, which goes
// to out[b][m]; a second, tiny launch adds the mean over m of the shares in
// index order.  Nothing larger than B x M reaches memory.
//
// Backward, two launches over the same grid.  The first plays the sample's
// own component (the source role, index m): it stores log-sum-exp_ms to work
// (B x M x S) and accumulates sum_m' pi g (g = L_m'^{-T} w) against 1 and z_s.
// The second plays the evaluating component (the target role, index m'): it
// walks all sources m, reads their log-sum-exp, and accumulates pi g against 1
// and w, and pi itself.  Both sums are outer products over samples: a chunk of
// 256 samples parks its vectors in LDS and the threads then own the (i, j)
// entries, each summing a fixed slice of the chunk in sample order; slices are
// combined in slice order at the end.  No atomics: a second call is
// bit-identical.  The second launch adds onto what the first one wrote (same
// stream).
#include "common.h"

namespace {

constexpr int BALD_MMAX = 64, BALD_QMAX = 16, BALD_SMAX = 1 << 20, BALD_T = 256;
constexpr double LOG_2PI = 1.83787706640934548356;

struct BaldDev {
  int M, q, S;
  int64_t B;
  const double *mean, *L, *Z;
  double *out, *work;
  const double* dout;
  double *dmean, *dL;
};

__host__ __device__ constexpr int tri(int i) { return i * (i + 1) / 2; }

// entries of the backward's outer products: QP + 1 against the constant 1
// (the last one sums pi), QP (QP + 1) / 2 of the lower triangle; EP: the next
// power of two (a slice of EP samples per thread, 256 / EP slices)
__host__ __device__ constexpr int bald_ne(int QP) { return QP + 1 + tri(QP); }
__host__ __device__ constexpr int bald_ep(int QP) {
  int e = 1;
  while (e < bald_ne(QP)) e <<= 1;
  return e;
}

// the sum of v over the workgroup's 256 threads in thread 0 (red: 4 doubles)
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int QP>
struct BaldLds {
  static constexpr int NT = tri(QP);
  double *Lp, *inv, *mu, *ld, *red, *A, *W;
  __device__ BaldLds(double* base, int M) {
    Lp = base;             // M x NT   packed lower triangles
    inv = Lp + M * NT;     // M x QP   1 / L_ii
    mu = inv + M * QP;     // M x QP
    ld = mu + M * QP;      // M        sum_i log L_ii
    red = ld + M;          // 256      reductions
    A = red + BALD_T;      // 256 x (QP + 1)  (backward)
    W = A + BALD_T * (QP + 1);
  }
  static size_t bytes(int M, bool grad) {
    size_t n = (size_t)M * (NT + 2 * QP + 1) + BALD_T;
    if (grad) n += 2 * (size_t)BALD_T * (QP + 1);
    return n * sizeof(double);
  }
};

// the M means and roots of t-batch b -> LDS, padded to QP by identity rows
template <int QP>
__device__ __forceinline__ void bald_stage(const BaldDev& a, int64_t b, const BaldLds<QP>& l) {
  constexpr int NT = tri(QP);
  const int t = threadIdx.x, q = a.q;
  for (int e = t; e < a.M * QP; e += BALD_T) {
    const int m = e / QP, i = e - m * QP;
    const int64_t row = (int64_t)m * a.B + b;
    l.inv[e] = i < q ? 1.0 / a.L[(row * q + i) * q + i] : 1.0;
    l.mu[e] = i < q ? a.mean[row * q + i] : 0.0;
  }
  for (int e = t; e < a.M * NT; e += BALD_T) {
    const int m = e / NT, r = e - m * NT;
    int i = 0;
    while (tri(i + 1) <= r) ++i;
    const int j = r - tri(i);
    const int64_t row = (int64_t)m * a.B + b;
    l.Lp[e] = i < q ? a.L[(row * q + i) * q + j] : (i == j ? 1.0 : 0.0);  // (j <= i < q)
  }
  __syncthreads();
  for (int m = t; m < a.M; m += BALD_T) {
    double s = 0.0;
    for (int i = 0; i < QP; ++i) s += log(l.Lp[m * NT + tri(i) + i]);
    l.ld[m] = s;
  }
  __syncthreads();
}

template <int QP>
__device__ __forceinline__ double bald_load_z(const BaldDev& a, int s, double (&z)[QP]) {
  double ss = 0.0;
#pragma unroll
  for (int i = 0; i < QP; ++i) {
    z[i] = (s < a.S && i < a.q) ? a.Z[(int64_t)s * a.q + i] : 0.0;
    ss = fma(z[i], z[i], ss);
  }
  return ss;
}

// y = mu_m + L_m z
template <int QP>
__device__ __forceinline__ void bald_y(const double* Lp, const double* mu, const double (&z)[QP],
                                       double (&y)[QP]) {
#pragma unroll
  for (int i = 0; i < QP; ++i) {
    double acc = mu[i];
#pragma unroll
    for (int j = 0; j <= i; ++j) acc = fma(Lp[tri(i) + j], z[j], acc);
    y[i] = acc;
  }
}

// w = L^{-1} (y - mu) by forward substitution; returns |w|^2
template <int QP>
__device__ __forceinline__ double bald_solve(const double* Lp, const double* inv, const double* mu,
                                             const double (&y)[QP], double (&w)[QP]) {
  double ss = 0.0;
#pragma unroll
  for (int i = 0; i < QP; ++i) {
    double acc = y[i] - mu[i];
#pragma unroll
    for (int k = 0; k < i; ++k) acc = fma(-Lp[tri(i) + k], w[k], acc);
    w[i] = acc * inv[i];
    ss = fma(w[i], w[i], ss);
  }
  return ss;
}

// g = L^{-T} w by back substitution
template <int QP>
__device__ __forceinline__ void bald_solve_t(const double* Lp, const double* inv,
                                             const double (&w)[QP], double (&g)[QP]) {
#pragma unroll
  for (int i = QP - 1; i >= 0; --i) {
    double acc = w[i];
#pragma unroll
    for (int k = i + 1; k < QP; ++k) acc = fma(-Lp[tri(k) + i], g[k], acc);
    g[i] = acc * inv[i];
  }
}

// log-sum-exp over the components m' of the log-density of y
template <int QP>
__device__ __forceinline__ double bald_lse(const BaldDev& a, const BaldLds<QP>& l,
                                           const double (&y)[QP]) {
  constexpr int NT = tri(QP);
  const double c = 0.5 * a.q * LOG_2PI;
  double mx = 0.0, sm = 0.0, w[QP];
  for (int mp = 0; mp < a.M; ++mp) {
    const double ss = bald_solve<QP>(l.Lp + mp * NT, l.inv + mp * QP, l.mu + mp * QP, y, w);
    const double lp = -0.5 * ss - l.ld[mp] - c;
    if (mp == 0) {
      mx = lp;
      sm = 1.0;
    } else if (lp > mx) {
      sm = fma(sm, exp(mx - lp), 1.0);
      mx = lp;
    } else {
      sm += exp(lp - mx);
    }
  }
  return mx + log(sm);
}

template <int QP>
__global__ __launch_bounds__(BALD_T) void bald_fwd_kernel(const BaldDev a) {
  extern __shared__ double bald_smem[];
  constexpr int NT = tri(QP);
  const BaldLds<QP> l(bald_smem, a.M);
  const int64_t b = blockIdx.x / a.M;
  const int m = blockIdx.x - b * a.M;
  bald_stage<QP>(a, b, l);
  double hs = 0.0, zs = 0.0, z[QP], y[QP];
  for (int s = threadIdx.x; s < a.S; s += BALD_T) {
    zs += bald_load_z<QP>(a, s, z);
    bald_y<QP>(l.Lp + m * NT, l.mu + m * QP, z, y);
    hs += bald_lse<QP>(a, l, y);
  }
  hs = block_sum(hs, l.red);
  zs = block_sum(zs, l.red);
  if (threadIdx.x == 0) {
    a.work[b * a.M + m] = log((double)a.M) - hs / a.S;
    a.out[b * a.M + m] = -(0.5 * zs / a.S + l.ld[m] + 0.5 * a.q * LOG_2PI);
  }
}

// out[b][m] += mean_m' work[b][m'], in index order
__global__ __launch_bounds__(BALD_T) void bald_finish_kernel(const BaldDev a) {
  const int64_t e = (int64_t)blockIdx.x * BALD_T + threadIdx.x;
  if (e >= a.B * a.M) return;
  const int64_t b = e / a.M;
  double h = 0.0;
  for (int mp = 0; mp < a.M; ++mp) h += a.work[b * a.M + mp];
  a.out[e] += h / a.M;
}

// The threads' entries of the outer products sum_s A_s[ia] W_s[jb] (row stride
// QP + 1; W_s[QP] = 1): thread t owns entry t % EP for the samples of slice
// t / EP of every chunk.
template <int QP>
struct BaldEntry {
  static constexpr int EP = bald_ep(QP), NE = bald_ne(QP);
  int e, k, ia, jb;
  double acc;
  __device__ BaldEntry() {
    e = threadIdx.x % EP;
    k = threadIdx.x / EP;
    acc = 0.0;
    if (e <= QP || e >= NE) {
      ia = e <= QP ? e : 0;
      jb = QP;
    } else {
      const int r = e - (QP + 1);
      ia = 0;
      while (tri(ia + 1) <= r) ++ia;
      jb = r - tri(ia);
    }
  }
  // between two barriers of the caller's
  __device__ __forceinline__ void add_chunk(const double* A, const double* W) {
    if (e >= NE) return;
    const double* pa = A + (size_t)k * EP * (QP + 1) + ia;
    const double* pw = W + (size_t)k * EP * (QP + 1) + jb;
#pragma unroll 8
    for (int s = 0; s < EP; ++s) acc = fma(pa[s * (QP + 1)], pw[s * (QP + 1)], acc);
  }
  // the slices in order; valid in the threads t < NE (red: 256 doubles)
  __device__ __forceinline__ double total(double* red) {
    __syncthreads();
    red[threadIdx.x] = acc;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x < NE)
      for (int kk = 0; kk < BALD_T / EP; ++kk) tot += red[kk * EP + threadIdx.x];
    return tot;
  }
};

// sum_m dout[b][m] / (M S): the weight of H_b
__device__ __forceinline__ double bald_hscale(const BaldDev& a, int64_t b) {
  double dh = 0.0;
  for (int mm = 0; mm < a.M; ++mm) dh += a.dout[b * a.M + mm];
  return dh / ((double)a.M * (double)a.S);
}

// backward, source role: lse_ms -> work, d mu_m and d L_m of the samples drawn
// from component m, and C_bm's diagonal term; writes the whole q x q block
template <int QP>
__global__ __launch_bounds__(BALD_T) void bald_bwd_source_kernel(const BaldDev a) {
  extern __shared__ double bald_smem[];
  constexpr int NT = tri(QP), RS = QP + 1;
  const BaldLds<QP> l(bald_smem, a.M);
  const int64_t b = blockIdx.x / a.M;
  const int m = blockIdx.x - b * a.M;
  const int t = threadIdx.x, q = a.q;
  bald_stage<QP>(a, b, l);
  BaldEntry<QP> ent;
  const double c = 0.5 * q * LOG_2PI;
  double z[QP], y[QP], w[QP], g[QP], acc[QP];
  for (int s0 = 0; s0 < a.S; s0 += BALD_T) {
    const int s = s0 + t;
    bald_load_z<QP>(a, s, z);
#pragma unroll
    for (int i = 0; i < QP; ++i) acc[i] = 0.0;
    if (s < a.S) {
      bald_y<QP>(l.Lp + m * NT, l.mu + m * QP, z, y);
      const double lse = bald_lse<QP>(a, l, y);
      a.work[(b * a.M + m) * a.S + s] = lse;
      for (int mp = 0; mp < a.M; ++mp) {
        const double ss = bald_solve<QP>(l.Lp + mp * NT, l.inv + mp * QP, l.mu + mp * QP, y, w);
        const double pi = exp(-0.5 * ss - l.ld[mp] - c - lse);
        bald_solve_t<QP>(l.Lp + mp * NT, l.inv + mp * QP, w, g);
#pragma unroll
        for (int i = 0; i < QP; ++i) acc[i] = fma(pi, g[i], acc[i]);
      }
    }
    __syncthreads();  // (the previous chunk's entries are summed)
#pragma unroll
    for (int i = 0; i < QP; ++i) {
      l.A[t * RS + i] = acc[i];
      l.W[t * RS + i] = z[i];
    }
    l.A[t * RS + QP] = 0.0;
    l.W[t * RS + QP] = 1.0;
    __syncthreads();
    ent.add_chunk(l.A, l.W);
  }
  const double tot = ent.total(l.red);
  const double scale = bald_hscale(a, b);
  const int64_t row = (int64_t)m * a.B + b;
  if (t < QP) {
    if (t < q) a.dmean[row * q + t] = scale * tot;
  } else if (t > QP && t < ent.NE) {
    const int i = ent.ia, j = ent.jb;
    if (i < q)
      a.dL[(row * q + i) * q + j] =
          scale * tot - (i == j ? a.dout[b * a.M + m] * l.inv[m * QP + i] : 0.0);
  }
  for (int e = t; e < q * q; e += BALD_T)
    if (e % q > e / q) a.dL[row * q * q + e] = 0.0;
}

// backward, target role: adds d mu_m' and d L_m' of every sample evaluated
// under component m' onto the source launch's output
template <int QP>
__global__ __launch_bounds__(BALD_T) void bald_bwd_target_kernel(const BaldDev a) {
  extern __shared__ double bald_smem[];
  constexpr int NT = tri(QP), RS = QP + 1;
  const BaldLds<QP> l(bald_smem, a.M);
  const int64_t b = blockIdx.x / a.M;
  const int mp = blockIdx.x - b * a.M;
  const int t = threadIdx.x, q = a.q;
  bald_stage<QP>(a, b, l);
  BaldEntry<QP> ent;
  const double c = 0.5 * q * LOG_2PI + l.ld[mp];
  double z[QP], y[QP], w[QP], g[QP];
  for (int m = 0; m < a.M; ++m) {
    for (int s0 = 0; s0 < a.S; s0 += BALD_T) {
      const int s = s0 + t;
      double pi = 0.0;
#pragma unroll
      for (int i = 0; i < QP; ++i) w[i] = g[i] = 0.0;
      if (s < a.S) {
        bald_load_z<QP>(a, s, z);
        bald_y<QP>(l.Lp + m * NT, l.mu + m * QP, z, y);
        const double ss = bald_solve<QP>(l.Lp + mp * NT, l.inv + mp * QP, l.mu + mp * QP, y, w);
        pi = exp(-0.5 * ss - c - a.work[(b * a.M + m) * a.S + s]);
        bald_solve_t<QP>(l.Lp + mp * NT, l.inv + mp * QP, w, g);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < QP; ++i) {
        l.A[t * RS + i] = pi * g[i];
        l.W[t * RS + i] = w[i];
      }
      l.A[t * RS + QP] = pi;
      l.W[t * RS + QP] = 1.0;
      __syncthreads();
      ent.add_chunk(l.A, l.W);
    }
  }
  const double tot = ent.total(l.red);
  __syncthreads();
  if (t == QP) l.red[0] = tot;  // sum of pi
  __syncthreads();
  const double spi = l.red[0];
  const double scale = bald_hscale(a, b);
  const int64_t row = (int64_t)mp * a.B + b;
  if (t < QP) {
    if (t < q) a.dmean[row * q + t] -= scale * tot;
  } else if (t > QP && t < ent.NE) {
    const int i = ent.ia, j = ent.jb;
    if (i < q)
      a.dL[(row * q + i) * q + j] -= scale * (tot - (i == j ? spi * l.inv[mp * QP + i] : 0.0));
  }
}

int bald_fill(const BoBaldArgs* a, const char* who, bool grad, BaldDev* v) {
  BO_CHECK_ARG(a->M >= 1 && a->M <= BALD_MMAX, "%s: 1 <= M <= %d (got %d)", who, BALD_MMAX, a->M);
  BO_CHECK_ARG(a->q >= 1 && a->q <= BALD_QMAX, "%s: 1 <= q <= %d (got %d)", who, BALD_QMAX, a->q);
  BO_CHECK_ARG(a->S >= 1 && a->S <= BALD_SMAX, "%s: 1 <= S <= %d (got %d)", who, BALD_SMAX, a->S);
  BO_CHECK_ARG(a->B >= 1 && a->B * a->M <= 0x7fffffff, "%s: B >= 1 and B M < 2^31", who);
  BO_CHECK_ARG(a->mean && a->L && a->Z, "%s: mean, L and Z are required", who);
  const int64_t need = a->B * a->M * (grad ? (int64_t)a->S : 1);
  BO_CHECK_ARG(a->work && a->work_size >= need,
               "%s: work of at least %lld doubles is required (work_size %lld)", who,
               (long long)need, (long long)a->work_size);
  v->M = a->M;
  v->q = a->q;
  v->S = a->S;
  v->B = a->B;
  v->mean = a->mean;
  v->L = a->L;
  v->Z = a->Z;
  v->out = a->out;
  v->work = a->work;
  v->dout = a->dout;
  v->dmean = a->dmean;
  v->dL = a->dL;
  return BO_OK;
}

template <typename K>
int bald_launch(K kernel, size_t lds, const BaldDev& v, void* stream) {
  if (lds > 48 * 1024)
    BO_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kernel<<<(unsigned)(v.B * v.M), BALD_T, lds, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

template <int QP>
int bald_run(const BaldDev& v, bool grad, void* stream) {
  const size_t lds = BaldLds<QP>::bytes(v.M, grad);
  if (!grad) {
    if (int st = bald_launch(bald_fwd_kernel<QP>, lds, v, stream); st != BO_OK) return st;
    bald_finish_kernel<<<(unsigned)ceil_div(v.B * v.M, BALD_T), BALD_T, 0, as_stream(stream)>>>(v);
    BO_LAUNCH_CHECK();
    return BO_OK;
  }
  if (int st = bald_launch(bald_bwd_source_kernel<QP>, lds, v, stream); st != BO_OK) return st;
  return bald_launch(bald_bwd_target_kernel<QP>, lds, v, stream);
}

int bald_dispatch(const BaldDev& v, bool grad, void* stream) {
  if (v.q <= 1) return bald_run<1>(v, grad, stream);
  if (v.q <= 2) return bald_run<2>(v, grad, stream);
  if (v.q <= 4) return bald_run<4>(v, grad, stream);
  if (v.q <= 8) return bald_run<8>(v, grad, stream);
  return bald_run<16>(v, grad, stream);
}

}  // namespace

// The C ABI entry points (include/botorch_amd.h): bo_bald_v and
// bo_bald_backward_v behind their header checks (abi_structs.cpp).
extern "C" int bo_bald_impl(const BoBaldArgs* a, void* stream) {
  BaldDev v;
  if (int st = bald_fill(a, "bo_bald", false, &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->out, "bo_bald: out is required");
  return bald_dispatch(v, false, stream);
}

extern "C" int bo_bald_backward_impl(const BoBaldArgs* a, void* stream) {
  BaldDev v;
  if (int st = bald_fill(a, "bo_bald_backward", true, &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->dout && a->dmean && a->dL,
               "bo_bald_backward: dout, dmean and dL are required");
  return bald_dispatch(v, true, stream);
}
