// Input transforms on the device: the affine (Normalize) + Kumaraswamy (Warp)
// map of botorch/models/transforms/input.py, its backward, and the gradient of
// the exact marginal log likelihood with respect to the (transformed) training
// inputs, which the fit of a warped model contracts into the gradients of the
// two concentration vectors.
//
//   bo_input_warp      X (R x d) -> Z        v = (x - offset) rscale
//                                            warped column: u = clamp(v (1 - 2 eps) + eps, eps, 1 - eps)
//                                            t = a log u, s = log(-expm1(t)), z = -expm1(b s)
//   bo_input_warp_bwd  dZ, X -> dX, da, db   (column sums in a fixed order, two stages)
//   bo_mll_dx          d ll / d X~ (n x d)   = -(o / l_t^2) sum_{k != i} G_ik (x_it - x_kt),
//                                            G = (alpha alpha^T - A^{-1}) o g
//
// The element-wise kernels are bound by their 16 bytes per element.  A
// workgroup walks the flat R d array in steps of S elements, S the largest
// multiple of lcm(d, 2) that 256 threads x 2 elements cover: every thread then
// meets the same two columns at every step, so the column parameters live in
// its registers, every access is one aligned 16-byte load or store, and its
// four running column sums need no index.
//
// bo_mll_dx: a workgroup (4 waves) owns 64 rows and a contiguous range of 64-
// column tiles.  Per tile it stages the tile of A^{-1} (only the lower tiles
// hold data: a tile above the diagonal is read as its mirror tile, and one of
// the two orientations is transposed on its way into LDS), the lengthscale-
// scaled rows [X~ | 1] of the tile and alpha.  Lane (i = l & 15, k = l >> 4) of
// a wave forms G_ik in registers -- exactly the A fragment of
// v_mfma_f64_16x16x4 -- and the wave contracts G [X~ | 1] on the matrix cores
// (FORM 0), or accumulates G_ik (x_k - x_i) with the differences it already
// holds (FORM 1).  Column ranges are partials in a fixed order; a second small
// kernel folds them.  No atomics anywhere.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAXD = 64;

// ---- the element-wise transform -----------------------------------------------------------------

struct WarpCol {
  double off, rs, a, b;
  bool warped;
};

__device__ __forceinline__ WarpCol warp_col(const BoInputWarpArgs& p, int c) {
  WarpCol w;
  w.off = p.offset[c];
  w.rs = p.rscale[c];
  w.warped = (p.warped_mask >> c) & 1;
  w.a = w.warped ? p.conc1[c] : 1.0;
  w.b = w.warped ? p.conc0[c] : 1.0;
  return w;
}

__device__ __forceinline__ double warp_fwd(const WarpCol& w, double x, double eps) {
  const double v = (x - w.off) * w.rs;
  const double u = fmin(fmax(fma(v, 1.0 - 2.0 * eps, eps), eps), 1.0 - eps);
  const double s = log(-expm1(w.a * log(u)));
  const double z = -expm1(w.b * s);
  return w.warped ? z : v;
}

// dz/dx and the two concentration derivatives at one element
__device__ __forceinline__ void warp_bwd(const WarpCol& w, double x, double eps, double g,
                                         double& dx, double& da, double& db) {
  const double v = (x - w.off) * w.rs;
  const double raw = fma(v, 1.0 - 2.0 * eps, eps);
  const double u = fmin(fmax(raw, eps), 1.0 - eps);
  const double pass = (raw >= eps && raw <= 1.0 - eps) ? (1.0 - 2.0 * eps) : 0.0;  // torch.clamp
  const double lu = log(u);
  const double t = w.a * lu;
  const double s = log(-expm1(t));
  const double bm1s = (w.b - 1.0) * s;
  const double dzdu = w.a * w.b * exp(fma(w.a - 1.0, lu, bm1s));
  const double dzda = w.b * lu * exp(t + bm1s);
  const double dzdb = -s * exp(w.b * s);
  dx = g * w.rs * (w.warped ? dzdu * pass : 1.0);
  da = w.warped ? g * dzda : 0.0;
  db = w.warped ? g * dzdb : 0.0;
}

// S: elements of one workgroup step (a multiple of d and of 2, <= 2 THREADS)
__host__ __device__ inline int warp_step(int d) {
  const int l = (d & 1) ? 2 * d : d;
  return (2 * THREADS / l) * l;
}

template <bool BWD>
__global__ __launch_bounds__(THREADS) void input_warp_kernel(BoInputWarpArgs p, int S, int ipw) {
  __shared__ double red[2][2 * THREADS];
  const int tid = threadIdx.x;
  const int64_t N = p.R * p.d;
  const bool active = 2 * tid < S;
  const int c0 = (2 * tid) % p.d, c1 = (2 * tid + 1) % p.d;
  const WarpCol w0 = warp_col(p, c0), w1 = warp_col(p, c1);
  double sa0 = 0.0, sb0 = 0.0, sa1 = 0.0, sb1 = 0.0;
  for (int it = 0; it < ipw; ++it) {
    const int64_t e = ((int64_t)blockIdx.x * ipw + it) * S + 2 * tid;
    if (!active || e >= N) continue;
    const bool pair = e + 1 < N;  // R d odd: the last element stands alone
    double2 x;
    if (pair) x = *reinterpret_cast<const double2*>(p.X + e);
    else x = make_double2(p.X[e], 0.5);
    if (!BWD) {
      const double z0 = warp_fwd(w0, x.x, p.eps), z1 = warp_fwd(w1, x.y, p.eps);
      if (pair) *reinterpret_cast<double2*>(p.Z + e) = make_double2(z0, z1);
      else p.Z[e] = z0;
    } else {
      double2 g;
      if (pair) g = *reinterpret_cast<const double2*>(p.dZ + e);
      else g = make_double2(p.dZ[e], 0.0);
      double dx0, dx1, da, db;
      warp_bwd(w0, x.x, p.eps, g.x, dx0, da, db);
      sa0 += da;
      sb0 += db;
      warp_bwd(w1, x.y, p.eps, g.y, dx1, da, db);
      sa1 += da;
      sb1 += db;
      if (pair) *reinterpret_cast<double2*>(p.dX + e) = make_double2(dx0, dx1);
      else p.dX[e] = dx0;
    }
  }
  if (BWD) {
    // slot j = 2 tid + h of the step holds column j % d: thread c folds its column's slots
    red[0][2 * tid] = sa0;
    red[1][2 * tid] = sb0;
    red[0][2 * tid + 1] = sa1;
    red[1][2 * tid + 1] = sb1;
    __syncthreads();
    if (tid < 2 * p.d) {
      const int c = tid % p.d, which = tid / p.d;
      double v = 0.0;
      for (int j = c; j < S; j += p.d) v += red[which][j];
      p.work[((int64_t)blockIdx.x * 2 + which) * p.d + c] = v;
    }
  }
}

__global__ void input_warp_fold_kernel(const double* __restrict__ work, int G, int d,
                                       double* __restrict__ da, double* __restrict__ db) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * d) return;
  const int c = t % d, which = t / d;
  double v = 0.0;
  for (int g = 0; g < G; ++g) v += work[((int64_t)g * 2 + which) * d + c];
  (which ? db : da)[c] = v;
}

// workgroups and steps per workgroup of a call
inline void warp_plan(int64_t R, int d, int& S, int& G, int& ipw) {
  S = warp_step(d);
  const int64_t steps = ceil_div(R * d, S);
  ipw = (int)ceil_div(steps, 256);
  if (ipw < 1) ipw = 1;
  G = (int)ceil_div(steps, ipw);
  if (G < 1) G = 1;
}

int input_warp_check(const BoInputWarpArgs* a, const char* who) {
  BO_CHECK_ARG(a->d >= 1 && a->d <= MAXD, "%s: d=%d (1..%d)", who, a->d, MAXD);
  BO_CHECK_ARG(a->R >= 0 && a->R * a->d < ((int64_t)1 << 40), "%s: R=%lld", who, (long long)a->R);
  BO_CHECK_ARG(a->X && a->offset && a->rscale, "%s: null X, offset or rscale", who);
  BO_CHECK_ARG(a->warped_mask == 0 || (a->conc1 && a->conc0), "%s: null concentrations", who);
  BO_CHECK_ARG(a->d == 64 || (a->warped_mask >> a->d) == 0, "%s: warped_mask beyond d", who);
  BO_CHECK_ARG(a->eps > 0.0 && a->eps < 0.5, "%s: eps=%g", who, a->eps);
  BO_CHECK_ARG(((uintptr_t)a->X & 15) == 0, "%s: X is not 16-byte aligned", who);
  return BO_OK;
}

// ---- d ll / d X~ ----------------------------------------------------------------------------------

constexpr int TILE = 64;
constexpr int LDT = TILE + 1;  // A^{-1} tile, k-major: T[k][i]

template <int DR>
struct DxDims {
  // 16-column blocks of [X~ | 1]: d + 1 <= DR columns below DR = 64 (d < DR), 65 at DR = 64
  static constexpr int NB = DR == 64 ? 5 : (DR < 16 ? 1 : DR / 16);
  static constexpr int LDB = NB * 16 + 2;   // row pitch of the staged rows (even: 16-byte reads)
};

template <int KIND, int DR, int FORM>
__global__ __launch_bounds__(THREADS) void mll_dx_kernel(BoMllDxArgs p, int tiles, int tpw) {
  constexpr int NB = DxDims<DR>::NB, LDB = DxDims<DR>::LDB;
  __shared__ double sT[TILE * LDT];
  __shared__ __attribute__((aligned(16))) double sB[TILE * LDB];
  __shared__ double sAl[TILE];
  __shared__ double sl[MAXD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = p.d;
  const int64_t n = p.n, ld = p.ld;
  const int rb = blockIdx.x, cs = blockIdx.y;
  if (tid < MAXD) sl[tid] = tid < d ? 1.0 / p.lengthscale[tid] : 0.0;
  __syncthreads();
  // this lane's row, scaled, slot d = 1 like the staged rows (the slot's difference is 0)
  const int il = wave * 16 + (lane & 15);
  const int64_t gi = (int64_t)rb * TILE + il;
  const bool irow = gi < n;
  double xi[DR];
#pragma unroll
  for (int t = 0; t < DR; ++t) xi[t] = (irow && t < d) ? p.X[gi * d + t] * sl[t] : (t == d ? 1.0 : 0.0);
  const double ai = irow ? p.alpha[gi] : 0.0;
  v4d acc[NB];
  double facc[FORM == 1 ? DR : 1];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = v4d_zero();
#pragma unroll
  for (int t = 0; t < (FORM == 1 ? DR : 1); ++t) facc[t] = 0.0;

  const int cb0 = cs * tpw, cb1 = min(tiles, cb0 + tpw);
  for (int cb = cb0; cb < cb1; ++cb) {
    __syncthreads();
    // A^{-1} tile (rb, cb) as T[k][i]; above the diagonal its mirror (cb, rb) holds the data
    {
      const bool direct = cb <= rb;
      const double* src = p.Ainv + (direct ? ((int64_t)rb * TILE * ld + (int64_t)cb * TILE)
                                           : ((int64_t)cb * TILE * ld + (int64_t)rb * TILE));
      for (int e = tid; e < TILE * TILE / 2; e += THREADS) {
        const int r = e / (TILE / 2), c = 2 * (e % (TILE / 2));
        const double2 v = *reinterpret_cast<const double2*>(src + (int64_t)r * ld + c);
        if (direct) {  // r = i, c = k
          sT[c * LDT + r] = v.x;
          sT[(c + 1) * LDT + r] = v.y;
        } else {       // r = k, c = i
          sT[r * LDT + c] = v.x;
          sT[r * LDT + c + 1] = v.y;
        }
      }
      for (int e = tid; e < TILE * LDB; e += THREADS) {
        const int r = e / LDB, c = e % LDB;
        const int64_t gk = (int64_t)cb * TILE + r;
        double v = 0.0;
        if (gk < n) v = c < d ? p.X[gk * d + c] * sl[c] : (c == d ? 1.0 : 0.0);
        sB[e] = v;
      }
      if (tid < TILE) {
        const int64_t gk = (int64_t)cb * TILE + tid;
        sAl[tid] = gk < n ? p.alpha[gk] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < TILE / 4; ++ks) {
      const int kl = ks * 4 + (lane >> 4);
      const int64_t gk = (int64_t)cb * TILE + kl;
      const double* xk = sB + kl * LDB;
      double df[DR];
      double r2 = 0.0;
#pragma unroll
      for (int t = 0; t < DR; t += 2) {
        const double2 v = *reinterpret_cast<const double2*>(xk + t);
        df[t] = v.x - xi[t];
        df[t + 1] = v.y - xi[t + 1];
        r2 = fma(df[t], df[t], r2);
        r2 = fma(df[t + 1], df[t + 1], r2);
      }
      double g;
      if (KIND == BO_RBF) {
        g = exp(-0.5 * r2);
      } else {
        const double s5r = 2.23606797749978969641 * sqrt(r2);
        g = (5.0 / 3.0) * (1.0 + s5r) * exp(-s5r);
      }
      const double W = ai * sAl[kl] - sT[kl * LDT + il];
      const double G = (irow && gk < n && gk != gi) ? W * g : 0.0;
      if (FORM == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = mfma_f64(G, xk[b * 16 + (lane & 15)], acc[b]);
      } else {
#pragma unroll
        for (int t = 0; t < DR; ++t) facc[t] = fma(G, df[t], facc[t]);
      }
    }
  }
  // partial[cs][i][0..d]: FORM 0 (G X~s)_it and, in slot d, sum_k G_ik; FORM 1 sum_k G_ik (xs_kt - xs_it)
  double* out = p.work + (int64_t)cs * n * (d + 1);
  if (FORM == 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = (int64_t)rb * TILE + wave * 16 + mfma_row(lane, r);
        const int col = b * 16 + mfma_col(lane);
        if (row < n && col <= d) out[row * (d + 1) + col] = acc[b][r];
      }
  } else {
#pragma unroll
    for (int t = 0; t < DR; ++t) {
      double v = facc[t];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (irow && lane < 16 && t <= d) out[gi * (d + 1) + t] = v;
    }
  }
}

// dX[i][t] from the column-range partials, folded in their order
template <int FORM>
__global__ void mll_dx_fold_kernel(BoMllDxArgs p, int CS) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int d = p.d;
  if (e >= p.n * d) return;
  const int64_t i = e / d;
  const int t = (int)(e % d);
  const int64_t stride = p.n * (d + 1);
  double v = 0.0, S = 0.0;
  for (int c = 0; c < CS; ++c) {
    v += p.work[c * stride + i * (d + 1) + t];
    if (FORM == 0) S += p.work[c * stride + i * (d + 1) + d];
  }
  const double s = 1.0 / p.lengthscale[t];
  if (FORM == 0) p.dX[e] = -(p.outputscale * s) * fma(p.X[e] * s, S, -v);
  else p.dX[e] = (p.outputscale * s) * v;
}

inline void dx_plan(int64_t n, int& tiles, int& CS, int& tpw) {
  tiles = (int)ceil_div(n, TILE);
  CS = (int)ceil_div(512, tiles);
  if (CS > tiles) CS = tiles;
  tpw = (int)ceil_div(tiles, CS);
  CS = (int)ceil_div(tiles, tpw);
}

template <int KIND, int FORM>
void dx_launch(const BoMllDxArgs& a, int tiles, int CS, int tpw, hipStream_t st) {
  const dim3 grid((unsigned)tiles, (unsigned)CS);
  if (a.d < 8) mll_dx_kernel<KIND, 8, FORM><<<grid, THREADS, 0, st>>>(a, tiles, tpw);
  else if (a.d < 16) mll_dx_kernel<KIND, 16, FORM><<<grid, THREADS, 0, st>>>(a, tiles, tpw);
  else if (a.d < 32) mll_dx_kernel<KIND, 32, FORM><<<grid, THREADS, 0, st>>>(a, tiles, tpw);
  else if (FORM == 0) mll_dx_kernel<KIND, 64, 0><<<grid, THREADS, 0, st>>>(a, tiles, tpw);
}  // FORM 1 at d >= 32 is refused by the entry point: its 3 x 64 fp64 registers per lane would spill

}  // namespace

extern "C" int bo_input_warp_work(int64_t R, int d, int64_t* elems) {
  BO_CHECK_ARG(d >= 1 && d <= MAXD && R >= 0 && elems, "bo_input_warp_work: R=%lld d=%d",
               (long long)R, d);
  int S, G, ipw;
  warp_plan(R, d, S, G, ipw);
  *elems = (int64_t)G * 2 * d;
  return BO_OK;
}

extern "C" int bo_input_warp_impl(const BoInputWarpArgs* a, void* stream) {
  if (int rc = input_warp_check(a, "bo_input_warp")) return rc;
  BO_CHECK_ARG(a->Z && ((uintptr_t)a->Z & 15) == 0, "bo_input_warp: Z null or not 16-byte aligned");
  if (a->R == 0) return BO_OK;
  int S, G, ipw;
  warp_plan(a->R, a->d, S, G, ipw);
  input_warp_kernel<false><<<G, THREADS, 0, as_stream(stream)>>>(*a, S, ipw);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_input_warp_bwd_impl(const BoInputWarpArgs* a, void* stream) {
  if (int rc = input_warp_check(a, "bo_input_warp_bwd")) return rc;
  BO_CHECK_ARG(a->dZ && a->dX && a->da && a->db, "bo_input_warp_bwd: null dZ, dX, da or db");
  BO_CHECK_ARG((((uintptr_t)a->dZ | (uintptr_t)a->dX) & 15) == 0,
               "bo_input_warp_bwd: dZ or dX not 16-byte aligned");
  int S, G, ipw;
  warp_plan(a->R, a->d, S, G, ipw);
  BO_CHECK_ARG(a->work && a->work_size >= (int64_t)G * 2 * a->d,
               "bo_input_warp_bwd: work holds %lld doubles, %lld needed", (long long)a->work_size,
               (long long)G * 2 * a->d);
  hipStream_t st = as_stream(stream);
  if (a->R == 0) G = 0;
  else input_warp_kernel<true><<<G, THREADS, 0, st>>>(*a, S, ipw);
  input_warp_fold_kernel<<<1, 2 * MAXD, 0, st>>>(a->work, G, a->d, a->da, a->db);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_mll_dx_work(int64_t n, int d, int64_t* elems) {
  BO_CHECK_ARG(d >= 1 && d <= MAXD && n >= 1 && elems, "bo_mll_dx_work: n=%lld d=%d",
               (long long)n, d);
  int tiles, CS, tpw;
  dx_plan(n, tiles, CS, tpw);
  *elems = (int64_t)CS * n * (d + 1);
  return BO_OK;
}

extern "C" int bo_mll_dx_impl(const BoMllDxArgs* a, void* stream) {
  BO_CHECK_ARG(a->d >= 1 && a->d <= MAXD, "bo_mll_dx: d=%d (1..%d)", a->d, MAXD);
  BO_CHECK_ARG(a->kind == BO_RBF || a->kind == BO_MATERN52, "bo_mll_dx: kind=%d", a->kind);
  BO_CHECK_ARG(a->form == 0 || (a->form == 1 && a->d < 32), "bo_mll_dx: form=%d at d=%d (form 1: d < 32)",
               a->form, a->d);
  BO_CHECK_ARG(a->n >= 1 && a->n < ((int64_t)1 << 24), "bo_mll_dx: n=%lld", (long long)a->n);
  int tiles, CS, tpw;
  dx_plan(a->n, tiles, CS, tpw);
  BO_CHECK_ARG(a->ld >= (int64_t)tiles * TILE && (a->ld & 1) == 0,
               "bo_mll_dx: ld=%lld for n=%lld (A^{-1} is read in whole 64 x 64 tiles)",
               (long long)a->ld, (long long)a->n);
  BO_CHECK_ARG(a->X && a->lengthscale && a->Ainv && a->alpha && a->dX, "bo_mll_dx: null operand");
  BO_CHECK_ARG(((uintptr_t)a->Ainv & 15) == 0, "bo_mll_dx: Ainv is not 16-byte aligned");
  BO_CHECK_ARG(a->work && a->work_size >= (int64_t)CS * a->n * (a->d + 1),
               "bo_mll_dx: work holds %lld doubles, %lld needed", (long long)a->work_size,
               (long long)CS * a->n * (a->d + 1));
  hipStream_t st = as_stream(stream);
  if (a->kind == BO_RBF) {
    if (a->form == 0) dx_launch<BO_RBF, 0>(*a, tiles, CS, tpw, st);
    else dx_launch<BO_RBF, 1>(*a, tiles, CS, tpw, st);
  } else {
    if (a->form == 0) dx_launch<BO_MATERN52, 0>(*a, tiles, CS, tpw, st);
    else dx_launch<BO_MATERN52, 1>(*a, tiles, CS, tpw, st);
  }
  const int64_t ne = a->n * a->d;
  if (a->form == 0) mll_dx_fold_kernel<0><<<(unsigned)ceil_div(ne, 256), 256, 0, st>>>(*a, CS);
  else mll_dx_fold_kernel<1><<<(unsigned)ceil_div(ne, 256), 256, 0, st>>>(*a, CS);
  BO_LAUNCH_CHECK();
  return BO_OK;
}
