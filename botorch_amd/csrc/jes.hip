// qJointEntropySearch, lower bound (botorch/acquisition/joint_entropy_search.py:
// 195-265): the mean over the P optima of the conditional entropies of R points
// in one launch.  Conditioning the GP on one pair (x*_j, f*_j) is a rank-one
// correction of the current posterior, so everything model j says about row i
// follows from the posterior covariance of x_i and x*_j.  With k the kernel
// without its outputscale o and V[j] = A^{-1} o k(Xt, x*_j):
//
//   c_ij   = o k(x_i, x*_j) - o sum_t k(x_i, Xt_t) V[j][t]
//   mu_ji  = mu_i + c_ij g_j          s2_ji = max(var_i - c_ij^2 sinv_j, 1e-10)
//   z      = (wf_j - w mu_ji) / sqrt(s2_ji)
//   r      = phi(z) / max(Phi(z), 1e-8),  Phi(z) = erfc(-z / sqrt 2) / 2
//   vt_ji  = s2_ji max(1 - (z + r) r, 1e-8) + tau2_j
//   H[i]   = (1 / P) sum_j log(vt_ji) / 2
//
// Tile plan (the row tile and its lane layout: rowtile.h).  A wave owns 16 rows
// of X; a lane's kernel value against a training point is its own B element,
// with V as the A operand: D[optimum][row] += V[optimum][t] k[t][row].  The
// accumulator leaves lane l with the optima (l >> 4) + 4 r of its own row, so the
// k(x_i, x*_j) term and the whole elementwise chain run on it in registers.  A
// pass covers up to 64 optima (four 16-optimum tiles, the tail tile padded with
// zeros); the sum over j runs in a fixed order per lane, over the passes, and is
// folded over the four slots by two lane exchanges.  No R x P array, no atomics,
// no workspace: repeated calls are bitwise identical.
//
// Backward, one launch: per pass the tile's c_ij is recomputed as above, the
// chain's derivative G_ij = d(sum_i H[i] dout[i]) / dc_ij goes to the wave's LDS
// (64 x 16) and, straight from the registers, through dk(x_i, x*_j) into dX;
// then the training points are swept again: coef[t][row] = sum_j V[j][t]
// G[j][row] (MFMA over j in steps of 4) times dk/dd2 is the lane's A element of
// dX[row][:] -= q[row][t] Xt[t][:] (with sum_t q x added at the end) -- the two
// contractions of paths.hip's backward with G in the place of dout.  dmu and
// dvar are the row sums of the chain's other two derivatives.
#include "normal.h"
#include "rowtile.h"

namespace {

constexpr int THREADS = 256;
constexpr int TR = ROWTILE;  // rows of X per wave
constexpr int NT = 4;        // 16-optimum tiles per pass
constexpr int PB = 16 * NT;
constexpr double S2_FLOOR = 1e-10, PHI_FLOOR = 1e-8, INNER_FLOOR = 1e-8;

struct Dev {
  int kind, d, P;
  int64_t R, n;
  const double *X, *ls, *Xts, *Xo, *V, *g, *sinv, *wf, *tau2, *mu, *var;
  double o, w;
  double* out;
  const double* dout;
  double *dX, *dmu, *dvar;
};

// acc[q][r] = sum_t V[jb + 16 q + (l >> 4) + 4 r][t] k(x_row, Xt_t) for the nt
// tiles of the pass at jb (nt is uniform over the workgroup)
template <int KIND>
__device__ __forceinline__ void contract_v(const Dev& a, const double* xr, int jb, int nt, int row,
                                           int kk, v4d* acc) {
  int64_t vrow[NT];  // the A operand's row: optimum jb + 16 q + row, or -1
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    const int j = jb + 16 * q + row;
    vrow[q] = q < nt && j < a.P ? j : -1;
    acc[q] = v4d_zero();
  }
  for (int64_t i0 = 0; i0 < a.n; i0 += 16) {
    const int64_t ib = i0 + 4 * kk;
    const double* xt[4];
    double d2[4];
    rowtile_dist2x4<1>(xr, a.Xts, ib, a.n, a.d, xt, d2);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t i = ib + m;
      const bool ok = i < a.n;
      const double kv = ok ? kernel_from_d2<KIND>(d2[m]) : 0.0;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        if (q < nt) {
          const double v = ok && vrow[q] >= 0 ? a.V[vrow[q] * a.n + i] : 0.0;
          acc[q] = mfma_f64(v, kv, acc[q]);
        }
      }
    }
  }
}

struct Chain {
  double h;                // log(vt) / 2
  double dc, dmu, dvar;    // dh / d(c, mu_i, var_i)
};

// the elementwise chain at one (row, optimum) pair; GRAD: its derivatives too
template <bool GRAD>
__device__ __forceinline__ Chain chain(double c, double mu, double var, double g, double sinv,
                                       double wf, double tau2, double w) {
  Chain o;
  const double s2u = var - c * c * sinv;
  const bool s2_free = s2u > S2_FLOOR;
  const double s2 = s2_free ? s2u : S2_FLOOR;
  const double rs = 1.0 / sqrt(s2);
  const double z = (wf - w * (mu + c * g)) * rs;
  const double Pz = Phi(z);
  const bool phi_free = Pz > PHI_FLOOR;
  const double r = phi(z) / (phi_free ? Pz : PHI_FLOOR);
  const double inu = 1.0 - (z + r) * r;
  const bool in_free = inu > INNER_FLOOR;
  const double inner = in_free ? inu : INNER_FLOOR;
  const double vt = s2 * inner + tau2;
  o.h = 0.5 * log(vt);
  if (GRAD) {
    const double e = 0.5 / vt;
    // r' = -r (z + r), or -z r on the floor of Phi; d inner / dz = -(r + r' (z + 2 r))
    const double rp = phi_free ? -r * (z + r) : -z * r;
    const double diz = in_free ? -(r + rp * (z + 2.0 * r)) : 0.0;
    // vt = s2 inner(z) + tau2,  z = (wf - w mu_j) / sqrt(s2)
    const double bs2 = s2_free ? e * (inner - 0.5 * z * diz) : 0.0;
    const double bmu = -e * s2 * diz * w * rs;
    o.dmu = bmu;
    o.dvar = bs2;
    o.dc = bmu * g - 2.0 * bs2 * c * sinv;
  } else {
    o.dc = o.dmu = o.dvar = 0.0;
  }
  return o;
}

template <int KIND>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(2))) void
jes_forward_kernel(const Dev a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int d = a.d, ldx = d | 1;
  double* xs = smem + wave * TR * ldx;
  const int64_t r0 = ((int64_t)blockIdx.x * nw + wave) * TR;
  rowtile_load(a.X, a.ls, r0, TR, a.R, d, ldx, xs, lane, BO_WAVE);
  __syncthreads();
  if (r0 >= a.R) return;  // (wave-uniform, and no barrier follows)
  const int row = lane & 15, kk = lane >> 4;
  const double* xr = xs + row * ldx;
  const bool rok = r0 + row < a.R;
  const double mu = rok ? a.mu[r0 + row] : 0.0, var = rok ? a.var[r0 + row] : 1.0;
  double hs = 0.0;
  for (int jb = 0; jb < a.P; jb += PB) {
    const int nt = min(NT, (a.P - jb + 15) >> 4);
    v4d acc[NT];
    contract_v<KIND>(a, xr, jb, nt, row, kk, acc);
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      if (q < nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = jb + 16 * q + mfma_row(lane, r);
          if (j < a.P) {
            const double kx = kernel_from_d2<KIND>(rowtile_dist2(xr, a.Xo + (int64_t)j * d, d));
            const double c = a.o * (kx - acc[q][r]);
            hs += chain<false>(c, mu, var, a.g[j], a.sinv[j], a.wf[j], a.tau2[j], a.w).h;
          }
        }
      }
    }
  }
  hs = rowtile_fold4(hs);
  if (kk == 0 && rok) a.out[r0 + row] = hs / a.P;
}

// NDT: 16-column tiles of dX (d <= 16 NDT); two waves per SIMD up to NDT = 4
// (at 8 the 64 accumulator registers of dX would spill under that budget)
template <int KIND, int NDT>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(NDT <= 4 ? 2 : 1))) void
jes_backward_kernel(const Dev a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int d = a.d, ldx = d | 1;
  double* xs = smem + wave * (TR * ldx + PB * TR);
  double* gs = xs + TR * ldx;  // G[optimum of the pass][row], the wave's own
  const int64_t r0 = ((int64_t)blockIdx.x * nw + wave) * TR;
  rowtile_load(a.X, a.ls, r0, TR, a.R, d, ldx, xs, lane, BO_WAVE);
  __syncthreads();
  // (every wave stays for the barriers below; rows past R are computed on
  // zeros and never written)
  const int row = lane & 15, kk = lane >> 4;
  const double* xr = xs + row * ldx;
  const bool rok = r0 + row < a.R;
  const double mu = rok ? a.mu[r0 + row] : 0.0, var = rok ? a.var[r0 + row] : 1.0;
  const double dh = rok ? a.dout[r0 + row] / a.P : 0.0;

  v4d accd[NDT];  // dX[row = (l >> 4) + 4 r][t = 16 tt + (l & 15)], scaled coordinates
#pragma unroll
  for (int tt = 0; tt < NDT; ++tt) accd[tt] = v4d_zero();
  double sumq = 0.0, smu = 0.0, svar = 0.0;

  for (int jb = 0; jb < a.P; jb += PB) {
    const int nt = min(NT, (a.P - jb + 15) >> 4);
    const int pend = min(a.P, jb + 16 * nt);
    {
      v4d acc[NT];
      contract_v<KIND>(a, xr, jb, nt, row, kk, acc);
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        if (q < nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int jl = 16 * q + mfma_row(lane, r), j = jb + jl;
            const bool ok = j < a.P;
            const double* xo = a.Xo + (int64_t)(ok ? j : 0) * d;
            const double d2 = rowtile_dist2(xr, xo, d);
            double G = 0.0;
            if (ok) {
              const double c = a.o * (kernel_from_d2<KIND>(d2) - acc[q][r]);
              const Chain ch =
                  chain<true>(c, mu, var, a.g[j], a.sinv[j], a.wf[j], a.tau2[j], a.w);
              G = dh * ch.dc;
              smu = fma(dh, ch.dmu, smu);
              svar = fma(dh, ch.dvar, svar);
            }
            gs[jl * TR + row] = G;
            // the direct term: dX[row] += G dk(x_row, x*_j)
            const double qd = G * dkernel_factor<KIND>(d2, a.o);
            sumq += qd;
            rowtile_dx_acc<NDT>(qd, ok, xo, d, row, accd);
          }
        }
      }
    }
    __syncthreads();
    // ---- the training points: coef[t][row] = -sum_j V[j][t] G[j][row] -----------
    for (int64_t i0 = 0; i0 < a.n; i0 += 16) {
      v4d cf = v4d_zero();
      const int64_t ia = i0 + row;  // A[i = l & 15][k = l >> 4] = V[j][i0 + i]
      for (int j0 = jb; j0 < pend; j0 += 4) {
        const int j = j0 + kk;
        const double v = j < a.P && ia < a.n ? a.V[(int64_t)j * a.n + ia] : 0.0;
        const double gg = j < pend ? gs[(j - jb) * TR + row] : 0.0;
        cf = mfma_f64(v, gg, cf);
      }
      const double* xt[4];
      double d2[4];
      rowtile_dist2x4<4>(xr, a.Xts, i0 + kk, a.n, d, xt, d2);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = i0 + kk + 4 * r < a.n;
        const double q = ok ? -cf[r] * dkernel_factor<KIND>(d2[r], a.o) : 0.0;
        sumq += q;
        rowtile_dx_acc<NDT>(q, ok, xt[r], d, row, accd);
      }
    }
    __syncthreads();  // gs is rewritten by the next pass
  }
  smu = rowtile_fold4(smu);
  svar = rowtile_fold4(svar);
  if (kk == 0 && rok) {
    a.dmu[r0 + row] = smu;
    a.dvar[r0 + row] = svar;
  }
  rowtile_dx_store<NDT>(a.dX, accd, xs, ldx, rowtile_fold4(sumq), 1.0, a.ls, r0, a.R, d, lane);
}

int fill(const BoJesArgs* a, const char* who, Dev* v) {
  if (int st = rowtile_check_common(a->kind, a->d, a->n, a->Xt_scaled, a->V, a->outputscale, who);
      st != BO_OK)
    return st;
  BO_CHECK_ARG(a->P >= 1, "%s: P >= 1 (got %d)", who, a->P);
  BO_CHECK_ARG(a->R >= 1 && a->n >= 0, "%s: R >= 1, n >= 0", who);
  BO_CHECK_ARG(a->R < (int64_t(1) << 34), "%s: R too large", who);
  BO_CHECK_ARG(a->X && a->lengthscale && a->Xopt_scaled, "%s: X, lengthscale and Xopt_scaled are "
               "required", who);
  BO_CHECK_ARG(a->g && a->sinv && a->wf && a->tau2, "%s: g, sinv, wf and tau2 are required", who);
  BO_CHECK_ARG(a->mu && a->var, "%s: mu and var are required", who);
  BO_CHECK_ARG(a->w == 1.0 || a->w == -1.0, "%s: w must be +1 or -1", who);
  v->kind = a->kind;
  v->d = a->d;
  v->P = a->P;
  v->R = a->R;
  v->n = a->n;
  v->X = a->X;
  v->ls = a->lengthscale;
  v->Xts = a->Xt_scaled;
  v->Xo = a->Xopt_scaled;
  v->V = a->V;
  v->g = a->g;
  v->sinv = a->sinv;
  v->wf = a->wf;
  v->tau2 = a->tau2;
  v->mu = a->mu;
  v->var = a->var;
  v->o = a->outputscale;
  v->w = a->w;
  v->out = a->out;
  v->dout = a->dout;
  v->dX = a->dX;
  v->dmu = a->dmu;
  v->dvar = a->dvar;
  return BO_OK;
}

}  // namespace

// bo_jes_v / bo_jes_backward_v behind their header checks (abi_structs.cpp).
extern "C" int bo_jes_impl(const BoJesArgs* a, void* stream) {
  Dev v;
  if (int st = fill(a, "bo_jes", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->out, "bo_jes: out is required");
  const int nw = v.d > 64 ? 2 : 4;
  const unsigned blocks = (unsigned)ceil_div(v.R, (int64_t)nw * TR);
  const size_t lds = sizeof(double) * (size_t)nw * TR * (v.d | 1);
  if (v.kind == BO_RBF)
    jes_forward_kernel<BO_RBF><<<blocks, nw * BO_WAVE, lds, as_stream(stream)>>>(v);
  else
    jes_forward_kernel<BO_MATERN52><<<blocks, nw * BO_WAVE, lds, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_jes_backward_impl(const BoJesArgs* a, void* stream) {
  Dev v;
  if (int st = fill(a, "bo_jes_backward", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->dout && a->dX && a->dmu && a->dvar,
               "bo_jes_backward: dout, dX, dmu and dvar are required");
  // rows + G per wave: at most 48.5 KiB of LDS per workgroup
  const int nw = v.d > 32 ? 2 : 4;
  const unsigned blocks = (unsigned)ceil_div(v.R, (int64_t)nw * TR);
  const size_t lds = sizeof(double) * (size_t)nw * (TR * (v.d | 1) + PB * TR);
#define BO_JES(KIND, NDT) \
  jes_backward_kernel<KIND, NDT><<<blocks, nw * BO_WAVE, lds, as_stream(stream)>>>(v)
  ROWTILE_DISPATCH(v.kind, v.d, BO_JES);
#undef BO_JES
  BO_LAUNCH_CHECK();
  return BO_OK;
}
