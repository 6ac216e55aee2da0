// Pathwise posterior samples (Matheron paths) of an exact GP, evaluated at R
// points in one launch (botorch/sampling/pathwise: features/generators.py:66-193,
// prior_samplers.py:52-106, update_strategies.py:72-135, posterior_samplers.py:
// 198-224).  With theta_j(x) = sum_t Omega[j][t] x_t / l_t, H = M / 2:
//
//   g_s(x) = c + sqrt(2 o / M) sum_{j<H} (W[s][j] sin theta_j + W[s][H+j] cos theta_j)
//              + sum_{i<n} V[s][i] o k(x, Xt_i)
//   f_s(x) = ymean + ystd g_s(x)
//
//   all    (inner = 0): out[s][r] = f_s(X_r)                  out: S x R
//   mapped (inner >= 1): out[r]   = f_p(X_r), p = (r / inner) % S
//   backward: dX[r][t] = sum_s dout[s][r] df_s/dx_t(X_r) over the paths of row r
//
// Tile plan (the row tile and its lane layout: rowtile.h).  A wave owns 16 rows
// of X for the whole feature range; a workgroup is 4 such waves (2 when d > 64,
// for the LDS), and the grid is plain tiles of rows.  A lane's number per
// feature is sincos of the phase (a runtime loop over d, like the squared
// distance), or the kernel value: the sin / cos features and the kernel row
// never leave the registers.
//   forward, all:  D[s][row] += W[s][k] feat[k][row]   (A = W, B = features),
//                  16 features per step, a lane's four at 4 (l >> 4) + m so
//                  that its W elements are 32 contiguous bytes; S in tiles of
//                  16 paths, NT tiles per workgroup, blockIdx.y beyond
//   forward, mapped: the lane's products with W[p(row)] summed on the VALU, the
//                  four feature slots of a row folded by two lane exchanges
//   backward:      coef[k][row] = sum_s W[s][k] dout[s][row] (MFMA over s in
//                  steps of 4; mapped: one product), which lands as the lane's
//                  features (l >> 4) + 4 r; q = coef * dfeature/dtheta is again
//                  the lane's own A element of dX[row][t] += q[row][k] Omega[k][t]
//                  (resp. -q Xt_scaled[k][t], with sum_k q x_t added at the end).
// No atomics and a fixed order of every sum: bitwise reproducible.  No global
// workspace at all.
#include "rowtile.h"

namespace {

constexpr int THREADS = 256;
constexpr int TR = ROWTILE;  // rows of X per wave

struct Dev {
  int kind, d, S, H;
  int64_t R, n, inner;
  const double *X, *ls, *Xts, *Om, *W, *V;
  double o, c, ymean, ystd, pscale;
  double* out;
  const double* dout;
  double* dX;
};

// NT: 16-path tiles per workgroup (all mode); MAPPED: one path per row
template <int KIND, int NT, bool MAPPED>
__global__ __launch_bounds__(THREADS) void paths_forward_kernel(const Dev a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int d = a.d, H = a.H, M = 2 * a.H, ldx = d | 1;
  double* xs = smem + wave * TR * ldx;
  const int64_t r0 = ((int64_t)blockIdx.x * nw + wave) * TR;
  rowtile_load(a.X, a.ls, r0, TR, a.R, d, ldx, xs, lane, BO_WAVE);
  __syncthreads();
  if (r0 >= a.R) return;  // (wave-uniform, and no barrier follows)
  const int row = lane & 15, kk = lane >> 4;
  const double* xr = xs + row * ldx;
  const int sb = MAPPED ? 0 : (int)blockIdx.y * NT * 16;
  // all: the lane's path of tile q is sb + 16 q + row (the A operand's row);
  // mapped: the path of the lane's row of X
  int64_t wrow[NT];  // path index, or -1
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    if (MAPPED) {
      wrow[q] = r0 + row < a.R ? ((r0 + row) / a.inner) % a.S : -1;
    } else {
      const int s = sb + 16 * q + row;
      wrow[q] = s < a.S ? s : -1;
    }
  }
  v4d accp[NT], accu[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) accp[q] = accu[q] = v4d_zero();
  double sp = 0.0, su = 0.0;  // mapped

  // ---- prior path: sine features, then cosine ---------------------------------
  for (int k0 = 0; k0 < H; k0 += 16) {
    const int jb = k0 + 4 * kk;
    const double* om[4];
    double th[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      om[m] = a.Om + (int64_t)(jb + m < H ? jb + m : 0) * d;
      th[m] = 0.0;
    }
    for (int t = 0; t < d; ++t) {
      const double x = xr[t];
#pragma unroll
      for (int m = 0; m < 4; ++m) th[m] = fma(om[m][t], x, th[m]);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int j = jb + m;
      const bool ok = j < H;
      double sn, cs;
      sincos(th[m], &sn, &cs);
      if (!ok) sn = cs = 0.0;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const bool wok = ok && wrow[q] >= 0;
        const double ws = wok ? a.W[wrow[q] * M + j] : 0.0;
        const double wc = wok ? a.W[wrow[q] * M + H + j] : 0.0;
        if (MAPPED) {
          sp = fma(ws, sn, sp);
          sp = fma(wc, cs, sp);
        } else {
          accp[q] = mfma_f64(ws, sn, accp[q]);
          accp[q] = mfma_f64(wc, cs, accp[q]);
        }
      }
    }
  }

  // ---- update path: the kernel row against V ----------------------------------
  for (int64_t i0 = 0; i0 < a.n; i0 += 16) {
    const int64_t ib = i0 + 4 * kk;
    const double* xt[4];
    double d2[4];
    rowtile_dist2x4<1>(xr, a.Xts, ib, a.n, d, xt, d2);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int64_t i = ib + m;
      const bool ok = i < a.n;
      const double kv = ok ? kernel_from_d2<KIND>(d2[m]) : 0.0;
#pragma unroll
      for (int q = 0; q < NT; ++q) {
        const double v = ok && wrow[q] >= 0 ? a.V[wrow[q] * a.n + i] : 0.0;
        if (MAPPED) {
          su = fma(v, kv, su);
        } else {
          accu[q] = mfma_f64(v, kv, accu[q]);
        }
      }
    }
  }

  if (MAPPED) {
    // the row's four feature slots, in a fixed order
    sp = rowtile_fold4(sp);
    su = rowtile_fold4(su);
    if (kk == 0 && r0 + row < a.R)
      a.out[r0 + row] = a.ymean + a.ystd * (a.c + a.pscale * sp + a.o * su);
  } else {
    // D[path = (l >> 4) + 4 r][row = l & 15]: 16 contiguous doubles per path
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = sb + 16 * q + mfma_row(lane, r);
        if (s < a.S && r0 + row < a.R)
          a.out[(int64_t)s * a.R + r0 + row] =
              a.ymean + a.ystd * (a.c + a.pscale * accp[q][r] + a.o * accu[q][r]);
      }
  }
}

// NDT: 16-column tiles of dX (d <= 16 NDT)
template <int KIND, int NDT, bool MAPPED>
__global__ __launch_bounds__(THREADS) void paths_backward_kernel(const Dev a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int d = a.d, H = a.H, M = 2 * a.H, ldx = d | 1;
  double* xs = smem + wave * TR * ldx;
  const int64_t r0 = ((int64_t)blockIdx.x * nw + wave) * TR;
  rowtile_load(a.X, a.ls, r0, TR, a.R, d, ldx, xs, lane, BO_WAVE);
  __syncthreads();
  if (r0 >= a.R) return;  // (wave-uniform, and no barrier follows)
  const int row = lane & 15, kk = lane >> 4;
  const double* xr = xs + row * ldx;
  const bool rok = r0 + row < a.R;
  // mapped: the row's path and cotangent
  const int64_t p = MAPPED && rok ? ((r0 + row) / a.inner) % a.S : 0;
  const double dd1 = MAPPED && rok ? a.dout[r0 + row] : 0.0;

  v4d accd[NDT];  // dX[row = (l >> 4) + 4 r][t = 16 tt + (l & 15)], scaled coordinates
#pragma unroll
  for (int tt = 0; tt < NDT; ++tt) accd[tt] = v4d_zero();
  double sumq = 0.0;  // sum_i q_i of the lane's row (update path)

  // coef[r] = sum_s Wm[s][k0 + (l >> 4) + 4 r] dout[s][row] for a matrix Wm of
  // row length ld (the lane's features of this step are (l >> 4) + 4 r)
  auto coefs = [&](const double* Wm, int64_t ld, int64_t k0, int64_t kend, double* co) {
    if (MAPPED) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t k = k0 + kk + 4 * r;
        co[r] = k < kend ? dd1 * Wm[p * ld + k] : 0.0;
      }
    } else {
      v4d acc = v4d_zero();
      const int64_t ka = k0 + row;  // A[i = l & 15][k = l >> 4] = Wm[s][k0 + i]
      for (int s0 = 0; s0 < a.S; s0 += 4) {
        const int s = s0 + kk;
        const double w = s < a.S && ka < kend ? Wm[(int64_t)s * ld + ka] : 0.0;
        const double dd = s < a.S && rok ? a.dout[(int64_t)s * a.R + r0 + row] : 0.0;
        acc = mfma_f64(w, dd, acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) co[r] = acc[r];
    }
  };

  // ---- prior path ---------------------------------------------------------------
  for (int k0 = 0; k0 < H; k0 += 16) {
    double ca[4], cb[4];
    coefs(a.W, M, k0, H, ca);
    coefs(a.W + H, M, k0, H, cb);
    const double* om[4];
    double th[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = k0 + kk + 4 * r;
      om[r] = a.Om + (int64_t)(j < H ? j : 0) * d;
      th[r] = 0.0;
    }
    for (int t = 0; t < d; ++t) {
      const double x = xr[t];
#pragma unroll
      for (int r = 0; r < 4; ++r) th[r] = fma(om[r][t], x, th[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = k0 + kk + 4 * r < H;
      double sn, cs;
      sincos(th[r], &sn, &cs);
      // d/dtheta (wa sin + wb cos); ca = cb = 0 past the end
      const double q = a.pscale * (ca[r] * cs - cb[r] * sn);
      rowtile_dx_acc<NDT>(-q, ok, om[r], d, row, accd);  // dX[row][:] += q Omega[k][:]
    }
  }

  // ---- update path: dk = g (x - xt) in scaled coordinates ------------------------
  for (int64_t i0 = 0; i0 < a.n; i0 += 16) {
    double cv[4];
    coefs(a.V, a.n, i0, a.n, cv);
    const double* xt[4];
    double d2[4];
    rowtile_dist2x4<4>(xr, a.Xts, i0 + kk, a.n, d, xt, d2);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = i0 + kk + 4 * r < a.n;
      const double q = ok ? cv[r] * dkernel_factor<KIND>(d2[r], a.o) : 0.0;
      sumq += q;
      rowtile_dx_acc<NDT>(q, ok, xt[r], d, row, accd);
    }
  }
  rowtile_dx_store<NDT>(a.dX, accd, xs, ldx, rowtile_fold4(sumq), a.ystd, a.ls, r0, a.R, d, lane);
}

int fill(const BoPathsArgs* a, const char* who, Dev* v) {
  if (int st = rowtile_check_common(a->kind, a->d, a->n, a->Xt_scaled, a->V, a->outputscale, who);
      st != BO_OK)
    return st;
  BO_CHECK_ARG(a->M >= 2 && a->M % 2 == 0, "%s: M must be even and >= 2 (got %d)", who, a->M);
  BO_CHECK_ARG(a->S >= 1 && a->R >= 0 && a->n >= 0 && a->inner >= 0,
               "%s: S >= 1, R >= 0, n >= 0, inner >= 0", who);
  BO_CHECK_ARG(a->R < (int64_t(1) << 34), "%s: R too large", who);
  BO_CHECK_ARG(a->X && a->lengthscale && a->Omega && a->W, "%s: X, lengthscale, Omega and W are required",
               who);
  v->kind = a->kind;
  v->d = a->d;
  v->S = a->S;
  v->H = a->M / 2;
  v->R = a->R;
  v->n = a->n;
  v->inner = a->inner;
  v->X = a->X;
  v->ls = a->lengthscale;
  v->Xts = a->Xt_scaled;
  v->Om = a->Omega;
  v->W = a->W;
  v->V = a->V;
  v->o = a->outputscale;
  v->c = a->constant;
  v->ymean = a->ymean;
  v->ystd = a->ystd;
  v->pscale = std::sqrt(2.0 * a->outputscale / a->M);
  v->out = a->out;
  v->dout = a->dout;
  v->dX = a->dX;
  return BO_OK;
}

// waves per workgroup and the launch geometry over the rows
struct Geo {
  int threads;
  unsigned blocks;
  size_t lds;
};
Geo geometry(const Dev& v) {
  const int nw = v.d > 64 ? 2 : 4;
  return {nw * BO_WAVE, (unsigned)ceil_div(v.R, (int64_t)nw * TR),
          sizeof(double) * (size_t)nw * TR * (v.d | 1)};
}

}  // namespace

// bo_paths_eval_v / bo_paths_eval_backward_v behind their header checks (abi_structs.cpp).
extern "C" int bo_paths_eval_impl(const BoPathsArgs* a, void* stream) {
  Dev v;
  if (int st = fill(a, "bo_paths_eval", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->out, "bo_paths_eval: out is required");
  if (v.R == 0) return BO_OK;
  const Geo g = geometry(v);
  const bool rbf = v.kind == BO_RBF;
#define BO_PATHS(KIND, NT, MAPPED, GY)                                                   \
  paths_forward_kernel<KIND, NT, MAPPED>                                                 \
      <<<dim3(g.blocks, GY), g.threads, g.lds, as_stream(stream)>>>(v)
  if (v.inner > 0) {
    if (rbf) BO_PATHS(BO_RBF, 1, true, 1);
    else BO_PATHS(BO_MATERN52, 1, true, 1);
  } else if (v.S <= 16) {
    if (rbf) BO_PATHS(BO_RBF, 1, false, 1);
    else BO_PATHS(BO_MATERN52, 1, false, 1);
  } else {
    const unsigned gy = (unsigned)ceil_div(v.S, 64);
    BO_CHECK_ARG(gy <= 65535, "bo_paths_eval: S too large");
    if (rbf) BO_PATHS(BO_RBF, 4, false, gy);
    else BO_PATHS(BO_MATERN52, 4, false, gy);
  }
#undef BO_PATHS
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_paths_eval_backward_impl(const BoPathsArgs* a, void* stream) {
  Dev v;
  if (int st = fill(a, "bo_paths_eval_backward", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->dout && a->dX, "bo_paths_eval_backward: dout and dX are required");
  if (v.R == 0) return BO_OK;
  const Geo g = geometry(v);
#define BO_PATHS(KIND, NDT, MAPPED) \
  paths_backward_kernel<KIND, NDT, MAPPED><<<g.blocks, g.threads, g.lds, as_stream(stream)>>>(v)
#define BO_PATHS_ALL(KIND, NDT) BO_PATHS(KIND, NDT, false)
#define BO_PATHS_MAPPED(KIND, NDT) BO_PATHS(KIND, NDT, true)
  if (v.inner > 0) ROWTILE_DISPATCH(v.kind, v.d, BO_PATHS_MAPPED);
  else ROWTILE_DISPATCH(v.kind, v.d, BO_PATHS_ALL);
#undef BO_PATHS_MAPPED
#undef BO_PATHS_ALL
#undef BO_PATHS
  BO_LAUNCH_CHECK();
  return BO_OK;
}
