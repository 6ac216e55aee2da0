// Max-value entropy search (botorch/acquisition/max_value_entropy_search.py):
// qMaxValueEntropy's information gain (lines 399-515, no fantasies, no trace
// observations), GIBBON's lower bound (537-664) and the three quantiles of the
// independence approximation of the maximum that the Gumbel sampler fits
// (983-1010).  The definitions stand in include/botorch_amd.h (BoMesArgs,
// BoGibbonArgs, BoMvQuantilesArgs) and DESIGN.md section 18.
//
// bo_mes: one wave per row.  The S_M * S_m pairs (j, k) are laid out flat,
// p = j S_m + k, and lane l takes p = l, l + 64, ...; the base samples z and
// the row's per-max-value constants (f*_j, log Phi0_j and its two derivatives)
// sit in the wave's LDS.  The centred second moments take a second pass that
// recomputes h1 (no array of the pairs exists anywhere); every sum is folded
// over the lanes by a xor butterfly in a fixed order, so a second call is
// bit-identical.  The backward runs the same two passes with the analytic
// derivatives of h1 in mu and sigma^2 added to the second.
//
// bo_gibbon: sixteen lanes per row, four rows per wave.  Lane i of the group
// forms u_i = sum_l (Binv[i][l] + Binv[l][i]) A_l (qf = sum_i A_i u_i / 2,
// dqf / dA_i = u_i) and takes the max values j = i, i + 16, ...
//
// bo_mv_quantiles: one workgroup per quantile, a bisection with one block
// reduction per iteration (fixed order), one launch.
#include "normal.h"

namespace {

constexpr double CLAMP_LB = 1e-8;
constexpr double LOG_2PI = 1.83787706640934548356;
constexpr double VDET_EPS = (1.0 + 1e-12) - 1.0;
constexpr int MES_SM_MAX = 1024, MES_SY_MAX = 4096, GIBBON_MMAX = 15;

// ---- MES ---------------------------------------------------------------------------------
struct MesDev {
  int SM, Sy;
  int64_t R;
  const double *mu, *var, *fstar, *z;
  double kappa, var_h0, zsq_mean, tau2, w;
  double* out;
  const double* dout;
  double *dmu, *dvar;
};

// the row's quantities that no pair changes
struct MesRow {
  double m, vM, vm, a, rs, lpc;  // a = vM / sqrt(vm), rs = 1 / sqrt(s2n), lpc = -log(2 pi vm) / 2
  double da_ds, ds2n_ds;         // d a / d sigma^2, d s2n / d sigma^2 (0 on its floor)
  double fM;                     // 1 where vM is off its floor
};

__device__ __forceinline__ MesRow mes_row(const MesDev& a, int64_t row) {
  MesRow r;
  const double s = a.var[row];
  r.m = a.w * a.mu[row];
  r.fM = s > CLAMP_LB ? 1.0 : 0.0;
  r.vM = s > CLAMP_LB ? s : CLAMP_LB;
  r.vm = s + a.tau2;
  const double isq = 1.0 / sqrt(r.vm);
  r.a = r.vM * isq;
  const double s2u = r.vM - r.vM * r.vM / r.vm;
  const bool free = s2u > CLAMP_LB;
  r.rs = 1.0 / sqrt(free ? s2u : CLAMP_LB);
  r.lpc = -0.5 * (LOG_2PI + log(r.vm));
  r.da_ds = r.fM * isq - 0.5 * r.vM * isq / r.vm;
  // d s2n / d sigma^2 = fM (1 - 2 t) + t^2: (1 - t)^2 off vM's floor, without
  // the cancellation (1 - t = tau2 / vm there)
  const double t = r.vM / r.vm, omt = (r.vm - r.vM) / r.vm;
  r.ds2n_ds = !free ? 0.0 : r.fM > 0.0 ? omt * omt : t * t;
  return r;
}

// per-max-value constants of the row -> LDS: f*_j, log Phi0_j and (GRAD) the
// derivatives of log Phi0_j in m and sigma^2
template <bool GRAD>
__device__ __forceinline__ void mes_stage(const MesDev& a, const MesRow& r, int lane, double* zs,
                                          double* fs, double* l0, double* d0m, double* d0s) {
  for (int k = lane; k < a.Sy; k += BO_WAVE) zs[k] = a.z[k];
  const double rM = 1.0 / sqrt(r.vM);
  for (int j = lane; j < a.SM; j += BO_WAVE) {
    const double f = a.fstar[j];
    const double g = (f - r.m) * rM;
    const double P0 = Phi(g);
    const bool free = P0 > CLAMP_LB;
    fs[j] = f;
    l0[j] = log(free ? P0 : CLAMP_LB);
    if (GRAD) {
      const double q = free ? phi(g) / P0 : 0.0;
      d0m[j] = -q * rM;
      d0s[j] = -0.5 * q * g * r.fM / r.vM;
    }
  }
}

struct MesPair {
  double h1, ck;
  double dm, ds;  // d h1 / d m, d h1 / d sigma^2
};

template <bool GRAD>
__device__ __forceinline__ MesPair mes_pair(const MesDev& a, const MesRow& r, double f, double l0,
                                            double d0m, double d0s, double z) {
  MesPair o;
  const double wz = a.w * z;
  const double u = (f - (r.m + r.a * wz)) * r.rs;
  const double Pn = Phi(u);
  const bool free = Pn > CLAMP_LB;
  const double Pc = free ? Pn : CLAMP_LB;
  const double lZ = log(Pc) - l0;
  const double Z = exp(lZ);
  const double lp = r.lpc - 0.5 * z * z;
  o.h1 = -Z * (lZ + lp);
  o.ck = 0.5 * (z * z - a.zsq_mean);
  if (GRAD) {
    const double q = free ? phi(u) / Pc : 0.0;  // d log Phin / du
    const double du_dm = -r.rs;
    const double du_ds = -(wz * r.da_ds) * r.rs - 0.5 * u * r.ds2n_ds * r.rs * r.rs;
    const double c = -(lZ + 1.0 + lp) * Z;
    o.dm = c * (q * du_dm - d0m);
    o.ds = c * (q * du_ds - d0s) + Z * 0.5 / r.vm;
  } else {
    o.dm = o.ds = 0.0;
  }
  return o;
}

template <bool GRAD>
__global__ __launch_bounds__(BO_WAVE) void mes_kernel(const MesDev a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;  // (the grid is R)
  double* zs = smem;
  double* fs = zs + a.Sy;
  double* l0 = fs + a.SM;
  double* d0m = l0 + a.SM;
  double* d0s = d0m + a.SM;
  const MesRow r = mes_row(a, row);
  mes_stage<GRAD>(a, r, lane, zs, fs, l0, d0m, d0s);
  __syncthreads();
  const int64_t N = (int64_t)a.SM * a.Sy;
  // pass 1: the mean of h1
  double s1 = 0.0;
  {
    int j = lane / a.Sy, k = lane - j * a.Sy;
    for (int64_t p = lane; p < N; p += BO_WAVE) {
      s1 += mes_pair<false>(a, r, fs[j], l0[j], 0.0, 0.0, zs[k]).h1;
      k += BO_WAVE;
      while (k >= a.Sy) {
        k -= a.Sy;
        ++j;
      }
    }
  }
  const double H1 = wave_sum(s1) / (double)N;
  // pass 2: the centred moments (and the three sums of each derivative)
  double sc = 0.0, sv = 0.0;
  double g1m = 0.0, g2m = 0.0, g3m = 0.0, g1s = 0.0, g2s = 0.0, g3s = 0.0;
  {
    int j = lane / a.Sy, k = lane - j * a.Sy;
    for (int64_t p = lane; p < N; p += BO_WAVE) {
      const MesPair e = mes_pair<GRAD>(a, r, fs[j], l0[j], GRAD ? d0m[j] : 0.0,
                                       GRAD ? d0s[j] : 0.0, zs[k]);
      const double c = e.h1 - H1;
      sc = fma(c, e.ck, sc);
      sv = fma(c, c, sv);
      if (GRAD) {
        g1m += e.dm;
        g2m = fma(e.ck, e.dm, g2m);
        g3m = fma(c, e.dm, g3m);
        g1s += e.ds;
        g2s = fma(e.ck, e.ds, g2s);
        g3s = fma(c, e.ds, g3s);
      }
      k += BO_WAVE;
      while (k >= a.Sy) {
        k -= a.Sy;
        ++j;
      }
    }
  }
  const double cov = wave_sum(sc) / (double)N;
  const double v1 = wave_sum(sv) / (double)(N - 1);
  const double den = 1.0 / sqrt(a.var_h0 * v1);
  const double beta = cov * den;
  if (!GRAD) {
    const double H0 = 0.5 * (LOG_2PI + 1.0 + log(r.vm));
    if (lane == 0) a.out[row] = H0 - H1 + beta * a.kappa;
  } else {
    g1m = wave_sum(g1m);
    g2m = wave_sum(g2m);
    g3m = wave_sum(g3m);
    g1s = wave_sum(g1s);
    g2s = wave_sum(g2s);
    g3s = wave_sum(g3s);
    // d ig = dH0 - dH1bar + kappa (dcov / sqrt(v0 v1) - beta dv1 / (2 v1))
    const double iN = 1.0 / (double)N, iN1 = 2.0 / (double)(N - 1);
    const double gm = -g1m * iN + a.kappa * (g2m * iN * den - 0.5 * beta * g3m * iN1 / v1);
    const double gs = 0.5 / r.vm - g1s * iN +
                      a.kappa * (g2s * iN * den - 0.5 * beta * g3s * iN1 / v1);
    if (lane == 0) {
      const double d = a.dout[row];
      a.dmu[row] = d * a.w * gm;
      a.dvar[row] = d * gs;
    }
  }
}

int mes_fill(const BoMesArgs* a, const char* who, MesDev* v) {
  BO_CHECK_ARG(a->S_M >= 1 && a->S_M <= MES_SM_MAX, "%s: 1 <= S_M <= %d (got %d)", who,
               MES_SM_MAX, a->S_M);
  BO_CHECK_ARG(a->S_m >= 2 && a->S_m <= MES_SY_MAX, "%s: 2 <= S_m <= %d (got %d)", who,
               MES_SY_MAX, a->S_m);
  BO_CHECK_ARG(a->R >= 1 && a->R <= 0x7fffffff, "%s: 1 <= R < 2^31", who);
  BO_CHECK_ARG(a->mu && a->var && a->fstar && a->z, "%s: mu, var, fstar and z are required", who);
  BO_CHECK_ARG(a->w == 1.0 || a->w == -1.0, "%s: w must be +1 or -1", who);
  BO_CHECK_ARG(a->tau2 >= 0.0 && a->var_h0 > 0.0, "%s: tau2 >= 0 and var_h0 > 0", who);
  v->SM = a->S_M;
  v->Sy = a->S_m;
  v->R = a->R;
  v->mu = a->mu;
  v->var = a->var;
  v->fstar = a->fstar;
  v->z = a->z;
  v->kappa = a->kappa;
  v->var_h0 = a->var_h0;
  v->zsq_mean = a->zsq_mean;
  v->tau2 = a->tau2;
  v->w = a->w;
  v->out = a->out;
  v->dout = a->dout;
  v->dmu = a->dmu;
  v->dvar = a->dvar;
  return BO_OK;
}

// ---- GIBBON ------------------------------------------------------------------------------
struct GibDev {
  int SM, m;
  int64_t R;
  const double *mu, *var, *A, *Binv, *fstar;
  double tau2, w;
  double* out;
  const double* dout;
  double *dmu, *dvar, *dA;
};

// the sum over the 16 lanes of a group, in every lane of it
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void gibbon_kernel(const GibDev a) {
  const int i = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool ok = row < a.R;  // (rows past R run on benign values and write nothing)
  const double s = ok ? a.var[row] : 1.0;
  const double m = ok ? a.w * a.mu[row] : 0.0;
  const double fM = s > CLAMP_LB ? 1.0 : 0.0;
  const double vM = s > CLAMP_LB ? s : CLAMP_LB;
  const double vmu = s + a.tau2;
  const double fm = vmu > CLAMP_LB ? 1.0 : 0.0;
  const double vm = vmu > CLAMP_LB ? vmu : CLAMP_LB;
  const double rM = 1.0 / sqrt(vM), rho2 = vM / vm;
  double sl = 0.0, sm = 0.0, ss = 0.0;
  for (int j = i; j < a.SM; j += 16) {
    const double g = (a.fstar[j] - m) * rM;
    const double P = Phi(g);
    const bool pfree = P > CLAMP_LB;
    const double r = phi(g) / (pfree ? P : CLAMP_LB);
    const double q = r * (g + r);
    const double inu = 1.0 - rho2 * q;
    const bool ifree = inu > CLAMP_LB;
    sl += log(ifree ? inu : CLAMP_LB);
    if (GRAD && ifree) {
      const double rp = pfree ? -q : -g * r;
      const double dq = rp * (g + r) + r * (1.0 + rp);
      // d inner = -q d rho2 - rho2 dq dgamma
      const double e = 1.0 / inu;
      sm += e * (-rho2 * dq * (-rM));
      ss += e * (-q * (fM / vm - fm * vM / (vm * vm)) - rho2 * dq * (-0.5 * g * fM / vM));
    }
  }
  sl = group_sum(sl);
  double acq = -0.5 * sl / a.SM;
  double gm = 0.0, gs = 0.0;
  if (GRAD) {
    gm = -0.5 * group_sum(sm) / a.SM;
    gs = -0.5 * group_sum(ss) / a.SM;
  }
  if (a.m > 0) {  // (uniform over the grid)
    double u = 0.0, Ai = 0.0;
    if (ok && i < a.m) {
      const double* Ar = a.A + row * a.m;
      Ai = Ar[i];
      for (int l = 0; l < a.m; ++l) u = fma(a.Binv[i * a.m + l] + a.Binv[l * a.m + i], Ar[l], u);
    }
    const double qf = 0.5 * group_sum(Ai * u);
    const double lim = qf * (1.0 + 1e-12);
    const bool vfree = vm >= lim;
    // on the clamped branch lim - qf is qf ((1 + 1e-12) - 1) without the
    // cancellation (which would cost four digits)
    acq += 0.5 * (log(vfree ? vm - qf : qf * VDET_EPS) - log(vm));
    if (GRAD) {
      // free: log(vm - qf) - log vm; clamped: log(eps qf) - log vm
      const double dq = vfree ? -0.5 / (vm - qf) : 0.5 / qf;
      gs += fm * ((vfree ? 0.5 / (vm - qf) : 0.0) - 0.5 / vm);
      if (ok && i < a.m) a.dA[row * a.m + i] = a.dout[row] * dq * u;
    }
  }
  if (ok && i == 0) {
    if (!GRAD) {
      a.out[row] = acq;
    } else {
      const double d = a.dout[row];
      a.dmu[row] = d * a.w * gm;
      a.dvar[row] = d * gs;
    }
  }
}

int gib_fill(const BoGibbonArgs* a, const char* who, GibDev* v) {
  BO_CHECK_ARG(a->S_M >= 1, "%s: S_M >= 1 (got %d)", who, a->S_M);
  BO_CHECK_ARG(a->m >= 0 && a->m <= GIBBON_MMAX, "%s: 0 <= m <= %d (got %d)", who, GIBBON_MMAX,
               a->m);
  BO_CHECK_ARG(a->R >= 1 && a->R < (int64_t(1) << 34), "%s: 1 <= R < 2^34", who);
  BO_CHECK_ARG(a->mu && a->var && a->fstar, "%s: mu, var and fstar are required", who);
  BO_CHECK_ARG(a->m == 0 || (a->A && a->Binv), "%s: A and Binv are required when m > 0", who);
  BO_CHECK_ARG(a->w == 1.0 || a->w == -1.0, "%s: w must be +1 or -1", who);
  BO_CHECK_ARG(a->tau2 >= 0.0, "%s: tau2 >= 0", who);
  v->SM = a->S_M;
  v->m = a->m;
  v->R = a->R;
  v->mu = a->mu;
  v->var = a->var;
  v->A = a->A;
  v->Binv = a->Binv;
  v->fstar = a->fstar;
  v->tau2 = a->tau2;
  v->w = a->w;
  v->out = a->out;
  v->dout = a->dout;
  v->dmu = a->dmu;
  v->dvar = a->dvar;
  v->dA = a->dA;
  return BO_OK;
}

// ---- the quantiles of the maximum under independence ---------------------------------------
constexpr int QT = 256;      // threads per quantile
constexpr int Q_ITERS = 200; // cap; fp64 bisection ends after ~60 halvings

// log Phi(x), usable in both tails (-inf once erfc underflows, below -37.5)
__device__ __forceinline__ double log_Phi(double x) {
  return x > 0.0 ? log1p(-0.5 * erfc(x * INV_SQRT2)) : log(0.5 * erfc(-x * INV_SQRT2));
}

// OP 0: sum, 1: min, 2: max over the block, in every thread, in a fixed order
template <int OP>
__device__ __forceinline__ double block_fold(double v, double* red) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_xor(v, o);
    v = OP == 0 ? v + t : OP == 1 ? fmin(v, t) : fmax(v, t);
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // red is free again
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int q = 1; q < QT / 64; ++q)
    r = OP == 0 ? r + red[q] : OP == 1 ? fmin(r, red[q]) : fmax(r, red[q]);
  return r;
}

struct QDev {
  int64_t N;
  const double *mu, *sigma;
  int have_bounds;
  double lo, hi;
  double* out;
  int32_t* status;
};

__device__ __forceinline__ double q_objective(const QDev& a, double y, double* red) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < a.N; i += QT) s += log_Phi((y - a.mu[i]) / a.sigma[i]);
  return block_fold<0>(s, red);
}

__global__ __launch_bounds__(QT) void mv_quantiles_kernel(const QDev a) {
  __shared__ double red[QT / 64];
  const double logp = blockIdx.x == 0 ? -1.38629436111989061883   // log 0.25
                      : blockIdx.x == 1 ? -0.69314718055994530942  // log 0.5
                                        : -0.28768207245178092744; // log 0.75
  double lo = a.lo, hi = a.hi;
  if (!a.have_bounds) {
    double l = INFINITY, h = -INFINITY;
    for (int64_t i = threadIdx.x; i < a.N; i += QT) {
      l = fmin(l, a.mu[i] - 3.0 * a.sigma[i]);
      h = fmax(h, a.mu[i] + 5.0 * a.sigma[i]);
    }
    lo = block_fold<1>(l, red);
    hi = block_fold<2>(h, red);
  }
  // (every thread holds the same lo, hi and sums: the branches below are uniform)
  const bool below_lo = q_objective(a, lo, red) < logp, below_hi = q_objective(a, hi, red) < logp;
  const int st = below_lo && !below_hi ? 0 : 1;
  double y = 0.5 * (lo + hi);
  if (st == 0) {
    for (int it = 0; it < Q_ITERS; ++it) {
      y = 0.5 * (lo + hi);
      if (!(y > lo && y < hi)) break;
      if (hi - lo <= 4.0 * 2.220446049250313e-16 * fmax(fabs(lo), fabs(hi))) break;
      if (q_objective(a, y, red) < logp) lo = y;
      else hi = y;
    }
  }
  if (threadIdx.x == 0) {
    a.out[blockIdx.x] = y;
    a.status[blockIdx.x] = st;
  }
}

}  // namespace

// bo_mes_v / bo_mes_backward_v, bo_gibbon_v / bo_gibbon_backward_v and
// bo_mv_quantiles_v behind their header checks (abi_structs.cpp).
extern "C" int bo_mes_impl(const BoMesArgs* a, void* stream) {
  MesDev v;
  if (int st = mes_fill(a, "bo_mes", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->out, "bo_mes: out is required");
  const size_t lds = sizeof(double) * ((size_t)v.Sy + 4 * (size_t)v.SM);
  mes_kernel<false><<<(unsigned)v.R, BO_WAVE, lds, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_mes_backward_impl(const BoMesArgs* a, void* stream) {
  MesDev v;
  if (int st = mes_fill(a, "bo_mes_backward", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->dout && a->dmu && a->dvar, "bo_mes_backward: dout, dmu and dvar are required");
  const size_t lds = sizeof(double) * ((size_t)v.Sy + 4 * (size_t)v.SM);
  mes_kernel<true><<<(unsigned)v.R, BO_WAVE, lds, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_gibbon_impl(const BoGibbonArgs* a, void* stream) {
  GibDev v;
  if (int st = gib_fill(a, "bo_gibbon", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->out, "bo_gibbon: out is required");
  gibbon_kernel<false><<<(unsigned)ceil_div(v.R, 16), 256, 0, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_gibbon_backward_impl(const BoGibbonArgs* a, void* stream) {
  GibDev v;
  if (int st = gib_fill(a, "bo_gibbon_backward", &v); st != BO_OK) return st;
  BO_CHECK_ARG(a->dout && a->dmu && a->dvar, "bo_gibbon_backward: dout, dmu and dvar are required");
  BO_CHECK_ARG(a->m == 0 || a->dA, "bo_gibbon_backward: dA is required when m > 0");
  gibbon_kernel<true><<<(unsigned)ceil_div(v.R, 16), 256, 0, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_mv_quantiles_impl(const BoMvQuantilesArgs* a, void* stream) {
  const char* who = "bo_mv_quantiles";
  BO_CHECK_ARG(a->N >= 1, "%s: N >= 1", who);
  BO_CHECK_ARG(a->mu && a->sigma && a->out && a->status, "%s: mu, sigma, out and status are "
               "required", who);
  BO_CHECK_ARG(!a->have_bounds || a->lo < a->hi, "%s: lo < hi", who);
  QDev v{a->N, a->mu, a->sigma, a->have_bounds, a->lo, a->hi, a->out, a->status};
  mv_quantiles_kernel<<<3, QT, 0, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}
