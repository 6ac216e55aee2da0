// The analytic q = 1 acquisition family (botorch/acquisition/analytic.py):
// LogExpectedImprovement, LogProbabilityOfImprovement, the constrained (Log)EI,
// UCB and the posterior standard deviation as one chain on the posterior
// moments.  The definitions stand in include/botorch_amd.h (BoAnalyticArgs) and
// DESIGN.md section 21.
//
// One thread per row (t-batch), 256-thread blocks; mean and var are Mt x R with
// row stride R, so the lanes of a wave read consecutive doubles of a member.
// The mode, the objective's member and the constraint table are kernel
// arguments: every branch on them is uniform over the grid.  The three
// branches of log_ei and the two of log Phi depend on the row; they are plain
// `if`s, which the compiler guards with an EXEC test, so a wave whose rows all
// lie on one side runs that side only.  No LDS, no atomics, no workspace: a
// second call is bit-identical.
//
// The backward is analytic in log space.  d log_ei / du = r / (1 + u r) with
// r = Phi / phi = sqrt(pi / 2) erfcx(-u / sqrt 2); 1 + u r cancels like u^2 eps,
// so below u = -5 the same quantity comes from Laplace's continued fraction of
// the Mills ratio, g = x + 2 / (x + 3 / (x + ...)), x = -u, which has positive
// terms only.  d log Phi / dx = 1 / r for x < 0.  The two-sided feasibility
// term is taken on the left tail as log phi(b) + log(r(b) - E r(a)),
// E = exp((b^2 - a^2) / 2) <= 1, with the derivatives 1 / (.) and -E / (.): no
// difference of two logarithms of size b^2 / 2.
#include "normal.h"

namespace {

constexpr double LOG_SQRT_2PI = 0.91893853320467274178, LOG_2 = 0.69314718055994530942;
constexpr double SQRT_PI_DIV_2 = 1.25331413731550025121, LOG_SQRT_PI_DIV_2 = 0.22579135264472743236;
constexpr double LOG_EI_UPPER = -1.0, LOG_EI_SERIES = -1e6;  // analytic.py:990, 1001
constexpr double LOG_EI_CF = -5.0;  // below: the continued fraction of d log_ei / du
constexpr int LOG_EI_CF_TERMS = 24;
constexpr int AN_BLOCK = 256;

struct AnDev {
  int mode, Mt, obj, ncon, bf_stride;
  int64_t R;
  const double *mean, *var, *best_f;
  double w, sqrt_beta, min_var;
  int con_member[BO_AN_CMAX + 1], con_kind[BO_AN_CMAX + 1];
  int member_con[BO_AN_CMAX + 1];  // the constraint on member j, -1 without one
  double con_lower[BO_AN_CMAX + 1], con_upper[BO_AN_CMAX + 1];
  double* acq;
  const double* dacq;
  double *dmean, *dvar;
};

__device__ __forceinline__ double log_phi(double x) { return -0.5 * x * x - LOG_SQRT_2PI; }
// Phi(x) / phi(x), x <= 0
__device__ __forceinline__ double mills(double x) { return SQRT_PI_DIV_2 * erfcx(-x * INV_SQRT2); }

// log(1 - e^x), x < 0 (utils/safe_math.py:72-82)
__device__ __forceinline__ double log1mexp(double x) {
  return x > -LOG_2 ? log(-expm1(x)) : log1p(-exp(x));
}

// log Phi(x) (utils/probability/utils.py:151-193) and, GRAD, phi(x) / Phi(x)
template <bool GRAD>
__device__ __forceinline__ double log_ndtr(double x, double& d) {
  const double z = -INV_SQRT2 * x;
  if (z > 0.0) {
    const double e = erfcx(z);
    if (GRAD) d = 1.0 / (SQRT_PI_DIV_2 * e);
    return log(e) - z * z - LOG_2;
  }
  const double c = erfc(z);
  if (GRAD) d = phi(x) / (0.5 * c);
  return log(c) - LOG_2;
}

// log(phi(u) + u Phi(u)) (analytic.py:975-1053) and, GRAD, its derivative g and
// k = 1 - g u (>= 0: phi / (phi + u Phi))
template <bool GRAD>
__device__ __forceinline__ double log_ei(double u, double& g, double& k) {
  if (u > LOG_EI_UPPER) {
    const double ph = phi(u), Ph = Phi(u);
    const double h = ph + u * Ph;
    if (GRAD) {
      g = Ph / h;
      k = ph / h;
    }
    return log(h);
  }
  const double x = -u;
  const double e = erfcx(x * INV_SQRT2);
  if (GRAD) {
    if (u >= LOG_EI_CF) {
      const double r = SQRT_PI_DIV_2 * e;
      const double D = 1.0 - x * r;
      g = r / D;
      k = 1.0 / D;
    } else {
      double K = 0.0;
      for (int i = LOG_EI_CF_TERMS + 1; i >= 2; --i) K = (double)i / (x + K);
      g = x + K;
      k = fma(x, g, 1.0);
    }
  }
  if (u > LOG_EI_SERIES) return log_phi(u) + log1mexp(log(e * x) + LOG_SQRT_PI_DIV_2);
  return log_phi(u) - 2.0 * log(x);
}

struct AnTerm {
  double val, dmu, dvar;
};

// the objective's term of a row: its value and, GRAD, its derivatives in the
// objective's mean and variance
template <bool GRAD>
__device__ __forceinline__ AnTerm an_base(const AnDev& a, int64_t row) {
  const double mu = a.mean[a.obj * a.R + row], v = a.var[a.obj * a.R + row];
  const bool off = v > a.min_var;  // off the floor
  const double s2 = off ? v : a.min_var;
  const double sg = sqrt(s2);
  const double fl = off ? 1.0 : 0.0;
  AnTerm o{0.0, 0.0, 0.0};
  if (a.mode == BO_AN_UCB) {
    o.val = a.w * mu + a.sqrt_beta * sg;
    if (GRAD) {
      o.dmu = a.w;
      o.dvar = fl * a.sqrt_beta * 0.5 / sg;
    }
    return o;
  }
  if (a.mode == BO_AN_STD) {
    o.val = a.w * sg;
    if (GRAD) o.dvar = fl * a.w * 0.5 / sg;
    return o;
  }
  const double bf = a.best_f[row * a.bf_stride];
  double u = (mu - bf) / sg;
  u = a.w > 0.0 ? u : -u;
  if (a.mode == BO_AN_LOG_EI) {
    double g = 0.0, k = 0.0;
    o.val = log_ei<GRAD>(u, g, k) + log(sg);
    if (GRAD) {
      o.dmu = a.w * g / sg;
      o.dvar = fl * 0.5 * k / s2;
    }
  } else if (a.mode == BO_AN_EI) {
    const double ph = phi(u), Ph = Phi(u);
    o.val = sg * (ph + u * Ph);
    if (GRAD) {
      o.dmu = a.w * Ph;
      o.dvar = fl * 0.5 * ph / sg;
    }
  } else {
    double q = 0.0;
    if (a.mode == BO_AN_LOG_PI) {
      o.val = log_ndtr<GRAD>(u, q);
    } else {
      o.val = Phi(u);
      if (GRAD) q = phi(u);
    }
    if (GRAD) {
      o.dmu = a.w * q / sg;
      o.dvar = -fl * 0.5 * q * u / s2;
    }
  }
  return o;
}

// the log feasibility probability of constraint c (analytic.py:1182-1220) and,
// GRAD, its derivatives in the member's mean and variance
template <bool GRAD>
__device__ __forceinline__ AnTerm an_con(const AnDev& a, int c, int64_t row) {
  const int j = a.con_member[c], kind = a.con_kind[c];
  const double mu = a.mean[j * a.R + row], v = a.var[j * a.R + row];
  const bool off = v > a.min_var;
  const double s2 = off ? v : a.min_var;
  const double sg = sqrt(s2);
  const double fl = off ? 1.0 : 0.0;
  AnTerm o{0.0, 0.0, 0.0};
  if (kind != BO_AN_CON_BOTH) {
    const bool lower = kind == BO_AN_CON_LOWER;
    const double x = lower ? -((a.con_lower[c] - mu) / sg) : (a.con_upper[c] - mu) / sg;
    double q = 0.0;
    o.val = log_ndtr<GRAD>(x, q);
    if (GRAD) {
      o.dmu = (lower ? q : -q) / sg;
      o.dvar = -fl * 0.5 * q * x / s2;
    }
    return o;
  }
  const double lo = (a.con_lower[c] - mu) / sg, hi = (a.con_upper[c] - mu) / sg;
  const bool rev = fabs(hi) > fabs(lo);  // utils/probability/utils.py:249-256
  const double al = rev ? -hi : lo, bl = rev ? -lo : hi;  // al < 0, |bl| <= |al|
  double dA, dB;  // d / d al, d / d bl
  if (bl <= 0.0) {
    const double E = exp(0.5 * (bl - al) * (bl + al));
    const double den = mills(bl) - E * mills(al);
    o.val = log_phi(bl) + log(den);
    dB = 1.0 / den;
    dA = -E / den;
  } else {
    // al < 0 < bl: Phi(bl) - Phi(al) as a sum of two positive terms
    const double P = 0.5 * (erf(bl * INV_SQRT2) + erf(-al * INV_SQRT2));
    o.val = log(P);
    dB = phi(bl) / P;
    dA = -phi(al) / P;
  }
  if (GRAD) {
    const double dlo = rev ? -dB : dA, dhi = rev ? -dA : dB;
    o.dmu = -(dlo + dhi) / sg;
    o.dvar = -fl * 0.5 * (lo * dlo + hi * dhi) / s2;
  }
  return o;
}

__device__ __forceinline__ bool an_log_mode(int mode) {
  return mode == BO_AN_LOG_EI || mode == BO_AN_LOG_PI;
}

__global__ __launch_bounds__(AN_BLOCK) void analytic_kernel(const AnDev a) {
  const int64_t row = (int64_t)blockIdx.x * AN_BLOCK + threadIdx.x;
  if (row >= a.R) return;
  const AnTerm b = an_base<false>(a, row);
  double lp = 0.0;
  for (int c = 0; c < a.ncon; ++c) lp += an_con<false>(a, c, row).val;
  a.acq[row] = an_log_mode(a.mode) ? b.val + lp : a.ncon > 0 ? b.val * exp(lp) : b.val;
}

__global__ __launch_bounds__(AN_BLOCK) void analytic_backward_kernel(const AnDev a) {
  const int64_t row = (int64_t)blockIdx.x * AN_BLOCK + threadIdx.x;
  if (row >= a.R) return;
  const AnTerm b = an_base<true>(a, row);
  const double d = a.dacq[row];
  // acq = val + lp (log modes) or val exp(lp): the factors of the objective's
  // and of the constraints' derivatives
  double fo = d, fc = d;
  if (!an_log_mode(a.mode) && a.ncon > 0) {
    double lp = 0.0;
    for (int c = 0; c < a.ncon; ++c) lp += an_con<false>(a, c, row).val;
    fo = d * exp(lp);
    fc = fo * b.val;
  }
  for (int j = 0; j < a.Mt; ++j) {
    double dm = 0.0, dv = 0.0;
    if (j == a.obj) {
      dm = fo * b.dmu;
      dv = fo * b.dvar;
    } else if (a.member_con[j] >= 0) {
      const AnTerm t = an_con<true>(a, a.member_con[j], row);
      dm = fc * t.dmu;
      dv = fc * t.dvar;
    }
    a.dmean[j * a.R + row] = dm;
    a.dvar[j * a.R + row] = dv;
  }
}

// the host-side checks of both entries; *empty: R = 0, nothing to launch
int an_fill(const BoAnalyticArgs* a, const char* who, AnDev* v, bool* empty) {
  BO_CHECK_ARG(a->Mt >= 1 && a->Mt <= BO_AN_CMAX + 1, "%s: 1 <= Mt <= %d (got %d)", who,
               BO_AN_CMAX + 1, a->Mt);
  BO_CHECK_ARG(a->mode >= BO_AN_LOG_EI && a->mode <= BO_AN_STD, "%s: mode must be 0..5 (got %d)",
               who, a->mode);
  BO_CHECK_ARG(a->ncon >= 0 && a->ncon <= BO_AN_CMAX, "%s: 0 <= ncon <= %d (got %d)", who,
               BO_AN_CMAX, a->ncon);
  BO_CHECK_ARG(a->obj >= 0 && a->obj < a->Mt, "%s: 0 <= obj < Mt (got %d)", who, a->obj);
  BO_CHECK_ARG(a->min_var > 0.0, "%s: min_var > 0", who);
  BO_CHECK_ARG(a->w == 1.0 || a->w == -1.0, "%s: w must be +1 or -1", who);
  BO_CHECK_ARG(a->beta >= 0.0, "%s: beta >= 0", who);
  BO_CHECK_ARG(a->best_f_stride == 0 || a->best_f_stride == 1, "%s: best_f_stride must be 0 or 1",
               who);
  BO_CHECK_ARG(a->R >= 0 && a->R < (int64_t(1) << 38), "%s: 0 <= R < 2^38", who);
  for (int j = 0; j <= BO_AN_CMAX; ++j) v->member_con[j] = -1;
  for (int c = 0; c < a->ncon; ++c) {
    const int j = a->con_member[c], kind = a->con_kind[c];
    BO_CHECK_ARG(j >= 0 && j < a->Mt, "%s: constraint %d: 0 <= member < Mt (got %d)", who, c, j);
    BO_CHECK_ARG(j != a->obj, "%s: constraint %d is on the objective's member %d", who, c, j);
    BO_CHECK_ARG(v->member_con[j] < 0, "%s: member %d carries more than one constraint", who, j);
    BO_CHECK_ARG(kind >= BO_AN_CON_LOWER && kind <= BO_AN_CON_BOTH,
                 "%s: constraint %d: kind must be 0..2 (got %d)", who, c, kind);
    BO_CHECK_ARG(kind != BO_AN_CON_BOTH || a->con_upper[c] > a->con_lower[c],
                 "%s: constraint %d: upper > lower", who, c);
    v->member_con[j] = c;
    v->con_member[c] = j;
    v->con_kind[c] = kind;
    v->con_lower[c] = a->con_lower[c];
    v->con_upper[c] = a->con_upper[c];
  }
  *empty = a->R == 0;
  if (*empty) return BO_OK;
  BO_CHECK_ARG(a->mean && a->var, "%s: mean and var are required", who);
  const bool needs_best_f = a->mode <= BO_AN_PI;
  BO_CHECK_ARG(!needs_best_f || a->best_f, "%s: best_f is required in this mode", who);
  v->mode = a->mode;
  v->Mt = a->Mt;
  v->obj = a->obj;
  v->ncon = a->ncon;
  v->bf_stride = a->best_f_stride;
  v->R = a->R;
  v->mean = a->mean;
  v->var = a->var;
  v->best_f = a->best_f;
  v->w = a->w;
  v->sqrt_beta = sqrt(a->beta);
  v->min_var = a->min_var;
  v->acq = a->acq;
  v->dacq = a->dacq;
  v->dmean = a->dmean;
  v->dvar = a->dvar;
  return BO_OK;
}

}  // namespace

// bo_analytic_v / bo_analytic_backward_v behind their header checks
// (abi_structs.cpp).
extern "C" int bo_analytic_impl(const BoAnalyticArgs* a, void* stream) {
  AnDev v{};
  bool empty = false;
  if (int st = an_fill(a, "bo_analytic", &v, &empty); st != BO_OK) return st;
  if (empty) return BO_OK;
  BO_CHECK_ARG(a->acq, "bo_analytic: acq is required");
  analytic_kernel<<<(unsigned)ceil_div(v.R, AN_BLOCK), AN_BLOCK, 0, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}

extern "C" int bo_analytic_backward_impl(const BoAnalyticArgs* a, void* stream) {
  AnDev v{};
  bool empty = false;
  if (int st = an_fill(a, "bo_analytic_backward", &v, &empty); st != BO_OK) return st;
  if (empty) return BO_OK;
  BO_CHECK_ARG(a->dacq && a->dmean && a->dvar,
               "bo_analytic_backward: dacq, dmean and dvar are required");
  analytic_backward_kernel<<<(unsigned)ceil_div(v.R, AN_BLOCK), AN_BLOCK, 0, as_stream(stream)>>>(v);
  BO_LAUNCH_CHECK();
  return BO_OK;
}
