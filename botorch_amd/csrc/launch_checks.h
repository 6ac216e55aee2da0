// Host-side argument checks shared by the launchers of mixed.hip and ltf.hip (no
// device code; includes nothing of HIP, so a host program can compile it alone).
#pragma once

#include <stdint.h>

#include "../../include/botorch_amd.h"

void bo_set_error(const char* fmt, ...);

// The two column lists a (na entries) and b (nb entries) must together name each of
// the columns 0..d-1 once.  The caller has checked d = na + nb <= 32.
inline int check_partition(const char* who, int d, int na, const int32_t* a, int nb,
                           const int32_t* b) {
  unsigned seen = 0;
  for (int t = 0; t < na + nb; ++t) {
    const int col = t < na ? a[t] : b[t - na];
    if (!(col >= 0 && col < d && !(seen >> col & 1u))) {
      bo_set_error("%s: column lists must partition 0..%d", who, d - 1);
      return BO_ERR_ARG;
    }
    seen |= 1u << col;
  }
  return BO_OK;
}

// The shape limits and required inputs of a cross / cross-grad record
// (BoMixedCrossArgs, BoLtfCrossArgs): B q query rows index with 32 bits.
template <class CrossArgs>
int check_cross(const char* who, const CrossArgs* a) {
  if (!(a->B >= 0 && a->q >= 1 && a->n >= 0 && a->B * a->q < (int64_t(1) << 31) &&
        a->q < (int64_t(1) << 20))) {
    bo_set_error("%s: B = %lld, q = %lld, n = %lld", who, (long long)a->B, (long long)a->q,
                 (long long)a->n);
    return BO_ERR_ARG;
  }
  if (!(a->hyper && (a->B == 0 || a->Xq) && (a->n == 0 || a->Xt))) {
    bo_set_error("%s: Xq, Xt and hyper are required", who);
    return BO_ERR_ARG;
  }
  return BO_OK;
}
