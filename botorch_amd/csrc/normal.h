// The standard normal's density and distribution function, fp64, for the
// acquisition kernels (mes.hip, analytic.hip, jes.hip).
#pragma once

#include "common.h"

constexpr double INV_SQRT2 = 0.70710678118654752440, INV_SQRT2PI = 0.39894228040143267794;

__device__ __forceinline__ double Phi(double x) { return 0.5 * erfc(-x * INV_SQRT2); }
__device__ __forceinline__ double phi(double x) { return INV_SQRT2PI * exp(-0.5 * x * x); }
