// fluhip_dd.h -- double-double arithmetic (an unevaluated sum hi + lo, |lo| <= ulp(hi) / 2) for the carried filter states of
// kernels_loudness.hip and kernels_amp.hip, host and device.  Every rounding counts: the units that include this are compiled
// with -ffp-contract=off.  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace fluhip {

struct dd
{
  double hi, lo;
};
__host__ __device__ __forceinline__ dd quick_two_sum(double a, double b)
{
  const double s = a + b;
  return {s, b - (s - a)};
}
__host__ __device__ __forceinline__ dd two_sum(double a, double b)
{
  const double s = a + b;
  const double bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__host__ __device__ __forceinline__ dd dd_add(dd a, dd b)
{
  dd s = two_sum(a.hi, b.hi);
  const dd t = two_sum(a.lo, b.lo);
  s.lo += t.hi;
  s = quick_two_sum(s.hi, s.lo);
  s.lo += t.lo;
  return quick_two_sum(s.hi, s.lo);
}
__host__ __device__ __forceinline__ dd dd_mul(dd a, dd b)
{
  const double p = a.hi * b.hi;
  double e = fma(a.hi, b.hi, -p);
  e += a.hi * b.lo + a.lo * b.hi;
  return quick_two_sum(p, e);
}

} // namespace fluhip
