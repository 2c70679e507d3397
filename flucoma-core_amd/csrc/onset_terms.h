// onset_terms.h -- device arithmetic of the onset detection functions, shared by the two forms of the curve kernel:
// onset_reduce_kernel (kernels_onset.hip, spectra from a workspace) and onset_fused_kernel (kernels_onset_fused.hip, spectra in
// the LDS).  One definition, so that both forms add the same terms in the same order:
// lane l visits the bins l, l + 64, l + 128, ... in that order and adds each bin's term to its partial sum; the 64 partial
// sums then meet in a butterfly (xor 32, 16, ... 1).  Every function switches floating-point contraction off for itself:
// the sums are the plain operations written here in whichever translation unit they are compiled.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

namespace fluhip {
namespace onsetdev {

typedef double d2 __attribute__((ext_vector_type(2)));

constexpr double kPi = 3.14159265358979323846;
constexpr double kTwoPi = 6.28318530717958647692;
constexpr double kEps = DBL_EPSILON;

// OnsetDetectionFuncs::wrapPhase, kept as written: only p > pi passes unchanged
__device__ __forceinline__ double wrap_phase(double p)
{
#pragma clang fp contract(off)
  return (p > -kPi && p > kPi) ? p : p + kTwoPi * (1.0 + floor((-kPi - p) / kTwoPi));
}

// real part of the complex arctangent of x + i y (what Eigen's atan() of a complex array yields; the reference takes its
// real part for a "phase").  After glibc's catan: 0.5 atan2(2 x, 1 - x^2 - y^2), +-pi/2 once a part reaches 16 / eps; the
// denominator carries the rounding errors of both squares, so it is good to an ulp of max(1, x^2, y^2) next to |z| = 1.
__device__ __forceinline__ double catan_re(double x, double y)
{
#pragma clang fp contract(off)
  const double ax = fabs(x), ay = fabs(y);
  if (ax >= 16.0 / kEps || ay >= 16.0 / kEps) return copysign(0.5 * kPi, x);
  const double hx = ax * ax, ex = __builtin_fma(ax, ax, -hx);
  const double hy = ay * ay, ey = __builtin_fma(ay, ay, -hy);
  double den = (((1.0 - hx) - hy) - ex) - ey;
  if (den == 0.0) den = 0.0; // (-0 would turn atan2's result by pi)
  return 0.5 * atan2(2.0 * x, den);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma clang fp contract(off)
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

// the value of function fn for one frame, in every lane of the wavefront: c the frame's F bins (the second transform of a
// frame-delta form), p / pp the bins of the frame before / two before (the frame's own transform twice in a frame-delta
// form), nullptr for a zero spectrum.  The pointers may lead to memory or to the LDS.
__device__ __forceinline__ double frame_value(int fn, int F, int lane, const d2* c, const d2* p, const d2* pp)
{
#pragma clang fp contract(off)
  const double hfcStep = F > 1 ? (double) F / ((double) F - 1.0) : 0.0; // LinSpaced(F, 0, F)
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int k = lane; k < F; k += 64)
  {
    const d2 zc = c[k];
    double v = 0.0;
    if (fn <= 1)
    {
      const double m = hypot(zc[0], zc[1]);
      v = m * m;
      if (fn == 1) v = ((double) k * hfcStep) * v;
    }
    else
    {
      const d2 zp = p ? p[k] : d2{0.0, 0.0};
      const double mc = hypot(zc[0], zc[1]), mp = hypot(zp[0], zp[1]);
      if (fn == 2) v = fmax(mc - mp, 0.0);
      else if (fn == 3) v = log(fmax(fmax(mc, kEps) / fmax(mp, kEps), kEps));
      else if (fn == 4)
      {
        const double q = fmax(mc, kEps) / fmax(mp, kEps);
        const double r = fmax(q * q, kEps);
        v = (r - log(r)) - 1.0;
      }
      else if (fn == 5)
      {
        const double m1 = fmax(mc, kEps), m2 = fmax(mp, kEps);
        v = m1 * m2;
        s1 = s1 + m1 * m1;
        s2 = s2 + m2 * m2;
      }
      else
      {
        const d2 zq = pp ? pp[k] : d2{0.0, 0.0};
        const double ap = catan_re(zp[0], zp[1]), aq = catan_re(zq[0], zq[1]);
        if (fn <= 7)
        {
          double acc = (catan_re(zc[0], zc[1]) - ap) - (ap - aq);
          if (fn == 7) acc = acc * fmax(mc, kEps);
          v = wrap_phase(acc);
        }
        else
        {
          const double est = wrap_phase(ap + (ap - aq));
          const double m2 = fmax(mp, kEps);
          double sn, cs;
          sincos(est, &sn, &cs);
          v = hypot(m2 * cs - zc[0], m2 * sn - zc[1]); // (function 9's max(0) of an absolute value changes nothing)
        }
      }
    }
    s0 = s0 + v;
  }
  s0 = wave_sum(s0);
  double out;
  if (fn == 5)
  {
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    out = 1.0 - s0 / (sqrt(s1) * sqrt(s2));
  }
  else
    out = s0 / (double) F;
  return out;
}

} // namespace onsetdev
} // namespace fluhip
