// range_scale.h -- the power-of-two rescalings that carry double-precision input of any magnitude through kernels whose
// intermediate values have a narrower range (host and device; tests/cpp/range_scale_host.cpp checks them on the host).
//
// NMF (fluhip_nmf_process_*_f64): the reciprocal trees of the factor updates (recip_tree.h) take one reciprocal of a product
// of up to six clamped W H values; with max|X| <= 2^128 every such product stays normal and finite.  A larger input is
// scaled by 2^-e with the smallest e that brings its maximum to <= 2^128 -- exact, and H scales with X through the
// multiplicative updates while W (normalised every iteration) does not -- and H1 / V1 are scaled back by 2^e.  Input at or
// below 2^128 is not touched (e = 0), so its arithmetic is bit for bit what it was without the rescaling.
//
// SVD (NNDSVD's one-sided Jacobi): the rows' sums of squares are formed unscaled; 2^-e with max|X| 2^-e in [0.5, 1) keeps
// them inside the double range from the smallest normal to DBL_MAX (as Eigen's and LAPACK's SVDs scale first).
#pragma once

#include <cfloat>
#include <cmath>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace fluhip {

constexpr int kNmfRangeLog2 = 128; // the largest max|X| the factor updates take unscaled: 2^128

// e >= 0 such that max_abs 2^-e <= 2^128, the smallest one; 0 for max_abs <= 2^128 (and for NaN / inf, which are not scaled)
__host__ __device__ inline int nmf_range_exponent(double max_abs)
{
  if (!(max_abs > 0x1p128 && max_abs <= DBL_MAX)) return 0;
  int x;
  const double f = frexp(max_abs, &x);     // max_abs = f 2^x, f in [0.5, 1)
  const int c = f == 0.5 ? x - 1 : x;      // ceil(log2(max_abs))
  return c - kNmfRangeLog2;
}

// e such that max_abs 2^-e lies in [0.5, 1); 0 for zero or a non-finite maximum
__host__ __device__ inline int svd_range_exponent(double max_abs)
{
  if (!(max_abs > 0 && max_abs <= DBL_MAX)) return 0;
  int x;
  frexp(max_abs, &x);
  return x;
}

} // namespace fluhip
