// spectral_terms.h -- the per-frame arithmetic of BufSpectralShape and BufChroma, one wavefront per frame, shared by the two
// kernel forms: the kernels of kernels_spectral.hip read a frame's row from a workspace in memory, spectral_fused_kernel
// (kernels_spectral_fused.hip) reads it from the wavefront's staging buffer in the LDS.  One text, so both forms sum and compare
// in the same order: lane l takes the bins l, l + 64, ... of the segment in that order, the 64 partial results meet in a
// butterfly (xor 32 .. 1); the rolloff's running sum walks chunks of 64 with a carry.  The order depends on the segment alone,
// so a frame's value does not depend on its batch, its run or its round.  Contraction is switched off in every function (the
// fused kernel's file is compiled with the default -ffp-contract); comparisons are plain IEEE comparisons.
#pragma once

#include "fluhip_spectral.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {
namespace spectraldev {

constexpr double kEps = 2.220446049250313e-16;         // util/AlgorithmUtils.hpp:19
constexpr double kInf = __builtin_huge_val();
constexpr double kMinNormal = 2.2250738585072014e-308; // DBL_MIN

__device__ __forceinline__ double wave_sum(double v)
{
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    const double u = __shfl_xor(v, o);
    if (u > v) v = u;
  }
  return v;
}

// amp(i) of SpectralShape.hpp:39-61: max(mag, epsilon) first, bin 1 with bin 0 folded in on the MIDI axis, squared for power
__device__ __forceinline__ double shape_amp(const double* m, int i, const ShapeParams& p)
{
#pragma clang fp contract(off)
  double v = fmax(m[p.lo + i], kEps);
  if (p.fold && i == 0) v += fmax(m[0], kEps);
  return p.power ? v * v : v;
}

// SpectralShape::processFrame on the magnitudes m: o[0 .. 6] = centroid, sqrt(spread), skewness, kurtosis, rolloff, flatness
// and crest in dB.  The moments are taken about the centroid in a second pass over m (:71-76), never from raw moments.
__device__ __forceinline__ void shape_frame(const double* m, int lane, const ShapeParams& p, double* o)
{
#pragma clang fp contract(off)
  const int size = p.size;
  double s = 0.0, sf = 0.0, sl = 0.0, mx = -kInf;
  for (int i = lane; i < size; i += 64)
  {
    const double a = shape_amp(m, i, p);
    s += a;
    sf += a * p.axis[i];
    sl += log(a);
    if (a > mx) mx = a;
  }
  s = wave_sum(s);
  sf = wave_sum(sf);
  sl = wave_sum(sl);
  mx = wave_max(mx);
  const double centroid = sf / s;
  double s2 = 0.0, s3 = 0.0, s4 = 0.0;
  for (int i = lane; i < size; i += 64)
  {
    const double a = shape_amp(m, i, p);
    const double d = p.axis[i] - centroid, d2 = d * d;
    s2 += a * d2;
    s3 += a * (d2 * d);
    s4 += a * (d2 * d2);
  }
  s2 = wave_sum(s2);
  s3 = wave_sum(s3);
  s4 = wave_sum(s4);
  // the rolloff (:79-92): the first bin whose running sum reaches the target, interpolated inside that bin
  const double target = s * p.percent / 100.0;
  double roll = p.miss, carry = 0.0;
  for (int i0 = 0; i0 < size; i0 += 64) // (wave-uniform)
  {
    const int i = i0 + lane;
    const double a = i < size ? shape_amp(m, i, p) : 0.0;
    double x = a;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
      const double u = __shfl_up(x, d);
      if (lane >= d) x += u;
    }
    const double run = carry + x;
    const unsigned long long hit = __ballot(i < size && run >= target);
    if (hit)
    {
      const int first = __ffsll((long long) hit) - 1;
      double r = 0.0;
      if (lane == first) r = i == 0 ? p.axis[0] : p.axis[i] - (p.axis[i] - p.axis[i - 1]) * (run - target) / a;
      roll = __shfl(r, first);
      break;
    }
    carry = __shfl(run, 63);
  }
  if (lane == 0)
  {
    const double n = (double) size;
    const double spread = s2 / s, mean = s / n;
    const double flat = exp(sl / n) / mean, crest = mx / mean;
    o[0] = centroid;
    o[1] = sqrt(spread);
    o[2] = s3 / (spread * sqrt(spread) * s);
    o[3] = s4 / (spread * spread * s);
    o[4] = roll;
    o[5] = 20.0 * log10(fmax(flat, kEps));
    o[6] = 20.0 * log10(fmax(crest, kEps));
  }
}

// ChromaFilterBank::processFrame's range zeroing and square (:91-104): row[j] = m[j]^2 for zlo < j < zhi, else 0.  The block
// STFT starts a bin's sum of squares from DBL_MIN (fft_core.h, mag_sumsq), so an exactly zero bin arrives as sqrt(DBL_MIN);
// its square is the zero it stands for.
__device__ __forceinline__ void chroma_power_row(const double* m, int F, int lane, int zlo, int zhi, double* row)
{
#pragma clang fp contract(off)
  for (int j = lane; j < F; j += 64)
  {
    const double q = m[j] * m[j];
    row[j] = (j > zlo && j < zhi) ? (q <= kMinNormal ? 0.0 : q) : 0.0;
  }
}

} // namespace spectraldev
} // namespace fluhip
