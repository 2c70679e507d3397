// pitch_terms.h -- the per-frame arithmetic of BufPitch, one wavefront per frame, shared by the two kernel forms: the
// kernels of kernels_pitch.hip read a frame's row from a workspace in memory, pitch_fused_kernel (kernels_pitch_fused.hip) reads
// it from the wavefront's staging buffer in the LDS.  One text, so both forms sum and compare in the same order: lane l
// takes the bins l, l + 64, ... in that order, the 64 partial results meet in a butterfly (xor 32 .. 1); the scan walks
// chunks of 64 with a carry.  Contraction is switched off in every function (the fused kernel's file is compiled with the
// default -ffp-contract); comparisons are plain IEEE comparisons, a NaN fails them all.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {
namespace pitchdev {

constexpr double kInf = __builtin_huge_val();
constexpr double kMinNormal = 2.2250738585072014e-308; // DBL_MIN

// YinFFT's squared magnitude.  The block STFT starts a bin's sum of squares from DBL_MIN (fft_core.h, mag_sumsq), so an
// exactly zero bin arrives as sqrt(DBL_MIN); its square is the zero it stands for.  YinFFT is invariant under scaling, so
// without this digital silence would be analysed as a flat spectrum where the reference returns (0, 0).
__device__ __forceinline__ double yin_square(double v)
{
#pragma clang fp contract(off)
  const double q = v * v;
  return q <= kMinNormal ? 0.0 : q;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// 2 sum(sq) over the F magnitudes m (YINFFT.hpp:56)
__device__ __forceinline__ double yin_energy2(const double* m, int F, int lane)
{
#pragma clang fp contract(off)
  double s = 0.0;
  for (int j = lane; j < F; j += 64) s += yin_square(m[j]);
  return 2.0 * wave_sum(s);
}

// z: the transform of the symmetric squares, interleaved complex.  c[i] = the normalised yin, i < F (YINFFT.hpp:54-64);
// returns the final running sum
__device__ __forceinline__ double yin_norm_frame(const double* z, double s2, int F, int lane, double* c)
{
#pragma clang fp contract(off)
  double carry = 0.0;
  for (int i0 = 0; i0 < F; i0 += 64)
  {
    const int i = i0 + lane;
    const double y = (i >= 1 && i < F) ? s2 - z[2 * (int64_t) i] : 0.0;
    double x = y;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
      const double u = __shfl_up(x, d);
      if (lane >= d) x += u;
    }
    const double run = carry + x;
    if (i < F) c[i] = i == 0 ? 1.0 : y * ((double) i / run);
    carry = __shfl(run, 63);
  }
  return carry;
}

// HPS.hpp:49-67 on the F magnitudes m: c[j] = m[j] m[2 j] m[3 j] where c is given, o = (f0, confidence)
__device__ __forceinline__ void hps_frame(const double* m, int F, int lane, int lo, int hi, double binHz, double* c, double* o)
{
#pragma clang fp contract(off)
  const int h2 = F / 2, h3 = F / 3;
  double s = 0.0, best = -kInf;
  int bi = 0x7fffffff;
  for (int j = lane; j < F; j += 64)
  {
    const double v = (m[j] * (j < h2 ? m[2 * j] : 0.0)) * (j < h3 ? m[3 * j] : 0.0);
    if (c) c[j] = v;
    s += v;
    if (j >= lo && j < hi && v > best)
    {
      best = v;
      bi = j;
    }
  }
  s = wave_sum(s);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
  {
    const double ov = __shfl_xor(best, d);
    const int oi = __shfl_xor(bi, d);
    if (ov > best || (ov == best && oi < bi))
    {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0)
  {
    const bool ok = hi > lo && s > 0.0 && bi != 0x7fffffff;
    o[0] = ok ? (double) bi * binHz : 0.0;
    o[1] = ok ? best / s : 0.0;
  }
}

// PeakDetection::process(seg, 1, seg.minCoeff(), true, true) and the algorithm's result from its first peak.
// seg[i] = sg base[i], i < len, sg = -1 for YinFFT; c0: the cepstrum's value 0; gate: YinFFT's final running sum
__device__ __forceinline__ void peak_frame(bool yin, const double* base, int len, double c0, double gate, int minBin,
                                           double sampleRate, int lane, double* o)
{
#pragma clang fp contract(off)
  const double sg = yin ? -1.0 : 1.0;
  double mn = kInf;
  for (int i = lane; i < len; i += 64)
  {
    const double v = sg * base[i];
    if (v < mn) mn = v;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
  {
    const double ov = __shfl_xor(mn, d);
    if (ov < mn) mn = ov;
  }
  double bh = -kInf;
  int bi = -1;
  for (int i = 1 + lane; i < len - 1; i += 64)
  {
    const double cur = sg * base[i], prev = sg * base[i - 1], next = sg * base[i + 1];
    if (cur > prev && cur > next && cur > mn)
    {
      const double q = 0.5 * (prev - next) / (prev - 2 * cur + next);
      const double h = cur - 0.25 * (prev - next) * q;
      if (h > bh)
      {
        bh = h;
        bi = i;
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
  {
    const double oh = __shfl_xor(bh, d);
    const int oi = __shfl_xor(bi, d);
    if (oi >= 0 && (oh > bh || (oh == bh && (bi < 0 || oi < bi))))
    {
      bh = oh;
      bi = oi;
    }
  }
  if (lane == 0)
  {
    double pitch = 0.0, conf = 0.0;
    if (bi >= 1 && gate > 0.0) // (bi <= len - 2: the neighbours are inside the segment)
    {
      const double cur = sg * base[bi], prev = sg * base[bi - 1], next = sg * base[bi + 1];
      const double q = 0.5 * (prev - next) / (prev - 2 * cur + next);
      const double pos = (double) bi + q;
      pitch = sampleRate / ((double) minBin + pos);
      if (yin)
        conf = (1.0 + bh) < 0.0 ? 0.0 : 1.0 + bh; // std::max(1. + height, 0.)
      else
        conf = 1.0 < fabs(bh / c0) ? 1.0 : fabs(bh / c0); // std::min(abs(height / cepstrum[0]), 1.0)
    }
    o[0] = pitch;
    o[1] = conf;
  }
}

} // namespace pitchdev
} // namespace fluhip
