// kernels_pitch.hip -- K12: the pitch arithmetic of BufPitch.
//   algorithm::YINFFT         include/flucoma/algorithms/public/YINFFT.hpp:33-91
//   algorithm::HPS            include/flucoma/algorithms/public/HPS.hpp:25-67
//   algorithm::CepstrumF0     include/flucoma/algorithms/public/CepstrumF0.hpp:44-75, DCT.hpp:36-62
//   algorithm::PeakDetection  include/flucoma/algorithms/util/PeakDetection.hpp:30-71
// The kernels here read the magnitudes a round's STFT launch left in a workspace (the two-pass form), doubles throughout;
// the per-frame arithmetic is in pitch_terms.h, which the on-chip form (pitch_fused_kernel, kernels_pitch_fused.hip) shares:
//   pitch_sym_kernel       the even-symmetric squared magnitudes of a frame as `fft` real samples; the STFT launch
//                          transforms them a second time (rectangular window, hop = window = fft)
//   pitch_yin_norm_kernel  one wavefront per frame: 2 sum(sq) - Re, then the running-sum normalisation as a wavefront scan
//                          with a carry over chunks of 64
//   pitch_hps_kernel       one wavefront per frame: the three-factor product, its sum and its argmax
//   pitch_log_kernel, pitch_dct_table_kernel   the operands of the cepstrum's GEMM (cross_gemm_kernel, FP64 MFMA)
//   pitch_peak_kernel      one wavefront per frame: minimum of the segment, the local maxima above it, their interpolated
//                          heights; a butterfly keeps (height, lowest index)
// Every order of summation depends on the bin count alone: lane l takes the bins l, l + 64, ... in that order, the 64
// partial results meet in a butterfly (xor 32 .. 1); the scan is the same for every frame.  So a batch gives the bits of
// single calls.  Comparisons are plain IEEE comparisons: a NaN or inf the normalisation leaves in a degenerate frame fails
// them all.  Compiled with -ffp-contract=off and without any fast-math flag.
// Every row pointer is formed at the top of its kernel, in front of the branches that use it.
#include "fluhip_kernels.h"
#include "fluhip_pitch.h"
#include "pitch_terms.h"

#include <cmath>

namespace fluhip {

namespace {

using namespace pitchdev;

__device__ __forceinline__ const double* frame_row(const PitchFrames& p, int64_t f)
{
  return p.mag + (f / p.T) * p.magStride + (f % p.T) * p.ld;
}

__global__ __launch_bounds__(256) void pitch_sym_kernel(PitchFrames p, double* sym)
{
  const int64_t fft = 2 * (int64_t) (p.F - 1);
  const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= p.nf * fft) return;
  const int64_t f = e / fft, i = e % fft;
  const int64_t j = i < p.F ? i : fft - i; // 1 .. F - 2 behind the Nyquist bin
  sym[e] = yin_square(frame_row(p, f)[j]);
}

__global__ __launch_bounds__(256) void pitch_yin_norm_kernel(PitchFrames p, const double* spec, double* curve, int64_t ldc,
                                                             double* aux)
{
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.nf) return; // (whole wavefronts leave: no partial shuffles)
  const double* m = frame_row(p, f);
  const double* z = spec + f * 2 * (int64_t) p.F;
  double* c = curve + f * ldc;
  const double carry = yin_norm_frame(z, yin_energy2(m, p.F, lane), p.F, lane, c);
  if (lane == 0) aux[f] = carry;
}

__global__ __launch_bounds__(256) void pitch_hps_kernel(PitchFrames p, int lo, int hi, double binHz, double* curve, int64_t ldc,
                                                        double* out)
{
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.nf) return;
  const double* m = frame_row(p, f);
  double* c = curve ? curve + f * ldc : nullptr;
  double* o = out + 2 * f;
  hps_frame(m, p.F, lane, lo, hi, binHz, c, o);
}

__global__ __launch_bounds__(256) void pitch_log_kernel(PitchFrames p, double* lg)
{
  const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= p.nf * p.F) return;
  const int64_t f = e / p.F, j = e % p.F;
  lg[e] = log(fmax(frame_row(p, f)[j], kEpsilon));
}

__global__ __launch_bounds__(256) void pitch_dct_table_kernel(double* table, int64_t n, int64_t first, int64_t rows)
{
  const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * n) return;
  const int64_t r = e / n, j = e % n;
  const int64_t i = r == 0 ? 0 : first + r - 1;
  // cos(pi i (j + 0.5) / n) = cos(pi k / (2 n)), k = i (2 j + 1) mod 4 n: the argument is reduced in integers
  const int64_t k = (i * (2 * j + 1)) % (4 * n);
  const double scale = i == 0 ? 1.0 / sqrt((double) n) : sqrt(2.0 / (double) n);
  table[e] = cospi((double) k / (double) (2 * n)) * scale;
}

// seg[i] = sg * base[i], i < len
__global__ __launch_bounds__(256) void pitch_peak_kernel(int algorithm, const double* curve, int64_t ldc, const double* aux,
                                                         int64_t nf, int off, int len, int minBin, double sampleRate, double* out)
{
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= nf) return;
  const double* row = curve + f * ldc;
  const double* base = row + off;
  double* o = out + 2 * f;
  const bool yin = algorithm == kPitchYinFFT;
  const double gate = yin ? aux[f] : 1.0; // YINFFT.hpp:67
  const double c0 = row[0];               // the cepstrum's value 0 (unused by YinFFT)
  peak_frame(yin, base, len, c0, gate, minBin, sampleRate, lane, o);
}

__global__ __launch_bounds__(256) void pitch_select_kernel(const double* res, int64_t count, int64_t T, int unit, int select,
                                                           float* out32)
{
  const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= count * T) return;
  const int64_t b = e / T, t = e % T;
  const int nsel = (select & 1) + ((select >> 1) & 1);
  float* o = out32 + b * nsel * T + t;
  const double x = res[2 * e], conf = res[2 * e + 1];
  const double pitch = unit == 1 ? (x == 0 ? -999.0 : 69.0 + 12.0 * log2(x / 440.0)) : x;
  int c = 0;
  if (select & 1) o[(int64_t) (c++) * T] = (float) pitch;
  if (select & 2) o[(int64_t) c * T] = (float) conf;
}

__global__ __launch_bounds__(256) void pitch_fill_kernel(double* p, int64_t n, double v)
{
  const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (e < n) p[e] = v;
}

inline unsigned blocks(int64_t n, int per) { return (unsigned) ((n + per - 1) / per); }

} // namespace

PitchPlan pitch_plan(int64_t fft, int64_t win, int algorithm)
{
  PitchPlan p;
  const bool chip = pitch_fused_supported(win, fft);
  p.form = chip ? kPitchFormOnChip : kPitchFormTwoPass;
  p.run = chip ? kPitchRun : 0;
  p.transforms = algorithm == kPitchYinFFT ? 2 : 1;
  return p;
}

void pitch_bins(int algorithm, int64_t F, double minFreq, double maxFreq, double sampleRate, int64_t* minBin, int64_t* maxBin)
{
  // a quotient at or beyond the bin count is clamped before it is rounded: lrint of a huge or infinite value is unspecified
  auto bin = [&](double q) { return q >= (double) F ? F : (int64_t) std::lrint(q); };
  int64_t lo, hi;
  if (algorithm == kPitchYinFFT)
  {
    if (maxFreq == 0) maxFreq = 1;
    if (minFreq == 0) minFreq = 1;
    lo = bin(sampleRate / maxFreq);
    hi = bin(sampleRate / minFreq);
    if (lo > F - 1) lo = F - 1;
    if (hi > F - lo - 1) hi = F - lo - 1;
  }
  else if (algorithm == kPitchHPS)
  {
    const double binHz = sampleRate / (double) ((F - 1) * 2);
    lo = bin(minFreq / binHz);
    hi = bin(maxFreq / binHz); // (the reference reads past the array above F: clamped here)
  }
  else
  {
    lo = bin(sampleRate / maxFreq);
    hi = bin(sampleRate / minFreq);
  }
  *minBin = lo;
  *maxBin = hi;
}

void launch_pitch_sym(const PitchFrames& p, double* sym, hipStream_t s)
{
  const int64_t n = p.nf * 2 * (int64_t) (p.F - 1);
  if (n < 1) return;
  hipLaunchKernelGGL(pitch_sym_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, p, sym);
}

void launch_pitch_yin_norm(const PitchFrames& p, const double* spec, double* curve, int64_t ldc, double* aux, hipStream_t s)
{
  if (p.nf < 1) return;
  hipLaunchKernelGGL(pitch_yin_norm_kernel, dim3(blocks(p.nf, 4)), dim3(256), 0, s, p, spec, curve, ldc, aux);
}

void launch_pitch_hps(const PitchFrames& p, int64_t minBin, int64_t maxBin, double sampleRate, double* curve, int64_t ldc,
                      double* out, hipStream_t s)
{
  if (p.nf < 1) return;
  const double binHz = sampleRate / (double) ((p.F - 1) * 2);
  const int lo = (int) std::min<int64_t>(minBin, p.F), hi = (int) std::min<int64_t>(maxBin, p.F);
  hipLaunchKernelGGL(pitch_hps_kernel, dim3(blocks(p.nf, 4)), dim3(256), 0, s, p, lo, hi, binHz, curve, ldc, out);
}

void launch_pitch_log(const PitchFrames& p, double* lg, hipStream_t s)
{
  const int64_t n = p.nf * p.F;
  if (n < 1) return;
  hipLaunchKernelGGL(pitch_log_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, p, lg);
}

void launch_pitch_dct_table(double* table, int64_t n, int64_t first, int64_t rows, hipStream_t s)
{
  if (rows * n < 1) return;
  hipLaunchKernelGGL(pitch_dct_table_kernel, dim3(blocks(rows * n, 256)), dim3(256), 0, s, table, n, first, rows);
}

void launch_pitch_peak(int algorithm, const double* curve, int64_t ldc, const double* aux, int64_t nf, int64_t minBin,
                       int64_t maxBin, double sampleRate, double* out, hipStream_t s)
{
  if (nf < 1) return;
  const int off = algorithm == kPitchYinFFT ? (int) minBin : 1;
  const int len = (int) std::max<int64_t>(0, maxBin - minBin);
  hipLaunchKernelGGL(pitch_peak_kernel, dim3(blocks(nf, 4)), dim3(256), 0, s, algorithm, curve, ldc, aux, nf, off, len,
                     (int) minBin, sampleRate, out);
}

void launch_pitch_select(const double* res, int64_t count, int64_t T, int unit, int select, float* out32, hipStream_t s)
{
  if (count * T < 1) return;
  hipLaunchKernelGGL(pitch_select_kernel, dim3(blocks(count * T, 256)), dim3(256), 0, s, res, count, T, unit, select, out32);
}

void launch_pitch_fill(double* p, int64_t n, double v, hipStream_t s)
{
  if (n < 1) return;
  hipLaunchKernelGGL(pitch_fill_kernel, dim3(blocks(n, 256)), dim3(256), 0, s, p, n, v);
}

} // namespace fluhip
