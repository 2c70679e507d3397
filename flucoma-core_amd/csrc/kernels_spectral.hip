// kernels_spectral.hip -- K13: the arithmetic of BufSpectralShape and BufChroma.
//   algorithm::SpectralShape      include/flucoma/algorithms/public/SpectralShape.hpp:32-102
//   algorithm::ChromaFilterBank   include/flucoma/algorithms/public/ChromaFilterBank.hpp:83-115
// The kernels here read the magnitudes a round's STFT launch left in a workspace (the two-pass form) or the caller's own
// (the _frames_f64 entry points), doubles throughout; the per-frame arithmetic is in spectral_terms.h, which the on-chip form
// (spectral_fused_kernel, kernels_spectral_fused.hip) shares:
//   shape_frames_kernel     one wavefront per frame: the sums, the central moments in a second pass, the rolloff's running sum
//                           as a wavefront scan with a carry, the log sum and the maximum; seven doubles per frame
//   chroma_power_kernel     one wavefront per frame: the range-zeroed squared magnitudes, the A operand of the GEMM
//                           (cross_gemm_kernel, FP64 MFMA, fluhip_cross.h) with the filter table
//   chroma_epilogue_kernel  one thread per frame: scale, normalize, and the client's channel-major float32 layout
//   shape_select_kernel     the selected descriptors in the client's layout
// Every order of summation depends on the segment alone (spectral_terms.h), so a batch gives the bits of single calls.
// Compiled with -ffp-contract=off and without any fast-math flag.
// Every row pointer is formed at the top of its kernel, in front of the branches that use it.
#include "fluhip_kernels.h"
#include "fluhip_spectral.h"
#include "spectral_terms.h"

#include <cmath>

namespace fluhip {

namespace {

using namespace spectraldev;

__device__ __forceinline__ const double* frame_row(const SpectralFrames& p, int64_t f)
{
  return p.mag + (f / p.T) * p.magStride + (f % p.T) * p.ld;
}

__global__ __launch_bounds__(256) void shape_frames_kernel(SpectralFrames p, ShapeParams sp, double* out)
{
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.nf) return; // (whole wavefronts leave: no partial shuffles)
  const double* m = frame_row(p, f);
  double* o = out + kShapeDescriptors * f;
  shape_frame(m, lane, sp, o);
}

__global__ __launch_bounds__(256) void chroma_power_kernel(SpectralFrames p, int zlo, int zhi, double* pw)
{
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.nf) return;
  const double* m = frame_row(p, f);
  double* row = pw + f * (int64_t) p.F;
  chroma_power_row(m, p.F, lane, zlo, zhi, row);
}

__global__ __launch_bounds__(256) void chroma_epilogue_kernel(const double* acc, int64_t nf, int64_t T, int nChroma, double scale,
                                                              int normalize, double* out64, float* out32)
{
  const int64_t f = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (f >= nf) return;
  const double* a = acc + f * nChroma;
  double* o64 = out64 ? out64 + f * nChroma : nullptr;
  float* o32 = out32 ? out32 + (f / T) * nChroma * T + (f % T) : nullptr;
  double sum = 0.0, mx = -kInf;
  for (int c = 0; c < nChroma; c++)
  {
    const double v = a[c] * scale;
    sum += v;
    if (v > mx) mx = v;
  }
  const double den = fmax(normalize == 1 ? sum : mx, kEps);
  for (int c = 0; c < nChroma; c++)
  {
    double v = a[c] * scale;
    if (normalize > 0) v = v / den;
    if (o64) o64[c] = v;
    if (o32) o32[(int64_t) c * T] = (float) v;
  }
}

__global__ __launch_bounds__(256) void shape_select_kernel(const double* res, int64_t count, int64_t T, int select, float* out32)
{
  const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= count * T) return;
  const int64_t b = e / T, t = e % T;
  const int nsel = __popc((unsigned) select & 127u);
  float* o = out32 + b * nsel * T + t;
  const double* r = res + kShapeDescriptors * e;
  int c = 0;
  for (int i = 0; i < kShapeDescriptors; i++)
    if (select >> i & 1) o[(int64_t) (c++) * T] = (float) r[i];
}

inline unsigned blocks(int64_t n, int per) { return (unsigned) ((n + per - 1) / per); }

} // namespace

SpectralPlan spectral_plan(int64_t fft, int64_t win, int kind)
{
  SpectralPlan p;
  const bool chip = spectral_fused_supported(win, fft);
  p.form = chip ? kSpectralFormOnChip : kSpectralFormTwoPass;
  p.run = chip ? kSpectralRun : 0;
  p.transforms = 1;
  p.gemm = kind == kSpectralChroma ? 1 : 0;
  return p;
}

void launch_shape_frames(const SpectralFrames& p, const ShapeParams& sp, double* out, hipStream_t s)
{
  if (p.nf < 1) return;
  hipLaunchKernelGGL(shape_frames_kernel, dim3(blocks(p.nf, 4)), dim3(256), 0, s, p, sp, out);
}

void launch_shape_select(const double* res, int64_t count, int64_t T, int select, float* out32, hipStream_t s)
{
  if (count * T < 1) return;
  hipLaunchKernelGGL(shape_select_kernel, dim3(blocks(count * T, 256)), dim3(256), 0, s, res, count, T, select, out32);
}

void launch_chroma_power(const SpectralFrames& p, int zlo, int zhi, double* pw, hipStream_t s)
{
  if (p.nf < 1) return;
  hipLaunchKernelGGL(chroma_power_kernel, dim3(blocks(p.nf, 4)), dim3(256), 0, s, p, zlo, zhi, pw);
}

void launch_chroma_epilogue(const double* acc, int64_t nf, int64_t T, int nChroma, double scale, int normalize, double* out64,
                            float* out32, hipStream_t s)
{
  if (nf < 1) return;
  hipLaunchKernelGGL(chroma_epilogue_kernel, dim3(blocks(nf, 256)), dim3(256), 0, s, acc, nf, T, nChroma, scale, normalize, out64,
                     out32);
}

} // namespace fluhip
