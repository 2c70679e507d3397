// kernels_range.hip -- what lets the double-precision algorithm entry points (api_algorithms.hip) take input of any finite
// magnitude without touching the kernels of the float hot path: the maximum of |X| on the device, the power-of-two
// rescalings of range_scale.h, and the magnitude of a spectrum by hypot (exact from the smallest subnormal to DBL_MAX, 0 for
// a silent bin: alg/STFT.hpp:61-66 takes std::abs of std::complex).
#include "fluhip_kernels.h"
#include "range_scale.h"

#include <algorithm>

namespace fluhip {

// *out = max(*out, max |p|) over rows x cols (row stride ld).  Non-negative doubles order as their bit patterns, so one
// 64-bit atomicMax per wavefront merges the partial maxima; *out starts at +0.
__global__ __launch_bounds__(256) void absmax_kernel(const double* p, int64_t ld, int rows, int cols, unsigned long long* out)
{
  const int64_t n = (int64_t) rows * cols;
  double m = 0.0;
  for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
    m = fmax(m, fabs(p[(i / cols) * ld + i % cols]));
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off));
  if ((threadIdx.x & 63) == 0 && m > 0.0) atomicMax(out, (unsigned long long) __double_as_longlong(m));
}

void launch_absmax(const double* p, int64_t ld, int rows, int cols, double* out, hipStream_t s)
{
  const int64_t n = (int64_t) rows * cols;
  const unsigned blocks = (unsigned) std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
  hipLaunchKernelGGL(absmax_kernel, dim3(blocks), dim3(256), 0, s, p, ld, rows, cols, reinterpret_cast<unsigned long long*>(out));
}

// p *= 2^(sign e) over rows x cols, e = nmf_range_exponent(*maxAbs) when maxAbs is given (decided on the device: nothing is
// written when e = 0), the fixed exponent otherwise
__global__ __launch_bounds__(256) void scale_pow2_kernel(double* p, int64_t ld, int rows, int cols, const double* maxAbs, int sign,
                                                         int fixedExp)
{
  const int e = maxAbs ? nmf_range_exponent(*maxAbs) : fixedExp;
  if (e == 0) return;
  const int64_t n = (int64_t) rows * cols;
  for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
  {
    double* q = p + (i / cols) * ld + i % cols;
    *q = ldexp(*q, sign * e);
  }
}

static unsigned range_blocks(int rows, int cols)
{
  return (unsigned) std::max<int64_t>(1, std::min<int64_t>(((int64_t) rows * cols + 255) / 256, 4096));
}

void launch_nmf_range_scale(double* p, int64_t ld, int rows, int cols, const double* maxAbs, int sign, hipStream_t s)
{
  hipLaunchKernelGGL(scale_pow2_kernel, dim3(range_blocks(rows, cols)), dim3(256), 0, s, p, ld, rows, cols, maxAbs, sign, 0);
}

void launch_scale_pow2(double* p, int64_t ld, int rows, int cols, int e, hipStream_t s)
{
  if (e == 0) return;
  hipLaunchKernelGGL(scale_pow2_kernel, dim3(range_blocks(rows, cols)), dim3(256), 0, s, p, ld, rows, cols, nullptr, 1, e);
}

// mag[t][k] (row stride ldMag) = |spec[t][k]| for the interleaved (re, im) spectrum [T][F]
__global__ __launch_bounds__(256) void mag_hypot_kernel(const double* spec, int T, int F, double* mag, int64_t ldMag)
{
  const int64_t n = (int64_t) T * F;
  for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t) gridDim.x * blockDim.x)
    mag[(i / F) * ldMag + i % F] = hypot(spec[2 * i], spec[2 * i + 1]);
}

void launch_mag_hypot(const double* spec, int T, int F, double* mag, int64_t ldMag, hipStream_t s)
{
  hipLaunchKernelGGL(mag_hypot_kernel, dim3(range_blocks(T, F)), dim3(256), 0, s, spec, T, F, mag, ldMag);
}

} // namespace fluhip
