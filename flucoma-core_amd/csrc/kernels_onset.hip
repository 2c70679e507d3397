// kernels_onset.hip -- K10: the spectral onset detection functions of BufOnsetSlice / BufOnsetFeature.
//   algorithm::OnsetDetectionFuncs      include/flucoma/algorithms/util/OnsetDetectionFuncs.hpp:31-128
//   algorithm::MedianFilter             include/flucoma/algorithms/util/MedianFilter.hpp:34-56
//   algorithm::OnsetDetectionFunctions  include/flucoma/algorithms/public/OnsetDetectionFunctions.hpp:70-114
//   algorithm::OnsetSegmentation        include/flucoma/algorithms/public/OnsetSegmentation.hpp:46-66
// Three kernels, doubles throughout:
//   onset_reduce_kernel  one wavefront per frame: every bin of the frame's spectrum against the one or two spectra before it
//                        (zero spectra before the start) or against the second transform of a frame-delta form; one double
//                        per frame.  The spectra are those the STFT launch of the round wrote (the two-pass form; the
//                        on-chip form for fft 1024 / 2048 / 4096 is onset_fused_kernel, kernels_onset_fused.hip).
//   onset_filter_kernel  one thread per frame: the value minus the median of the last filterSize values.
//   onset_detect_kernel  one wavefront per buffer: threshold crossings in parallel, the debounce as a scan over them.
// The order of a frame's sum is fixed: lane l adds the bins l, l + 64, l + 128, ... in that order, the 64 partial sums
// then meet in a butterfly (xor 32, 16, ... 1).  Nothing in it depends on the batch, the round or the frame's place in
// it, so a batch gives the bits of single calls.  Compiled with -ffp-contract=off: the sums are the plain operations
// written here.
#include "fluhip_onset.h"
#include "onset_terms.h"

namespace fluhip {

namespace {

using onsetdev::d2;

__global__ __launch_bounds__(256) void onset_reduce_kernel(OnsetReduceArgs a)
{
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.count * a.nt) return; // (whole wavefronts leave: no partial shuffles)
  const int64_t b = w / a.nt;
  const int t = a.t0 + (int) (w % a.nt);
  const int F = a.F;
  const int64_t row = (int64_t) (t - a.f0) * F;
  const d2* base = reinterpret_cast<const d2*>(a.spec + b * a.specStride);
  const d2* cur = base + row;
  // f(cur = second transform, prev = own transform) with a frame delta; else the stored frames, zero before the start
  const d2* c = a.spec2 ? reinterpret_cast<const d2*>(a.spec2 + b * a.specStride) + row : cur;
  // (rows in front of `cur` exist only as far as the plan's history goes: f0 <= t - history whenever t >= history)
  const d2* p = a.spec2 ? cur : (a.history >= 1 && t >= 1 ? cur - F : nullptr);
  const d2* pp = a.spec2 ? cur : (a.history >= 2 && t >= 2 ? cur - 2 * (int64_t) F : nullptr);
  const double out = onsetdev::frame_value(a.function, F, lane, c, p, pp);
  if (lane == 0) a.raw[b * a.T + t] = out;
}

__global__ __launch_bounds__(256) void onset_filter_kernel(const double* raw, double* filtered, int T, int64_t count, int f)
{
  const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= count * T) return;
  const int t = (int) (i % T);
  const double v = raw[i];
  if (f < 3)
  {
    filtered[i] = v;
    return;
  }
  // the value of rank f / 2 among the last f values (zeros before the start), by counting: no sorted copy is kept
  const double* r = raw + (i - t);
  const int lo = t - f + 1, k = f / 2;
  double med = v;
  for (int j = 0; j < f; j++)
  {
    const double wj = lo + j >= 0 ? r[lo + j] : 0.0;
    int less = 0, eq = 0;
    for (int q = 0; q < f; q++)
    {
      const double wq = lo + q >= 0 ? r[lo + q] : 0.0;
      less += wq < wj;
      eq += wq == wj;
    }
    if (less <= k && k < less + eq)
    {
      med = wj;
      break;
    }
  }
  filtered[i] = v - med;
}

__global__ __launch_bounds__(64) void onset_detect_kernel(const double* filtered, int T, int64_t count, double threshold,
                                                           int minSlice, unsigned char* det, int64_t* counts)
{
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const double* f = filtered + b * T;
  unsigned char* d = det + b * T;
  // a frame detects when it crosses the threshold upwards with the debounce counter at zero; the counter is set to minSlice
  // by a detection and falls by one per frame after it, so it is zero again minSlice + 1 frames on
  int64_t last = -1, n = 0;
  bool any = false;
  for (int t0 = 0; t0 < T; t0 += 64)
  {
    const int t = t0 + lane;
    bool cand = false;
    if (t < T)
    {
      const double prev = t >= 1 ? f[t - 1] : 0.0;
      cand = f[t] > threshold && prev < threshold;
    }
    unsigned long long mask = __ballot(cand);
    unsigned long long hit = 0;
    while (mask)
    {
      const int i = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int64_t tt = (int64_t) t0 + i;
      if (!any || tt - last > (int64_t) minSlice)
      {
        hit |= 1ull << i;
        last = tt;
        any = true;
        n++;
      }
    }
    if (t < T) d[t] = (unsigned char) ((hit >> lane) & 1ull);
  }
  if (lane == 0) counts[b] = n;
}

} // namespace

OnsetPlan onset_plan(int64_t fft, int64_t win, int function, int64_t frameDelta)
{
  OnsetPlan p;
  p.form = onset_fused_supported(win, fft) ? kOnsetFormOnChip : kOnsetFormTwoPass;
  p.history = onset_history(function, frameDelta);
  p.transforms = onset_uses_delta(function, frameDelta) ? 2 : 1;
  p.run = p.form == kOnsetFormOnChip ? kOnsetRun : 0;
  return p;
}

void launch_onset_reduce(const OnsetReduceArgs& a, hipStream_t s)
{
  const int64_t waves = a.count * a.nt;
  if (waves < 1) return;
  hipLaunchKernelGGL(onset_reduce_kernel, dim3((unsigned) ((waves + 3) / 4)), dim3(256), 0, s, a);
}

void launch_onset_filter(const double* raw, double* filtered, int T, int64_t count, int filterSize, hipStream_t s)
{
  const int64_t n = count * T;
  if (n < 1) return;
  hipLaunchKernelGGL(onset_filter_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, raw, filtered, T, count, filterSize);
}

void launch_onset_detect(const double* filtered, int T, int64_t count, double threshold, int minSlice, unsigned char* det,
                         int64_t* counts, hipStream_t s)
{
  if (count < 1 || T < 1) return;
  hipLaunchKernelGGL(onset_detect_kernel, dim3((unsigned) count), dim3(64), 0, s, filtered, T, count, threshold, minSlice, det,
                     counts);
}

} // namespace fluhip
