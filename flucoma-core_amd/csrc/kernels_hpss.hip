// kernels_hpss.hip -- K11: the median-filter masks of BufHPSS.
//   algorithm::HPSS::processFrame   include/flucoma/algorithms/public/HPSS.hpp:66-152
//   algorithm::MedianFilter         include/flucoma/algorithms/util/MedianFilter.hpp:34-56
// One launch over the magnitude plane(s) mag [count][T][ldMag], row t = frame m = t + 1.  A workgroup of 256 threads owns
// one frame and 256 consecutive bins of it, lane = bin, so every read of the row-major plane is coalesced.  Per (t, f):
//   V median  the value of rank vSize / 2 among the bins f .. f + vSize - 1 of row t, zeros past the last bin (the
//             reference filters a zero-padded copy and reads it back at offset 3 v2: forward-looking, not centred);
//   H median  the value of rank hSize / 2 among the rows t - h2 - 1 .. t + h2 - 1 of bin f, zeros outside 0 .. T - 1 BY INDEX
//             TEST (the reference writes the filter's output to column h2 + 1 and reads column 0: centred one frame before
//             the frame it masks); no row outside the plane is ever addressed;
//   masks     HPSS.hpp:106-151, plain IEEE double division and comparison (0 / 0 is NaN and compares false, x / 0 is +inf
//             and compares true), every mask through min(1, .); the three masked spectra and / or the planes are written.
// A median is a SELECTION (MedianFilter returns mSorted[size / 2]; no arithmetic touches the values): the value w with
// #(x < w) <= size / 2 < #(x <= w), found by counting as in onset_filter_kernel -- O(size^2) compares per value, bit-identical
// to a sort of the same magnitudes.  On-chip form (either filter, size <= kHpssMaxOnChip = 63): the window is copied once
// to the LDS -- [hSize][256] doubles for H, 256 + vSize - 1 for V, both read without bank conflicts (consecutive lanes,
// consecutive doubles) -- and counted from there.  Beyond that the same count runs straight on the plane in memory.
// Compiled with -ffp-contract=off: the mask arithmetic is the plain operations written here.
#include "fluhip_hpss.h"
#include "fluhip_kernels.h"

#include <algorithm>

namespace fluhip {

namespace {

typedef double d2 __attribute__((ext_vector_type(2)));

// the value of rank size / 2 among get(0 .. size - 1)
template <class Get> __device__ __forceinline__ double select_median(Get get, int size)
{
  const int k = size / 2;
  double med = 0.0;
  for (int j = 0; j < size; j++)
  {
    const double wj = get(j);
    int less = 0, eq = 0;
    for (int q = 0; q < size; q++)
    {
      const double wq = get(q);
      less += wq < wj;
      eq += wq == wj;
    }
    if (less <= k && k < less + eq)
    {
      med = wj;
      break;
    }
  }
  return med;
}

template <bool HOnChip, bool VOnChip> __global__ __launch_bounds__(kHpssBinTile) void hpss_mask_kernel(HpssArgs a, int64_t b0, int tiles)
{
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const int64_t blk = blockIdx.x;
  const int tile = (int) (blk % tiles);
  const int t = (int) ((blk / tiles) % a.T);
  const int64_t b = b0 + blk / ((int64_t) tiles * a.T);
  const int T = a.T, F = a.F;
  const int f = tile * kHpssBinTile + tid;
  const int h2 = (a.hSize - 1) / 2;
  const double* plane = a.mag + b * a.magStride;
  const double* row = plane + (int64_t) t * a.ldMag;
  double* ldsH = lds;                                                       // [hSize][256] (on-chip H only)
  double* ldsV = lds + (HOnChip ? (int64_t) a.hSize * kHpssBinTile : 0);    // [256 + vSize - 1] (on-chip V only)
  const int r0 = t - h2 - 1; // first row of the H window
  if (HOnChip)
    for (int j = 0; j < a.hSize; j++)
    {
      const int r = r0 + j;
      ldsH[j * kHpssBinTile + tid] = (r >= 0 && r < T && f < F) ? plane[(int64_t) r * a.ldMag + f] : 0.0;
    }
  if (VOnChip)
    for (int i = tid; i < kHpssBinTile + a.vSize - 1; i += kHpssBinTile)
    {
      const int g = tile * kHpssBinTile + i;
      ldsV[i] = g < F ? row[g] : 0.0;
    }
  if (HOnChip || VOnChip) __syncthreads();
  if (f >= F) return;
  // every address and every load of the mask stage is formed HERE, in front of the mode's branches, which are then
  // arithmetic only: with the index formed behind them the compiler left it undefined on the mode 2 path
  const int64_t tf = (int64_t) t * F + f;
  const int64_t at = (int64_t) b * T * F + tf;
  const double thH = a.thrH[f], thP = a.thrP[f]; // (both tables are always there)

  double h, v;
  if (HOnChip)
    h = select_median([&](int j) { return ldsH[j * kHpssBinTile + tid]; }, a.hSize);
  else
    h = select_median([&](int j) { const int r = r0 + j; return (r >= 0 && r < T) ? plane[(int64_t) r * a.ldMag + f] : 0.0; }, a.hSize);
  if (VOnChip)
    v = select_median([&](int q) { return ldsV[tid + q]; }, a.vSize);
  else
    v = select_median([&](int q) { return f + q < F ? row[f + q] : 0.0; }, a.vSize);

  double hm, pm, rm;
  if (a.mode == 0)
  {
    const double mult = 1.0 / fmax(h + v, kEpsilon); // :115
    hm = h * mult;
    pm = v * mult;
    rm = 0.0;
  }
  else if (a.mode == 1)
  {
    hm = (h / v) > thH ? 1.0 : 0.0; // :121-124
    pm = 1.0 - hm;
    rm = 0.0;
  }
  else
  {
    hm = (h / v) > thH ? 1.0 : 0.0; // :129-136
    pm = (v / h) > thP ? 1.0 : 0.0;
    rm = 1.0 * (1.0 - hm);                // :138-139
    rm = rm * (1.0 - pm);
    const double norm = fmax(1.0 / (hm + pm + rm), kEpsilon); // :141-142
    hm = hm * norm;
    pm = pm * norm;
    rm = rm * norm;
  }
  hm = fmin(hm, 1.0); // :149-151
  pm = fmin(pm, 1.0);
  rm = fmin(rm, 1.0);

  if (a.hmed) a.hmed[at] = h;
  if (a.vmed) a.vmed[at] = v;
  if (a.masks[0]) a.masks[0][at] = hm;
  if (a.masks[1]) a.masks[1][at] = pm;
  if (a.masks[2]) a.masks[2][at] = rm;
  if (a.out)
  {
    const d2 x = reinterpret_cast<const d2*>(a.spec + b * a.specStride)[tf];
    d2* o = reinterpret_cast<d2*>(a.out + b * a.outStride) + tf;
    const int64_t one = (int64_t) T * F;
    o[0] = d2{x[0] * hm, x[1] * hm};
    o[one] = d2{x[0] * pm, x[1] * pm};
    o[2 * one] = d2{x[0] * rm, x[1] * rm};
  }
}

template <bool HOnChip, bool VOnChip> void launch_form(const HpssArgs& a, const HpssPlan& p, hipStream_t s)
{
  const int tiles = (a.F + kHpssBinTile - 1) / kHpssBinTile;
  const int64_t perBuffer = (int64_t) tiles * a.T;
  const int64_t per = std::max<int64_t>(1, ((int64_t) 1 << 30) / perBuffer); // buffers per launch: the grid stays below 2^31
  request_dynamic_lds(hpss_mask_kernel<HOnChip, VOnChip>, (size_t) (160 * 1024));
  for (int64_t b0 = 0; b0 < a.count; b0 += per)
  {
    const int64_t nb = std::min(per, a.count - b0);
    hipLaunchKernelGGL((hpss_mask_kernel<HOnChip, VOnChip>), dim3((unsigned) (nb * perBuffer)), dim3(kHpssBinTile),
                       (size_t) p.ldsBytes, s, a, b0, tiles);
  }
}

} // namespace

HpssPlan hpss_plan(int64_t hSize, int64_t vSize)
{
  HpssPlan p;
  p.formH = hSize <= kHpssMaxOnChip ? kHpssFormOnChip : kHpssFormMemory;
  p.formV = vSize <= kHpssMaxOnChip ? kHpssFormOnChip : kHpssFormMemory;
  p.ldsBytes = 0;
  if (p.formH == kHpssFormOnChip) p.ldsBytes += hSize * kHpssBinTile * (int64_t) sizeof(double);
  if (p.formV == kHpssFormOnChip) p.ldsBytes += (kHpssBinTile + vSize - 1) * (int64_t) sizeof(double);
  p.binTile = kHpssBinTile;
  return p;
}

void launch_hpss_masks(const HpssArgs& a, hipStream_t s)
{
  if (a.count < 1 || a.T < 1 || a.F < 1) return;
  const HpssPlan p = hpss_plan(a.hSize, a.vSize);
  const bool hc = p.formH == kHpssFormOnChip, vc = p.formV == kHpssFormOnChip;
  if (hc && vc) launch_form<true, true>(a, p, s);
  else if (hc) launch_form<true, false>(a, p, s);
  else if (vc) launch_form<false, true>(a, p, s);
  else launch_form<false, false>(a, p, s);
}

} // namespace fluhip
