// kernels_amp.hip -- K15: BufAmpSlice / BufAmpFeature, the clients without frames: every sample depends on the one before.
//   algorithm::Envelope              include/flucoma/algorithms/public/Envelope.hpp:36-61
//   algorithm::EnvelopeSegmentation  include/flucoma/algorithms/public/EnvelopeSegmentation.hpp:36-60
//   algorithm::ButterworthHPFilter   include/flucoma/algorithms/util/ButterworthHPFilter.hpp:23-46
//   algorithm::SlideUDFilter         include/flucoma/algorithms/util/SlideUDFilter.hpp:19-37
// What is linear in the samples is parallel in time, what is not is not:
//   amp_hold_kernel            lane = chunk of kAmpChunk samples: the last finite sample of the chunk, and of the chunk less its
//                              last sample (NaN: there is none) -- the hold of non-finite samples is a max-scan of "index of the
//                              last finite sample", and a chunk asks the chunks before it only when it starts with samples that
//                              are not finite
//   amp_filter_kernel<false>   lane = chunk: the two high-pass sections run over the held samples from ZERO output state (the
//                              inputs in front of the chunk are known), the end state q_c, carried as double-doubles
//   amp_scan_kernel            4 lanes per signal: s_{c+1} = M s_c + q_c, M = A^kAmpChunk.  The poles of a low cutoff sit next
//                              to z = 1 and M's entries reach 9.2e2 (1 Hz at 44.1 kHz): M (built on the host), q and the
//                              carried state are double-double pairs, as in kernels_loudness.hip; the state is rounded to
//                              double once per chunk, where the chunk takes it
//   amp_filter_kernel<true>    lane = chunk: the chunk run again from its true entering state, in plain double and in the
//                              reference's order of operations; 20 log10 |.| clipped at the floor, to the level workspace
//   amp_follow_pair_kernel     a lane PAIR per signal, serial in time: one SlideUDFilter each, the fast one's lane also
//                              the detector's three words of state.  A follower picks its coefficient by comparing the input
//                              with its own state, so the map of a chunk is not affine and there is no scan; nothing here
//                              approximates one.  The parallelism is the signals of the call
// Lanes that own consecutive chunks (or signals) read kAmpChunk (or n) samples apart: a wavefront stages kAmpTile samples of each
// of its 64 rows through the LDS (rows of kAmpTile + 1 doubles), so that global reads and writes are runs of consecutive
// samples.  The follower kernel holds the next tile in registers while it walks the current one.
// Every order of operations depends on the sample's position in its signal alone (the chunk length is a constant), so a batch
// gives the bits of single calls.  Compiled with -ffp-contract=off: the reference's y0 + (b * (x - y0)) is three roundings.
#include "fluhip_amp.h"
#include "fluhip_dd.h"

#include <cmath>

namespace fluhip {

namespace {

constexpr int kPitch = kAmpTile + 1;
constexpr int kPerLane = kAmpTile; // elements of a 64 x kAmpTile tile a lane moves

template <typename TIn> __device__ __forceinline__ const TIn* rows_of(const AmpSignals& p);
template <> __device__ __forceinline__ const float* rows_of<float>(const AmpSignals& p) { return p.x32; }
template <> __device__ __forceinline__ const double* rows_of<double>(const AmpSignals& p) { return p.x64; }

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; } // false for NaN and +-inf

// hold[(sig chunks + c) 2 + {0, 1}]: chunk c's last finite sample, and the last one in front of its last sample; NaN where
// there is none.  Only whole chunks are asked (a chunk behind them exists).
template <typename TIn> __global__ __launch_bounds__(256) void amp_hold_kernel(AmpSignals p, int64_t chunks, double* hold)
{
  const int64_t slot = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (slot >= p.count * chunks) return;
  const int64_t sig = slot / chunks, c = slot % chunks;
  const double none = __longlong_as_double(0x7ff8000000000000ll);
  double v1 = none, v2 = none;
  if ((c + 1) * kAmpChunk <= p.n)
  {
    const TIn* x = rows_of<TIn>(p) + sig * p.stride + c * kAmpChunk;
    int i = kAmpChunk - 1;
    for (; i >= 0; i--)
    {
      const double v = (double) x[i];
      if (finite_d(v)) { v1 = v; break; }
    }
    if (i >= 0 && i < kAmpChunk - 1) v2 = v1;
    else if (i == kAmpChunk - 1)
      for (i = kAmpChunk - 2; i >= 0; i--)
      {
        const double v = (double) x[i];
        if (finite_d(v)) { v2 = v; break; }
      }
  }
  hold[slot * 2] = v1;
  hold[slot * 2 + 1] = v2;
}

// the held sample at the last position of chunk j or in front of it (0 before the first finite sample: mPrevValid's start)
__device__ __forceinline__ double held_before(const double* holdSig, int64_t j)
{
  for (; j >= 0; j--)
  {
    const double v = holdSig[j * 2];
    if (v == v) return v;
  }
  return 0.0;
}

// a double times a double, and a double-double times a double, as double-doubles
__device__ __forceinline__ dd two_prod(double a, double b)
{
  const double p = a * b;
  return {p, fma(a, b, -p)};
}
__device__ __forceinline__ dd dd_mul_d(dd a, double b)
{
  const double p = a.hi * b;
  const double e = fma(a.hi, b, -p) + a.lo * b;
  return quick_two_sum(p, e);
}

// Wavefront w owns slots w 64 .. w 64 + 63 of the count x chunks chunks, lane r slot w 64 + r.
// kSecond false: from zero output state, writes the end state to io[slot][4][2] (hi, lo).  This pass alone carries its four
// outputs as double-doubles: started from zero against the true inputs a chunk's outputs run up to |M| times the size of
// the true ones (8.97 against 0.002 on the drum loop at 1 Hz) and cancel against M s in the scan, so roundings of THEIR size
// would come back |M| times too large -- measured on the CPU, plain double here left the 1 Hz envelope 82 floors from the
// model, long double 1.0.  kSecond true: from st[slot][4], in plain double and the reference's order, writes the clipped
// level of every sample to io[sig n + i].  highPass 0: no filter (only kSecond is launched then).
template <typename TIn, bool kSecond>
__global__ __launch_bounds__(64) void amp_filter_kernel(AmpSignals p, int64_t chunks, AmpHighPass f, const double* hold, double floorDb,
                                                        const double* st, double* io)
{
  __shared__ double tile[64 * kPitch];
  __shared__ int64_t rowSrc[64], rowDst[64];
  __shared__ int rowLen[64];
  const int r = threadIdx.x;
  const int64_t slot = (int64_t) blockIdx.x * 64 + r;
  const bool live = slot < p.count * chunks;
  const int64_t sig = live ? slot / chunks : 0, c = live ? slot % chunks : 0;
  const int64_t left = p.n - c * kAmpChunk;
  const int len = !live ? 0 : left < kAmpChunk ? (int) left : kAmpChunk;
  rowSrc[r] = sig * p.stride + c * kAmpChunk;
  rowDst[r] = sig * p.n + c * kAmpChunk;
  rowLen[r] = len;
  // Envelope::processSample :44-45 and the two sections' mXnz1 / mXnz2 entering the chunk: the held samples at c0 - 1, c0 - 2
  double prevValid = 0, x1 = 0, x2 = 0;
  if (live && c > 0)
  {
    const double* hs = hold + sig * chunks * 2;
    prevValid = held_before(hs, c - 1);
    const double v2 = hs[(c - 1) * 2 + 1];
    x1 = prevValid;
    x2 = v2 == v2 ? v2 : held_before(hs, c - 2);
  }
  double y1a = 0, y1b = 0, y2a = 0, y2b = 0; // y1[n-1], y1[n-2], y2[n-1], y2[n-2]
  dd z1a = {0, 0}, z1b = {0, 0}, z2a = {0, 0}, z2b = {0, 0}; // the same of the zero-state pass
  if (kSecond && f.on && live)
  {
    const double* s = st + slot * kAmpState;
    y1a = s[0]; y1b = s[1]; y2a = s[2]; y2b = s[3];
  }
  const TIn* x = rows_of<TIn>(p);
  __syncthreads();
  for (int k0 = 0; k0 < kAmpChunk; k0 += kAmpTile)
  {
#pragma unroll 4
    for (int e = 0; e < kPerLane; e++)
    {
      const int idx = e * 64 + r, rr = idx / kAmpTile, kk = idx % kAmpTile;
      if (k0 + kk < rowLen[rr]) tile[rr * kPitch + kk] = (double) x[rowSrc[rr] + k0 + kk]; // < n: inside the row
    }
    __syncthreads();
    double* mine = tile + r * kPitch;
    const int m = len - k0 < kAmpTile ? len - k0 : kAmpTile;
    for (int kk = 0; kk < m; kk++)
    {
      const double in = mine[kk];
      if (finite_d(in)) prevValid = in;
      double v = prevValid;
      if (!kSecond)
      {
        dd y1 = dd_add(two_prod(f.b0, v), two_prod(f.b1, x1));
        y1 = dd_add(y1, two_prod(f.b2, x2));
        y1 = dd_add(y1, dd_mul_d(z1a, -f.a0));
        y1 = dd_add(y1, dd_mul_d(z1b, -f.a1));
        dd y2 = dd_add(dd_mul_d(y1, f.b0), dd_mul_d(z1a, f.b1));
        y2 = dd_add(y2, dd_mul_d(z1b, f.b2));
        y2 = dd_add(y2, dd_mul_d(z2a, -f.a0));
        y2 = dd_add(y2, dd_mul_d(z2b, -f.a1));
        x2 = x1; x1 = v;
        z1b = z1a; z1a = y1;
        z2b = z2a; z2a = y2;
      }
      else if (f.on)
      {
        // ButterworthHPFilter::processSample :40, left to right, twice
        const double y1 = f.b0 * v + f.b1 * x1 + f.b2 * x2 - f.a0 * y1a - f.a1 * y1b;
        const double y2 = f.b0 * y1 + f.b1 * y1a + f.b2 * y1b - f.a0 * y2a - f.a1 * y2b;
        x2 = x1; x1 = v;
        y1b = y1a; y1a = y1;
        y2b = y2a; y2a = y2;
        v = y2;
      }
      if (kSecond)
      {
        const double dB = 20 * log10(fabs(v)); // -inf at 0
        mine[kk] = dB < floorDb ? floorDb : dB; // std::max(dB, floor)
      }
    }
    __syncthreads();
    if (kSecond)
    {
#pragma unroll 4
      for (int e = 0; e < kPerLane; e++)
      {
        const int idx = e * 64 + r, rr = idx / kAmpTile, kk = idx % kAmpTile;
        if (k0 + kk < rowLen[rr]) io[rowDst[rr] + k0 + kk] = tile[rr * kPitch + kk];
      }
      __syncthreads();
    }
  }
  if (!kSecond && live)
  {
    double* q = io + slot * kAmpState * 2;
    q[0] = z1a.hi; q[1] = z1a.lo; q[2] = z1b.hi; q[3] = z1b.lo;
    q[4] = z2a.hi; q[5] = z2a.lo; q[6] = z2b.hi; q[7] = z2b.lo;
  }
}

// lane i of a group of 4 owns row i of M and entry i of the state of its signal
__global__ __launch_bounds__(64) void amp_scan_kernel(const double* q, int64_t count, int64_t chunks, AmpTransition M, double* st)
{
  const int64_t gid = (int64_t) blockIdx.x * 64 + threadIdx.x;
  const int64_t sig = gid / kAmpState;
  const int i = (int) (gid % kAmpState);
  if (sig >= count) return; // (whole groups of 4 leave together)
  dd m[kAmpState];
  for (int c = 0; c < kAmpState; c++) m[c] = {M.hi[i * kAmpState + c], M.lo[i * kAmpState + c]};
  const double* qs = q + (sig * chunks * kAmpState + i) * 2; // [chunk][4][hi, lo]
  double* ss = st + sig * chunks * kAmpState + i;
  dd s = {0.0, 0.0};
  dd qn = {qs[0], qs[1]};
  for (int64_t j = 0; j < chunks; j++)
  {
    ss[j * kAmpState] = s.hi + s.lo;
    dd acc = qn;
    if (j + 1 < chunks) qn = {qs[(j + 1) * kAmpState * 2], qs[(j + 1) * kAmpState * 2 + 1]};
    for (int c = 0; c < kAmpState; c++)
    {
      const dd sc = {__shfl(s.hi, c, kAmpState), __shfl(s.lo, c, kAmpState)};
      acc = dd_add(acc, dd_mul(m[c], sc));
    }
    s = acc;
  }
}

#ifdef FLUHIP_AB_SWITCHES
// The measurement form (FLUHIP_AMP_PAIR=0 in the measurement build only; DESIGN K15): one lane carries both followers of its
// signal.  Wavefront g owns signals g 64 .. g 64 + 63, lane r signal g 64 + r, from its first sample to its last.
__global__ __launch_bounds__(64) void amp_follow_kernel(const double* level, int64_t count, int64_t n, AmpFollow f, double* env64,
                                                        float* env32, unsigned char* det, int64_t* counts)
{
  __shared__ double tile[64 * kPitch];
  __shared__ unsigned masks[64];
  const int r = threadIdx.x;
  const int64_t sig0 = (int64_t) blockIdx.x * 64;
  const int64_t sig = sig0 + r;
  const int rows = (int) (count - sig0 < 64 ? count - sig0 : 64);
  // SlideUDFilter::init(floor) for both; EnvelopeSegmentation::init :30-33
  double fast = f.floorDb, slow = f.floorDb, prev = 0.0;
  int64_t debounce = 0, found = 0;
  bool state = false;

  double next[kPerLane]; // the tile behind the one in the LDS, in flight while that one is walked
  auto fetch = [&](int64_t t0) {
#pragma unroll
    for (int e = 0; e < kPerLane; e++)
    {
      const int idx = e * 64 + r, rr = idx / kAmpTile, kk = idx % kAmpTile;
      next[e] = (rr < rows && t0 + kk < n) ? level[(sig0 + rr) * n + t0 + kk] : 0.0;
    }
  };
  fetch(0);
  for (int64_t t0 = 0; t0 < n; t0 += kAmpTile)
  {
#pragma unroll
    for (int e = 0; e < kPerLane; e++)
    {
      const int idx = e * 64 + r;
      tile[(idx / kAmpTile) * kPitch + idx % kAmpTile] = next[e];
    }
    __syncthreads();
    if (t0 + kAmpTile < n) fetch(t0 + kAmpTile);
    double* mine = tile + r * kPitch;
    const int m = n - t0 < kAmpTile ? (int) (n - t0) : kAmpTile;
    unsigned mask = 0;
    for (int kk = 0; kk < m; kk++)
    {
      const double c = mine[kk];
      // SlideUDFilter::processSample :27-37: the comparison strict, y0 + (b * (x - y0)) in three roundings
      fast = fast + ((c > fast ? f.fastUp : f.fastDown) * (c - fast));
      slow = slow + ((c > slow ? f.slowUp : f.slowDown) * (c - slow));
      const double value = fast - slow;
      mine[kk] = value;
      if (f.detect)
      {
        // EnvelopeSegmentation::processSample :46-58
        if (!state && value > f.on && prev < f.on && debounce == 0)
        {
          mask |= 1u << kk;
          debounce = f.minSlice;
          state = true;
        }
        else if (debounce > 0)
          debounce--;
        if (state && value < f.off) state = false;
        prev = value;
      }
    }
    found += __popc(mask);
    masks[r] = mask;
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < kPerLane; e++)
    {
      const int idx = e * 64 + r, rr = idx / kAmpTile, kk = idx % kAmpTile;
      if (rr < rows && t0 + kk < n)
      {
        const int64_t o = (sig0 + rr) * n + t0 + kk;
        const double v = tile[rr * kPitch + kk];
        if (env64) env64[o] = v;
        if (env32) env32[o] = (float) v;
        if (det) det[o] = (unsigned char) (masks[rr] >> kk & 1u);
      }
    }
    __syncthreads();
  }
  if (f.detect && counts && sig < count) counts[sig] = found;
}

#endif

// A lane PAIR shares a signal: wavefront g owns signals g 32 .. g 32 + 31 from their first sample to their last, lane r < 32
// the fast follower of signal g 32 + r, lane r + 32 the slow one; the difference crosses the halves once per sample, off either
// chain; the fast half carries the detector.  (Measured against one lane carrying both followers, which gives the same bits:
// 6 % faster on one buffer, 14 % on 128; DESIGN K15.)
__global__ __launch_bounds__(64) void amp_follow_pair_kernel(const double* level, int64_t count, int64_t n, AmpFollow f, double* env64,
                                                             float* env32, unsigned char* det, int64_t* counts)
{
  constexpr int kSig = 32, kPer = kSig * kAmpTile / 64;
  __shared__ double tile[kSig * kPitch], vals[kSig * kPitch];
  __shared__ unsigned masks[kSig];
  const int r = threadIdx.x, row = r & 31;
  const bool slowHalf = r >= 32;
  const int64_t sig0 = (int64_t) blockIdx.x * kSig;
  const int rows = (int) (count - sig0 < kSig ? count - sig0 : kSig);
  const double up = slowHalf ? f.slowUp : f.fastUp, down = slowHalf ? f.slowDown : f.fastDown;
  double y = f.floorDb, prev = 0.0;
  int64_t debounce = 0, found = 0;
  bool state = false;
  double next[kPer];
  auto fetch = [&](int64_t t0) {
#pragma unroll
    for (int e = 0; e < kPer; e++)
    {
      const int idx = e * 64 + r, rr = idx / kAmpTile, kk = idx % kAmpTile;
      next[e] = (rr < rows && t0 + kk < n) ? level[(sig0 + rr) * n + t0 + kk] : 0.0;
    }
  };
  fetch(0);
  for (int64_t t0 = 0; t0 < n; t0 += kAmpTile)
  {
#pragma unroll
    for (int e = 0; e < kPer; e++)
    {
      const int idx = e * 64 + r;
      tile[(idx / kAmpTile) * kPitch + idx % kAmpTile] = next[e];
    }
    __syncthreads();
    if (t0 + kAmpTile < n) fetch(t0 + kAmpTile);
    const double* mine = tile + row * kPitch;
    const int m = n - t0 < kAmpTile ? (int) (n - t0) : kAmpTile;
    unsigned mask = 0;
    for (int kk = 0; kk < m; kk++)
    {
      const double c = mine[kk];
      y = y + ((c > y ? up : down) * (c - y));
      const double other = __shfl_xor(y, 32);
      const double value = y - other; // (meaningful in the fast half)
      if (!slowHalf)
      {
        vals[row * kPitch + kk] = value;
        if (f.detect)
        {
          if (!state && value > f.on && prev < f.on && debounce == 0)
          {
            mask |= 1u << kk;
            debounce = f.minSlice;
            state = true;
          }
          else if (debounce > 0)
            debounce--;
          if (state && value < f.off) state = false;
          prev = value;
        }
      }
    }
    found += __popc(mask);
    if (!slowHalf) masks[row] = mask;
    __syncthreads();
#pragma unroll 4
    for (int e = 0; e < kPer; e++)
    {
      const int idx = e * 64 + r, rr = idx / kAmpTile, kk = idx % kAmpTile;
      if (rr < rows && t0 + kk < n)
      {
        const int64_t o = (sig0 + rr) * n + t0 + kk;
        const double v = vals[rr * kPitch + kk];
        if (env64) env64[o] = v;
        if (env32) env32[o] = (float) v;
        if (det) det[o] = (unsigned char) (masks[rr] >> kk & 1u);
      }
    }
    __syncthreads();
  }
  if (f.detect && counts && !slowHalf && sig0 + row < count) counts[sig0 + row] = found;
}

inline unsigned blocks(int64_t n, int64_t per) { return (unsigned) ((n + per - 1) / per); }

template <typename TIn>
void launch_level(const AmpSignals& p, const AmpHighPass& f, const AmpTransition& M, double floorDb, double* work, double* level,
                  hipStream_t s)
{
  const int64_t chunks = p.chunks(), slots = p.count * chunks;
  double* hold = work;
  double* q = hold + slots * 2;
  double* st = q + slots * kAmpState * 2;
  hipLaunchKernelGGL((amp_hold_kernel<TIn>), dim3(blocks(slots, 256)), dim3(256), 0, s, p, chunks, hold);
  if (f.on)
  {
    hipLaunchKernelGGL((amp_filter_kernel<TIn, false>), dim3(blocks(slots, 64)), dim3(64), 0, s, p, chunks, f, hold, floorDb, nullptr, q);
    hipLaunchKernelGGL(amp_scan_kernel, dim3(blocks(p.count * kAmpState, 64)), dim3(64), 0, s, q, p.count, chunks, M, st);
  }
  hipLaunchKernelGGL((amp_filter_kernel<TIn, true>), dim3(blocks(slots, 64)), dim3(64), 0, s, p, chunks, f, hold, floorDb, st, level);
}

} // namespace

AmpHighPass amp_highpass(double hipass)
{
  // ButterworthHPFilter::init :25-31, the reference's own sequence of double operations (util/AlgorithmUtils.hpp:21-23)
  const double pi = 3.14159265358979323846, sqrtTwo = 1.41421356237309504880;
  AmpHighPass f;
  const double c = std::tan(pi * hipass);
  f.b0 = 1.0 / (1.0 + sqrtTwo * c + std::pow(c, 2.0));
  f.b1 = -2.0 * f.b0;
  f.b2 = f.b0;
  f.a0 = 2.0 * f.b0 * (std::pow(c, 2.0) - 1.0);
  f.a1 = f.b0 * (1.0 - sqrtTwo * c + std::pow(c, 2.0));
  f.on = hipass > 0 ? 1 : 0; // Envelope.hpp:51
  return f;
}

AmpTransition amp_transition(const AmpHighPass& f)
{
  // A: the state [y1[n-1], y1[n-2], y2[n-1], y2[n-2]] behind one sample of zero input (the second section's inputs are the
  // first one's outputs); M = A^kAmpChunk by repeated squaring, every entry a double-double throughout
  constexpr int S = kAmpState;
  struct Mat
  {
    dd v[S][S];
  };
  auto mul = [](const Mat& a, const Mat& b) {
    Mat c;
    for (int i = 0; i < S; i++)
      for (int j = 0; j < S; j++)
      {
        dd acc = {0.0, 0.0};
        for (int l = 0; l < S; l++) acc = dd_add(acc, dd_mul(a.v[i][l], b.v[l][j]));
        c.v[i][j] = acc;
      }
    return c;
  };
  Mat A, M;
  for (int i = 0; i < S; i++)
    for (int j = 0; j < S; j++)
    {
      A.v[i][j] = {0.0, 0.0};
      M.v[i][j] = {i == j ? 1.0 : 0.0, 0.0};
    }
  // y1 = -a0 y1a - a1 y1b;  y2 = b0 y1 + b1 y1a + b2 y1b - a0 y2a - a1 y2b
  const dd na0 = {-f.a0, 0.0}, na1 = {-f.a1, 0.0}, b0 = {f.b0, 0.0};
  A.v[0][0] = na0;
  A.v[0][1] = na1;
  A.v[1][0] = {1.0, 0.0};
  A.v[2][0] = dd_add(dd_mul(b0, na0), dd{f.b1, 0.0});
  A.v[2][1] = dd_add(dd_mul(b0, na1), dd{f.b2, 0.0});
  A.v[2][2] = na0;
  A.v[2][3] = na1;
  A.v[3][2] = {1.0, 0.0};
  for (int64_t e = kAmpChunk; e > 0; e >>= 1)
  {
    if (e & 1) M = mul(M, A);
    if (e > 1) A = mul(A, A);
  }
  AmpTransition out;
  for (int i = 0; i < S; i++)
    for (int j = 0; j < S; j++)
    {
      out.hi[i * S + j] = M.v[i][j].hi;
      out.lo[i * S + j] = M.v[i][j].lo;
    }
  return out;
}

void launch_amp_level(const AmpSignals& p, const AmpHighPass& f, const AmpTransition& M, double floorDb, double* work, double* level,
                      hipStream_t s)
{
  if (p.count < 1 || p.n < 1) return;
  if (p.x32)
    launch_level<float>(p, f, M, floorDb, work, level, s);
  else
    launch_level<double>(p, f, M, floorDb, work, level, s);
}

void launch_amp_follow(const double* level, int64_t count, int64_t n, const AmpFollow& f, double* env64, float* env32,
                       unsigned char* det, int64_t* counts, hipStream_t s)
{
  if (count < 1 || n < 1) return;
#ifdef FLUHIP_AB_SWITCHES
  if (!f.pair)
  {
    hipLaunchKernelGGL(amp_follow_kernel, dim3(blocks(count, 64)), dim3(64), 0, s, level, count, n, f, env64, env32, det, counts);
    return;
  }
#endif
  hipLaunchKernelGGL(amp_follow_pair_kernel, dim3(blocks(count, kAmpSignals)), dim3(64), 0, s, level, count, n, f, env64, env32, det, counts);
}

} // namespace fluhip
