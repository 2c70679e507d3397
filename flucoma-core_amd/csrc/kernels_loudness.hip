// kernels_loudness.hip -- K14: BufLoudness, the first client whose frames are not independent.
//   algorithm::Loudness::processFrame   include/flucoma/algorithms/public/Loudness.hpp:43-61
//   algorithm::KWeightingFilter         include/flucoma/algorithms/util/KWeightingFilter.hpp:23-92  (never reset between frames)
//   algorithm::TruePeak / Interpolator  include/flucoma/algorithms/util/TruePeak.hpp:48-182         (ring buffer kept between frames)
// The reference feeds overlapping frames, one after the other, through one filter and one interpolator: a chain of T win
// dependent steps per channel.  Here no chain across frames is longer than a scan of 8-value states:
//   loudness_filter_kernel<.., false>  lane = frame: the frame run from ZERO state, its end state q_f (frames independent)
//   loudness_scan_kernel               8 lanes per buffer: s_{f+1} = M s_f + q_f, M = A^win.  The high-pass poles at 38 Hz sit
//                                      next to z = 1 and M's entries reach 5e3 (44.1 kHz) to 3e5 (192 kHz) with alternating
//                                      signs: M (built on the host) and the carried state are double-double pairs; the state
//                                      is rounded to double once, where a frame takes it
//   loudness_filter_kernel<.., true>   lane = frame: the frame run again from its true entering state, in plain double and in
//                                      the reference's order of operations, the squares of the actual filtered samples summed
//                                      (never the expanded quadratic form: the high-pass cancels a zero-state transient against
//                                      the carried state)
//   loudness_peak_kernel               one wavefront per frame: the polyphase FIR over the frame stream, read with its
//                                      ring - 1 samples of history from the frames before (zeros before frame 0), max |.|;
//                                      a lane loads the ring behind its sample once for all phases; the unweighted mean
//                                      square when kWeighting is off
//   loudness_select_kernel             the kept frames and selected columns in the client's float32 layout
// Lanes that own consecutive frames read `hop` samples apart: a workgroup stages plan.chunk samples of each of its plan.run
// frames through the LDS (rows of chunk + 1 doubles), so the global reads are rows of consecutive samples and the LDS need is
// run (chunk + 1) 8 bytes whatever the window.  The kernels take run and chunk from the launch: nothing assumes them.
// Every order of operations depends on (win, hop, the frame's position in its buffer) alone, so a batch gives the bits of
// single calls.  Compiled with -ffp-contract=off (the double-double arithmetic needs each rounding) and no fast-math flag.
#include "fluhip_dd.h"
#include "fluhip_kernels.h"
#include "fluhip_loudness.h"

#include <cmath>

namespace fluhip {

namespace {

constexpr double kOffset = -0.691; // Loudness.hpp:55

template <typename TIn> __device__ __forceinline__ const TIn* rows_of(const LoudnessFrames& p);
template <> __device__ __forceinline__ const float* rows_of<float>(const LoudnessFrames& p) { return p.x32; }
template <> __device__ __forceinline__ const double* rows_of<double>(const LoudnessFrames& p) { return p.x64; }

// Workgroup g owns frames t0 .. t0 + run of buffer b (blocksPerBuf workgroups per buffer), lane r frame t0 + r.
// kSecond false: from zero state, writes the end state to io[f][8].  kSecond true: from st[f][8], writes the loudness to
// io[f][0] (row stride 2).
template <typename TIn, bool kSecond>
__global__ __launch_bounds__(256) void loudness_filter_kernel(LoudnessFrames p, int run, int chunk, int64_t blocksPerBuf, KWeighting k,
                                                              const double* st, double* io)
{
  extern __shared__ double tile[]; // [run][chunk + 1]
  const int r = threadIdx.x;
  const int64_t b = blockIdx.x / blocksPerBuf;
  const int64_t t0 = (blockIdx.x % blocksPerBuf) * run;
  const int64_t t = t0 + r;
  const bool live = t < p.T;
  const int64_t f = b * p.T + (live ? t : 0);
  const TIn* row = rows_of<TIn>(p) + b * p.stride;
  const int rows = (int) (p.T - t0 < run ? p.T - t0 : run); // frames of this workgroup that exist
  const int pitch = chunk + 1;

  double x1 = 0, x2 = 0, x3 = 0, x4 = 0, y0 = 0, y1 = 0, y2 = 0, y3 = 0;
  if (kSecond && live)
  {
    const double* s = st + f * kLoudnessState;
    x1 = s[0]; x2 = s[1]; x3 = s[2]; x4 = s[3];
    y0 = s[4]; y1 = s[5]; y2 = s[6]; y3 = s[7];
  }
  double acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0; // four partial sums of squares, sample i into i mod 4 (chunk is a multiple of 4 or the whole window)
  for (int64_t c0 = 0; c0 < p.win; c0 += chunk)
  {
    const int len = (int) (p.win - c0 < chunk ? p.win - c0 : chunk);
    for (int idx = r; idx < rows * chunk; idx += run)
    {
      const int rr = idx / chunk, kk = idx % chunk;
      if (kk < len) tile[rr * pitch + kk] = (double) row[(t0 + rr) * p.hop + c0 + kk]; // < (T - 1) hop + win: inside the row
    }
    __syncthreads();
    if (live)
    {
      const double* mine = tile + r * pitch;
      for (int kk = 0; kk < len; kk++)
      {
        const double x0 = mine[kk];
        // KWeightingFilter::processSample :78-92, operation by operation
        double y = 0;
        y -= k.a[1] * y0;
        y -= k.a[2] * y1;
        y -= k.a[3] * y2;
        y -= k.a[4] * y3;
        y += k.b[0] * x0;
        y += k.b[1] * x1;
        y += k.b[2] * x2;
        y += k.b[3] * x3;
        y += k.b[4] * x4;
        x4 = x3; x3 = x2; x2 = x1; x1 = x0;
        y3 = y2; y2 = y1; y1 = y0; y0 = y;
        if (kSecond)
        {
          const double sq = y * y;
          switch (kk & 3)
          {
          case 0: acc0 += sq; break;
          case 1: acc1 += sq; break;
          case 2: acc2 += sq; break;
          default: acc3 += sq; break;
          }
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
  if (kSecond)
  {
    const double mean = ((acc0 + acc1) + (acc2 + acc3)) / (double) p.win;
    io[2 * f] = kOffset + 10 * log10(mean + kEpsilon);
  }
  else
  {
    double* q = io + f * kLoudnessState;
    q[0] = x1; q[1] = x2; q[2] = x3; q[3] = x4;
    q[4] = y0; q[5] = y1; q[6] = y2; q[7] = y3;
  }
}

// (the double-double arithmetic of the scan and of frame_transition is in fluhip_dd.h)
// lane i of a group of 8 owns row i of M and entry i of the state of its buffer
__global__ __launch_bounds__(64) void loudness_scan_kernel(const double* q, int64_t B, int64_t T, LoudnessTransition M, double* st)
{
  const int64_t gid = (int64_t) blockIdx.x * 64 + threadIdx.x;
  const int64_t b = gid / kLoudnessState;
  const int i = (int) (gid % kLoudnessState);
  if (b >= B) return; // (whole groups of 8 leave together)
  dd m[kLoudnessState];
  for (int c = 0; c < kLoudnessState; c++) m[c] = {M.hi[i * kLoudnessState + c], M.lo[i * kLoudnessState + c]};
  const double* qb = q + b * T * kLoudnessState + i;
  double* sb = st + b * T * kLoudnessState + i;
  dd s = {0.0, 0.0};
  double qn = qb[0];
  for (int64_t j = 0; j < T; j++)
  {
    sb[j * kLoudnessState] = s.hi + s.lo;
    const double qj = qn;
    if (j + 1 < T) qn = qb[(j + 1) * kLoudnessState];
    dd acc = {qj, 0.0};
    for (int c = 0; c < kLoudnessState; c++)
    {
      const dd sc = {__shfl(s.hi, c, kLoudnessState), __shfl(s.lo, c, kLoudnessState)};
      acc = dd_add(acc, dd_mul(m[c], sc));
    }
    s = acc;
  }
}

// sample p of the frame stream of one buffer (frame p / win, sample p % win of it); zeros before the first frame
template <typename TIn> __device__ __forceinline__ double stream_sample(const TIn* row, int64_t pos, int64_t win, int64_t hop)
{
  if (pos < 0) return 0.0;
  return (double) row[(pos / win) * hop + pos % win];
}

// the 49 coefficients in tap order, 0 where the reference drops the tap: tap i belongs to phase i % factor and reads the sample
// i / factor back
struct FlatTaps
{
  double c[kLoudnessTaps];
};

// kFactor 1: no interpolator (max |x|); 2, 4: the polyphase FIR.  A lane loads the (49 + kFactor - 1) / kFactor samples behind
// its own once and feeds every phase from them; each phase accumulates in tap order, as Interpolator::processFrame does.
template <typename TIn, int kFactor>
__global__ __launch_bounds__(256) void loudness_peak_kernel(LoudnessFrames p, FlatTaps taps, int unweighted, double* res)
{
  const int lane = threadIdx.x & 63;
  const int64_t f = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= p.B * p.T) return; // (whole wavefronts leave: no partial shuffles)
  const int64_t b = f / p.T, t = f % p.T;
  const TIn* row = rows_of<TIn>(p) + b * p.stride;
  const TIn* mine = row + t * p.hop;
  constexpr int kRing = (kLoudnessTaps + kFactor - 1) / kFactor;
  double peak = 0.0, sum = 0.0;
  for (int64_t i = lane; i < p.win; i += 64)
  {
    const double x0 = (double) mine[i];
    sum += x0 * x0;
    if (kFactor == 1)
    {
      peak = fmax(peak, fabs(x0));
      continue;
    }
    // Interpolator::processFrame :100-119: the ring buffer holds the last samples fed, whatever frame they came from
    double acc[kFactor];
#pragma unroll
    for (int ph = 0; ph < kFactor; ph++) acc[ph] = 0;
    for (int d = 0; d < kRing; d++)
    {
      const double v = d == 0 ? x0 : d <= i ? (double) mine[i - d] : stream_sample(row, t * p.win + i - d, p.win, p.hop);
#pragma unroll
      for (int ph = 0; ph < kFactor; ph++)
      {
        const int tap = d * kFactor + ph;
        if (tap < kLoudnessTaps && taps.c[tap] != 0.0) acc[ph] += v * taps.c[tap]; // (wave-uniform: a dropped tap is skipped)
      }
    }
#pragma unroll
    for (int ph = 0; ph < kFactor; ph++) peak = fmax(peak, fabs(acc[ph]));
  }
  for (int o = 32; o > 0; o >>= 1)
  {
    peak = fmax(peak, __shfl_xor(peak, o));
    sum += __shfl_xor(sum, o);
  }
  if (lane) return;
  res[2 * f + 1] = 20 * log10(peak + kEpsilon);
  if (unweighted) res[2 * f] = kOffset + 10 * log10(sum / (double) p.win + kEpsilon); // (the offset stays: Loudness.hpp:55)
}

__global__ __launch_bounds__(256) void loudness_select_kernel(const double* res, int64_t B, int64_t T, int64_t drop, int64_t keep,
                                                              int select, float* out32)
{
  const int64_t e = (int64_t) blockIdx.x * 256 + threadIdx.x;
  if (e >= B * keep) return;
  const int64_t b = e / keep, t = e % keep;
  const int nsel = (select & 1) + (select >> 1 & 1);
  const double* r = res + 2 * (b * T + drop + t);
  float* o = out32 + b * nsel * keep + t;
  int c = 0;
  if (select & 1) o[(int64_t) (c++) * keep] = (float) r[0];
  if (select & 2) o[(int64_t) c * keep] = (float) r[1];
}

inline unsigned blocks(int64_t n, int64_t per) { return (unsigned) ((n + per - 1) / per); }

template <bool kSecond>
void launch_filter(const LoudnessFrames& p, const LoudnessPlan& plan, const KWeighting& k, const double* st, double* io, hipStream_t s)
{
  if (p.B * p.T < 1) return;
  const int64_t perBuf = (p.T + plan.run - 1) / plan.run;
  const size_t lds = (size_t) plan.ldsBytes();
  if (p.x32)
    hipLaunchKernelGGL((loudness_filter_kernel<float, kSecond>), dim3((unsigned) (p.B * perBuf)), dim3(plan.run), lds, s, p, plan.run,
                       plan.chunk, perBuf, k, st, io);
  else
    hipLaunchKernelGGL((loudness_filter_kernel<double, kSecond>), dim3((unsigned) (p.B * perBuf)), dim3(plan.run), lds, s, p, plan.run,
                       plan.chunk, perBuf, k, st, io);
}

} // namespace

LoudnessPlan loudness_plan(int64_t win, int64_t hop, double sampleRate)
{
  (void) hop; // the rows staged are per frame: the hop changes which samples a row holds, not how many
  LoudnessPlan p;
  p.form = kLoudnessFormFrames;
  // a chunk of 32 samples (a multiple of 4: the partial sums) or the whole of a shorter window; as many frames as lanes of a
  // wavefront, fewer only if the tile would not fit what a workgroup may take (it always does at these sizes: 16.5 KiB, so
  // several workgroups share a CU's 160 KiB)
  p.chunk = (int) (win < 32 ? (win < 1 ? 1 : win) : 32);
  p.run = 64;
  while (p.run > 1 && p.ldsBytes() > kLoudnessLdsBudget) p.run /= 2;
  p.factor = sampleRate >= 4 * 44100.0 ? 1 : sampleRate < 2 * 44100.0 ? 4 : 2; // TruePeak.hpp:160, :171
  p.history = p.factor == 1 ? 0 : (kLoudnessTaps + p.factor - 1) / p.factor - 1;
  return p;
}

KWeighting kweighting_coefficients(double sampleRate)
{
  // KWeightingFilter::init :30-70, the reference's own sequence of double operations (util/AlgorithmUtils.hpp:21 pi)
  const double pi = 3.14159265358979323846;
  KWeighting k;
  double f0 = 1681.974450955533;
  const double G = 3.999843853973347;
  double Q = 0.7071752369554196;
  double K = std::tan(pi * f0 / sampleRate);
  const double Vh = std::pow(10.0, G / 20.0);
  const double Vb = std::pow(Vh, 0.4996667741545416);
  double shelvB[3] = {0.0, 0.0, 0.0};
  double shelvA[3] = {1.0, 0.0, 0.0};
  const double a0 = 1.0 + K / Q + K * K;
  shelvB[0] = (Vh + Vb * K / Q + K * K) / a0;
  shelvB[1] = 2.0 * (K * K - Vh) / a0;
  shelvB[2] = (Vh - Vb * K / Q + K * K) / a0;
  shelvA[1] = 2.0 * (K * K - 1.0) / a0;
  shelvA[2] = (1.0 - K / Q + K * K) / a0;
  f0 = 38.13547087602444;
  Q = 0.5003270373238773;
  K = std::tan(pi * f0 / sampleRate);
  const double hiB[3] = {1.0, -2.0, 1.0};
  double hiA[3] = {1.0, 0.0, 0.0};
  hiA[1] = 2.0 * (K * K - 1.0) / (1.0 + K / Q + K * K);
  hiA[2] = (1.0 - K / Q + K * K) / (1.0 + K / Q + K * K);
  k.b[0] = shelvB[0] * hiB[0];
  k.b[1] = shelvB[0] * hiB[1] + shelvB[1] * hiB[0];
  k.b[2] = shelvB[0] * hiB[2] + shelvB[1] * hiB[1] + shelvB[2] * hiB[0];
  k.b[3] = shelvB[1] * hiB[2] + shelvB[2] * hiB[1];
  k.b[4] = shelvB[2] * hiB[2];
  k.a[0] = shelvA[0] * hiA[0];
  k.a[1] = shelvA[0] * hiA[1] + shelvA[1] * hiA[0];
  k.a[2] = shelvA[0] * hiA[2] + shelvA[1] * hiA[1] + shelvA[2] * hiA[0];
  k.a[3] = shelvA[1] * hiA[2] + shelvA[2] * hiA[1];
  k.a[4] = shelvA[2] * hiA[2];
  return k;
}

LoudnessTransition frame_transition(const KWeighting& k, int64_t win)
{
  // A: the state [mX[1..4], mY[0..3]] behind one sample of zero input; M = A^win by repeated squaring, every entry a
  // double-double throughout.  (A long double is not enough: M built by win successive long double steps left the loudness
  // 63 floors off at 192 kHz, where M's entries reach 2.8e5; tests/test_loudness_ref.py has the figures.)
  constexpr int S = kLoudnessState;
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
  for (int i = 0; i < 3; i++)
  {
    A.v[i + 1][i] = {1.0, 0.0};     // mX[i] = mX[i - 1] (mX[1] = the sample = 0)
    A.v[5 + i][4 + i] = {1.0, 0.0}; // mY[i] = mY[i - 1]
  }
  for (int i = 0; i < 4; i++)
  {
    A.v[4][i] = {k.b[i + 1], 0.0};
    A.v[4][4 + i] = {-k.a[i + 1], 0.0};
  }
  for (int64_t e = win; e > 0; e >>= 1)
  {
    if (e & 1) M = mul(M, A);
    if (e > 1) A = mul(A, A);
  }
  LoudnessTransition out;
  for (int i = 0; i < S; i++)
    for (int j = 0; j < S; j++)
    {
      out.hi[i * S + j] = M.v[i][j].hi;
      out.lo[i * S + j] = M.v[i][j].lo;
    }
  return out;
}

InterpolatorTaps interpolator_taps(int factor)
{
  // Interpolator::init :58-86
  const double pi = 3.14159265358979323846, twoPi = 2 * pi;
  InterpolatorTaps t{};
  t.factor = factor;
  if (factor < 2) return t;
  for (int i = 0; i < kLoudnessTaps; i++)
  {
    const double m = i - (kLoudnessTaps - 1) / 2.0;
    double c = 1.0;
    if (std::abs(m) > 1e-6) c = std::sin(m * pi / factor) / (m * pi / factor);
    c *= 0.5 * (1 - std::cos(twoPi * i / (kLoudnessTaps - 1)));
    if (std::abs(c) > 1e-6)
    {
      const int ph = i % factor;
      const int n = t.count[ph]++;
      t.coeff[ph][n] = c;
      t.delay[ph][n] = i / factor;
    }
  }
  return t;
}

void launch_loudness_zero_state(const LoudnessFrames& p, const LoudnessPlan& plan, const KWeighting& k, double* q, hipStream_t s)
{
  launch_filter<false>(p, plan, k, nullptr, q, s);
}

void launch_loudness_scan(const double* q, int64_t B, int64_t T, const LoudnessTransition& M, double* st, hipStream_t s)
{
  if (B * T < 1) return;
  hipLaunchKernelGGL(loudness_scan_kernel, dim3(blocks(B * kLoudnessState, 64)), dim3(64), 0, s, q, B, T, M, st);
}

void launch_loudness_filtered(const LoudnessFrames& p, const LoudnessPlan& plan, const KWeighting& k, const double* st, double* res,
                              hipStream_t s)
{
  launch_filter<true>(p, plan, k, st, res, s);
}

template <typename TIn>
static void launch_peak(const LoudnessFrames& p, const FlatTaps& flat, int factor, int unweighted, double* res, hipStream_t s)
{
  const dim3 grid(blocks(p.B * p.T, 4)), block(256);
  if (factor == 4)
    hipLaunchKernelGGL((loudness_peak_kernel<TIn, 4>), grid, block, 0, s, p, flat, unweighted, res);
  else if (factor == 2)
    hipLaunchKernelGGL((loudness_peak_kernel<TIn, 2>), grid, block, 0, s, p, flat, unweighted, res);
  else
    hipLaunchKernelGGL((loudness_peak_kernel<TIn, 1>), grid, block, 0, s, p, flat, unweighted, res);
}

void launch_loudness_peak(const LoudnessFrames& p, const InterpolatorTaps& taps, int truePeak, int unweighted, double* res,
                          hipStream_t s)
{
  if (p.B * p.T < 1) return;
  const int factor = truePeak && (taps.factor == 2 || taps.factor == 4) ? taps.factor : 1;
  FlatTaps flat{};
  if (factor > 1)
    for (int ph = 0; ph < factor; ph++)
      for (int j = 0; j < taps.count[ph]; j++) flat.c[taps.delay[ph][j] * factor + ph] = taps.coeff[ph][j];
  if (p.x32)
    launch_peak<float>(p, flat, factor, unweighted, res, s);
  else
    launch_peak<double>(p, flat, factor, unweighted, res, s);
}

void launch_loudness_select(const double* res, int64_t B, int64_t T, int64_t drop, int64_t keep, int select, float* out32, hipStream_t s)
{
  if (B * keep < 1) return;
  hipLaunchKernelGGL(loudness_select_kernel, dim3(blocks(B * keep, 256)), dim3(256), 0, s, res, B, T, drop, keep, select, out32);
}

} // namespace fluhip
