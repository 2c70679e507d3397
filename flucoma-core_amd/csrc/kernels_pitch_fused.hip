// kernels_pitch_fused.hip -- K12, the on-chip form of BufPitch (the arithmetic is in pitch_terms.h, which switches
// contraction off for itself: kernels_pitch.hip is compiled with -ffp-contract=off, this file is not).
// A workgroup of NW wavefronts takes kPitchRun consecutive frames of one buffer; wavefront w transforms the frames
// t0 + w, t0 + w + NW, ... with FftCore (fft_core.h), which leaves |X| in the wavefront's staging buffer, and finishes each
// of them alone: no frame looks at another, so there is no ring and no barrier in the loop.
//   HPS       the three-factor product from the staged magnitudes, its sum and its argmax
//   YinFFT    the even-symmetric squared magnitudes are laid out as the core's input points (point m = x[2m] + i x[2m+1]) and
//             the core runs a second time, its complex bins going to a row of the LDS; the running-sum normalisation writes
//             the curve over the staging buffer, the peak search reads it there
//   Cepstrum  log(max(|X|, epsilon)) goes to the workspace the GEMM reads: no magnitude is written
// YinFFT and HPS read the samples and write two doubles per frame.  Every address is formed in front of the branches.
#include "fft_core.h"
#include "fluhip_pitch.h"
#include "pitch_terms.h"

namespace fluhip {

template <int R1, int R2, int R3, int NW>
__global__ __launch_bounds__(64 * NW) void pitch_fused_kernel(StftBArgs a, PitchFusedArgs o, int runsPerBuf)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, PPL = Core::PPL, BUFD = Core::BUFD, NB1 = Core::NB1;
  constexpr int F = N + 1;
  static_assert((NW * BUFD) % 2 == 0, "the rows of complex bins start on a 16-byte boundary");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  d2* tw2 = reinterpret_cast<d2*>(lds);
  double* xall = reinterpret_cast<double*>(tw2 + Core::TW);
  d2* zall = reinterpret_cast<d2*>(xall + NW * BUFD); // [NW][F] the second transform's bins
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const d2* twg = reinterpret_cast<const d2*>(a.twiddle);
  Core::fill_tables(tw2, twg, threadIdx.x, 64 * NW);
  const d2* wsrc = reinterpret_cast<const d2*>(a.window);
  __syncthreads();
  double* xb = xall + wave * BUFD;
  d2* zrow = zall + wave * F;
  Core core;
  core.init(xb, tw2, twg, lane);

  const int b = (int) (blockIdx.x / (unsigned) runsPerBuf);
  const int t0 = (int) (blockIdx.x % (unsigned) runsPerBuf) * kPitchRun;
  const int t1 = t0 + kPitchRun < a.T ? t0 + kPitchRun : a.T;
  const double binHz = o.sampleRate / (double) (2 * N);
  const int len = o.hi > o.lo ? o.hi - o.lo : 0;
  for (int t = t0 + wave; t < t1; t += NW) // (wave-uniform: whole wavefronts leave)
  {
    const int64_t f = (int64_t) b * a.T + t;
    double* res = o.out + 2 * f;
    double* lgRow = o.lg ? o.lg + f * F : nullptr;
    cx pts[PPL];
    gather_points<R1, N>(a, b, t, lane, wsrc, pts, a.n);
    SCHED_FENCE();
    core.template run<false>(pts, nullptr);
    if (o.algorithm == kPitchHPS)
      pitchdev::hps_frame(xb, F, lane, o.lo, o.hi, binHz, nullptr, res);
    else if (o.algorithm == kPitchCepstrum)
    {
      if (lgRow)
        for (int j = lane; j < F; j += 64) lgRow[j] = log(fmax(xb[j], kEpsilon));
    }
    else
    {
      const double s2 = pitchdev::yin_energy2(xb, F, lane);
      // x[i] = sq[i <= N ? i : 2 N - i], i < 2 N (YINFFT.hpp:48-50): every index lies in [0, N]
#pragma unroll
      for (int bb = 0; bb < NB1; bb++)
#pragma unroll
        for (int r = 0; r < R1; r++)
        {
          const int i0 = 2 * (lane + 64 * bb + r * (N / R1)), i1 = i0 + 1;
          const int j0 = i0 <= N ? i0 : 2 * N - i0, j1 = i1 <= N ? i1 : 2 * N - i1;
          pts[bb * R1 + r] = cx{pitchdev::yin_square(xb[j0]), pitchdev::yin_square(xb[j1])};
        }
      SCHED_FENCE();
      core.template run<true>(pts, zrow);
      const double gate = pitchdev::yin_norm_frame(reinterpret_cast<const double*>(zrow), s2, F, lane, xb);
      pitchdev::peak_frame(true, xb + o.lo, len, 0.0, gate, o.lo, o.sampleRate, lane, res);
    }
  }
}

template <int R1, int R2, int R3, int NW>
constexpr size_t pitch_fused_lds()
{
  using Core = FftCore<R1, R2, R3>;
  return (size_t) Core::TW * 16 + (size_t) NW * Core::BUFD * 8 + (size_t) NW * (Core::N + 1) * 16;
}
// twiddle tables + NW staging buffers + NW rows of complex bins: 58, 65 and 81 KB
static_assert(pitch_fused_lds<8, 8, 8, 4>() == 59392 && pitch_fused_lds<16, 8, 8, 2>() == 66368 &&
              pitch_fused_lds<16, 8, 16, 1>() == 82720, "LDS footprint of the on-chip pitch form (DESIGN K12)");

template <int R1, int R2, int R3, int NW>
static bool launch_pitch_fused_t(const StftBArgs& k, const PitchFusedArgs& o, hipStream_t s)
{
  constexpr size_t shmem = pitch_fused_lds<R1, R2, R3, NW>();
  static_assert(shmem <= 160 * 1024, "LDS");
  const int runsPerBuf = (k.T + kPitchRun - 1) / kPitchRun;
  const int64_t grid = (int64_t) k.B * runsPerBuf;
  if (grid < 1) return true;
  if (grid > 0x7fffffffLL) return false;
  auto kern = pitch_fused_kernel<R1, R2, R3, NW>;
  request_dynamic_lds(kern, shmem);
  hipLaunchKernelGGL(kern, dim3((unsigned) grid), dim3(64 * NW), shmem, s, k, o, runsPerBuf);
  return true;
}

bool pitch_fused_supported(int64_t win, int64_t fft) { return win >= 2 && fft_core_supported(win, fft); }

bool launch_pitch_fused(const StftArgs& a, const PitchFusedArgs& o, hipStream_t s)
{
  if (!pitch_fused_supported(a.win, a.fft) || a.F != a.fft / 2 + 1) return false;
  // the bins the kernel indexes its staging buffer with: YinFFT's segment [lo, hi) and HPS's both end inside the F bins
  if (o.lo < 0 || o.hi > a.F || (o.algorithm != kPitchHPS && o.lo > a.F) || !o.out) return false;
  if (o.algorithm == kPitchCepstrum && !o.lg) return false;
  const StftBArgs k = block_args(a);
  // wavefronts per workgroup as in the onset form: 4, 2 and 1
  if (a.fft == 1024) return launch_pitch_fused_t<8, 8, 8, 4>(k, o, s);
  if (a.fft == 2048) return launch_pitch_fused_t<16, 8, 8, 2>(k, o, s);
  return launch_pitch_fused_t<16, 8, 16, 1>(k, o, s);
}

} // namespace fluhip
