// kernels_onset_fused.hip -- K10, the on-chip form of the onset curve (BufOnsetSlice / BufOnsetFeature; the arithmetic is in
// onset_terms.h, which switches contraction off for itself: kernels_onset.hip is compiled with -ffp-contract=off, this file is not).
// A workgroup of NW wavefronts takes kOnsetRun consecutive frames of one buffer and walks them in rounds of NW: wavefront w
// transforms frame r0 + w with FftCore (fft_core.h), the complex bins going into a slot of a ring in the LDS instead of to
// memory; behind a barrier it reduces its frame against the one or two frames before it, which lie in the ring, and
// writes one double.  The `history` frames in front of the run are transformed again (the halo is recomputed, not
// exchanged); frames before the start of the signal are zero spectra (a null pointer, nothing is transformed).  The
// ring has NW + history slots: a round overwrites exactly the slots that do not hold the last `history` frames.  With a
// frame delta a wavefront transforms its frame twice, `delta` samples apart, into two slots of its own.
// No spectrum leaves the chip: the launch reads the samples and writes 8 bytes per frame.
#include "fft_core.h"
#include "fluhip_onset.h"
#include "onset_terms.h"

namespace fluhip {

template <int R1, int R2, int R3, int NW>
__global__ __launch_bounds__(64 * NW) void onset_fused_kernel(StftBArgs a, OnsetFusedArgs o, int runsPerBuf)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, PPL = Core::PPL, BUFD = Core::BUFD;
  constexpr int SLOT = N + 1; // d2 per spectrum
  static_assert((NW * BUFD) % 2 == 0, "the ring starts on a 16-byte boundary");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  d2* tw2 = reinterpret_cast<d2*>(lds);
  double* xall = reinterpret_cast<double*>(tw2 + Core::TW);
  d2* ring = reinterpret_cast<d2*>(xall + NW * BUFD);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const d2* twg = reinterpret_cast<const d2*>(a.twiddle);
  Core::fill_tables(tw2, twg, threadIdx.x, 64 * NW);
  const d2* wsrc = reinterpret_cast<const d2*>(a.window);
  __syncthreads();
  Core core;
  core.init(xall + wave * BUFD, tw2, twg, lane);

  const int b = (int) (blockIdx.x / (unsigned) runsPerBuf);
  const int t0 = (int) (blockIdx.x % (unsigned) runsPerBuf) * kOnsetRun;
  const int t1 = t0 + kOnsetRun < o.T ? t0 + kOnsetRun : o.T;
  const bool two = o.delta != 0;
  const int h = two ? 0 : o.history;
  const int slots = two ? 2 * NW : NW + h;
  const int first = t0 - h;
  StftBArgs a2 = a;
  a2.frameOffset += o.delta;
  for (int r0 = first; r0 < t1; r0 += NW)
  {
    const int t = r0 + wave;
    const int seq = t - first;
    d2* own = ring + (two ? wave : seq % slots) * SLOT;
    if (t >= 0 && t < t1)
    {
      cx pts[PPL];
      gather_points<R1, N>(a, b, t, lane, wsrc, pts, a.n);
      SCHED_FENCE();
      core.template run<true>(pts, own);
      if (two)
      {
        gather_points<R1, N>(a2, b, t, lane, wsrc, pts, a.n);
        SCHED_FENCE();
        core.template run<true>(pts, own + NW * SLOT);
      }
    }
    __syncthreads(); // the round's spectra are in the ring
    if (t >= t0 && t < t1)
    {
      using od2 = onsetdev::d2;
      const od2* cur = reinterpret_cast<const od2*>(own);
      const od2* c = two ? reinterpret_cast<const od2*>(own + NW * SLOT) : cur;
      const od2* p = two ? cur : (h >= 1 && t >= 1 ? reinterpret_cast<const od2*>(ring + ((seq - 1) % slots) * SLOT) : nullptr);
      const od2* pp = two ? cur : (h >= 2 && t >= 2 ? reinterpret_cast<const od2*>(ring + ((seq - 2) % slots) * SLOT) : nullptr);
      const double out = onsetdev::frame_value(o.function, N + 1, lane, c, p, pp);
      if (lane == 0) o.raw[(int64_t) b * o.T + t] = out;
    }
    __syncthreads(); // nobody reads the ring any more: the next round may overwrite it
  }
}

template <int R1, int R2, int R3, int NW>
static bool launch_onset_fused_t(const StftBArgs& k, const OnsetFusedArgs& o, hipStream_t s)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int SLOTS = 2 * NW > NW + 2 ? 2 * NW : NW + 2;
  constexpr size_t shmem = (size_t) Core::TW * 16 + (size_t) NW * Core::BUFD * 8 + (size_t) SLOTS * (Core::N + 1) * 16;
  static_assert(shmem <= 160 * 1024, "LDS");
  const int runsPerBuf = (o.T + kOnsetRun - 1) / kOnsetRun;
  const int64_t grid = (int64_t) k.B * runsPerBuf;
  if (grid < 1) return true;
  if (grid > 0x7fffffffLL) return false;
  auto kern = onset_fused_kernel<R1, R2, R3, NW>;
  request_dynamic_lds(kern, shmem);
  hipLaunchKernelGGL(kern, dim3((unsigned) grid), dim3(64 * NW), shmem, s, k, o, runsPerBuf);
  return true;
}

bool onset_fused_supported(int64_t win, int64_t fft)
{
  return win >= 2 && fft_core_supported(win, fft);
}

bool launch_onset_fused(const StftArgs& a, const OnsetFusedArgs& o, hipStream_t s)
{
  if (!onset_fused_supported(a.win, a.fft)) return false;
  const StftBArgs k = block_args(a);
  // wavefronts per workgroup by what the ring of spectra leaves of the LDS: 92, 99 and 148 KB
  if (a.fft == 1024) return launch_onset_fused_t<8, 8, 8, 4>(k, o, s);
  if (a.fft == 2048) return launch_onset_fused_t<16, 8, 8, 2>(k, o, s);
  return launch_onset_fused_t<16, 8, 16, 1>(k, o, s);
}

} // namespace fluhip
