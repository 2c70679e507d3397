// kernels_spectral_fused.hip -- K13, the on-chip form of BufSpectralShape and BufChroma (the arithmetic is in spectral_terms.h,
// which switches contraction off for itself: kernels_spectral.hip is compiled with -ffp-contract=off, this file is not).
// A workgroup of NW wavefronts takes kSpectralRun consecutive frames of one buffer; wavefront w transforms the frames
// t0 + w, t0 + w + NW, ... with FftCore (fft_core.h), which leaves |X| in the wavefront's staging buffer, and finishes each
// of them alone: no frame looks at another, so there is no ring and no barrier in the loop.
//   SpectralShape  the sums, the central moments in a second pass over the staged magnitudes, the rolloff's running sum and
//                  the log sum: seven doubles leave the chip per frame
//   Chroma         the range-zeroed squared magnitudes go to the workspace the GEMM reads: no magnitude is written
// Every address is formed in front of the branches.
#include "fft_core.h"
#include "fluhip_spectral.h"
#include "spectral_terms.h"

namespace fluhip {

template <int R1, int R2, int R3, int NW>
__global__ __launch_bounds__(64 * NW) void spectral_fused_kernel(StftBArgs a, SpectralFusedArgs o, int runsPerBuf)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, PPL = Core::PPL, BUFD = Core::BUFD;
  constexpr int F = N + 1;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  d2* tw2 = reinterpret_cast<d2*>(lds);
  double* xall = reinterpret_cast<double*>(tw2 + Core::TW);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const d2* twg = reinterpret_cast<const d2*>(a.twiddle);
  Core::fill_tables(tw2, twg, threadIdx.x, 64 * NW);
  const d2* wsrc = reinterpret_cast<const d2*>(a.window);
  __syncthreads();
  double* xb = xall + wave * BUFD;
  Core core;
  core.init(xb, tw2, twg, lane);

  const int b = (int) (blockIdx.x / (unsigned) runsPerBuf);
  const int t0 = (int) (blockIdx.x % (unsigned) runsPerBuf) * kSpectralRun;
  const int t1 = t0 + kSpectralRun < a.T ? t0 + kSpectralRun : a.T;
  for (int t = t0 + wave; t < t1; t += NW) // (wave-uniform: whole wavefronts leave)
  {
    const int64_t f = (int64_t) b * a.T + t;
    double* res = o.out ? o.out + kShapeDescriptors * f : nullptr;
    double* row = o.pw ? o.pw + f * F : nullptr;
    cx pts[PPL];
    gather_points<R1, N>(a, b, t, lane, wsrc, pts, a.n);
    SCHED_FENCE();
    core.template run<false>(pts, nullptr);
    if (o.kind == kSpectralShape)
    {
      if (res) spectraldev::shape_frame(xb, lane, o.shape, res);
    }
    else if (row)
      spectraldev::chroma_power_row(xb, F, lane, o.zlo, o.zhi, row);
  }
}

template <int R1, int R2, int R3, int NW>
constexpr size_t spectral_fused_lds()
{
  using Core = FftCore<R1, R2, R3>;
  return (size_t) Core::TW * 16 + (size_t) NW * Core::BUFD * 8;
}
// twiddle tables + NW staging buffers: 26, 33 and 49 KB
static_assert(spectral_fused_lds<8, 8, 8, 4>() == 26560 && spectral_fused_lds<16, 8, 8, 2>() == 33568 &&
              spectral_fused_lds<16, 8, 16, 1>() == 49936, "LDS footprint of the on-chip spectral form (DESIGN K13)");

template <int R1, int R2, int R3, int NW>
static bool launch_spectral_fused_t(const StftBArgs& k, const SpectralFusedArgs& o, hipStream_t s)
{
  constexpr size_t shmem = spectral_fused_lds<R1, R2, R3, NW>();
  static_assert(shmem <= 160 * 1024, "LDS");
  const int runsPerBuf = (k.T + kSpectralRun - 1) / kSpectralRun;
  const int64_t grid = (int64_t) k.B * runsPerBuf;
  if (grid < 1) return true;
  if (grid > 0x7fffffffLL) return false;
  auto kern = spectral_fused_kernel<R1, R2, R3, NW>;
  request_dynamic_lds(kern, shmem);
  hipLaunchKernelGGL(kern, dim3((unsigned) grid), dim3(64 * NW), shmem, s, k, o, runsPerBuf);
  return true;
}

bool spectral_fused_supported(int64_t win, int64_t fft) { return win >= 2 && fft_core_supported(win, fft); }

bool launch_spectral_fused(const StftArgs& a, const SpectralFusedArgs& o, hipStream_t s)
{
  if (!spectral_fused_supported(a.win, a.fft) || a.F != a.fft / 2 + 1) return false;
  if (o.kind == kSpectralShape)
  {
    // the bins the kernel indexes its staging buffer with: the segment [lo, lo + size) ends inside the F bins
    const ShapeParams& p = o.shape;
    if (!o.out || !p.axis || p.size < 1 || p.lo < 0 || p.lo + p.size > a.F || (p.fold && p.lo != 1)) return false;
  }
  else if (o.kind != kSpectralChroma || !o.pw)
    return false;
  const StftBArgs k = block_args(a);
  // wavefronts per workgroup as in the onset and pitch forms: 4, 2 and 1
  if (a.fft == 1024) return launch_spectral_fused_t<8, 8, 8, 4>(k, o, s);
  if (a.fft == 2048) return launch_spectral_fused_t<16, 8, 8, 2>(k, o, s);
  return launch_spectral_fused_t<16, 8, 16, 1>(k, o, s);
}

} // namespace fluhip
