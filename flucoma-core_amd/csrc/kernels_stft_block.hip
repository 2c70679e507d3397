// kernels_stft_block.hip -- K1 in its block form: a workgroup of NW wavefronts transforms NW CONSECUTIVE frames of one
// buffer (one frame per wavefront, registers + a private LDS exchange buffer) and writes the magnitudes in BOTH
// layouts the factor updates stream -- frame-major rows straight from the registers, and the bin-major copy
// (`magT`, frame index contiguous) through an LDS staging step, NW frames of a bin at a time -- so no separate
// pass over V is needed after the STFT (the transpose kernel read and rewrote all of V: +1.8 GB on the bench shard).
// With its stores disabled the kernel transforms the bench shard's 110 336 frames in 430 us (the FP64 VALU ~70 % busy);
// writing V twice (1.86 GB, half of it as 64-byte pieces of 1025 different rows) brings it to 775-815 us -- against
// 973-1030 us for the wave kernel plus the transposing copy on the same boxes.  The stores, not the transform, set
// the pace: tools/hbm_write_probe.hip reproduces the figure with a plain FMA loop and the same two store patterns.
#include "fft_core.h"

namespace fluhip {

// FPW frames per wavefront and round: a block stages NW * FPW consecutive frames before the bin-major flush, so a bin's
// piece of the transposed copy is NW * FPW * 8 bytes -- a full 128-byte line at fft 2048 with 8 wavefronts x 2 frames
// (64-byte pieces measured 3.3 TB/s against 4.4 - 5.9 for full lines, tools/hbm_write_probe.hip).
// DB (round 5): TWO sets of staging buffers, used in turn -- the flush of round r reads set r & 1 while the transforms of
// round r + 1 fill the other, so the barrier behind the flush goes (a wavefront reaches the next round's barrier only after its
// own flush reads, and nobody writes a set before everybody has passed that barrier).
template <int R1, int R2, int R3, int NW, int WINLDS, bool SPEC, int FPW = 1, bool DB = false>
__global__ __launch_bounds__(64 * NW) void stft_block_kernel(StftBArgs a)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, PPL = Core::PPL, BUFD = Core::BUFD;   // complex points per frame = fft / 2, points per lane, doubles per wavefront
  extern __shared__ __attribute__((aligned(16))) double lds[];
  d2* tw2 = reinterpret_cast<d2*>(lds);       // [R2-1][NS2], then [R3-1][NS3]
  d2* wl = tw2 + Core::TW;                    // [N] window pairs when WINLDS
  double* xall = reinterpret_cast<double*>(wl + (WINLDS ? N : 0));
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* xb = xall + wave * FPW * BUFD;
  constexpr int FPB = NW * FPW; // frames per block and round

  const d2* twg = reinterpret_cast<const d2*>(a.twiddle);
  Core::fill_tables(tw2, twg, threadIdx.x, 64 * NW);
  const d2* wsrc = reinterpret_cast<const d2*>(a.window);
  if (WINLDS)
  {
    for (int m = threadIdx.x; m < N; m += 64 * NW) wl[m] = wsrc[m];
    wsrc = wl;
  }
  __syncthreads();

  Core core;
  core.init(xb, tw2, twg, lane);

  // blocks are dealt so that workgroups on one XCD (blockIdx & 7) take neighbouring blocks of a buffer: their
  // segments of a bin-major row fall into the same L2
  const int64_t chunk = (a.totalBlocks + 7) / 8;
  // block L of the dealing order -> (buffer, first frame); false past the end
  auto decode = [&](int64_t L, int& b, int& t0) -> bool {
    const int64_t slot = L >> 3;
    const int64_t blk = (L & 7) * chunk + slot;
    if (slot >= chunk || blk >= a.totalBlocks) return false;
    b = (int) (blk / a.blocksPerBuf);
    t0 = (int) (blk % a.blocksPerBuf) * FPB;
    return true;
  };
  // Prefetch (one frame per round, float audio): the samples of the NEXT round's frame are requested before this round's
  // stores are issued.  vmcnt counts loads and stores in one in-order counter, so samples requested AFTER the stores (as in
  // round 2's loop) can only be waited for by waiting for every store of the round before -- the store drain sat exposed
  // in front of every frame's arithmetic (the ISA had s_waitcnt vmcnt(7) behind eight fresh loads: "all stores done").
  // Requested BEFORE them, the samples are older than the stores and the wait leaves the stores in flight: 793 / 838 us
  // -> 697 / 691 us for the bench workload's STFT phase (profiles/r03/stft_prefetch.txt; FLUHIP_STFT_PREFETCH=0 is the
  // round-2 order).  Requesting them before the transform instead (35 more registers) measured the same, and two
  // 4-wavefront blocks per CU instead of one of 8 measured slower (754 / 763 us): neither is kept.
  constexpr bool PREFETCH = FPW == 1 && PPL == 16 && NW <= 12; // fft 2048 at two or three wavefronts per SIMD only: fft 1024 (4 wavefronts per SIMD) measures the same either way, fft 4096 has no registers to spare, and 16 wavefronts of fft 2048 need the 32 registers
  float2 raw[PPL];
  int rawB = -1, rawT = -1;
  auto prefetch = [&](int64_t Ln) {
    rawB = -1;
    if constexpr (PREFETCH)
    {
      int bn, t0n;
      if (!a.audio || !a.prefetch || (Ln >> 3) >= chunk || !decode(Ln, bn, t0n)) return;
      const int tn = t0n + wave;
      const int64_t nS = a.nTab ? a.nTab[bn] : a.n;
      const int Tn = a.nTab ? (int) ((nS + a.hop) / a.hop) : a.T;
      if (tn >= Tn) return;
      if (!request_samples<R1, N>(a, bn, tn, nS, lane, raw)) return;
      rawB = bn;
      rawT = tn;
    }
  };
  for (int64_t L = blockIdx.x;; L += gridDim.x)
  {
    int b, t0;
    if ((L >> 3) >= chunk) break;
    if (!decode(L, b, t0)) continue;
    [[maybe_unused]] double* const xcur = DB ? core.xb - wave * FPW * BUFD : xall;   // this round's set of staging buffers
    [[maybe_unused]] double* const xbw = DB ? core.xb : xb;
    // ragged corpora: the buffer's own length decides its frame count (alg/STFT.hpp:98-99); frames past it are padding
    const int64_t nSamples = a.nTab ? a.nTab[b] : a.n;
    const int Tb = a.nTab ? (int) ((nSamples + a.hop) / a.hop) : a.T;
#pragma unroll 1
    for (int fj = 0; fj < FPW; fj++)
    {
      const int t = t0 + wave * FPW + fj;
      if (t < Tb)
      {
        cx pts[PPL];
        if (PREFETCH && rawB == b && rawT == t)
          window_samples<R1, N>(raw, lane, wsrc, pts);
        else
          gather_points<R1, N>(a, b, t, lane, wsrc, pts, nSamples);
        SCHED_FENCE();
        core.template run<SPEC>(pts, SPEC ? reinterpret_cast<d2*>(a.spec + (int64_t) b * a.specStride + (int64_t) t * a.F * 2) : nullptr);
      }
      else if (a.magT)
      {
        // frames past the end of the buffer: zeros into the padding columns of the bin-major copy
#pragma unroll
        for (int i = 0; i < PPL; i++) core.xb[lane + 64 * i] = 0.0;
        if (lane == 0) core.xb[N] = 0.0;
      }
      if (FPW > 1) core.shift(fj + 1 < FPW ? BUFD : -(FPW - 1) * BUFD);
    }
    prefetch(L + gridDim.x);                          // ahead of this round's stores

    if (a.magT) LDS_BARRIER();                        // every wavefront of the block has staged its frames
    if (a.mag)
    {
#pragma unroll 1
      for (int fj = 0; fj < FPW; fj++)
      {
        const int t = t0 + wave * FPW + fj;
        if (t >= Tb) break;
        // frame-major row from the wavefront's own staging buffer, 16 bytes per lane
        double* magRow = a.mag + (int64_t) b * a.magStride + (int64_t) t * a.ldMag;
        const double* xs = xbw + fj * BUFD;
#pragma unroll
        for (int q = 0; q < N / 128; q++)
        {
          const int k = 2 * (lane + 64 * q);
          store_mag16(magRow + k, *reinterpret_cast<const d2*>(xs + k));
        }
        if (lane == 0) magRow[N] = xs[N];
      }
    }
    if (a.magT)
    {
      // ---- bin-major copy: the block's frames of a bin leave as one piece ------------------------------------------
      constexpr int HP = FPB / 2;                     // 16-byte pieces (two frames) per bin
      double* outT = a.magT + (int64_t) b * a.magTStride;
      constexpr int ITEMS = (N + 1) * HP, NTHR = 64 * NW, TRIPS = (ITEMS + NTHR - 1) / NTHR; // (a.F == N + 1)
      constexpr int UNR = PREFETCH ? TRIPS : 1;       // (a compile-time count of stores is what lets the wait ahead of the next transform skip them)
#pragma unroll UNR
      for (int k = 0; k < TRIPS; k++)
      {
        const int i = (int) threadIdx.x + k * NTHR;
        const int f = i / HP, p = i - f * HP;
        const int tc = t0 + 2 * p;
        if (i < ITEMS && tc < a.ldMagT)
        {
          const double v0 = xcur[(2 * p) * BUFD + f], v1 = xcur[(2 * p + 1) * BUFD + f];
          store_mag16(outT + (int64_t) f * a.ldMagT + tc, d2{v0, v1});
        }
      }
      if constexpr (!DB) LDS_BARRIER();
    }
    if constexpr (DB)
    {
      // the other set of staging buffers for the next round
      const int set = (int) ((core.xb - xall) >= NW * FPW * BUFD);
      core.shift(set ? -NW * FPW * BUFD : NW * FPW * BUFD);
    }
  }
}

template <int R1, int R2, int R3, int NW, int WINLDS, int FPW = 1, bool DB = false>
static bool launch_block_t(const StftBArgs& k0, hipStream_t s)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr size_t shmem = ((size_t) Core::TW + (WINLDS ? Core::N : 0)) * 16 + (size_t) (DB ? 2 : 1) * NW * FPW * Core::BUFD * 8;
  static_assert(shmem <= 160 * 1024, "LDS");
  StftBArgs k = k0;
  static const int pf = [] { const char* e = fluhip::ab_getenv("FLUHIP_STFT_PREFETCH"); return e ? std::atoi(e) : 1; }();
  k.prefetch = pf;
  k.blocksPerBuf = (k.T + NW * FPW - 1) / (NW * FPW);
  k.totalBlocks = (int64_t) k.B * k.blocksPerBuf;
  if (k.totalBlocks < 1) return true;
  auto kern = k.spec ? stft_block_kernel<R1, R2, R3, NW, WINLDS, true, FPW, DB> : stft_block_kernel<R1, R2, R3, NW, WINLDS, false, FPW, DB>;   // the complex spectrum is kept for resynthesis / BufSTFT only
  request_dynamic_lds(kern, (size_t) (shmem));
  const int64_t chunk = (k.totalBlocks + 7) / 8;
  int64_t grid = 8 * chunk;
  const int perCu = (int) ((160 * 1024) / shmem);
  const int64_t cap = 256 * (int64_t) (perCu < 1 ? 1 : perCu);
  if (grid > cap) grid = cap;
  hipLaunchKernelGGL(kern, dim3((unsigned) grid), dim3(64 * NW), shmem, s, k);
  return true;
}

// both magnitude layouts from one kernel; false when the shape has no block form (the caller then falls back to
// launch_stft + launch_transpose)
bool launch_stft_block(const StftArgs& a, double* magT, int64_t magTStride, int64_t ldMagT, hipStream_t s)
{
  if (!fft_core_supported(a.win, a.fft)) return false;
  static const bool off = [] { const char* e = fluhip::ab_getenv("FLUHIP_STFT_BLOCK"); return e && std::atoi(e) == 0; }();
  if (off) return false;   // A/B: the round-1 wave kernel + transposing copy
  StftBArgs k = block_args(a);
  k.mag = a.mag; k.magStride = a.magStride; k.ldMag = a.ldMag;
  k.magT = magT; k.magTStride = magTStride; k.ldMagT = ldMagT;
  k.spec = a.spec; k.specStride = a.specStride; k.nTab = a.nTab;
  if (magT && (ldMagT % 2) != 0) return false;
  if (a.fft == 2048)
  {
    // 8 frames per block, two wavefronts per SIMD (143 registers without the spectrum output; 12 per workgroup fit too and
    // measured the same).  FLUHIP_STFT_FPW=2: TWO frames per wavefront and round, so that 16 frames of a bin leave as one
    // 128-byte line of the bin-major copy instead of 64-byte pieces (the 16 staging buffers leave no room for the window in
    // the LDS: it is read through the L1).  Built on the round-2 review's suggestion and measured on one box, back to back:
    // 803 / 820 us against 765 / 783 us for the one-frame form (profiles/r03/stft_fpw.txt) -- full lines are not what the
    // phase waits for (fft 1024 already writes 128-byte pieces and runs at the same bytes per second), so it stays off.
    static const int fpw = [] { const char* e = fluhip::ab_getenv("FLUHIP_STFT_FPW"); return e ? std::atoi(e) : 1; }();
    if (fpw == 2) return launch_block_t<16, 8, 8, 8, 0, 2>(k, s);
    // Two sets of staging buffers used in turn (round 5): the bin-major flush of round r runs under the transforms of round
    // r + 1 and the barrier behind the flush goes -- 565 - 580 -> 513 - 542 us per launch of the bench corpus's STFT, same box,
    // alternating (profiles/r05/stft_double_buffer.txt).  The second set takes the room of the window table: the window is
    // read through the L1.  Without a bin-major copy there is no barrier to save; FLUHIP_STFT_DB=0 (A/B build): one set.
    static const int db = [] { const char* e = fluhip::ab_getenv("FLUHIP_STFT_DB"); return e ? std::atoi(e) : 1; }();
#ifdef FLUHIP_AB_SWITCHES
    // FLUHIP_STFT_NW=16 (A/B build, round 5): sixteen frames per block, four wavefronts per SIMD, one set of staging buffers, no
    // sample prefetch -- the form fft 1024 runs in; a bin's piece of the bin-major copy is a full 128-byte line.  At 128
    // registers the 16-point-per-lane transform spills 41 of them: 878 - 887 us per STFT phase of the bench corpus against
    // 651 - 652 for the production form (tools/stft_timing.py, profiles/r05/stft_nw16.txt; twelve wavefronts at 168 registers
    // spill 59: 1 240 us).  Not adopted.
    {
      static const int nw = [] { const char* e = fluhip::ab_getenv("FLUHIP_STFT_NW"); return e ? std::atoi(e) : 8; }();
      if (nw == 16) return launch_block_t<16, 8, 8, 16, 0>(k, s);
    }
#endif
    if (db == 1 && magT) return launch_block_t<16, 8, 8, 8, 0, 1, true>(k, s);
    return launch_block_t<16, 8, 8, 8, 1>(k, s);
  }
  if (a.fft == 4096)
  {
    // BASELINE config 3: 32 points per lane (one wavefront per SIMD), 4 frames per block
    return launch_block_t<16, 8, 16, 4, 1>(k, s);
  }
  if (a.fft == 1024)
  {
    // 16 frames per block (128 registers, four wavefronts per SIMD): 128-byte pieces of the bin-major rows
    // (two sets of staging buffers, as at fft 2048, measured slower here -- 681 - 690 against 659 - 663 us for 128 x 10 s at hop
    //  256: four wavefronts per SIMD already overlap the flush, and the window through the L1 costs more than the barrier)
    return launch_block_t<8, 8, 8, 16, 1>(k, s);
  }
  return false;
}

} // namespace fluhip
