// kernels_stft_feat.hip -- the fused feature form (STFT -> MelBands -> MFCC in one kernel, see below) on the core of fft_core.h
#include "fft_core.h"

#include <algorithm>
#include <cstdio>
#include <type_traits>
#include <vector>

namespace fluhip {

// ---- wavefront scan of doubles with DPP moves (no LDS crossbar): lanes a DPP source does not reach read 0 ----------------
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_f64(double x)
{
  const long long b = __double_as_longlong(x);
  if constexpr (ROWMASK == 0xf)
  {
    // every row enabled: bound_ctrl supplies the zeros of the lanes a shift does not reach, and the move has no `old`
    // operand to initialise (update_dpp(0, ...) cost a v_mov_b32 per half: 20 per frame of the feature kernel)
    const int lo = __builtin_amdgcn_mov_dpp((int) (b & 0xffffffff), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp((int) (b >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long) hi << 32) | (unsigned) lo);
  }
  const int lo = __builtin_amdgcn_update_dpp(0, (int) (b & 0xffffffff), CTRL, ROWMASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int) (b >> 32), CTRL, ROWMASK, 0xf, false);
  return __longlong_as_double(((long long) hi << 32) | (unsigned) lo);
}
// inclusive prefix sum over the 64 lanes, lane order
__device__ __forceinline__ double wave_scan(double x)
{
  x += dpp_f64<0x111, 0xf>(x);   // row_shr:1
  x += dpp_f64<0x112, 0xf>(x);   // row_shr:2
  x += dpp_f64<0x114, 0xf>(x);   // row_shr:4
  x += dpp_f64<0x118, 0xf>(x);   // row_shr:8
  x += dpp_f64<0x142, 0xa>(x);   // row_bcast:15 into rows 1 and 3
  x += dpp_f64<0x143, 0xc>(x);   // row_bcast:31 into rows 2 and 3
  return x;
}
// value of the lane below (0 for lane 0)
__device__ __forceinline__ double wave_shr1(double x) { return dpp_f64<0x138, 0xf>(x); } // wave_shr:1

// ---------------------------------------------------------------------------------------------------------------
// Fused feature form (BASELINE config 5: STFT -> MelBands -> MFCC): the frame's magnitudes never leave the
// wavefront's LDS buffer -- per frame the kernel reads hop 4 bytes of samples and writes nOut 4 bytes of features.
//   algorithm::MelBands::processFrame   include/flucoma/algorithms/public/MelBands.hpp:79-97
//   algorithm::DCT::processFrame        include/flucoma/algorithms/public/DCT.hpp:65-75
//   client glue                         include/flucoma/clients/rt/MFCCClient.hpp:122-130, rt/MelBandsClient.hpp:104-113
// A mel filter bank is a row of overlapping triangles: every bin lies on the rising edge of at most one band and on the
// falling edge of at most one (the one below).  With up[f] / dn[f] the two weights of bin f, band b is
//   sum_{f in interval b} up[f] m[f] + sum_{f in interval b+1} dn[f] m[f],   interval s = bins between centres s and s+1,
// two segment sums of two running sums over the bins: lane l forms the running sums of its CH consecutive bins, a
// wavefront scan gives each lane its offset, the lanes holding the last bin before an interval boundary publish the
// running sums there, and lane b takes band b as two differences.  (The host checks that the filter bank at hand has
// this shape -- api_features.hip features_common -- and falls back to the two-kernel path otherwise.)
// No workgroup barrier anywhere in the frame loop: wavefronts are independent.
// ---------------------------------------------------------------------------------------------------------------
// alg/MelBands.hpp:95  20 log10(max(eps, band)) of the fused kernels.  The feature leaves as a float: the logarithm is
// taken in single precision (hardware log2; the band energy rounds to float with 6e-8 relative error = 5e-7 dB, below the
// float output's own resolution).  A band energy past the float range (float audio within a few orders of FLT_MAX: a band
// sums hundreds of bins of a window's worth of samples) would round to infinity and the DCT behind it would make NaNs of a
// whole frame: there, and only there, the exponent is split off first -- frexp, then log2 of the mantissa plus the exponent
__device__ __forceinline__ float band_db(double v)
{
  const float x = (float) fmax(v, kEpsilon);
  float l = __log2f(x);
  if (__builtin_expect(x > 3.402823466e38f, 0))
  {
    int e;
    const double m = __builtin_frexp(v, &e);
    l = __log2f((float) m) + (float) e;
  }
  return 6.020599913279624f * l;
}

struct FeatFusedArgs
{
  const double* up;    // [64 CH] rising-edge weight of bin f (0 where none)
  const double* dn;    // [64 CH] falling-edge weight of bin f
  const short* slot;   // [64 CH] s if bin f is the last bin before interval s starts (publishes the running sums), else -1
  const double* dct;   // [nDct][nBands] or nullptr
  int nBands, nDct, startCoeff, nOut;
  int magNorm, usePower, logOutput;
  float* out;          // [B][nOut][T]
  long long* dbg = nullptr; // FLUHIP_FEAT_CLOCK (A/B build): shader-cycle and 100 MHz stamps of workgroup 0's first wavefront
};

// DYN (round 4): the wavefronts of a workgroup take their frames from a counter in the LDS instead of a fixed share.  The issue
// arbiter of a SIMD serves its oldest wavefront first: with equal shares the first wavefront of every SIMD was done after
// 2.0 ms of a 3.86 ms launch (config 5, per-wavefront stamps) and the youngest ran the last third of the launch alone, at a
// quarter of the VALU's rate -- the counters show the VALU 87 % busy while four wavefronts are alive and 64 % over the launch.
// Handing out frames as wavefronts come free makes them finish together.
// SMALL (round 4): the layout for TWO workgroups per CU (20 wavefronts, five per SIMD, where one workgroup of 1024 threads stops
// at four): the window pairs come through the L1 instead of the LDS and the per-wavefront scratch of the band stage lies in
// the wavefront's staging buffer, which is idle by then -- 67 KB per workgroup of ten wavefronts at fft 1024.
// FASTMAG (round 5): the magnitudes behind one Goldschmidt step (mag_sqrt2<true>: 2e-14 relative, 24 VALU instructions per frame
// fewer at fft 1024) -- they feed band sums that leave as float32.  FLUHIP_FEAT_FASTMAG=0 (A/B build): the full square root.
template <int R1, int R2, int R3, int NW, bool DYN = true, bool SMALL = false, bool FASTMAG = true>
__global__ __launch_bounds__(64 * NW, SMALL ? 5 : 1) void stft_feat_kernel(StftBArgs a, FeatFusedArgs fa)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, PPL = Core::PPL, BUFD = Core::BUFD;
  constexpr int CH = (N + 1 + 63) / 64;           // consecutive bins per lane in the band sums
  // per-wavefront scratch: boundary sums (rising, falling) -- 66 boundary slots, then one DUMP slot per lane: bins that end no
  // interval publish there, so that the publishing needs no compare, no exec mask and no select (36 v_cndmask + 9 v_cmp per
  // frame as the compiler had if-converted it) -- and the band values
  constexpr int WB = 66 + 64;
  constexpr int WS = SMALL ? 0 : 2 * WB + 64;
  static_assert(!SMALL || BUFD >= 2 * WB + 64, "the band stage's scratch inside the staging buffer");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  d2* tw2 = reinterpret_cast<d2*>(lds);
  d2* wl = tw2 + Core::TW;                        // [N] window pairs
  constexpr bool TAB = R1 == 8;                   // (fft 2048 has no LDS to spare for the table)
  d2* tws = wl + (SMALL ? 0 : N);                 // [N] the split's twiddles, halved
  double* xall = reinterpret_cast<double*>(tws + (TAB ? N : 0));
  double* scr = xall + NW * BUFD;                 // [NW][WS]
  double* upl = scr + NW * WS;                    // [64 CH]
  double* dnl = upl + 64 * CH;                    // [64 CH]
  double* dctl = dnl + 64 * CH;                   // [nDct * nBands]
  const int dq = (fa.nBands + 3) >> 2;            // bands per quarter row (four lanes share a coefficient)
  const int dld = 4 * dq + 1;                     // DCT rows: four quarters, zero-padded past nBands, one double apart in bank phase
                                                  // (rows of 40 doubles would put rows j and j + 4 on one bank)
  short* slotl = reinterpret_cast<short*>(dctl + (fa.dct ? fa.nDct * dld : 0));   // [64 CH]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* xb = xall + wave * BUFD;
  double* bu = SMALL ? xb : scr + wave * WS;
  double* bd = bu + WB;
  double* bands = bd + WB;

  const d2* twg = reinterpret_cast<const d2*>(a.twiddle);
  Core::fill_tables(tw2, twg, threadIdx.x, 64 * NW);
  if constexpr (!SMALL)
    for (int m = threadIdx.x; m < N; m += 64 * NW) wl[m] = reinterpret_cast<const d2*>(a.window)[m];
  if constexpr (TAB)
    for (int m = threadIdx.x; m < N; m += 64 * NW) { const d2 w = twg[m]; tws[m] = d2{0.5 * w[0], 0.5 * w[1]}; }
  // (per-lane tables lie [i][lane] in the LDS: a lane's CH consecutive bins are CH rows apart, a row is read without bank conflicts)
  for (int i = threadIdx.x; i < 64 * CH; i += 64 * NW)
  {
    const int q = (i % CH) * 64 + i / CH;
    upl[q] = fa.up[i]; dnl[q] = fa.dn[i];
    const short sl = fa.slot[i];
    slotl[q] = sl >= 0 ? sl : (short) (66 + i / CH);           // (the lane's dump slot)
  }
  if (fa.dct)
    for (int i = threadIdx.x; i < fa.nDct * dld; i += 64 * NW)
    {
      const int row = i / dld, col = i % dld;
      dctl[i] = col < fa.nBands ? fa.dct[row * fa.nBands + col] : 0.0;
    }
  if constexpr (!SMALL)
    for (int i = lane; i < WS; i += 64) bu[i] = 0.0;  // boundaries nobody publishes (before the first bin) stay 0
  __shared__ unsigned nextFrame;                      // DYN: frames of this workgroup handed out so far
  if (threadIdx.x == 0) nextFrame = 0;
  __syncthreads();

#ifdef FLUHIP_AB_SWITCHES
  if (fa.dbg && threadIdx.x == 0)
  {
    if (blockIdx.x == 0) fa.dbg[0] = (long long) __builtin_readcyclecounter();
    fa.dbg[4 + 2 * blockIdx.x] = (long long) wall_clock64();
  }
#endif
  Core core;
  core.init(xb, tw2, twg, lane);
  core.splitTab = tws;
  // FLUHIP_FEAT_PRIO (A/B): the wavefronts of a SIMD (wave, wave + 4, ...) at different issue priorities.  They run the same
  // instruction stream from the same start; under fair round-robin issue they stay in phase -- all in their LDS exchanges,
  // then all in their butterflies -- and the two pipes take turns instead of overlapping (PMC: VALU busy 46 % + LDS active
  // 42 % of the launch).  With strict priorities the first one runs ahead and the others fill its waits.
#ifdef FLUHIP_AB_SWITCHES
  if (a.prefetch & 2) { const int pr = (wave ^ (wave >> 2)) & 3; if (pr == 0) __builtin_amdgcn_s_setprio(0); else if (pr == 1) __builtin_amdgcn_s_setprio(1); else if (pr == 2) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(3); }
#endif
  const double scale1 = 1.0 / ((double) a.win / 4.0);                          // alg/MelBands.hpp:49
  const double scale2 = 1.0 / (2.0 * (double) (2 * N) / (double) a.win);       // :52
  // Lane constants of the band stage kept in registers across the frame loop (round 5: the kernel sits at 101 of its 128
  // registers, and the LDS pipe co-limits it): the boundary slot of each of the lane's CH bins (was a ds_read_i16 and a shift
  // per bin and frame) and, for the MFCC default's ten products per lane, the lane's quarter row of the DCT table.
  constexpr bool HOIST = !SMALL;
  [[maybe_unused]] int slotReg[CH];
  if constexpr (HOIST)
  {
#pragma unroll
    for (int i = 0; i < CH; i++) slotReg[i] = slotl[i * 64 + lane];
  }
  // (the A/B build's kernel carries the experiment switches of rounds 3 - 4 and has no room for the ten coefficients: with them it
  //  spills 16 registers to scratch -- 3.4 ms on config 5)
  const bool dct10 = HOIST && !kAbSwitches && fa.dct && 4 * fa.nOut <= 64 && dq == 10;
  [[maybe_unused]] double drowReg[10];
  {
    const int j = lane >> 2, part = lane & 3;
    const bool live = j < fa.nOut && fa.startCoeff + j < fa.nDct;
    const double* drow = dctl + (live ? fa.startCoeff + j : 0) * dld + part * dq;
#pragma unroll
    for (int i = 0; i < 10; i++) drowReg[i] = dct10 ? drow[i] : 0.0;
  }

  const int64_t chunk = (a.totalBlocks + 7) / 8;
  // (Round 4: what these measurements were really showing is in the DYN comment at the head of the kernel.)
  // Round 3 measurements of this loop (config 5, 1.417 M frames, one box; profiles/r03/c5_breakdown.txt), parts switched off
  // one at a time: everything 3.93 ms; without the sample gather 3.38; without the transform 1.92; without the band sums /
  // DCT / stores 2.95 (the stores alone: 0.05); the loop with nothing in it 0.38.  Alone, the gather takes 0.82 ms (the HBM
  // time of 2.9 GB of samples), the transform 2.0, the band part 1.0 -- the parts add up: 93 KB of LDS traffic per frame
  // (transform exchanges 32, twiddles 14, window 8, staging 8 + 8, weights and DCT rows 23) keep the LDS pipe busy through
  // all three.  Requesting the next frame's samples ahead of the feature stores (as stft_block_kernel does) changes
  // nothing here (3.94 / 3.94 ms without, 3.92 / 3.92 with): four wavefronts per SIMD cover that wait.
  // Block index -> (buffer, frame block) WITHOUT a division per frame: the workgroup's blocks are blk0, blk0 + step, ...
  // (step = gridDim.x / 8 inside its XCD's chunk), so (buffer, frame block) advance by (step / blocksPerBuf, step %
  // blocksPerBuf) with a carry -- scalar adds.  The 64-bit blk / blocksPerBuf, blk % blocksPerBuf of rounds 2 - 3 ran on the
  // VALU (quarter-rate v_mul_hi / v_mul_lo sequences) once per frame and wavefront: most of the 0.38 ms the EMPTY frame
  // loop measured at config 5 (profiles/r03/c5_breakdown.txt).
  const int64_t blk0 = (int64_t) (blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
  const int step = (int) (gridDim.x >> 3);                      // (launch_feat_t: the grid is a multiple of 8)
  const int stepB = step / a.blocksPerBuf, stepF = step % a.blocksPerBuf;
  int bCur = __builtin_amdgcn_readfirstlane((int) (blk0 / a.blocksPerBuf));
  int fCur = __builtin_amdgcn_readfirstlane((int) (blk0 % a.blocksPerBuf));
  int64_t slot8 = blockIdx.x >> 3, blk = blk0;
  // DYN: unit u of the workgroup = wavefront slot u % NW of its block u / NW (block i of the workgroup is block blk0 + i step of
  // the launch); the division by blocksPerBuf is a multiplication by its reciprocal on the scalar unit
  const unsigned bpb = (unsigned) a.blocksPerBuf, bpbInv = (unsigned) (((unsigned long long) 1 << 32) / bpb);
  for (;; slot8 += step, blk += step, bCur += stepB, fCur += stepF)
  {
    int b, t;
    if constexpr (DYN)
    {
      unsigned u = 0;
      if (lane == 0) u = atomicAdd(&nextFrame, 1u);
      u = (unsigned) __builtin_amdgcn_readfirstlane((int) u);
      const unsigned i = u / NW, slot = u % NW;
      const int64_t bl = blk0 + (int64_t) i * step;
      if ((int64_t) (blockIdx.x >> 3) + (int64_t) i * step >= chunk || bl >= a.totalBlocks) break; // (blocks ascend: nothing behind this one either)
      const unsigned x = (unsigned) bl;               // (totalBlocks < 2^31: launch_feat_t)
      unsigned q = __umulhi(x, bpbInv), r = x - q * bpb;
      while (r >= bpb) { q++; r -= bpb; }
      b = (int) q;
      t = (int) (r * NW + slot);
      if (t >= a.T) continue;
    }
    else
    {
      if (fCur >= a.blocksPerBuf) { fCur -= a.blocksPerBuf; bCur += 1; }
      if (slot8 >= chunk) break;
      if (blk >= a.totalBlocks) continue;
      b = bCur;
      t = fCur * NW + wave;
      if (t >= a.T) continue;
    }
    {
      cx pts[PPL];
#ifdef FLUHIP_AB_SWITCHES
      // FLUHIP_FEAT_SAMEFRAME=1 (bit 2; a TIMING experiment, wrong output): every frame gathers frame 2 of buffer 0 -- cache hits
      // instead of the HBM's latency: the upper bound of what requesting the samples a frame ahead could buy
      gather_points<R1, N>(a, (a.prefetch & 4) ? 0 : b, (a.prefetch & 4) ? 2 : t, lane, (SMALL || (a.prefetch & 1)) ? reinterpret_cast<const d2*>(a.window) : wl, pts, a.n);
#else
      gather_points<R1, N>(a, b, t, lane, SMALL ? reinterpret_cast<const d2*>(a.window) : wl, pts, a.n);
#endif
      SCHED_FENCE();
      core.template run<false, TAB, FASTMAG>(pts, nullptr);
    }
    SCHED_FENCE();
    // ---- band sums ------------------------------------------------------------------------------------------
    int ln = lane;
    asm volatile("" : "+v"(ln));                    // (opaque: per-bin LDS positions are recomputed, not kept)
    double pu[CH], pd[CH];
    double su = 0.0, sd = 0.0, en = 0.0;
    // (the two options are launch-wide: a scalar branch around two copies of the loop -- if-converted they were two selects per
    //  bin, 36 v_cndmask + 18 multiplications per frame that the MFCC / mel-band defaults never use)
    auto band_sums = [&](auto plainTag) {
      constexpr bool PLAIN = decltype(plainTag)::value;
#pragma unroll
      for (int i = 0; i < CH; i++)
      {
        const int f = CH * ln + i;
        // (bins past N have zero weights: the clamped read costs a v_min where the select cost a compare and two v_cndmask)
        double m = xb[min(f, N)];
        if constexpr (!PLAIN)
        {
          if (fa.magNorm) { m = f <= N ? m * scale1 : 0.0; en += m; }     // :86-90
          if (fa.usePower) m = m * m;
        }
        su = __builtin_fma(lds_read1(upl + i * 64 + ln), m, su);    // (single ds_read_b64s: paired they run at half the rate)
        sd = __builtin_fma(lds_read1(dnl + i * 64 + ln), m, sd);
        pu[i] = su;
        pd[i] = sd;
      }
    };
    if (fa.magNorm | fa.usePower) band_sums(std::false_type{});
    else band_sums(std::true_type{});
    // inclusive scan of the lane totals over the wavefront (DPP: four shifts inside a row of 16, then the row totals
    // broadcast upwards), then shifted by one lane: what the lanes below contribute
    const double xu = wave_scan(su), xd = wave_scan(sd);
    const double eu = wave_shr1(xu), ed = wave_shr1(xd);
    if constexpr (SMALL)
    {
      // the boundary sums live in the staging buffer (the magnitudes have been read: LDS operations of a wavefront complete
      // in order): boundaries nobody publishes read 0
      bu[lane] = 0.0; bd[lane] = 0.0;
      if (lane < 2) { bu[64 + lane] = 0.0; bd[64 + lane] = 0.0; }
    }
#pragma unroll
    for (int i = 0; i < CH; i++)
    {
      int sl;
      if constexpr (HOIST) sl = slotReg[i];
      else sl = slotl[i * 64 + ln];
      bu[sl] = eu + pu[i];
      bd[sl] = ed + pd[i];
    }
    double v = 0.0;
    if (ln < fa.nBands) v = (bu[ln + 1] - bu[ln]) + (bd[ln + 2] - bd[ln + 1]);   // (predicates from the opaque lane: recomputed per frame, not kept as spilled exec masks)
    if (fa.magNorm)
    {
      // :93  bands * energy / max(eps, sum of the bands), energy = sum_f (m scale1) * scale2 (:86-87)
      double bs = v;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { bs += __shfl_xor(bs, off); en += __shfl_xor(en, off); }
      v = v * (en * scale2) / fmax(kEpsilon, bs);
    }
    // :95  20 log10(max(eps, band)), in single precision (band_db)
    if (fa.logOutput) v = (double) band_db(v);
    if (!fa.dct)
    {
      if (ln < fa.nBands) fa.out[((int64_t) b * fa.nOut + ln) * a.T + t] = (float) v;
      continue;
    }
    bands[ln] = ln < fa.nBands ? v : 0.0;                // (the DCT rows are zero there too: the quarters need no bounds)
    // ---- DCT-II rows startCoeff .. startCoeff + nOut - 1 (alg/DCT.hpp:73-75) -----------------------------------------
    if (4 * fa.nOut <= 64)
    {
      // four lanes per coefficient, a quarter of the bands each (ascending), then two exchange-adds.  Every lane walks dq
      // products -- a wave-uniform trip count, positions past nBands multiply zeros, lanes without a coefficient walk row 0
      // and store nothing -- instead of a loop whose bounds depend on the lane (exec-mask bookkeeping per product).
      const int j = ln >> 2, part = ln & 3;
      const bool live = j < fa.nOut && fa.startCoeff + j < fa.nDct;
      const double* drow = dctl + (live ? fa.startCoeff + j : 0) * dld + part * dq;
      const double* bq = bands + part * dq;
      double sacc = 0.0;
      if (dct10)
      {
        // 37 .. 40 bands (the MFCC default): the lane's quarter row of the table from registers, the bands at immediate offsets
#pragma unroll
        for (int i = 0; i < 10; i++) sacc = __builtin_fma(drowReg[i], lds_read1(bq + i), sacc);
      }
      else if (dq == 10)
      {
        // (the same unrolled: as a loop with a trip count from a register the compiler kept an address add per read -- 18
        //  v_add_u32 per eight products)
#pragma unroll
        for (int i = 0; i < 10; i++) sacc = __builtin_fma(lds_read1(drow + i), lds_read1(bq + i), sacc);
      }
      else
      {
#pragma unroll
        for (int i = 0; i < 16; i++)                            // (nBands <= 64: dq <= 16)
        {
          if (i >= dq) break;
          sacc = __builtin_fma(lds_read1(drow + i), lds_read1(bq + i), sacc);
        }
      }
      sacc += __shfl_xor(sacc, 1);
      sacc += __shfl_xor(sacc, 2);
      if (part == 0 && j < fa.nOut) fa.out[((int64_t) b * fa.nOut + j) * a.T + t] = (float) (live ? sacc : 0.0);
    }
    else
    {
      for (int j = lane; j < fa.nOut; j += 64)
      {
        double sacc = 0.0;
        if (fa.startCoeff + j < fa.nDct)
        {
          const double* drow = dctl + (fa.startCoeff + j) * dld;
          for (int band = 0; band < fa.nBands; band++) sacc = __builtin_fma(drow[band], bands[band], sacc);
        }
        fa.out[((int64_t) b * fa.nOut + j) * a.T + t] = (float) sacc;
      }
    }
  }
#ifdef FLUHIP_AB_SWITCHES
  if (fa.dbg && threadIdx.x == 0)
  {
    if (blockIdx.x == 0) fa.dbg[2] = (long long) __builtin_readcyclecounter();
    fa.dbg[5 + 2 * blockIdx.x] = (long long) wall_clock64();
  }
#endif
}

#ifdef FLUHIP_AB_SWITCHES
// The same kernel with FPW frames per wavefront in ONE instruction stream (FftCore::passesN): a block is NW * FPW
// consecutive frames, wavefront w takes frames w FPW .. w FPW + FPW - 1 of it.  Half the wavefronts per SIMD (twice the
// registers per wavefront), the same number of frames in flight -- but the frames of a wavefront are scheduled against each
// other by the compiler instead of against the luck of the round-robin.
template <int R1, int R2, int R3, int NW, int FPW>
__global__ __launch_bounds__(64 * NW) void stft_feat2_kernel(StftBArgs a, FeatFusedArgs fa)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, PPL = Core::PPL, BUFD = Core::BUFD;
  constexpr int CH = (N + 1 + 63) / 64;
  constexpr int WS = 66 + 66 + 64;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  d2* tw2 = reinterpret_cast<d2*>(lds);
  d2* wl = tw2 + Core::TW;
  double* xall = reinterpret_cast<double*>(wl + N);
  double* scr = xall + NW * FPW * BUFD;           // [NW][FPW][WS]
  double* upl = scr + NW * FPW * WS;
  double* dnl = upl + 64 * CH;
  double* dctl = dnl + 64 * CH;
  const int dld = fa.nBands + 1;
  short* slotl = reinterpret_cast<short*>(dctl + (fa.dct ? fa.nDct * dld : 0));
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* xb = xall + wave * FPW * BUFD;
  double* bu0 = scr + wave * FPW * WS;

  const d2* twg = reinterpret_cast<const d2*>(a.twiddle);
  Core::fill_tables(tw2, twg, threadIdx.x, 64 * NW);
  for (int m = threadIdx.x; m < N; m += 64 * NW) wl[m] = reinterpret_cast<const d2*>(a.window)[m];
  for (int i = threadIdx.x; i < 64 * CH; i += 64 * NW) { const int q = (i % CH) * 64 + i / CH; upl[q] = fa.up[i]; dnl[q] = fa.dn[i]; slotl[q] = fa.slot[i]; }
  if (fa.dct)
    for (int i = threadIdx.x; i < fa.nDct * fa.nBands; i += 64 * NW) dctl[(i / fa.nBands) * dld + (i % fa.nBands)] = fa.dct[i];
  for (int i = lane; i < FPW * WS; i += 64) bu0[i] = 0.0;
  __syncthreads();

  Core core;
  core.init(xb, tw2, twg, lane);
  const double scale1 = 1.0 / ((double) a.win / 4.0);
  const double scale2 = 1.0 / (2.0 * (double) (2 * N) / (double) a.win);

  const int64_t chunk = (a.totalBlocks + 7) / 8;
  for (int64_t L = blockIdx.x;; L += gridDim.x)
  {
    const int64_t slot8 = L >> 3;
    if (slot8 >= chunk) break;
    const int64_t blk = (L & 7) * chunk + slot8;
    if (blk >= a.totalBlocks) continue;
    const int b = (int) (blk / a.blocksPerBuf);
    const int t0 = ((int) (blk % a.blocksPerBuf) * NW + wave) * FPW;
    if (t0 >= a.T) continue;
    {
      cx pts[FPW][PPL], p3[FPW][PPL];
#pragma unroll
      for (int f = 0; f < FPW; f++) gather_points<R1, N>(a, b, min(t0 + f, a.T - 1), lane, wl, pts[f], a.n); // (a frame past the last repeats it; not stored)
      SCHED_FENCE();
      core.template passesN<FPW>(pts, p3);
      core.template splitN<FPW>(p3);
    }
    SCHED_FENCE();
    // ---- band sums of the FPW frames, stage by stage ----------------------------------------------------------------
    int ln = lane;
    asm volatile("" : "+v"(ln));
    double v[FPW];
    {
      double pu[FPW][CH], pd[FPW][CH];
      double su[FPW], sd[FPW], en[FPW];
#pragma unroll
      for (int f = 0; f < FPW; f++) su[f] = sd[f] = en[f] = 0.0;
#pragma unroll
      for (int i = 0; i < CH; i++)
      {
        const int fb = CH * ln + i;
        const double wu = upl[i * 64 + ln], wd = dnl[i * 64 + ln];
#pragma unroll
        for (int f = 0; f < FPW; f++)
        {
          double m = fb <= N ? xb[f * BUFD + fb] : 0.0;
          if (fa.magNorm) { m *= scale1; en[f] += m; }
          if (fa.usePower) m = m * m;
          su[f] = __builtin_fma(wu, m, su[f]);
          sd[f] = __builtin_fma(wd, m, sd[f]);
          pu[f][i] = su[f];
          pd[f][i] = sd[f];
        }
      }
      double eu[FPW], ed[FPW];
#pragma unroll
      for (int f = 0; f < FPW; f++)
      {
        const double xu = wave_scan(su[f]), xd = wave_scan(sd[f]);
        eu[f] = wave_shr1(xu);
        ed[f] = wave_shr1(xd);
      }
#pragma unroll
      for (int i = 0; i < CH; i++)
      {
        const int sl = slotl[i * 64 + ln];
        if (sl >= 0)
        {
#pragma unroll
          for (int f = 0; f < FPW; f++) { bu0[f * WS + sl] = eu[f] + pu[f][i]; bu0[f * WS + 66 + sl] = ed[f] + pd[f][i]; }
        }
      }
#pragma unroll
      for (int f = 0; f < FPW; f++)
      {
        const double* bu = bu0 + f * WS;
        const double* bd = bu + 66;
        double vv = 0.0;
        if (lane < fa.nBands) vv = (bu[lane + 1] - bu[lane]) + (bd[lane + 2] - bd[lane + 1]);
        if (fa.magNorm)
        {
          double bs = vv, e = en[f];
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) { bs += __shfl_xor(bs, off); e += __shfl_xor(e, off); }
          vv = vv * (e * scale2) / fmax(kEpsilon, bs);
        }
        if (fa.logOutput) vv = (double) band_db(vv);
        v[f] = vv;
      }
    }
    if (!fa.dct)
    {
#pragma unroll
      for (int f = 0; f < FPW; f++)
        if (lane < fa.nBands && t0 + f < a.T) fa.out[((int64_t) b * fa.nOut + lane) * a.T + t0 + f] = (float) v[f];
      continue;
    }
#pragma unroll
    for (int f = 0; f < FPW; f++) bu0[f * WS + 132 + lane] = v[f];
    if (4 * fa.nOut <= 64)
    {
      const int j = lane >> 2, part = lane & 3;
      const int q = (fa.nBands + 3) >> 2;
      double sacc[FPW];
#pragma unroll
      for (int f = 0; f < FPW; f++) sacc[f] = 0.0;
      if (j < fa.nOut && fa.startCoeff + j < fa.nDct)
      {
        const double* drow = dctl + (fa.startCoeff + j) * dld;
        const int b1 = min((part + 1) * q, fa.nBands);
        for (int band = part * q; band < b1; band++)
        {
          const double dv = drow[band];
#pragma unroll
          for (int f = 0; f < FPW; f++) sacc[f] = __builtin_fma(dv, bu0[f * WS + 132 + band], sacc[f]);
        }
      }
#pragma unroll
      for (int f = 0; f < FPW; f++)
      {
        sacc[f] += __shfl_xor(sacc[f], 1);
        sacc[f] += __shfl_xor(sacc[f], 2);
        if (part == 0 && j < fa.nOut && t0 + f < a.T) fa.out[((int64_t) b * fa.nOut + j) * a.T + t0 + f] = (float) sacc[f];
      }
    }
    else
    {
      for (int j = lane; j < fa.nOut; j += 64)
#pragma unroll
        for (int f = 0; f < FPW; f++)
        {
          double sacc = 0.0;
          if (fa.startCoeff + j < fa.nDct)
          {
            const double* drow = dctl + (fa.startCoeff + j) * dld;
            for (int band = 0; band < fa.nBands; band++) sacc = __builtin_fma(drow[band], bu0[f * WS + 132 + band], sacc);
          }
          if (t0 + f < a.T) fa.out[((int64_t) b * fa.nOut + j) * a.T + t0 + f] = (float) sacc;
        }
    }
  }
}

template <int R1, int R2, int R3, int NW, int FPW>
static bool launch_feat2_t(const StftBArgs& k0, const FeatFusedArgs& fa, hipStream_t s)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, CH = (N + 1 + 63) / 64, WS = 66 + 66 + 64;
  const size_t shmem = ((size_t) Core::TW + N) * 16 + ((size_t) NW * FPW * (Core::BUFD + WS) + 2 * 64 * CH) * 8 +
                       (fa.dct ? (size_t) fa.nDct * (fa.nBands + 1) * 8 : 0) + (size_t) 64 * CH * 2 + 16;
  if (shmem > 160 * 1024) return false;
  StftBArgs k = k0;
  k.blocksPerBuf = (k.T + NW * FPW - 1) / (NW * FPW);
  k.totalBlocks = (int64_t) k.B * k.blocksPerBuf;
  if (k.totalBlocks < 1) return true;
  auto kern = stft_feat2_kernel<R1, R2, R3, NW, FPW>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int) shmem) != hipSuccess)
    return false;
  const int64_t chunk = (k.totalBlocks + 7) / 8;
  int64_t grid = 8 * chunk;
  if (grid > 256) grid = 256;
  hipLaunchKernelGGL(kern, dim3((unsigned) grid), dim3(64 * NW), shmem, s, k, fa);
  return true;
}

#endif // FLUHIP_AB_SWITCHES

// dynamic LDS of stft_feat_kernel<R1, R2, R3, NW, *, SMALL> with nDct DCT rows over nBands bands (nDct 0: mel bands only)
template <int R1, int R2, int R3, int NW, bool SMALL = false>
static size_t feat_shmem(int nBands, int nDct)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, CH = (N + 1 + 63) / 64, WS = SMALL ? 0 : 2 * (66 + 64) + 64;
  return ((size_t) Core::TW + (SMALL ? 0 : N) + (R1 == 8 ? N : 0)) * 16 + ((size_t) NW * (Core::BUFD + WS) + 2 * 64 * CH) * 8 +
         (size_t) nDct * (4 * ((nBands + 3) / 4) + 1) * 8 + (size_t) 64 * CH * 2 + 16;
}

template <int R1, int R2, int R3, int NW, bool SMALL = false>
static bool launch_feat_t(const StftBArgs& k0, const FeatFusedArgs& fa, hipStream_t s)
{
  const size_t shmem = feat_shmem<R1, R2, R3, NW, SMALL>(fa.nBands, fa.dct ? fa.nDct : 0);
  if (shmem > (SMALL ? 80 : 160) * 1024) return false;
  StftBArgs k = k0;
  k.blocksPerBuf = (k.T + NW - 1) / NW;
  k.totalBlocks = (int64_t) k.B * k.blocksPerBuf;
  if (k.totalBlocks < 1) return true;
  if (k.totalBlocks >= ((int64_t) 1 << 31)) return false; // (the kernel's block arithmetic is 32-bit; the two-kernel path takes it)
  auto kern = stft_feat_kernel<R1, R2, R3, NW, true, SMALL>;
#ifdef FLUHIP_AB_SWITCHES // FLUHIP_FEAT_DYN=0: a fixed share of the frames per wavefront (rounds 2 - 3)
  static const int dynOff = [] { const char* e = fluhip::ab_getenv("FLUHIP_FEAT_DYN"); return e && std::atoi(e) == 0 ? 1 : 0; }();
  if (dynOff && !SMALL) kern = stft_feat_kernel<R1, R2, R3, NW, false>;
  static const int slowMag = [] { const char* e = fluhip::ab_getenv("FLUHIP_FEAT_FASTMAG"); return e && std::atoi(e) == 0 ? 1 : 0; }();
  if (slowMag && !dynOff && !SMALL) kern = stft_feat_kernel<R1, R2, R3, NW, true, false, false>;
#endif
  request_dynamic_lds(kern, (size_t) (shmem));
  const int64_t chunk = (k.totalBlocks + 7) / 8;
  int64_t grid = 8 * chunk;
  if (grid > (SMALL ? 512 : 256)) grid = SMALL ? 512 : 256;
  if constexpr (kAbSwitches)
  {
    static const int clk = [] { const char* e = fluhip::ab_getenv("FLUHIP_FEAT_CLOCK"); return e ? std::atoi(e) : 0; }();
    if (clk)
    {
      FeatFusedArgs f2 = fa;
      long long* d = nullptr;
      if (hipMalloc(&d, (4 + 2 * 256) * 8) == hipSuccess)
      {
        f2.dbg = d;
        hipLaunchKernelGGL(kern, dim3((unsigned) grid), dim3(64 * NW), shmem, s, k, f2);
        std::vector<long long> h(4 + 2 * 256, 0);
        (void) hipStreamSynchronize(s);
        (void) hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost);
        (void) hipFree(d);
        long long t0 = h[4], t1 = h[5];
        for (int g = 0; g < (int) grid; g++) { t0 = std::min(t0, h[4 + 2 * g]); t1 = std::max(t1, h[5 + 2 * g]); }
        const double us = (h[5] - h[4]) / 100.0;
        std::fprintf(stderr, "stft_feat_kernel: workgroup 0 alive %.1f us, %lld shader cycles -> %.0f MHz; all %d workgroups: %.1f us first start to last end\n",
                     us, h[2] - h[0], (h[2] - h[0]) / us, (int) grid, (t1 - t0) / 100.0);
        std::fprintf(stderr, "  start offsets / lifetimes (us) of workgroups 0, 1, 8, 9, 64, 128, 255:");
        for (int g : {0, 1, 8, 9, 64, 128, 255})
          if (g < (int) grid) std::fprintf(stderr, "  %.0f/%.0f", (h[4 + 2 * g] - t0) / 100.0, (h[5 + 2 * g] - h[4 + 2 * g]) / 100.0);
        int late = 0;
        for (int g = 0; g < (int) grid; g++) late += (h[4 + 2 * g] - t0) > 10000 ? 1 : 0;   // started more than 100 us after the first
        std::fprintf(stderr, "\n  workgroups that started more than 100 us after the first: %d\n", late);
        return true;
      }
    }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned) grid), dim3(64 * NW), shmem, s, k, fa);
  return true;
}

// STFT -> mel bands [-> DCT] in one kernel; false when the shape has no fused form
bool launch_stft_features(const StftArgs& a, const FeatArgs& f, const double* up, const double* dn, const short* slot,
                          hipStream_t s)
{
  if (!fft_core_supported(a.win, a.fft) || f.nBands > 64 || f.nBands < 1) return false;
  StftBArgs k = block_args(a);
  if constexpr (kAbSwitches) // FLUHIP_FEAT_WINDOW_GLOBAL=1: the window pairs through the L1 instead of the LDS (A/B; `prefetch` is unused by this kernel)
  {
    static const int wg = [] { const char* e = fluhip::ab_getenv("FLUHIP_FEAT_WINDOW_GLOBAL"); return e ? std::atoi(e) : 0; }();
    static const int pr = [] { const char* e = fluhip::ab_getenv("FLUHIP_FEAT_PRIO"); return e ? std::atoi(e) : 0; }();
    static const int sf = [] { const char* e = fluhip::ab_getenv("FLUHIP_FEAT_SAMEFRAME"); return e ? std::atoi(e) : 0; }();
    k.prefetch = (wg ? 1 : 0) | (pr ? 2 : 0) | (sf ? 4 : 0);
  }
  FeatFusedArgs fa;
  fa.up = up; fa.dn = dn; fa.slot = slot; fa.dct = f.dct;
  fa.nBands = f.nBands; fa.nDct = f.nDct; fa.startCoeff = f.startCoeff; fa.nOut = f.nOut;
  fa.magNorm = f.magNorm; fa.usePower = f.usePower; fa.logOutput = f.logOutput; fa.out = f.out;
  if (a.fft == 1024)
  {
#ifdef FLUHIP_AB_SWITCHES // (forms measured no faster than the production one, profiles/r04/c5_experiments.md: compiled into the A/B build only)
    // FLUHIP_FEAT_FPW=2: two frames per wavefront in one instruction stream, eight wavefronts per workgroup
    {
      static const int fpw = [] { const char* e = fluhip::ab_getenv("FLUHIP_FEAT_FPW"); return e ? std::atoi(e) : 1; }();
      if (fpw == 2) return launch_feat2_t<8, 8, 8, 8, 2>(k, fa, s);
      if (fpw == 22) return launch_feat2_t<8, 8, 8, 12, 2>(k, fa, s);
      if (fpw == 3) return launch_feat2_t<8, 8, 8, 4, 3>(k, fa, s);
    }
    // FLUHIP_FEAT_NW=8|12: wavefronts per workgroup of the fused feature kernel (production 16)
    {
      static const int nw = [] { const char* e = fluhip::ab_getenv("FLUHIP_FEAT_NW"); return e ? std::atoi(e) : 16; }();
      if (nw == 8) return launch_feat_t<8, 8, 8, 8>(k, fa, s);
      if (nw == 12) return launch_feat_t<8, 8, 8, 12>(k, fa, s);
      if (nw == 10) return launch_feat_t<8, 8, 8, 10, true>(k, fa, s);   // two workgroups per CU
      if (nw == 9) return launch_feat_t<8, 8, 8, 9, true>(k, fa, s);
    }
#endif
    return launch_feat_t<8, 8, 8, 16>(k, fa, s);
  }
  if (a.fft == 2048) return launch_feat_t<16, 8, 8, 8>(k, fa, s);
  return false;
}
int stft_features_bins_per_lane(int fft) { return (fft / 2 + 1 + 63) / 64; }
bool stft_features_fits(int fft, int nBands, int nDct)
{
  // the production forms launch_stft_features picks
  if (fft == 1024) return feat_shmem<8, 8, 8, 16>(nBands, nDct) <= 160 * 1024;
  if (fft == 2048) return feat_shmem<16, 8, 8, 8>(nBands, nDct) <= 160 * 1024;
  return false;
}

} // namespace fluhip
