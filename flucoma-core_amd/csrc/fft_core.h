// fft_core.h -- the on-chip FFT core (FftCore<R1, R2, R3>: one wavefront transforms one frame of fft = 2 R1 R2 R3 samples in
// registers and a private LDS exchange buffer), the argument block of the kernels built on it and the gather / window helpers
// that feed it.  Device header of kernels_{stft_block, stft_feat, resynth_batch, onset_fused, pitch_fused}.hip.
// Same mathematics and DFT convention as kernels_stft.hip (see there for the reference lines):
//   algorithm::STFT::process / magnitude   include/flucoma/algorithms/public/STFT.hpp:90-108, 61-66
//   algorithm::FFT::process                include/flucoma/algorithms/util/FFT.hpp:92-108
// What changed against stft_wave_kernel (kernels_stft.hip), and what was measured (profiles/r02/stft_notes.md):
//   * the points cross the LDS as separate real and imaginary planes through ONE 8-byte-per-point buffer (the
//     wavefront's LDS instructions execute in order, so the imaginary plane may overwrite the real one as soon as
//     the reads of the real plane have issued): half the LDS per wavefront, and the same buffer then stages the
//     frame's magnitudes for the bin-major copy;
//   * the last pass is laid out so that the two bins of every real-FFT pair (k, N - k) end up in the SAME lane
//     (lane l owns butterflies l and Ns - l; lane 0 owns the two self-paired ones): the split needs no third
//     exchange (transforms with one last-pass butterfly per lane fetch the partner with ds_bpermute);
//   * the split's twiddle e^{-2 pi i k / fft}, k = j + Ns r, is (a per-lane constant) x (a compile-time constant),
//     so nothing is loaded for it inside the frame loop;
//   * everything the compiler would hoist out of the frame loop and keep in registers (per-point address offsets,
//     twiddle products) is either expressed as per-lane base + compile-time offset or kept opaque: 190 registers at
//     fft 2048 (two wavefronts per SIMD), 112 at fft 1024 (four).
#pragma once

#include "fluhip_kernels.h"
#include "frame_window.h"

namespace fluhip {

typedef double d2 __attribute__((ext_vector_type(2)));

// register arithmetic runs on (re, im) scalar pairs, not on 128-bit vectors: the two planes cross the LDS separately,
// and a vector register tuple cannot be half dead
struct cx
{
  double re, im;
};
__device__ __forceinline__ cx operator+(cx a, cx b) { return cx{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cx operator-(cx a, cx b) { return cx{a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cx tocx(d2 v) { return cx{v[0], v[1]}; }

struct StftBArgs
{
  const float* audio;
  const double* audio64;
  int64_t n, audioStride;
  int win, fft, hop, T, F, B;
  const double* window;   // [max(win, fft)] zero past win
  const double* twiddle;  // [fft/2] e^{-2 pi i m / fft}
  double* mag;            // [B][*][ldMag] or nullptr
  int64_t magStride, ldMag;
  double* magT;           // [B][*][ldMagT] or nullptr
  int64_t magTStride, ldMagT;
  double* spec;
  int64_t specStride;
  int frameOffset;
  int blocksPerBuf;
  int64_t totalBlocks;
  const int64_t* nTab;    // ragged corpora: samples of every buffer (n is then the longest), or nullptr
  int prefetch;           // block kernel: request the next frame's samples ahead of this frame's stores
};

#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// The magnitudes leave once and are not read again before the whole corpus's transform is done (the factor updates stream them
// back much later, 1.9 GB on the bench shard): the two layouts' stores are NON-TEMPORAL (round 6) -- bench shard's STFT phase
// 0.560 - 0.586 -> 0.487 - 0.499 ms per launch with both layouts, 0.475 - 0.484 -> 0.444 - 0.451 with the frame-major one alone,
// alternating on one box (profiles/r06/stft_nt.txt).  -DFLUHIP_STFT_NT=0: plain stores.
#ifndef FLUHIP_STFT_NT
#define FLUHIP_STFT_NT 1
#endif
__device__ __forceinline__ void store_mag16(double* p, double __attribute__((ext_vector_type(2))) v)
{
#if FLUHIP_STFT_NT
  __builtin_nontemporal_store(v, reinterpret_cast<double __attribute__((ext_vector_type(2)))*>(p));
#else
  *reinterpret_cast<double __attribute__((ext_vector_type(2)))*>(p) = v;
#endif
}
// -DFLUHIP_SPLIT_VIA_LDS=0: the ds_bpermute partner exchange of rounds 1 - 4 (FftCore::split)
#ifndef FLUHIP_SPLIT_VIA_LDS
#define FLUHIP_SPLIT_VIA_LDS 1
#endif
// workgroup barrier that orders LDS traffic only: __syncthreads() also drains the wavefront's global stores
// (s_waitcnt vmcnt(0)), which here would serialise every frame's stores with the next frame's arithmetic
#define LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

__device__ __forceinline__ cx cmul2(cx a, cx b) { return cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cx mul_mi2(cx a) { return cx{a.im, -a.re}; } // a * (-i)

// sqrt(x), x >= DBL_MIN: v_rsq_f64 seed y = (1 + e) / sqrt(x), |e| ~ 2^-23; one coupled Goldschmidt step leaves g = sqrt(x) (1 - 1.5 e^2)
// (~2e-14) and h = 1 / (2 g) to the same order; the exact residual d = x - g^2 times h then squares that again: rounding
// error only, in 8 FP64 operations behind the seed (the wave kernel of round 1 ran a second Goldschmidt step first: 12).
// FAST (the fused feature kernel, whose bands leave as float32 behind a single-precision logarithm): the Goldschmidt step
// alone, 2e-14 relative -- nine orders below the float output's resolution -- in 5 operations.
// The callers keep x >= DBL_MIN by starting the sum of squares from DBL_MIN (mag_sumsq: adding it is exact-no-op for any
// power above 1e-290 and costs nothing, where fmax(x, DBL_MIN) was an instruction per bin).
constexpr double kDblMin = 2.2250738585072014e-308;
__device__ __forceinline__ double mag_sumsq(double re, double im) { return __builtin_fma(re, re, __builtin_fma(im, im, kDblMin)); }
template <bool FAST = false>
__device__ __forceinline__ double mag_sqrt2(double x)
{
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  if constexpr (FAST) return g;
  h = __builtin_fma(h, r, h);
  const double d = __builtin_fma(-g, g, x);
  return __builtin_fma(d, h, g);
}

__device__ __forceinline__ void bf4(cx& a0, cx& a1, cx& a2, cx& a3)
{
  const cx t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = mul_mi2(a1 - a3);
  a0 = t0 + t2; a1 = t1 + t3; a2 = t0 - t2; a3 = t1 - t3;
}

constexpr double kC1 = 0.92387953251128673848; // cos(pi/8)
constexpr double kS1 = 0.38268343236508977173; // sin(pi/8)
constexpr double kC2 = 0.70710678118654752440; // sqrt(2)/2

template <int R>
__device__ __forceinline__ void bfr(cx (&v)[R]);

template <>
__device__ __forceinline__ void bfr<8>(cx (&v)[8])
{
  cx e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
  cx o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
  bf4(e0, e1, e2, e3);
  bf4(o0, o1, o2, o3);
  o1 = cx{kC2 * (o1.re + o1.im), kC2 * (o1.im - o1.re)};
  o2 = mul_mi2(o2);
  o3 = cx{kC2 * (o3.im - o3.re), -kC2 * (o3.re + o3.im)};
  v[0] = e0 + o0; v[4] = e0 - o0;
  v[1] = e1 + o1; v[5] = e1 - o1;
  v[2] = e2 + o2; v[6] = e2 - o2;
  v[3] = e3 + o3; v[7] = e3 - o3;
}

template <>
__device__ __forceinline__ void bfr<16>(cx (&v)[16])
{
  cx s[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
  {
    s[a][0] = v[a]; s[a][1] = v[a + 4]; s[a][2] = v[a + 8]; s[a][3] = v[a + 12];
    bf4(s[a][0], s[a][1], s[a][2], s[a][3]);
  }
  s[1][1] = cmul2(s[1][1], cx{kC1, -kS1});
  s[1][2] = cx{kC2 * (s[1][2].re + s[1][2].im), kC2 * (s[1][2].im - s[1][2].re)};
  s[1][3] = cmul2(s[1][3], cx{kS1, -kC1});
  s[2][1] = cx{kC2 * (s[2][1].re + s[2][1].im), kC2 * (s[2][1].im - s[2][1].re)};
  s[2][2] = mul_mi2(s[2][2]);
  s[2][3] = cx{kC2 * (s[2][3].im - s[2][3].re), -kC2 * (s[2][3].re + s[2][3].im)};
  s[3][1] = cmul2(s[3][1], cx{kS1, -kC1});
  s[3][2] = cx{kC2 * (s[3][2].im - s[3][2].re), -kC2 * (s[3][2].re + s[3][2].im)};
  s[3][3] = cmul2(s[3][3], cx{-kC1, kS1});
#pragma unroll
  for (int b = 0; b < 4; b++)
  {
    bf4(s[0][b], s[1][b], s[2][b], s[3][b]);
    v[b] = s[0][b]; v[b + 4] = s[1][b]; v[b + 8] = s[2][b]; v[b + 12] = s[3][b];
  }
}

// cos / sin of 2 pi r / (2 R) for the split's constant factor e^{-2 pi i r / (2 R)}
template <int R>
__device__ __forceinline__ cx split_const(int r)
{
  // e^{-2 pi i r / (2 R)}: R = 16: thirty-second roots of unity; R = 8: every second one; R = 4: every fourth
  constexpr double c32[16] = {1, 0.98078528040323043058, 0.92387953251128673848, 0.83146961230254523567, 0.70710678118654757274, 0.55557023301960228867, 0.38268343236508983729, 0.19509032201612833135, 0, -0.19509032201612819257, -0.38268343236508972627, -0.5555702330196019556, -0.70710678118654746172, -0.83146961230254534669, -0.92387953251128673848, -0.98078528040323043058};
  constexpr double s32[16] = {0, 0.19509032201612824808, 0.38268343236508978178, 0.55557023301960217765, 0.70710678118654746172, 0.83146961230254523567, 0.92387953251128673848, 0.98078528040323043058, 1, 0.98078528040323043058, 0.92387953251128673848, 0.83146961230254545772, 0.70710678118654757274, 0.55557023301960217765, 0.3826834323650898928, 0.19509032201612860891};
  static_assert(R == 16 || R == 8 || R == 4, "last-pass radix");
  const int q = r * (16 / R);
  return cx{c32[q], -s32[q]};
}

// ---- register <-> lane transposes without the LDS (round 6, gfx950) --------------------------------------------------
// One step swaps a bit of the register index with a bit of the lane index: for the register pair (A, B) that differs in the
// register bit, A keeps its lanes with the lane bit clear and takes B's partner lanes, B the reverse.  Lane bits 5 and 4 are
// ONE instruction per pair and dword (v_permlane32_swap / v_permlane16_swap: the upper half of A against the lower half of B;
// the odd rows of A against the even rows of B), lane bit 3 two DPP moves with a bank mask (row_ror:8 = lane ^ 8 inside a
// row of 16) and the copy that keeps A alive.
#ifndef FLUHIP_FFT_PERMLANE
#define FLUHIP_FFT_PERMLANE 0
#endif
template <int LANEBIT>
__device__ __forceinline__ void xpose_dword(int& a, int& b)
{
  static_assert(LANEBIT == 5 || LANEBIT == 4 || LANEBIT == 3, "lane bit of the transpose step");
  if constexpr (LANEBIT == 5)
  {
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0]; b = r[1];
  }
  else if constexpr (LANEBIT == 4)
  {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0]; b = r[1];
  }
  else
  {
    const int na = __builtin_amdgcn_update_dpp(a, b, 0x128, 0xf, 0xc, false);   // lanes 8 .. 15 of a row <- b[lane - 8]
    const int nb = __builtin_amdgcn_update_dpp(b, a, 0x128, 0xf, 0x3, false);   // lanes 0 .. 7           <- a[lane + 8]
    a = na; b = nb;
  }
}
template <int LANEBIT>
__device__ __forceinline__ void xpose_f64(double& a, double& b)
{
  const long long la = __double_as_longlong(a), lb = __double_as_longlong(b);
  int a0 = (int) (la & 0xffffffff), a1 = (int) (la >> 32), b0 = (int) (lb & 0xffffffff), b1 = (int) (lb >> 32);
  xpose_dword<LANEBIT>(a0, b0);
  xpose_dword<LANEBIT>(a1, b1);
  a = __longlong_as_double(((long long) a1 << 32) | (unsigned) a0);
  b = __longlong_as_double(((long long) b1 << 32) | (unsigned) b0);
}
// eight values per lane: register bits (2, 1, 0) <-> lane bits (5, 4, 3)
[[maybe_unused]] __device__ __forceinline__ void xpose8_hi(double (&v)[8])
{
#pragma unroll
  for (int r = 0; r < 4; r++) xpose_f64<5>(v[r], v[r + 4]);
#pragma unroll
  for (int r = 0; r < 8; r++) if (!(r & 2)) xpose_f64<4>(v[r], v[r + 2]);
#pragma unroll
  for (int r = 0; r < 8; r += 2) xpose_f64<3>(v[r], v[r + 1]);
}

// One frame's transform from the windowed points to the staged magnitudes, shared by the kernel forms below: pass 1,
// exchange, pass 2, exchange, pass 3, real-FFT split, |X|.  `pts` holds the windowed points m = lane + 64 bb + r N/R1
// (x[2m], x[2m+1]); on return the wavefront's buffer xb holds |X[k]| at xb[k], k = 0 .. N (plain index), and the
// complex bins have been written to specRow when that is not null.
// One ds_read_b64 that stays one: the compiler pairs neighbouring loads off one base into ds_read2(st64)_b64, which the LDS
// serves as two passes of 16-lane groups at 128 B per clock where two ds_read_b64 run at 256 (MI355X_MICROARCH.md, LDS
// table) -- and whose lane groups are not the ones the swizzled layouts below are laid out for.
__device__ __forceinline__ double lds_read1(const double* p)
{
  // (volatile keeps the load single; the explicit LDS address space keeps it a ds_read: address-space inference leaves
  //  volatile accesses through generic pointers as flat loads)
  return *(const volatile __attribute__((address_space(3))) double*) p;
}

template <int R1, int R2, int R3>
struct FftCore
{
  static constexpr int N = R1 * R2 * R3, PPL = N / 64;
  static constexpr int NB1 = N / (64 * R1), NB2 = N / (64 * R2), NB3 = N / (64 * R3);
  static_assert(NB1 >= 1 && NB2 >= 1 && (NB3 == 1 || NB3 == 2), "tiling");
  static constexpr int NS2 = R1, NS3 = R1 * R2;
  static constexpr bool LOCAL = NB3 == 2;        // both bins of a split pair in one lane
  // XL (round 5, the one-butterfly-per-lane transform of fft 1024): the real-FFT split fetches its partner bins through the
  // staging buffer instead of with ds_bpermute -- a plane of N + 64 slots, see split()
  static constexpr bool XL = FLUHIP_SPLIT_VIA_LDS != 0 && NB3 == 1;
  static constexpr int BUFD = N + N / 16 + (XL ? 34 : 2);    // doubles per wavefront (the + 2 staggers the buffers over the banks)
  // (the XL split writes slot N from every lane -- slots up to N + 63 -- so the padding must cover 64 slots; today's one
  //  XL form, N = 512, leaves 2 to spare, a smaller one would overrun into the next wavefront's buffer without this)
  static_assert(!XL || BUFD >= N + 64, "XL split: the staging buffer must hold slots N .. N + 63");
  static constexpr int T2 = (R2 - 1) * NS2, T3 = (R3 - 1) * NS3, TW = T2 + T3;   // entries of the pass tables; TW: of both, one behind the other
  // SWZ (round 4, the 8 x 8 x 8 transform of fft 1024): the exchange buffer is addressed through bit swizzles instead of the
  // one-in-sixteen padding.  The padding serves the first exchange's stores (ds_write_b64: groups of 16 lanes over 32 dword
  // banks) and costs every read behind both exchanges a third cycle (ds_read_b64: groups of 32 lanes over 64 banks -- 32
  // consecutive points span 33 slots) and the second exchange's stores a 2-way conflict: 19 % of the feature kernel's LDS
  // cycles (profiles/r04/c5_experiments.md).  Point i of the first exchange sits at slot s with
  //   s0 = i0 ^ i5, s1 = i1 ^ i6, s2 = i3, s3 = i4, s4 = i2, s5.. = i5..      (stores vary i3..i6, loads vary i0..i4)
  // and point i of the second at i ^ (i6 << 3) (stores vary i0..i2 and i6, loads i0..i4): every lane group of either
  // instruction meets every bank once.  Per lane that is four store bases + two load bases for the first exchange and two +
  // two for the second, all loop invariant; the offsets stay compile-time immediates.
  static constexpr bool SWZ = R1 == 8 && R2 == 8 && R3 == 8;
  // PLX (round 6): the first exchange of the 8 x 8 x 8 transform does not touch the LDS.  Pass 1 leaves point
  // i = 64 a + 8 b + r in register r of lane (a, b) (a = lane >> 3, b = lane & 7); pass 2 wants register a to hold it.  Swapping
  // the register index with the UPPER lane bits (xpose8_hi: 32 permlane swaps + 48 DPP moves per frame against 16
  // ds_write_b64 + 16 ds_read_b64, 128 cycles of the CU's one LDS pipe) puts it into lane (r, b): that lane runs butterfly
  // j = 8 b + r = 8 (lane & 7) + (lane >> 3) of pass 2 -- twiddle row k = j mod 8 = lane >> 3 -- and its outputs go to
  // i' = 64 (lane & 7) + (lane >> 3) + 8 r of the second exchange, whose slots are i' + 2 (i' >> 6): both the stores (16
  // consecutive lanes: 2 b + k over 16 bank pairs) and the loads (lane + 66 r) meet every bank once, one base each.
  // The data movement is exact: the results are the LDS form's bit for bit.
  static constexpr bool PLX = SWZ && FLUHIP_FFT_PERMLANE != 0;
  static_assert(!PLX || BUFD >= 7 * 66 + 64, "PLX: slots of the second exchange");
  static_assert(R1 == 16 || R1 == 8, "pass-1 radix");
  static_assert(NS2 % 8 == 0 && NS3 % 16 == 0 && (N / R2) % 16 == 0, "index arithmetic of the exchanges");
  int lane, jA, jB;
  cx wA, wB;
  double* xb;
  // LDS positions as (per-lane base) + (compile-time offset): slot i of the exchange buffer sits at i + (i >> 4)
  double* w1p;
  const double* r2p;
  double* w2p;
  const double *r3pA, *r3pB;
  const d2 *tw2p, *tw3pA, *tw3pB;
  // SWZ: store bases of the first exchange by r & 3, load bases by r & 1; second exchange: both by r & 1
  double* w1q[4];
  const double* r2q[2];
  double* w2q[2];
  const double* r3q[2];

  // the pass tables [R2-1][NS2] and [R3-1][NS3] from the natural table e^{-2 pi i m / fft} (m < fft/2)
  static __device__ __forceinline__ void fill_tables(d2* tw2, const d2* twg, int tid, int nthreads)
  {
    for (int i = tid; i < TW; i += nthreads)
    {
      int m;
      if (i < T2) { const int r = i / NS2 + 1, k = i % NS2; m = k * r * (2 * N / (NS2 * R2)); }
      else { const int ii = i - T2; const int r = ii / NS3 + 1, k = ii % NS3; m = k * r * (2 * N / (NS3 * R3)); }
      d2 w = twg[m >= N ? m - N : m];
      if (m >= N) w = d2{-w[0], -w[1]};
      tw2[i] = w;
    }
  }

  __device__ __forceinline__ void init(double* xb_, const d2* tw2, const d2* twg, int lane_)
  {
    const d2* tw3 = tw2 + T2;
    lane = lane_;
    xb = xb_;
    // last-pass butterflies of this lane and the split's per-lane twiddle factors e^{-2 pi i j / fft}
    jA = lane;
    jB = LOCAL ? (lane == 0 ? NS3 / 2 : NS3 - lane) : 0;
    wA = tocx(twg[jA]);
    wB = LOCAL ? tocx(twg[jB]) : cx{0.0, 0.0};
    wA = cx{0.5 * wA.re, 0.5 * wA.im};   // the split's 1/2 rides on its twiddle
    wB = cx{0.5 * wB.re, 0.5 * wB.im};
    //   pass-1 outputs  (lane + 64 bb) R1 + r    pass-2 inputs   lane + 64 bb + r N/R2
    //   pass-2 outputs  (j - k) R2 + k + r NS2   pass-3 inputs   j + r NS3
    w1p = xb + (R1 == 16 ? 17 * lane : 8 * lane + (lane >> 1));
    r2p = xb + lane + (lane >> 4);
    const int k2 = PLX ? (lane >> 3) : (lane & (NS2 - 1));
    const int hi2 = lane - k2;                                  // multiple of NS2
    w2p = xb + hi2 * R2 + ((hi2 * R2) >> 4) + k2;
    r3pA = xb + jA + (jA >> 4);
    r3pB = xb + jB + (jB >> 4);
    tw2p = tw2 + k2;
    tw3pA = tw3 + jA;
    tw3pB = tw3 + jB;
    if constexpr (SWZ)
    {
      const int l = lane;
      const int l0 = l & 1, l1 = (l >> 1) & 1, l2 = (l >> 2) & 1, l3 = (l >> 3) & 1, l4 = (l >> 4) & 1, l5 = (l >> 5) & 1;
      // first exchange, stores: i = 8 l + r -> (q ^ c) + 16 (r >> 2) + L, q = r & 3, c = (l >> 2) & 3
      const int c = (l >> 2) & 3, L = 4 * l0 + 8 * l1 + 32 * l2 + 64 * l3 + 128 * l4 + 256 * l5;
      for (int q = 0; q < 4; q++) w1q[q] = xb + L + (q ^ c);
      // first exchange, loads: i = l + 64 r -> (l0 ^ l5) + 2 (l1 ^ r0) + 4 l3 + 8 l4 + 16 l2 + 32 l5 + 64 r
      const int A = (l0 ^ l5) + 4 * l3 + 8 * l4 + 16 * l2 + 32 * l5;
      r2q[0] = xb + A + 2 * l1;
      r2q[1] = xb + A + 2 * (l1 ^ 1);
      // second exchange, stores: i = 64 a + k + 8 r (a = l >> 3, k = l & 7) -> i ^ (l3 << 3): r0 flips where l3 is set
      const int E = 64 * (l >> 3) + (l & 7);
      w2q[0] = xb + E + 8 * l3;
      w2q[1] = xb + E + 8 * (l3 ^ 1) - 8;                 // (+ 8 r with r odd)
      // second exchange, loads: i = l + 64 r -> i ^ ((r & 1) << 3)
      r3q[0] = xb + l;
      r3q[1] = xb + (l ^ 8);
      if constexpr (PLX)
      {
        w2q[0] = xb + 66 * (l & 7) + (l >> 3);
        r3q[0] = xb + l;
      }
    }
  }

  // the same lane positions in another staging buffer `delta` doubles further on (a wavefront that transforms several
  // frames per round keeps one buffer per frame)
  __device__ __forceinline__ void shift(int delta)
  {
    xb += delta; w1p += delta; r2p += delta; w2p += delta; r3pA += delta; r3pB += delta;
    if constexpr (SWZ)
    {
      for (int q = 0; q < 4; q++) w1q[q] += delta;
      for (int q = 0; q < 2; q++) { r2q[q] += delta; w2q[q] += delta; r3q[q] += delta; }
    }
  }

  // TAB: the split's twiddles e^{-2 pi i k / fft} / 2 come from a table in the LDS (splitTab[k], k < N) instead of being
  // formed per frame as products of the lane's factor with compile-time constants (28 FP64 instructions at R3 = 8)
  const d2* splitTab = nullptr;
  template <bool SPEC, bool TAB = false, bool FASTMAG = false>
  __device__ __forceinline__ void run(cx (&pts)[PPL], d2* specRow)
  {
    cx p3[PPL];
    passes(pts, p3);
    split<SPEC, TAB, FASTMAG>(p3, specRow);
  }

  // the three passes of the complex transform: points m = lane + 64 bb + r N/R1 in, bins j + r NS3 out (j = lane, and for
  // the two-butterfly forms jB = NS3 - lane as well: registers bb R3 + r)
  __device__ __forceinline__ void passes(cx (&pts)[PPL], cx (&p3)[PPL])
  {
  SCHED_FENCE();
  // ---- pass 1 (Ns = 1): butterfly j = lane + 64 bb, outputs at j R1 + r ------------------------------
#pragma unroll
  for (int bb = 0; bb < NB1; bb++)
  {
    cx v[R1];
#pragma unroll
    for (int r = 0; r < R1; r++) v[r] = pts[bb * R1 + r];
    bfr<R1>(v);
#pragma unroll
    for (int r = 0; r < R1; r++) pts[bb * R1 + r] = v[r];
  }
  SCHED_FENCE();
  cx p2[PPL];
  // exchange 1 -> distribution of pass 2 (butterfly j = lane + 64 bb reads j + r N/R2): real plane, then imaginary
  if constexpr (PLX)
  {
    double re[8], im[8];
#pragma unroll
    for (int r = 0; r < 8; r++) { re[r] = pts[r].re; im[r] = pts[r].im; }
    xpose8_hi(re);
    xpose8_hi(im);
#pragma unroll
    for (int r = 0; r < 8; r++) p2[r] = cx{re[r], im[r]};
  }
  else if constexpr (SWZ)
  {
#pragma unroll
    for (int r = 0; r < R1; r++) w1q[r & 3][16 * (r >> 2)] = pts[r].re;
#pragma unroll
    for (int r = 0; r < R2; r++) p2[r].re = lds_read1(r2q[r & 1] + 64 * r);
#pragma unroll
    for (int r = 0; r < R1; r++) w1q[r & 3][16 * (r >> 2)] = pts[r].im;
#pragma unroll
    for (int r = 0; r < R2; r++) p2[r].im = lds_read1(r2q[r & 1] + 64 * r);
  }
  else
  {
#pragma unroll
  for (int bb = 0; bb < NB1; bb++)
#pragma unroll
    for (int r = 0; r < R1; r++) w1p[(64 * R1 + 4 * R1) * bb + ((R1 == 8 && r >= 8) ? 0 : r)] = pts[bb * R1 + r].re;
#pragma unroll
  for (int bb = 0; bb < NB2; bb++)
#pragma unroll
    for (int r = 0; r < R2; r++) p2[bb * R2 + r].re = r2p[68 * bb + (N / R2 + N / R2 / 16) * r];
#pragma unroll
  for (int bb = 0; bb < NB1; bb++)
#pragma unroll
    for (int r = 0; r < R1; r++) w1p[(64 * R1 + 4 * R1) * bb + ((R1 == 8 && r >= 8) ? 0 : r)] = pts[bb * R1 + r].im;
#pragma unroll
  for (int bb = 0; bb < NB2; bb++)
#pragma unroll
    for (int r = 0; r < R2; r++) p2[bb * R2 + r].im = r2p[68 * bb + (N / R2 + N / R2 / 16) * r];
  }
  SCHED_FENCE();
  // ---- pass 2 (Ns = R1): twiddle e^{-2 pi i k r / (R1 R2)}, k = j mod R1 = lane mod R1 -----------------
#pragma unroll
  for (int bb = 0; bb < NB2; bb++)
  {
    cx v[R2];
    v[0] = p2[bb * R2];
#pragma unroll
    for (int r = 1; r < R2; r++) v[r] = cmul2(p2[bb * R2 + r], tocx(tw2p[(r - 1) * NS2]));
    bfr<R2>(v);
#pragma unroll
    for (int r = 0; r < R2; r++) p2[bb * R2 + r] = v[r];
  }
  SCHED_FENCE();
  // exchange 2 -> distribution of pass 3: outputs of butterfly j at (j - k) R2 + k + r NS2
  auto in3 = [&](int bb, int r) -> const double* {
    return (LOCAL && bb == 1 ? r3pB : r3pA) + (NS3 + NS3 / 16) * r;
  };
  if constexpr (PLX)
  {
#pragma unroll
    for (int r = 0; r < R2; r++) w2q[0][8 * r] = p2[r].re;
#pragma unroll
    for (int r = 0; r < R3; r++) p3[r].re = lds_read1(r3q[0] + 66 * r);
#pragma unroll
    for (int r = 0; r < R2; r++) w2q[0][8 * r] = p2[r].im;
#pragma unroll
    for (int r = 0; r < R3; r++) p3[r].im = lds_read1(r3q[0] + 66 * r);
  }
  else if constexpr (SWZ)
  {
#pragma unroll
    for (int r = 0; r < R2; r++) w2q[r & 1][8 * r] = p2[r].re;
#pragma unroll
    for (int r = 0; r < R3; r++) p3[r].re = lds_read1(r3q[r & 1] + 64 * r);
#pragma unroll
    for (int r = 0; r < R2; r++) w2q[r & 1][8 * r] = p2[r].im;
#pragma unroll
    for (int r = 0; r < R3; r++) p3[r].im = lds_read1(r3q[r & 1] + 64 * r);
  }
  else
  {
#pragma unroll
  for (int bb = 0; bb < NB2; bb++)
#pragma unroll
    for (int r = 0; r < R2; r++)
      w2p[(64 * R2 + 4 * R2) * bb + NS2 * r + ((NS2 * r) >> 4)] = p2[bb * R2 + r].re;
#pragma unroll
  for (int bb = 0; bb < NB3; bb++)
#pragma unroll
    for (int r = 0; r < R3; r++) p3[bb * R3 + r].re = *in3(bb, r);
#pragma unroll
  for (int bb = 0; bb < NB2; bb++)
#pragma unroll
    for (int r = 0; r < R2; r++)
      w2p[(64 * R2 + 4 * R2) * bb + NS2 * r + ((NS2 * r) >> 4)] = p2[bb * R2 + r].im;
#pragma unroll
  for (int bb = 0; bb < NB3; bb++)
#pragma unroll
    for (int r = 0; r < R3; r++) p3[bb * R3 + r].im = *in3(bb, r);
  }
  SCHED_FENCE();
  // ---- pass 3 (Ns = R1 R2 = N / R3, so k = j): the outputs are the bins j + r NS3 and stay in registers -----
#pragma unroll
  for (int bb = 0; bb < NB3; bb++)
  {
    cx v[R3];
    v[0] = p3[bb * R3];
#pragma unroll
    for (int r = 1; r < R3; r++) v[r] = cmul2(p3[bb * R3 + r], tocx((LOCAL && bb == 1 ? tw3pB : tw3pA)[(r - 1) * NS3]));
    bfr<R3>(v);
#pragma unroll
    for (int r = 0; r < R3; r++) p3[bb * R3 + r] = v[r];
  }
  SCHED_FENCE();
  }

  template <bool SPEC, bool TAB = false, bool FASTMAG = false>
  __device__ __forceinline__ void split(cx (&p3)[PPL], d2* specRow)
  {
  // ---- real-FFT split (util/FFT.hpp:99-106) + magnitude (alg/STFT.hpp:61-66) ------------------------------
  // bin k = j + r NS3 pairs with N - k = (NS3 - j) + (R3 - 1 - r) NS3  (j > 0), or r -> R3 - r for j = 0
  // the products of the per-lane factors with the compile-time constants are loop invariant, and hoisted they
  // would sit in 56 registers for the whole frame loop: keep the factors opaque so they are formed where used
  asm volatile("" : "+v"(wA.re), "+v"(wA.im), "+v"(wB.re), "+v"(wB.im));
  int lq = lane;
  asm volatile("" : "+v"(lq));                    // (opaque: `lane == 0` is compared where it is used, not kept as a spilled exec mask)
  const bool l0 = lq == 0;
  const int srcAddr = ((64 - lane) & 63) * 4;
  (void) srcAddr;
  auto partner = [&](int bb, int r) -> cx {
    if constexpr (LOCAL)
    {
      // lane 0: butterfly 0 pairs within itself (r <-> R3 - r, bin 0 with itself), butterfly NS3/2 within itself
      if (bb == 0)
      {
        const cx x0 = p3[(R3 - r) & (R3 - 1)], x1 = p3[R3 + R3 - 1 - r];
        return cx{l0 ? x0.re : x1.re, l0 ? x0.im : x1.im};
      }
      const cx x1 = p3[R3 + R3 - 1 - r], y1 = p3[R3 - 1 - r];
      return cx{l0 ? x1.re : y1.re, l0 ? x1.im : y1.im};
    }
    else
    {
      // one butterfly per lane: the partner bin lives in lane 64 - l (register R3 - 1 - r); lane 0 pairs within itself
      const cx z = p3[R3 - 1 - r];
      const int lo0 = __builtin_amdgcn_ds_bpermute(srcAddr, (int) (__double_as_longlong(z.re) & 0xffffffff));
      const int hi0 = __builtin_amdgcn_ds_bpermute(srcAddr, (int) (__double_as_longlong(z.re) >> 32));
      const int lo1 = __builtin_amdgcn_ds_bpermute(srcAddr, (int) (__double_as_longlong(z.im) & 0xffffffff));
      const int hi1 = __builtin_amdgcn_ds_bpermute(srcAddr, (int) (__double_as_longlong(z.im) >> 32));
      const double re = __longlong_as_double(((long long) hi0 << 32) | (unsigned) lo0);
      const double im = __longlong_as_double(((long long) hi1 << 32) | (unsigned) lo1);
      const cx own = p3[(R3 - r) & (R3 - 1)];
      return cx{l0 ? own.re : re, l0 ? own.im : im};
    }
  };
  // XL: the partner of bin k = j + r NS3 is bin N - k = (NS3 - j) + (R3 - 1 - r) NS3 in lane NS3 - j -- and for j = 0 the same
  // expression names bin N - r NS3, which is lane 0's own register R3 - r once bin N is read as bin 0 (the transform is
  // periodic).  So the lanes lay one plane of Z (real parts, then imaginary parts) into the staging buffer, slot = bin, with
  // bin 0 once more at slot N, and every lane reads slot (NS3 - lane) + (R3 - 1 - r) NS3: no lane is special, where the
  // ds_bpermute form needed a select per dword for lane 0 (32 v_cndmask + 32 ds_bpermute per frame; now 18 + 16 LDS accesses of
  // 8 bytes and no VALU).  One plane at a time, and the magnitudes go to the same slots: the real parts of all R3 partners
  // are fetched before the imaginary plane overwrites them, and the magnitudes wait in registers for the last partner read
  // (lane 0's partners lie in its own column of slots).
  [[maybe_unused]] double pre[R3], mg[R3];
  [[maybe_unused]] const double* rpx = nullptr;
  if constexpr (XL)
  {
    double* wpx = xb + lq;
    rpx = xb + (NS3 - lq);
#pragma unroll
    for (int r = 0; r < R3; r++) wpx[NS3 * r] = p3[r].re;
    wpx[N] = p3[0].re;
#pragma unroll
    for (int r = 0; r < R3; r++) pre[r] = lds_read1(rpx + NS3 * (R3 - 1 - r));
#pragma unroll
    for (int r = 0; r < R3; r++) wpx[NS3 * r] = p3[r].im;
    wpx[N] = p3[0].im;
  }
#pragma unroll
  for (int bb = 0; bb < NB3; bb++)
  {
    const int j = LOCAL ? (bb == 0 ? jA : jB) : lane;
    const cx wj = (LOCAL && bb == 1) ? wB : wA;
#pragma unroll
    for (int r = 0; r < R3; r++)
    {
      const int i = bb * R3 + r;
      // X[k] = (Z[k] + conj Z[N-k]) / 2 - i / 2 e^{-2 pi i k / fft} (Z[k] - conj Z[N-k]); the halves ride on the twiddle
      // (wj = e^{...} / 2) and on one multiplier of the sum
      cx Bc;
      if constexpr (XL) Bc = cx{pre[r], lds_read1(rpx + NS3 * (R3 - 1 - r))};
      else Bc = partner(bb, r);
      const cx A = p3[i];
      const double er = A.re + Bc.re, ei = A.im - Bc.im;
      const double dr = A.re - Bc.re, di = A.im + Bc.im;
      cx w;
      if constexpr (TAB) w = tocx(splitTab[j + r * NS3]);
      else w = r == 0 ? wj : cmul2(wj, split_const<R3>(r));
      const double xr = __builtin_fma(0.5, er, __builtin_fma(w.re, di, w.im * dr));
      double xi = __builtin_fma(0.5, ei, __builtin_fma(w.im, di, -(w.re * dr)));
      const int k = j + r * NS3;
      if (k == 0) xi = 0.0;                     // DC is purely real (util/FFT.hpp:99-101)
      const double m = mag_sqrt2<FASTMAG>(mag_sumsq(xr, xi));
      if constexpr (XL) mg[r] = m;
      else xb[k] = m;                           // staged (the exchange buffer is idle now)
      if constexpr (SPEC) specRow[k] = d2{xr, xi};
      if (r & 1) SCHED_FENCE();                 // two bins' chains in flight, not sixteen
    }
  }
  if constexpr (XL)
  {
#pragma unroll
    for (int r = 0; r < R3; r++) xb[lq + NS3 * r] = mg[r];
  }
  if (lane == 0)
  {
    const cx z = p3[0];                         // Z[0]: Nyquist = Re - Im, purely real
    const double xr = z.re - z.im;
    xb[N] = fabs(xr);
    if constexpr (SPEC) specRow[N] = d2{xr, 0.0};
  }
  }

  // ---- NF frames at once (round 4, the fused feature kernel) ---------------------------------------------------------
  // The same passes with NF independent frames between the same fences: frame f stages through the buffer f * BUFD doubles
  // behind xb.  One frame's chain -- pass, exchange (write, read, wait), pass, ... -- leaves the wavefront waiting on the
  // LDS most of its life (a single wavefront at top priority needs 11.8 k cycles per frame for 2 760 cycles of VALU issue,
  // and four of them per SIMD fill the VALU to a half); two frames in one instruction stream give the scheduler something
  // to put into every one of those waits.
  template <int NF>
  __device__ __forceinline__ void passesN(cx (&pts)[NF][PPL], cx (&p3)[NF][PPL])
  {
  SCHED_FENCE();
#pragma unroll
  for (int f = 0; f < NF; f++)
#pragma unroll
    for (int bb = 0; bb < NB1; bb++)
    {
      cx v[R1];
#pragma unroll
      for (int r = 0; r < R1; r++) v[r] = pts[f][bb * R1 + r];
      bfr<R1>(v);
#pragma unroll
      for (int r = 0; r < R1; r++) pts[f][bb * R1 + r] = v[r];
    }
  SCHED_FENCE();
  cx p2[NF][PPL];
#pragma unroll
  for (int f = 0; f < NF; f++)
  {
#pragma unroll
    for (int bb = 0; bb < NB1; bb++)
#pragma unroll
      for (int r = 0; r < R1; r++) w1p[f * BUFD + (64 * R1 + 4 * R1) * bb + ((R1 == 8 && r >= 8) ? 0 : r)] = pts[f][bb * R1 + r].re;
#pragma unroll
    for (int bb = 0; bb < NB2; bb++)
#pragma unroll
      for (int r = 0; r < R2; r++) p2[f][bb * R2 + r].re = r2p[f * BUFD + 68 * bb + (N / R2 + N / R2 / 16) * r];
#pragma unroll
    for (int bb = 0; bb < NB1; bb++)
#pragma unroll
      for (int r = 0; r < R1; r++) w1p[f * BUFD + (64 * R1 + 4 * R1) * bb + ((R1 == 8 && r >= 8) ? 0 : r)] = pts[f][bb * R1 + r].im;
#pragma unroll
    for (int bb = 0; bb < NB2; bb++)
#pragma unroll
      for (int r = 0; r < R2; r++) p2[f][bb * R2 + r].im = r2p[f * BUFD + 68 * bb + (N / R2 + N / R2 / 16) * r];
  }
  SCHED_FENCE();
#pragma unroll
  for (int bb = 0; bb < NB2; bb++)
  {
    // (one read of a pass-2 twiddle serves every frame)
    cx tw[R2];
#pragma unroll
    for (int r = 1; r < R2; r++) tw[r] = tocx(tw2p[(r - 1) * NS2]);
#pragma unroll
    for (int f = 0; f < NF; f++)
    {
      cx v[R2];
      v[0] = p2[f][bb * R2];
#pragma unroll
      for (int r = 1; r < R2; r++) v[r] = cmul2(p2[f][bb * R2 + r], tw[r]);
      bfr<R2>(v);
#pragma unroll
      for (int r = 0; r < R2; r++) p2[f][bb * R2 + r] = v[r];
    }
  }
  SCHED_FENCE();
  auto in3 = [&](int f, int bb, int r) -> const double* {
    return (LOCAL && bb == 1 ? r3pB : r3pA) + f * BUFD + (NS3 + NS3 / 16) * r;
  };
#pragma unroll
  for (int f = 0; f < NF; f++)
  {
#pragma unroll
    for (int bb = 0; bb < NB2; bb++)
#pragma unroll
      for (int r = 0; r < R2; r++)
        w2p[f * BUFD + (64 * R2 + 4 * R2) * bb + NS2 * r + ((NS2 * r) >> 4)] = p2[f][bb * R2 + r].re;
#pragma unroll
    for (int bb = 0; bb < NB3; bb++)
#pragma unroll
      for (int r = 0; r < R3; r++) p3[f][bb * R3 + r].re = *in3(f, bb, r);
#pragma unroll
    for (int bb = 0; bb < NB2; bb++)
#pragma unroll
      for (int r = 0; r < R2; r++)
        w2p[f * BUFD + (64 * R2 + 4 * R2) * bb + NS2 * r + ((NS2 * r) >> 4)] = p2[f][bb * R2 + r].im;
#pragma unroll
    for (int bb = 0; bb < NB3; bb++)
#pragma unroll
      for (int r = 0; r < R3; r++) p3[f][bb * R3 + r].im = *in3(f, bb, r);
  }
  SCHED_FENCE();
#pragma unroll
  for (int bb = 0; bb < NB3; bb++)
  {
    cx tw[R3];
#pragma unroll
    for (int r = 1; r < R3; r++) tw[r] = tocx((LOCAL && bb == 1 ? tw3pB : tw3pA)[(r - 1) * NS3]);
#pragma unroll
    for (int f = 0; f < NF; f++)
    {
      cx v[R3];
      v[0] = p3[f][bb * R3];
#pragma unroll
      for (int r = 1; r < R3; r++) v[r] = cmul2(p3[f][bb * R3 + r], tw[r]);
      bfr<R3>(v);
#pragma unroll
      for (int r = 0; r < R3; r++) p3[f][bb * R3 + r] = v[r];
    }
  }
  SCHED_FENCE();
  }

  // the split + magnitude of frame f of NF (staged at xb + f * BUFD); one frame's worth of the single-frame split()
  template <int NF>
  __device__ __forceinline__ void splitN(cx (&p3)[NF][PPL])
  {
    double* const xb0 = xb;
#pragma unroll
    for (int f = 0; f < NF; f++)
    {
      xb = xb0 + f * BUFD;
      split<false>(p3[f], nullptr);
    }
    xb = xb0;
  }
};

// gather + window of frame t of buffer b: point m = x[2m] + i x[2m+1], m = lane + 64 bb + r N/R1 (alg/STFT.hpp:94-105;
// clients/nrt/NMFClient.hpp:240 float -> double); zero outside [0, n)
template <int R1, int N>
__device__ __forceinline__ void gather_points(const StftBArgs& a, int b, int t, int lane, const d2* wsrc, cx (&pts)[N / 64],
                                              int64_t nSamples)
{
  constexpr int NB1 = N / (64 * R1);
  const int64_t s0 = (int64_t) t * a.hop - a.win / 2 + a.frameOffset;
  // ---- gather + window: point m = x[2m] + i x[2m+1], m = lane + 64 bb + r N/R1 --------------------
  // sample positions are 32-bit offsets from the frame's first sample (a wave-uniform 64-bit base); only frames
  // that stick out of the buffer (or an odd base) take the clamped path.  Which offsets are samples of the buffer and
  // where the load of every other one goes is frame_window.h's rule: always a sample of [0, n), counted from the
  // buffer's own first sample for a frame that lies wholly outside it (a wave-uniform choice: s0 and n decide it)
  const FrameWindow fw = frame_window(s0, 2 * N, nSamples);
  if (!fw.loads)
  {
    // an empty buffer: every sample reads as zero and nothing is loaded
#pragma unroll
    for (int i = 0; i < N / 64; i++) pts[i] = cx{0.0, 0.0};
    return;
  }
  if (a.audio)
  {
    const float* fp = a.audio + (int64_t) b * a.audioStride + fw.origin;
    const bool fast = fw.lo == 0 && fw.hi == 2 * N && ((reinterpret_cast<uintptr_t>(fp) & 7) == 0);
    if (fast)
    {
      const float2* lp = reinterpret_cast<const float2*>(fp) + lane;
#pragma unroll
      for (int bb = 0; bb < NB1; bb++)
#pragma unroll
        for (int r = 0; r < R1; r++)
        {
          const int mo = 64 * bb + r * (N / R1);
          const float2 x = lp[mo];
          const d2 w = wsrc[lane + mo];
          pts[bb * R1 + r] = cx{(double) x.x * w[0], (double) x.y * w[1]};
        }
    }
    else
    {
      int ln = lane;                       // (opaque: the per-point offsets of this rare path are not worth registers
      asm volatile("" : "+v"(ln));         //  across the whole frame loop, where the compiler would hoist them)
#pragma unroll
      for (int bb = 0; bb < NB1; bb++)
#pragma unroll
        for (int r = 0; r < R1; r++)
        {
          const int mo = 64 * bb + r * (N / R1);
          const int i0 = 2 * (ln + mo), i1 = i0 + 1;
          const bool ok0 = frame_ok(fw, i0), ok1 = frame_ok(fw, i1);
          const float v0 = fp[frame_load_offset(fw, i0)], v1 = fp[frame_load_offset(fw, i1)];
          const d2 w = wsrc[lane + mo];
          pts[bb * R1 + r] = cx{(ok0 ? (double) v0 : 0.0) * w[0], (ok1 ? (double) v1 : 0.0) * w[1]};
        }
    }
  }
  else
  {
    const double* dp = a.audio64 + (int64_t) b * a.audioStride + fw.origin;
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int bb = 0; bb < NB1; bb++)
#pragma unroll
      for (int r = 0; r < R1; r++)
      {
        const int mo = 64 * bb + r * (N / R1);
        const int i0 = 2 * (ln + mo), i1 = i0 + 1;
        const bool ok0 = frame_ok(fw, i0), ok1 = frame_ok(fw, i1);
        const double v0 = dp[frame_load_offset(fw, i0)], v1 = dp[frame_load_offset(fw, i1)];
        const d2 w = wsrc[lane + mo];
        pts[bb * R1 + r] = cx{(ok0 ? v0 : 0.0) * w[0], (ok1 ? v1 : 0.0) * w[1]};
      }
  }
}

// The interior frames' samples as they lie in memory (the fast path of gather_points, split in two): requested early
// by the frame loop -- ahead of the stores of the frame before, see stft_block_kernel -- and windowed when their turn comes.
// false: an edge frame, an odd base or double-precision input (gather_points takes those).
template <int R1, int N>
__device__ __forceinline__ bool request_samples(const StftBArgs& a, int b, int t, int64_t nSamples, int lane, float2 (&raw)[N / 64])
{
  constexpr int NB1 = N / (64 * R1);
  if (!a.audio) return false;
  const int64_t s0 = (int64_t) t * a.hop - a.win / 2 + a.frameOffset;
  const float* fp = a.audio + (int64_t) b * a.audioStride + s0;
  if (s0 < 0 || s0 + 2 * N > nSamples || (reinterpret_cast<uintptr_t>(fp) & 7) != 0) return false;
  const float2* lp = reinterpret_cast<const float2*>(fp) + lane;
#pragma unroll
  for (int bb = 0; bb < NB1; bb++)
#pragma unroll
    for (int r = 0; r < R1; r++) raw[bb * R1 + r] = lp[64 * bb + r * (N / R1)];
  return true;
}
template <int R1, int N>
__device__ __forceinline__ void window_samples(const float2 (&raw)[N / 64], int lane, const d2* wsrc, cx (&pts)[N / 64])
{
  constexpr int NB1 = N / (64 * R1);
#pragma unroll
  for (int bb = 0; bb < NB1; bb++)
#pragma unroll
    for (int r = 0; r < R1; r++)
    {
      const float2 x = raw[bb * R1 + r];
      const d2 w = wsrc[lane + 64 * bb + r * (N / R1)];
      pts[bb * R1 + r] = cx{(double) x.x * w[0], (double) x.y * w[1]};
    }
}

// A launch's frames as the kernels here take them: no output array and no table of buffer lengths (a launcher that has
// them sets mag, magT, spec and nTab behind this); the dealing of blocks is the launcher's
inline StftBArgs block_args(const StftArgs& a)
{
  StftBArgs k;
  k.audio = a.audio; k.audio64 = a.audio64; k.n = a.n; k.audioStride = a.audioStride;
  k.win = a.win; k.fft = a.fft; k.hop = a.hop; k.T = a.T; k.F = a.F; k.B = a.B;
  k.window = a.window; k.twiddle = a.twiddle;
  k.mag = nullptr; k.magStride = 0; k.ldMag = 0; k.magT = nullptr; k.magTStride = 0; k.ldMagT = 0;
  k.spec = nullptr; k.specStride = 0; k.frameOffset = a.frameOffset; k.blocksPerBuf = 0; k.totalBlocks = 0;
  k.nTab = nullptr; k.prefetch = 0;
  return k;
}
// the sizes FftCore is instantiated for, under an even window no longer than the transform
inline bool fft_core_supported(int64_t win, int64_t fft) { return (win % 2) == 0 && win <= fft && (fft == 1024 || fft == 2048 || fft == 4096); }

} // namespace fluhip
