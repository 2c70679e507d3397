// kernels_resynth_batch.hip -- batched resynthesis on the FFT core of fft_core.h (fluhip_kernels.h ResynthBatchArgs):
//   algorithm::NMF::estimate      include/flucoma/algorithms/public/NMF.hpp:33-42       est[t][f] = H1[t][k] W1[k][f]
//   algorithm::RatioMask::process include/flucoma/algorithms/public/RatioMask.hpp:33-57  Y = X min(est (1/max(Vhat,eps)), 1)
//   algorithm::ISTFT::process     include/flucoma/algorithms/public/STFT.hpp:178-199     inverse real FFT, 1/fft, window,
//                                                                                       overlap-add, / max(sum w^2, eps), trim
//   driver                        include/flucoma/clients/nrt/NMFClient.hpp:302-334
// Arithmetic as in resynth_frames_kernel / resynth_ola_kernel (kernels_istft.hip): Z[k] = conj(E[k] + i O[k]) from the
// masked bins k and N - k, forward transform of N = fft/2 points, x[2m] = Re z / N, x[2m+1] = -Im z / N, times the window.
// The input point k = lane + 64 r pairs with N - k, the point of lane 64 - l in register N/64 - 1 - r (lane 0 pairs
// within itself: register N/64 - r, and bin 0 with the Nyquist bin): one ds_bpermute round, no LDS buffer.
// The transform's outputs m = j + r NS3 (j = lane, and NS3 - lane for the two-butterfly forms) are 2 NS3 samples apart
// from register to register: a hop of S 2 NS3 samples shifts the overlap-add state by S registers, all in the lane.
#include "fft_core.h"

#ifndef FLUHIP_RESYNTH_NT
#define FLUHIP_RESYNTH_NT 0
#endif

namespace fluhip {
namespace {

template <int R1, int R2, int R3, int NW, int S, bool SHARED = false>
__global__ __launch_bounds__(64 * NW) void resynth_seq_kernel(ResynthBatchArgs a, int runSlots, int runsPerBuf, int kGroups)
{
  using Core = FftCore<R1, R2, R3>;
  constexpr int N = Core::N, PPL = Core::PPL, BUFD = Core::BUFD, NS3 = Core::NS3, NB3 = Core::NB3;
  static_assert(Core::NB1 == 1, "one pass-1 butterfly per lane: point k = lane + 64 r");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  d2* tw2 = reinterpret_cast<d2*>(lds);
  d2* wl = tw2 + Core::TW;                        // [N] window pairs
  double* nrml = reinterpret_cast<double*>(wl + N); // [hop]
  double* xall = nrml + a.hop;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  double* xb = xall + wave * BUFD;
  // SHARED: the eight wavefronts of the workgroup are eight components of one (buffer, run) and walk the same frames: the
  // frame's spectrum row and reciprocal V-hat row are brought into the LDS once per workgroup, by LDS-DMA, a frame ahead
  // (two row buffers), instead of every wavefront loading them through its registers at the head of its frame
  constexpr int XROW = (N + 2) * 2, MROW = N + 2;  // doubles per row buffer (spectrum complex, reciprocal V-hat), 16-byte multiples
  double* xrow = xall + NW * BUFD;                // [2][XROW]
  double* mrowS = xrow + 2 * XROW;                // [2][MROW]
  const d2* twg = reinterpret_cast<const d2*>(a.twiddle);
  Core::fill_tables(tw2, twg, threadIdx.x, 64 * NW);
  for (int m = threadIdx.x; m < N; m += 64 * NW) wl[m] = reinterpret_cast<const d2*>(a.window)[m];
  for (int m = threadIdx.x; m < a.hop; m += 64 * NW) nrml[m] = a.nrmTab[m];
  __syncthreads();
  Core core;
  core.init(xb, tw2, twg, lane);

  // task: the workgroups of one (buffer, run) sit on one XCD (workgroup i runs on XCD i & 7), NW components each; at
  // ranks below NW a workgroup takes NW / K (buffer, run) pairs instead
  const int64_t wg = blockIdx.x;
  const int64_t slot8 = wg >> 3;
  int64_t pair = (slot8 / kGroups) * 8 + (wg & 7);
  int comp = (int) (slot8 % kGroups) * NW + wave;
  if (a.K < NW)
  {
    const int ppw = NW / a.K;
    if (wave >= ppw * a.K) return;
    pair = pair * ppw + wave / a.K;
    comp = wave % a.K;
  }
  const int b = (int) (pair / runsPerBuf), run = (int) (pair % runsPerBuf);
  if (b >= a.B) return;                           // (the whole workgroup)
  const bool active = comp < a.K;                 // SHARED: idle wavefronts still fetch and meet the barriers
  if (!SHARED && !active) return;                 // (no workgroup barrier below)
  if (!active) comp = 0;
  const int64_t nSamples = a.nTab ? a.nTab[b] : a.n;
  const int Tb = a.nTab ? (int) ((nSamples + a.hop) / a.hop) : a.T;
  const int cover = a.win / a.hop;                // frames over a position (hop | win)
  static_assert(S >= 1 && S <= R3 / 2, "registers the state shifts per frame: hop = S 2 NS3 samples");
  const int sFirst = (int) (a.trim / a.hop);
  const int sLast = (int) ((nSamples - 1 + a.trim) / a.hop);
  const int sa = sFirst + run * runSlots;
  const int sb = min(sa + runSlots, sLast + 1);
  if (sa > sLast) return;

  const double* spec = a.spec + (int64_t) b * a.specStride;
  const double* mult = a.mult + (int64_t) b * a.multStride;
  const double* wrow = a.Wt + (int64_t) b * a.wtStride + (int64_t) comp * a.F;
  const double* hcol = a.H1 + (int64_t) b * a.hStride + comp;
  float* out = a.out32 + ((int64_t) b * a.K + comp) * a.outStride;
  const bool pairStores = (reinterpret_cast<uintptr_t>(out) & 7) == 0 && (a.trim & 1) == 0;
  const double inv = 1.0 / (double) N;
  const int srcAddr = ((64 - lane) & 63) * 4;
  const bool l0 = lane == 0;
  // output samples of this lane in a frame: 2 m, 2 m + 1 with m = jA + r NS3 (and jB + r NS3)
  const int jA = lane, jB = NB3 == 2 ? (lane == 0 ? NS3 / 2 : NS3 - lane) : 0;

  cx acc[PPL];
#pragma unroll
  for (int i = 0; i < PPL; i++) acc[i] = cx{0.0, 0.0};

  // SHARED: rows of frame t into row buffer `which` (every wavefront of the workgroup takes its 1 KB pieces)
  auto fetch_rows = [&](int t, int which) {
    if constexpr (SHARED)
    {
      if (t < 0 || t >= Tb) return;
      const char* xs = reinterpret_cast<const char*>(spec + (int64_t) t * a.F * 2);
      const char* ms = reinterpret_cast<const char*>(mult + (int64_t) t * a.F);
      char* xd = reinterpret_cast<char*>(xrow + which * XROW);
      char* md = reinterpret_cast<char*>(mrowS + which * MROW);
      constexpr int XI = N / (64 * NW) > 0 ? N / (64 * NW) : 1;   // spectrum: N 16-byte bins, 1 KB per instruction
#pragma unroll
      for (int j = 0; j < XI; j++)
      {
        const int cb = (XI * wave + j) * 64;
        if (cb < N)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*) (xs + (int64_t) (cb + lane) * 16),
                                           (__attribute__((address_space(3))) void*) (xd + cb * 16), 16, 0, 0);
      }
      const int cbm = wave * 64;                                  // reciprocal V-hat: N / 2 16-byte pairs
      if (cbm < N / 2)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*) (ms + (int64_t) (cbm + lane) * 16),
                                         (__attribute__((address_space(3))) void*) (md + cbm * 16), 16, 0, 0);
    }
  };
  const int tFirst = sa - (cover - 1);
  if constexpr (SHARED)
  {
    fetch_rows(tFirst, 0);
    __syncthreads();                                 // (drains the DMA: s_waitcnt vmcnt(0) is part of the barrier)
  }

  for (int t = tFirst; t < sb; t++)
  {
    const int which = (t - tFirst) & 1;
    fetch_rows(t + 1 < sb ? t + 1 : -1, which ^ 1);   // the next frame's rows, a frame ahead
    if (active && t >= 0 && t < Tb)
    {
      // ---- masked bins of this lane: k = lane + 64 r ----------------------------------------------------------------
      int ln = lane;
      asm volatile("" : "+v"(ln));                  // (opaque: nothing of the frame-invariant loads is kept across frames)
      const double hk = hcol[(int64_t) t * a.Kp];
      const d2* srow = reinterpret_cast<const d2*>(spec + (int64_t) t * a.F * 2);
      const double* mrow = mult + (int64_t) t * a.F;
      const d2* srowL = reinterpret_cast<const d2*>(xrow + which * XROW);
      const double* mrowL = mrowS + which * MROW;
      cx Y[PPL];
#pragma unroll
      for (int r = 0; r < PPL; r++)
      {
        const int f = ln + 64 * r;
        const d2 x = SHARED ? srowL[f] : srow[f];
        const double mu = SHARED ? mrowL[f] : mrow[f];
        const double m = fmin((hk * wrow[f]) * mu, 1.0);        // NMF.hpp:41, RatioMask.hpp:52-56 (exponent 1)
        Y[r] = cx{x[0] * m, x[1] * m};
      }
      if (l0) Y[0].im = 0.0;                         // packed DC (util/FFT.hpp:155-160)
      // the Nyquist bin, partner of bin 0 (lane 0)
      double yn = 0.0;
      {
        const d2 x = srow[N];
        const double m = fmin((hk * wrow[N]) * mrow[N], 1.0);
        yn = x[0] * m;
      }
      cx pts[PPL];
#pragma unroll
      for (int ii = 0; ii < PPL; ii++)
      {
        // (order 0, PPL-1, 1, PPL-2, ...: point r needs the bins of registers r, PPL-1-r and -- lane 0 -- PPL-r, so the
        //  masked bins die as the points are formed instead of all sixteen living beside all sixteen points)
        const int r = (ii & 1) ? PPL - 1 - (ii >> 1) : (ii >> 1);
        // partner N - k: lane 64 - l, register PPL - 1 - r; lane 0: its own register PPL - r (r > 0), the Nyquist bin (r = 0)
        const cx z = Y[PPL - 1 - r];
        const int lo0 = __builtin_amdgcn_ds_bpermute(srcAddr, (int) (__double_as_longlong(z.re) & 0xffffffff));
        const int hi0 = __builtin_amdgcn_ds_bpermute(srcAddr, (int) (__double_as_longlong(z.re) >> 32));
        const int lo1 = __builtin_amdgcn_ds_bpermute(srcAddr, (int) (__double_as_longlong(z.im) & 0xffffffff));
        const int hi1 = __builtin_amdgcn_ds_bpermute(srcAddr, (int) (__double_as_longlong(z.im) >> 32));
        cx Xn = cx{__longlong_as_double(((long long) hi0 << 32) | (unsigned) lo0),
                   __longlong_as_double(((long long) hi1 << 32) | (unsigned) lo1)};
        const cx own = r == 0 ? cx{yn, 0.0} : Y[PPL - r];
        if (l0) Xn = own;
        const cx X = Y[r];
        // E = (X + conj Xn) / 2, D = (X - conj Xn) / 2, O = D conj(w), Z = E + i O, point = conj Z
        const double er = 0.5 * (X.re + Xn.re), ei = 0.5 * (X.im - Xn.im);
        const double dr = 0.5 * (X.re - Xn.re), di = 0.5 * (X.im + Xn.im);
        const d2 w = twg[ln + 64 * r];               // e^{-2 pi i k / fft}
        const double orr = dr * w[0] + di * w[1], oi = di * w[0] - dr * w[1];
        pts[r] = cx{er - oi, -(ei + orr)};
      }
      cx p3[PPL];
      core.passes(pts, p3);
      // ---- x[2m] = Re / N, x[2m+1] = -Im / N, times the window, onto the running state -----------------------------------
#pragma unroll
      for (int bb = 0; bb < NB3; bb++)
#pragma unroll
        for (int r = 0; r < R3; r++)
        {
          const int i = bb * R3 + r;
          const int m = (bb == 0 ? jA : jB) + r * NS3;
          const d2 w = wl[m];
          acc[i].re += (p3[i].re * inv) * w[0];
          acc[i].im += (-p3[i].im * inv) * w[1];
        }
    }
    // ---- the oldest hop samples are final: slot t --------------------------------------------------------------------
    if (active && t >= sa)
    {
      const int64_t p0 = (int64_t) t * a.hop;
      const bool interior = t - (cover - 1) >= 0 && t <= Tb - 1;
#pragma unroll
      for (int bb = 0; bb < NB3; bb++)
#pragma unroll
        for (int r = 0; r < R3; r++)
        {
          if (r >= S) continue;
          const int i = bb * R3 + r;
          const int m = (bb == 0 ? jA : jB) + r * NS3;
          const int q = 2 * m;
          double n0, n1;
          if (interior) { n0 = nrml[q]; n1 = nrml[q + 1]; }
          else
          {
            // frames t' with t' hop <= p < t' hop + win, 0 <= t' < T, in increasing order (resynth_ola_kernel)
            n0 = 0.0; n1 = 0.0;
            for (int tt = max(0, t - (cover - 1)); tt <= min(t, Tb - 1); tt++)
            {
              const int off = (t - tt) * a.hop + q;
              const d2 w = wl[off >> 1];
              n0 += w[0] * w[0];
              n1 += w[1] * w[1];
            }
          }
          const double y0 = acc[i].re / fmax(n0, kEpsilon), y1 = acc[i].im / fmax(n1, kEpsilon);
          const int64_t i0 = p0 + q - a.trim;
          if (pairStores && i0 >= 0 && i0 + 1 < nSamples)
          {
            // (K x the input's samples leave here and nobody on the device reads them again: non-temporal, FLUHIP_RESYNTH_NT)
            typedef float f2v __attribute__((ext_vector_type(2)));
#if FLUHIP_RESYNTH_NT
            __builtin_nontemporal_store(f2v{(float) y0, (float) y1}, reinterpret_cast<f2v*>(out + i0));
#else
            *reinterpret_cast<f2v*>(out + i0) = f2v{(float) y0, (float) y1};
#endif
          }
          else
          {
            if (i0 >= 0 && i0 < nSamples) out[i0] = (float) y0;
            if (i0 + 1 >= 0 && i0 + 1 < nSamples) out[i0 + 1] = (float) y1;
          }
        }
    }
    // ---- shift the state by one hop ---------------------------------------------------------------------------------
#pragma unroll
    for (int bb = 0; bb < NB3; bb++)
#pragma unroll
      for (int r = 0; r < R3; r++)
      {
        const int i = bb * R3 + r;
        if constexpr (true) acc[i] = (r + S < R3) ? acc[bb * R3 + ((r + S < R3) ? r + S : 0)] : cx{0.0, 0.0};
      }
    if constexpr (SHARED) __syncthreads();          // the next frame's rows have landed; everyone is done with this frame's
  }
}

__global__ void resynth_mult_kernel(const double* Wt, int64_t strideWt, const double* H1, int64_t strideH, double* mult, int T,
                                    int F, int K, int Kp)
{
  // block = (8 frames, buffer): thread f sums k ascending for the 8 frames, W read component-major (Wt[k][f]: consecutive
  // threads, consecutive addresses -- with W as it lies, [f][Kp], every thread walked its own 256-byte row: 1.4 ms on
  // the bench shard)
  extern __shared__ double hs[]; // [8][Kp]
  const int b = blockIdx.y, t0 = blockIdx.x * 8;
  const double* W = Wt + (int64_t) b * strideWt;
  const double* H = H1 + (int64_t) b * strideH;
  for (int i = threadIdx.x; i < 8 * Kp; i += blockDim.x)
  {
    const int tt = i / Kp, k = i % Kp;
    hs[i] = t0 + tt < T ? H[(int64_t) (t0 + tt) * Kp + k] : 0.0;
  }
  __syncthreads();
  for (int f = threadIdx.x; f < F; f += blockDim.x)
  {
    double s[8];
#pragma unroll
    for (int tt = 0; tt < 8; tt++) s[tt] = 0.0;
    for (int k = 0; k < K; k++)
    {
      const double wk = W[(int64_t) k * F + f];
#pragma unroll
      for (int tt = 0; tt < 8; tt++) s[tt] = __builtin_fma(wk, hs[tt * Kp + k], s[tt]);
    }
#pragma unroll
    for (int tt = 0; tt < 8; tt++)
      if (t0 + tt < T) mult[((int64_t) b * T + t0 + tt) * F + f] = 1.0 / fmax(s[tt], kEpsilon); // RatioMask.hpp:39-41
  }
}

} // namespace

__global__ void resynth_nrm_kernel(const double* window, int win, int hop, double* tab)
{
  // normaliser of a padded position covered by all win / hop frames: sum of window^2 over the covering frames in
  // increasing frame order, i.e. decreasing offset (resynth_ola_kernel)
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= hop) return;
  double acc = 0.0;
  for (int j = win / hop - 1; j >= 0; j--)
  {
    const double w = window[q + j * hop];
    acc += w * w;
  }
  tab[q] = acc;
}
void launch_resynth_normaliser(const double* window, int win, int hop, double* tab, hipStream_t s)
{
  hipLaunchKernelGGL(resynth_nrm_kernel, dim3((unsigned) ((hop + 255) / 256)), dim3(256), 0, s, window, win, hop, tab);
}

void launch_resynth_mult(const double* Wf, int64_t strideW, const double* H1, int64_t strideH, double* Wt, double* mult,
                         int T, int F, int K, int Kp, int B, hipStream_t s)
{
  // Wt[b][k][f] = W[b][f][k] (Kp rows of F per buffer), then the reciprocal V-hat from it
  launch_transpose(Wf, Kp, strideW, Wt, F, (int64_t) Kp * F, F, Kp, B, s);
  hipLaunchKernelGGL(resynth_mult_kernel, dim3((unsigned) ((T + 7) / 8), (unsigned) B), dim3(256), (size_t) 8 * Kp * sizeof(double), s,
                     Wt, (int64_t) Kp * F, H1, strideH, mult, T, F, K, Kp);
}

bool resynth_batch_supported(int win, int fft, int hop)
{
  // the transform's outputs lie 2 NS3 samples apart from register to register (256 at fft 2048, 128 at fft 1024): the hop
  // 1, 2 or 4 of those (and so a divisor of the window)
  // (a window shorter than the transform: the samples past it meet a zero window and the state's upper registers stay zero)
  if (win > fft || win < hop || win % hop != 0 || (win & 1)) return false;
  if (fft == 2048) return hop == 256 || hop == 512 || hop == 1024;
  if (fft == 1024) return hop == 128 || hop == 256 || hop == 512;
  return false;
}

template <int R1, int R2, int R3, int NW>
static bool launch_resynth_batch_t(const ResynthBatchArgs& a, hipStream_t s)
{
  using Core = FftCore<R1, R2, R3>;
  const size_t shmem = ((size_t) Core::TW + Core::N) * 16 + (size_t) a.hop * 8 + (size_t) NW * Core::BUFD * 8;
  const int64_t sFirst = a.trim / a.hop, sLast = (a.n - 1 + a.trim) / a.hop;
  const int64_t slots = sLast - sFirst + 1;
  static const int runEnv = [] { const char* e = fluhip::ab_getenv("FLUHIP_RESYNTH_RUN"); return e ? std::atoi(e) : 0; }();
  // A run's first win / hop - 1 frames only fill the state (2 % at 128 slots and hop = win / 4; measured on the bench shard:
  // 32 slots 26.1 ms, 64: 26.1, 128: 25.3, 256: 28.8 -- too few workgroups per buffer there).  Few buffers / components:
  // shorter runs, down to 8 slots, until there are some 1024 workgroups (a single buffer's frames are otherwise walked by
  // a handful of wavefronts one after the other).
  const int kGroups = (a.K + NW - 1) / NW;
  const int ppw = a.K < NW ? NW / a.K : 1;
  int runSlots = 128;
  while (runSlots > 8 && (((slots + runSlots - 1) / runSlots) * a.B + ppw - 1) / ppw * kGroups < 1024) runSlots /= 2;
  if (runEnv > 0) runSlots = runEnv;
  const int runsPerBuf = (int) ((slots + runSlots - 1) / runSlots);
  const int64_t pairs = ((int64_t) a.B * runsPerBuf + ppw - 1) / ppw;
  const int64_t wgs = ((pairs + 7) / 8) * 8 * kGroups;
  // the workgroup's spectrum / V-hat rows through the LDS (see the kernel) from rank NW on: 25.3 -> 19.2 ms on the bench shard,
  // alternating on one box; FLUHIP_RESYNTH_SHARED=0: every wavefront loads its own
  static const int sharedEnv = [] { const char* e = fluhip::ab_getenv("FLUHIP_RESYNTH_SHARED"); return e ? std::atoi(e) : 1; }();
  const bool shared = sharedEnv != 0 && a.K >= NW;
  const size_t shmemS = shmem + (size_t) (2 * (Core::N + 2) * 2 + 2 * (Core::N + 2)) * 8;
  auto go = [&](auto kern, size_t sh) {
    request_dynamic_lds(kern, (size_t) (sh));
    hipLaunchKernelGGL(kern, dim3((unsigned) wgs), dim3(64 * NW), sh, s, a, runSlots, runsPerBuf, kGroups);
  };
  if (shared && shmemS <= 160 * 1024)
  {
    switch (a.hop / (2 * Core::NS3))
    {
    case 1: go(resynth_seq_kernel<R1, R2, R3, NW, 1, true>, shmemS); break;
    case 2: go(resynth_seq_kernel<R1, R2, R3, NW, 2, true>, shmemS); break;
    case 4: go(resynth_seq_kernel<R1, R2, R3, NW, 4, true>, shmemS); break;
    default: return false;
    }
    return true;
  }
  switch (a.hop / (2 * Core::NS3))
  {
  case 1: go(resynth_seq_kernel<R1, R2, R3, NW, 1>, shmem); break;
  case 2: go(resynth_seq_kernel<R1, R2, R3, NW, 2>, shmem); break;
  case 4: go(resynth_seq_kernel<R1, R2, R3, NW, 4>, shmem); break;
  default: return false;
  }
  return true;
}

bool launch_resynth_batch(const ResynthBatchArgs& a, hipStream_t s)
{
  if (!resynth_batch_supported(a.win, a.fft, a.hop) || a.F != a.fft / 2 + 1) return false;
  if (a.fft == 2048) return launch_resynth_batch_t<16, 8, 8, 8>(a, s);
  return launch_resynth_batch_t<8, 8, 8, 8>(a, s);
}

} // namespace fluhip
