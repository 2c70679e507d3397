// kernels_nmfcross.hip -- BufNMFCross (audio mosaicing, Driedger et al. 2015):
//   algorithm::NMFCross     include/flucoma/algorithms/public/NMFCross.hpp:99-186   constraint stencils + KL H update, W fixed
//   algorithm::NMFCross::synthesize                                   :49-57    result = H1 . srcSpectrum
//   algorithm::GriffinLim   include/flucoma/algorithms/public/GriffinLim.hpp:26-52  magnitude / momentum phase update
//
// The rank is the number of SOURCE frames (hundreds to tens of thousands), so the H update is two large FP64 GEMMs on
// the matrix cores (v_mfma_f64_16x16x4) with the element-wise steps in their epilogues:
//   GEMM1  Q[t][f] = X[t][f] / max(sum_k Hc[t][k] W[k][f], eps)          (W H never reaches memory)
//   GEMM2  H[t][k] = Hc[t][k] * (sum_f Q[t][f] W[k][f]) / max(colsum[k], eps)
// Layouts (row-major, doubles): X, Q [T][F]; W [K][F] (the source magnitudes, clamped to eps); H, Hc, Hs [T][ldh].
// A GEMM whose output has too few tiles to fill the chip splits its contraction: the splits leave partial sums and a
// reduce launch adds them in split order (deterministic) and applies the same epilogue.  Quotients are correctly rounded
// divisions (no reciprocal trees, so no magnitude limit beyond the double range itself).
// The file is compiled with -ffp-contract=off: the element-wise steps round like the reference's separate operations.
#include "fluhip_kernels.h"
#include "fluhip_cross.h"

namespace fluhip {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int kTK = 16; // contraction depth of one LDS stage

__device__ __forceinline__ double cross_epilogue(int epi, double acc, int64_t m, int64_t n, const CrossGemm& g)
{
  if (epi == kCrossEpiRatio) return g.V[m * g.ldv + n] / fmax(acc, kEpsilon);        // NMFCross.hpp:178-179
  if (epi == kCrossEpiHUpdate) return (g.Hc[m * g.ldh + n] * acc) / fmax(g.den[n], kEpsilon); // :180-181
  return acc;
}

// C(m, n) = sum_k A(m, k) B(n, k), A(m, k) = A[m lda + k] (TA = 0) or A[k lda + m] (TA = 1), B likewise.  A workgroup of
// four wavefronts owns a (32 MI) x (32 NI) tile, a wavefront a (16 MI) x (16 NI) quadrant of MI x NI MFMA tiles.
// blockIdx.z = split of the contraction ([z kChunk, (z + 1) kChunk)); epi == kCrossEpiPartial leaves the raw sums at
// C + z splitStride.  The next stage's global loads are issued before the current stage's MFMAs.
template <int TA, int TB, int MI, int NI>
__global__ __launch_bounds__(256) void cross_gemm_kernel(CrossGemm g, int epi)
{
  constexpr int TM = 32 * MI, TN = 32 * NI;
  constexpr int LA = TM * kTK / 256, LB = TN * kTK / 256; // elements per thread and stage
  __shared__ double As[kTK][TM + 1], Bs[kTK][TN + 1];
  const int64_t m0 = (int64_t) blockIdx.y * TM, n0 = (int64_t) blockIdx.x * TN;
  const int64_t kBeg = (int64_t) blockIdx.z * g.kChunk;
  const int64_t kEnd = kBeg + g.kChunk < g.Kd ? kBeg + g.kChunk : g.Kd;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 16 * MI, wn = (wave & 1) * 16 * NI;
  const int lr = lane & 15, lk = lane >> 4;
  d4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < NI; j++) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
  double ra[LA], rb[LB];
  auto load = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < LA; q++)
    {
      const int e = threadIdx.x + 256 * q;
      const int m = TA ? e % TM : e / kTK, k = TA ? e / TM : e % kTK;
      const int64_t gm = m0 + m, gk = k0 + k;
      ra[q] = (gm < g.M && gk < kEnd) ? (TA ? g.A[gk * g.lda + gm] : g.A[gm * g.lda + gk]) : 0.0;
    }
#pragma unroll
    for (int q = 0; q < LB; q++)
    {
      const int e = threadIdx.x + 256 * q;
      const int n = TB ? e % TN : e / kTK, k = TB ? e / TN : e % kTK;
      const int64_t gn = n0 + n, gk = k0 + k;
      rb[q] = (gn < g.N && gk < kEnd) ? (TB ? g.B[gk * g.ldb + gn] : g.B[gn * g.ldb + gk]) : 0.0;
    }
  };
  if (kBeg < kEnd) load(kBeg);
  for (int64_t k0 = kBeg; k0 < kEnd; k0 += kTK)
  {
#pragma unroll
    for (int q = 0; q < LA; q++)
    {
      const int e = threadIdx.x + 256 * q;
      As[TA ? e / TM : e % kTK][TA ? e % TM : e / kTK] = ra[q];
    }
#pragma unroll
    for (int q = 0; q < LB; q++)
    {
      const int e = threadIdx.x + 256 * q;
      Bs[TB ? e / TN : e % kTK][TB ? e % TN : e / kTK] = rb[q];
    }
    __syncthreads();
    if (k0 + kTK < kEnd) load(k0 + kTK);
#pragma unroll
    for (int kk = 0; kk < kTK; kk += 4)
    {
      double a[MI], b[NI];
#pragma unroll
      for (int i = 0; i < MI; i++) a[i] = As[kk + lk][wm + 16 * i + lr];
#pragma unroll
      for (int j = 0; j < NI; j++) b[j] = Bs[kk + lk][wn + 16 * j + lr];
#pragma unroll
      for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < NI; j++) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // result register e of lane l: row l / 16 + 4 e, column l % 16 of the 16 x 16 tile
  double* C = g.C + (epi == kCrossEpiPartial ? (int64_t) blockIdx.z * g.splitStride : 0);
#pragma unroll
  for (int i = 0; i < MI; i++)
#pragma unroll
    for (int j = 0; j < NI; j++)
#pragma unroll
      for (int e = 0; e < 4; e++)
      {
        const int64_t gm = m0 + wm + 16 * i + lk + 4 * e, gn = n0 + wn + 16 * j + lr;
        if (gm < g.M && gn < g.N) C[gm * g.ldc + gn] = cross_epilogue(epi, acc[i][j][e], gm, gn, g);
      }
}

// the splits' partial sums added in split order, then the epilogue
__global__ void cross_reduce_kernel(CrossGemm g, const double* part, int nsplit, int epi)
{
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t) g.M * g.N) return;
  const int64_t m = i / g.N, n = i % g.N;
  double s = part[m * g.N + n];
  for (int z = 1; z < nsplit; z++) s += part[(int64_t) z * g.splitStride + m * g.N + n];
  g.C[m * g.ldc + n] = cross_epilogue(epi, s, m, n, g);
}

template <int TA, int TB, int MI, int NI>
static void launch_form(const CrossGemm& g, int epi, int nsplit, hipStream_t s)
{
  const dim3 grid((unsigned) ((g.N + 32 * NI - 1) / (32 * NI)), (unsigned) ((g.M + 32 * MI - 1) / (32 * MI)), (unsigned) nsplit);
  hipLaunchKernelGGL((cross_gemm_kernel<TA, TB, MI, NI>), grid, dim3(256), 0, s, g, epi);
}

CrossGemmPlan cross_gemm_plan(int64_t M, int64_t N, int64_t Kd, int cus)
{
  CrossGemmPlan p;
  const int64_t bigTiles = ((M + 127) / 128) * ((N + 127) / 128);
  p.big = bigTiles >= cus;
  const int64_t tm = p.big ? 128 : 64;
  const int64_t tiles = ((M + tm - 1) / tm) * ((N + tm - 1) / tm);
  // enough workgroups for two per CU, each split at least 256 deep, at most 32 splits
  const int64_t want = (2 * (int64_t) cus + tiles - 1) / tiles;
  int64_t ns = std::min<int64_t>({want, (Kd + 255) / 256, 32});
  if (ns < 1) ns = 1;
  p.kChunk = round_up((Kd + ns - 1) / ns, kTK);
  p.nsplit = (int) ((Kd + p.kChunk - 1) / p.kChunk);
  if (p.nsplit < 1) p.nsplit = 1;
  // measurement / test builds only (fluhip_env.h): FLUHIP_CROSS_TILE=64|128 and FLUHIP_CROSS_SPLIT=n force the form, so that
  // every form can be held against the restatement at small shapes whatever the device's CU count
  if (const char* e = ab_getenv("FLUHIP_CROSS_TILE")) p.big = std::atoi(e) == 128;
  if (const char* e = ab_getenv("FLUHIP_CROSS_SPLIT"))
  {
    const int64_t want = std::max<int64_t>(1, std::min<int64_t>(std::atoi(e), (Kd + kTK - 1) / kTK));
    p.kChunk = round_up((Kd + want - 1) / want, kTK);
    p.nsplit = (int) ((Kd + p.kChunk - 1) / p.kChunk);
  }
  p.partDoubles = p.nsplit > 1 ? (int64_t) p.nsplit * M * N : 0;
  return p;
}

void launch_cross_gemm(CrossGemm g, int ta, int tb, int epi, const CrossGemmPlan& p, double* part, hipStream_t s)
{
  g.kChunk = p.kChunk;
  const bool split = p.nsplit > 1;
  CrossGemm k = g;
  if (split) { k.C = part; k.ldc = g.N; k.splitStride = (int64_t) g.M * g.N; }
  const int e = split ? kCrossEpiPartial : epi;
  if (ta == 0 && tb == 1)
  {
    if (p.big) launch_form<0, 1, 4, 4>(k, e, p.nsplit, s); else launch_form<0, 1, 2, 2>(k, e, p.nsplit, s);
  }
  else
  {
    if (p.big) launch_form<0, 0, 4, 4>(k, e, p.nsplit, s); else launch_form<0, 0, 2, 2>(k, e, p.nsplit, s);
  }
  if (split)
  {
    CrossGemm r = g;
    r.splitStride = (int64_t) g.M * g.N;
    const int64_t total = g.M * g.N;
    hipLaunchKernelGGL(cross_reduce_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, s, r, part, p.nsplit, epi);
  }
}

// ---- the fixed dictionary ------------------------------------------------------------------------------------------
// W = max(W, eps) in place (NMFCross.hpp:164); colsum[k] = sum_f W[k][f] (W^T 1, :180) and energy[k] = sum_f W[k][f]^2
// (:167), summed in bin order.  One thread per source frame walking its row: uncoalesced and ~0.4 ms (measured, K = 259 ..
// 10 336), but it runs once per job, outside the iteration loop
__global__ void cross_dict_kernel(double* W, int64_t ldw, int K, int F, double* colsum, double* energy)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  double* w = W + (int64_t) k * ldw;
  double s = 0.0, e = 0.0;
  for (int f = 0; f < F; f++)
  {
    const double v = fmax(w[f], kEpsilon);
    w[f] = v;
    s += v;
    e += v * v;
  }
  colsum[k] = s;
  energy[k] = e;
}

void launch_cross_dict(double* W, int64_t ldw, int K, int F, double* colsum, double* energy, hipStream_t s)
{
  hipLaunchKernelGGL(cross_dict_kernel, dim3((unsigned) ((K + 255) / 256)), dim3(256), 0, s, W, ldw, K, F, colsum, energy);
}

// ---- constraint stencils (H as [T][ldh], k contiguous) -------------------------------------------------------------
// promoteContinuity (:99-115): Hc[t][k] = sum_{d < c} H[t + d - h][k + d - h], h = (c - 1) / 2, out-of-range terms 0
__global__ void cross_continuity_kernel(const double* H, double* Hc, int64_t ldh, int T, int K, int c)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int h = (c - 1) / 2;
  for (int t = blockIdx.y; t < T; t += gridDim.y) // (frames beyond the grid's 65535 rows: strided)
  {
    double s = 0.0;
    for (int d = 0; d < c; d++)
    {
      const int tt = t + d - h, kk = k + d - h;
      if (tt >= 0 && tt < T && kk >= 0 && kk < K) s += H[(int64_t) tt * ldh + kk];
    }
    Hc[(int64_t) t * ldh + k] = s;
  }
}

void launch_cross_continuity(const double* H, double* Hc, int64_t ldh, int T, int K, int c, hipStream_t s)
{
  hipLaunchKernelGGL(cross_continuity_kernel, dim3((unsigned) ((K + 255) / 256), (unsigned) std::min(T, 65535)), dim3(256), 0, s, H, Hc, ldh, T, K, c);
}

// enforceTemporalSparseness (:117-140) on the iteration where its factor is 0: H[t][k] is kept when the FIRST maximum of
// the zero-padded window t - h .. t - h + r - 1 of row k is its centre, else 0
__global__ void cross_sparsity_kernel(const double* H, double* out, int64_t ldh, int T, int K, int r)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const int h = (r - 1) / 2;
  for (int t = blockIdx.y; t < T; t += gridDim.y)
  {
    const double v = H[(int64_t) t * ldh + k];
    bool keep = true;
    for (int j = 0; j < r; j++)
    {
      const int tt = t - h + j;
      if (tt == t) continue;
      const double u = (tt >= 0 && tt < T) ? H[(int64_t) tt * ldh + k] : 0.0;
      if (tt < t ? u >= v : u > v) keep = false;
    }
    out[(int64_t) t * ldh + k] = keep ? v : 0.0;
  }
}

void launch_cross_sparsity(const double* H, double* out, int64_t ldh, int T, int K, int r, hipStream_t s)
{
  hipLaunchKernelGGL(cross_sparsity_kernel, dim3((unsigned) ((K + 255) / 256), (unsigned) std::min(T, 65535)), dim3(256), 0, s, H, out, ldh, T, K, r);
}

// restrictPolyphony (:143-155) on the iteration where its factor is 0: in frame t the p entries with the largest
// H[t][k] * energy[k] are kept, the others set to 0.  One workgroup per frame: a radix select over the bit patterns of
// the (non-negative) products finds the p-th largest value v, then every product above v is kept and, among those equal
// to v, the ones of lowest k (std::sort is not stable, so the reference leaves the order of ties open; among the exact
// ties real data produces -- zeros -- the choice does not change the result).  In place.
__global__ __launch_bounds__(256) void cross_polyphony_kernel(double* H, int64_t ldh, int K, const double* energy, int p)
{
  __shared__ unsigned hist[256];
  __shared__ unsigned long long sPrefix;
  __shared__ int sNeed;
  __shared__ int waveCnt[4];
  double* row = H + (int64_t) blockIdx.x * ldh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long prefix = 0, mask = 0;
  int need = p; // rank of the wanted value among the entries that match the prefix so far
  for (int shift = 56; shift >= 0; shift -= 8)
  {
    hist[tid] = 0;
    __syncthreads();
    for (int k = tid; k < K; k += 256)
    {
      const unsigned long long b = (unsigned long long) __double_as_longlong(row[k] * energy[k]);
      if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255], 1u);
    }
    __syncthreads();
    if (tid == 0)
    {
      int d = 255;
      for (; d > 0; d--)
      {
        if ((int) hist[d] >= need) break;
        need -= (int) hist[d];
      }
      sPrefix = prefix | ((unsigned long long) d << shift);
      sNeed = need;
    }
    __syncthreads();
    prefix = sPrefix;
    need = sNeed;
    mask |= 255ull << shift;
    __syncthreads();
  }
  // keep everything above the p-th largest value and the first `need` entries equal to it, in k order
  int taken = 0;
  for (int base = 0; base < K; base += 256)
  {
    const int k = base + tid;
    unsigned long long b = 0;
    if (k < K) b = (unsigned long long) __double_as_longlong(row[k] * energy[k]);
    const bool eq = k < K && b == prefix;
    const unsigned long long bal = __ballot(eq);
    const int below = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) waveCnt[wave] = __popcll(bal);
    __syncthreads();
    int before = taken;
    for (int w = 0; w < wave; w++) before += waveCnt[w];
    const int chunk = waveCnt[0] + waveCnt[1] + waveCnt[2] + waveCnt[3];
    if (k < K)
    {
      const bool keep = b > prefix || (eq && before + below < need);
      if (!keep) row[k] = 0.0;
    }
    taken += chunk;
    __syncthreads();
  }
}

void launch_cross_polyphony(double* H, int64_t ldh, int T, int K, const double* energy, int p, hipStream_t s)
{
  hipLaunchKernelGGL(cross_polyphony_kernel, dim3((unsigned) T), dim3(256), 0, s, H, ldh, K, energy, p);
}

// ---- Griffin-Lim (GriffinLim.hpp:26-52); spectra [T][F] interleaved complex --------------------------------------------
// spec = mag * phase (the complex product with magnitude + 0i: m re, m im)
__global__ void gl_apply_kernel(const double* mag, const double* phase, double* spec, int64_t n)
{
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double m = mag[i];
  spec[2 * i] = m * phase[2 * i];
  spec[2 * i + 1] = m * phase[2 * i + 1];
}

void launch_gl_apply(const double* mag, const double* phase, double* spec, int64_t n, hipStream_t s)
{
  hipLaunchKernelGGL(gl_apply_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, mag, phase, spec, n);
}

// phase = est - (0.9 / 1.9) prev; phase /= |phase| + eps; spec = mag * phase  (:44-47 and the next iteration's :42)
__global__ void gl_update_kernel(const double* mag, const double* est, const double* prev, double* spec, int64_t n)
{
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double momentum = 0.9;
  const double c = momentum / (1 + momentum);
  double re = est[2 * i] - c * prev[2 * i];
  double im = est[2 * i + 1] - c * prev[2 * i + 1];
  const double a = hypot(re, im) + kEpsilon;
  re = re / a;
  im = im / a;
  const double m = mag[i];
  spec[2 * i] = m * re;
  spec[2 * i + 1] = m * im;
}

void launch_gl_update(const double* mag, const double* est, const double* prev, double* spec, int64_t n, hipStream_t s)
{
  hipLaunchKernelGGL(gl_update_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, mag, est, prev, spec, n);
}

} // namespace fluhip
