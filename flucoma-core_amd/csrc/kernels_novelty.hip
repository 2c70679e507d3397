// kernels_novelty.hip -- Foote's novelty curve, its smoothing and the peak picking (BufNoveltySlice / BufNoveltyFeature):
//   algorithm::Novelty              include/flucoma/algorithms/util/Novelty.hpp:48-100
//   algorithm::NoveltyFeature       include/flucoma/algorithms/public/NoveltyFeature.hpp:44-62
//   algorithm::NoveltySegmentation  include/flucoma/algorithms/public/NoveltySegmentation.hpp:44-63
//
// The reference keeps a k x k similarity matrix that shifts by one frame per call; an entry never changes once written, so
//   nov[t] = sum_{a, b < k} K[a][b] C(t - k + 1 + a, t - k + 1 + b) / sum(K .* K)
//   C(p, q) = <x_p, x_q> / max(max(|x_lo|, eps) |x_hi|, eps),  lo = min(p, q), hi = max(p, q),  x_p = 0 for p < 0
// and every frame is independent of every other.  A workgroup owns `frames` consecutive curve values of one buffer and the
// rows = frames + k - 1 feature rows they look at: it forms the Gram matrix of those rows in the LDS (16 x 16 blocks of
// v_mfma_f64_16x16x4 fed from a staged strip of the rows, or plain FMAs when a row is shorter than an MFMA wants), turns it
// into C in place with the norms from its diagonal, and contracts it with the checkerboard kernel.  The feature rows are
// read once per workgroup (plus the k - 1 rows of halo); the band never reaches memory.  Kernel sizes whose window does not
// fit (k > kNoveltyOnChipKernel) take the tiled form: the band [T][k] goes through a workspace in memory.
// The summation order depends on (T, D, k) only, never on the number of buffers: a batch gives the bits of single calls.
#include "fluhip_kernels.h"
#include "fluhip_novelty.h"

#include <cmath>

namespace fluhip {

typedef double d4n __attribute__((ext_vector_type(4)));
constexpr int kNovTK = 16;   // contraction depth of one LDS stage (MFMA form)
constexpr int kNovGkPad = 80; // room for the gaussian of the on-chip forms (k <= 65)

double novelty_sigma(int k) { return (double) (k / 3); } // WindowFuncs.hpp:68: `double sigma = size / 3` on integers

static double novelty_gauss(int i, double sigma) { return std::exp((double) (-(int64_t) i * i) / (2 * sigma * sigma)); }

double novelty_kernel_norm(int k)
{
  // mKernel.square().sum() of K = +- g g^T (Novelty.hpp:104-117)
  const int h = (k - 1) / 2;
  const double sigma = novelty_sigma(k);
  double s = 0.0;
  for (int b = 0; b < k; b++)
    for (int a = 0; a < k; a++)
    {
      const double v = novelty_gauss(a - h, sigma) * novelty_gauss(b - h, sigma);
      s += v * v;
    }
  return s;
}

NoveltyPlan novelty_plan(int64_t count, int64_t T, int64_t D, int64_t k)
{
  NoveltyPlan p;
  if (k > kNoveltyOnChipKernel)
  {
    p.form = kNoveltyFormTiled;
    p.rows = 16;
    p.frames = 16;
    p.workDoubles = count * T * (k + 1);
    return p;
  }
  p.form = D >= kNoveltyValuDims ? kNoveltyFormMfma : kNoveltyFormValu;
  p.rows = k <= 17 ? 32 : (k <= 33 ? 64 : 96); // at least 16 (k <= 17) / 32 curve values per workgroup
  p.frames = p.rows - (int) k + 1;
  return p;
}

__device__ __forceinline__ double nov_kernel_entry(const double* gk, int a, int b, int h)
{
  // tmp = g g^T; rows h.., columns < h and rows < h, columns h.. negated (Novelty.hpp:112-114)
  const double v = gk[a] * gk[b];
  return ((a >= h) != (b >= h)) ? -v : v;
}

template <int RB, bool MFMA>
__global__ __launch_bounds__(256) void novelty_tile_kernel(NoveltyArgs a, int B, int nt, int dp)
{
  constexpr int R = 16 * RB, LDG = R + 1;
  extern __shared__ double lds[];
  double* G = lds;              // [R][LDG] Gram matrix, then C
  double* nrm = G + R * LDG;    // [R]
  double* gk = nrm + R;         // [k]
  double* P = gk + kNovGkPad;   // [B][k] row sums of the contraction
  double* Xs = P + B * a.k;     // MFMA: [kNovTK][LDG] strip of the rows, transposed; VALU: [R][dp] the rows
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / nt;
  const int tile = (int) (blockIdx.x % nt);
  const int t0 = tile * B;              // first curve value of the tile
  const int f0 = t0 - (a.k - 1);        // frame of local row 0
  const double* X = a.X + b * a.strideX;
  const int h = (a.k - 1) / 2;

  if (tid < a.k)
  {
    const int i = tid - h;
    const double sigma = (double) (a.k / 3);
    gk[tid] = exp((double) (-i * i) / (2 * sigma * sigma));
  }

  if constexpr (MFMA)
  {
    constexpr int NBLK = RB * (RB + 1) / 2, NPW = (NBLK + 3) / 4;
    const int lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    int bi[NPW], bj[NPW];
    d4n acc[NPW];
#pragma unroll
    for (int s = 0; s < NPW; s++)
    {
      const int n = wave + 4 * s;
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= n) I++;
      bi[s] = n < NBLK ? I : 0;
      bj[s] = n < NBLK ? n - I * (I + 1) / 2 : 0;
      acc[s] = d4n{0.0, 0.0, 0.0, 0.0};
    }
    double rx[RB];
    auto load = [&](int k0) {
#pragma unroll
      for (int q = 0; q < RB; q++)
      {
        const int e = tid + 256 * q;
        const int r = e / kNovTK, kk = e % kNovTK;
        const int fr = f0 + r, col = k0 + kk;
        rx[q] = (fr >= 0 && fr < a.T && col < a.D) ? X[(int64_t) fr * a.ldx + col] : 0.0;
      }
    };
    load(0);
    for (int k0 = 0; k0 < a.D; k0 += kNovTK)
    {
#pragma unroll
      for (int q = 0; q < RB; q++)
      {
        const int e = tid + 256 * q;
        Xs[(e % kNovTK) * LDG + e / kNovTK] = rx[q];
      }
      __syncthreads();
      if (k0 + kNovTK < a.D) load(k0 + kNovTK);
#pragma unroll
      for (int kk = 0; kk < kNovTK; kk += 4)
#pragma unroll
        for (int s = 0; s < NPW; s++)
        {
          const double va = Xs[(kk + lk) * LDG + 16 * bi[s] + lr];
          const double vb = Xs[(kk + lk) * LDG + 16 * bj[s] + lr];
          acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(va, vb, acc[s], 0, 0, 0);
        }
      __syncthreads();
    }
    // result register e of lane l: row l / 16 + 4 e, column l % 16 of the 16 x 16 block
#pragma unroll
    for (int s = 0; s < NPW; s++)
      if (wave + 4 * s < NBLK)
#pragma unroll
        for (int e = 0; e < 4; e++)
        {
          const int r = 16 * bi[s] + lk + 4 * e, c = 16 * bj[s] + lr;
          G[r * LDG + c] = acc[s][e];
          if (bi[s] != bj[s]) G[c * LDG + r] = acc[s][e];
        }
  }
  else
  {
    for (int e = tid; e < R * a.D; e += 256)
    {
      const int r = e / a.D, d = e % a.D;
      const int fr = f0 + r;
      Xs[r * dp + d] = (fr >= 0 && fr < a.T) ? X[(int64_t) fr * a.ldx + d] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < R * R; e += 256)
    {
      const int r = e / R, c = e % R;
      if (c > r || r - c >= a.k) continue;
      double s = 0.0;
      for (int d = 0; d < a.D; d++) s += Xs[r * dp + d] * Xs[c * dp + d];
      G[r * LDG + c] = s;
      G[c * LDG + r] = s;
    }
  }
  __syncthreads();
  if (tid < R) nrm[tid] = sqrt(G[tid * LDG + tid]);
  __syncthreads();
  // C(p, q): the older frame's norm is the one clamped first (Novelty.hpp:62-68: the ring's rows against the new frame)
  for (int e = tid; e < R * R; e += 256)
  {
    const int r = e / R, c = e % R;
    const int d = r > c ? r - c : c - r;
    if (d >= a.k) continue;
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    const double den = fmax(fmax(nrm[lo], kEpsilon) * nrm[hi], kEpsilon);
    G[r * LDG + c] = G[r * LDG + c] / den;
  }
  __syncthreads();
  for (int idx = tid; idx < B * a.k; idx += 256)
  {
    const int j = idx / a.k, aa = idx % a.k;
    const double* row = G + (j + aa) * LDG + j;
    double s = 0.0;
    for (int bb = 0; bb < a.k; bb++) s += nov_kernel_entry(gk, aa, bb, h) * row[bb];
    P[idx] = s;
  }
  __syncthreads();
  if (tid < B && t0 + tid < a.T)
  {
    double s = 0.0;
    for (int aa = 0; aa < a.k; aa++) s += P[tid * a.k + aa];
    a.nov[b * a.T + t0 + tid] = s / a.norm;
  }
}

// ---- tiled form ------------------------------------------------------------------------------------------------------
// band[b][p][d] = <x_p, x_{p - d}>, d < k; nrm[b][p] = |x_p|.  A workgroup owns 16 rows p and walks the 16-row blocks of q
// the band touches, one block per wavefront and step; the MFMA operands come straight from memory.
__global__ __launch_bounds__(256) void novelty_band_kernel(NoveltyArgs a, int nrb)
{
  const int64_t b = blockIdx.x / nrb;
  const int I = (int) (blockIdx.x % nrb);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const double* X = a.X + b * a.strideX;
  double* band = a.work + b * (int64_t) a.T * (a.k + 1);
  double* nrm = band + (int64_t) a.T * a.k;
  const int jmin = max(0, I - (a.k + 14) / 16);
  for (int J = I - wave; J >= jmin; J -= 4)
  {
    d4n acc = d4n{0.0, 0.0, 0.0, 0.0};
    const int ra = 16 * I + lr, rb = 16 * J + lr;
    for (int d0 = 0; d0 < a.D; d0 += 4)
    {
      const int col = d0 + lk;
      const double va = (ra < a.T && col < a.D) ? X[(int64_t) ra * a.ldx + col] : 0.0;
      const double vb = (rb < a.T && col < a.D) ? X[(int64_t) rb * a.ldx + col] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va, vb, acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
    {
      const int p = 16 * I + lk + 4 * e, q = 16 * J + lr;
      const int d = p - q;
      if (p < a.T && d >= 0 && d < a.k)
      {
        band[(int64_t) p * a.k + d] = acc[e];
        if (d == 0) nrm[p] = sqrt(acc[e]);
      }
    }
  }
}

__global__ void novelty_band_quotient_kernel(NoveltyArgs a)
{
  const int64_t per = (int64_t) a.T * a.k;
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count * per) return;
  const int64_t b = i / per;
  const int p = (int) ((i % per) / a.k), d = (int) (i % a.k);
  if (p - d < 0) return;
  double* band = a.work + b * (int64_t) a.T * (a.k + 1);
  const double* nrm = band + per;
  const double den = fmax(fmax(nrm[p - d], kEpsilon) * nrm[p], kEpsilon);
  band[(int64_t) p * a.k + d] = band[(int64_t) p * a.k + d] / den;
}

// one wavefront per curve value: the k x k window of the band against the checkerboard kernel
__global__ __launch_bounds__(256) void novelty_band_contract_kernel(NoveltyArgs a)
{
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.count * (int64_t) a.T) return;
  const int64_t b = w / a.T;
  const int t = (int) (w % a.T);
  const double* band = a.work + b * (int64_t) a.T * (a.k + 1);
  const int h = (a.k - 1) / 2;
  const double sigma = (double) (a.k / 3);
  const double inv = 1.0 / (2 * sigma * sigma);
  double s = 0.0;
  for (int idx = lane; idx < a.k * a.k; idx += 64)
  {
    const int aa = idx / a.k, bb = idx % a.k;
    const int pa = t - (a.k - 1) + aa, pb = t - (a.k - 1) + bb;
    const int hi = pa > pb ? pa : pb, lo = pa > pb ? pb : pa;
    if (lo < 0) continue;
    const int ia = aa - h, ib = bb - h;
    const double v = exp((double) (-ia * ia) * inv) * exp((double) (-ib * ib) * inv);
    const double kv = ((aa >= h) != (bb >= h)) ? -v : v;
    s += kv * band[(int64_t) hi * a.k + (hi - lo)];
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) a.nov[b * a.T + t] = s / a.norm;
}

template <int RB, bool MFMA>
static void launch_tile(const NoveltyArgs& a, const NoveltyPlan& p, hipStream_t s)
{
  constexpr int R = 16 * RB;
  const int B = p.frames;
  const int nt = (a.T + B - 1) / B;
  const int dp = a.D | 1;
  const size_t doubles = (size_t) R * (R + 1) + R + kNovGkPad + (size_t) B * a.k + (MFMA ? (size_t) kNovTK * (R + 1) : (size_t) R * dp);
  request_dynamic_lds(novelty_tile_kernel<RB, MFMA>, (size_t) (160 * 1024));
  hipLaunchKernelGGL((novelty_tile_kernel<RB, MFMA>), dim3((unsigned) (a.count * nt)), dim3(256), doubles * sizeof(double), s, a, B,
                     nt, dp);
}

void launch_novelty_raw(const NoveltyArgs& a, const NoveltyPlan& p, hipStream_t s)
{
  if (a.T < 1 || a.count < 1) return;
  if (p.form == kNoveltyFormTiled)
  {
    const int nrb = (a.T + 15) / 16;
    hipLaunchKernelGGL(novelty_band_kernel, dim3((unsigned) (a.count * nrb)), dim3(256), 0, s, a, nrb);
    const int64_t n = a.count * (int64_t) a.T * a.k;
    hipLaunchKernelGGL(novelty_band_quotient_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, a);
    const int64_t waves = a.count * (int64_t) a.T;
    hipLaunchKernelGGL(novelty_band_contract_kernel, dim3((unsigned) ((waves + 3) / 4)), dim3(256), 0, s, a);
    return;
  }
  const bool m = p.form == kNoveltyFormMfma;
  if (p.rows == 32) m ? launch_tile<2, true>(a, p, s) : launch_tile<2, false>(a, p, s);
  else if (p.rows == 64) m ? launch_tile<4, true>(a, p, s) : launch_tile<4, false>(a, p, s);
  else m ? launch_tile<6, true>(a, p, s) : launch_tile<6, false>(a, p, s);
}

// ---- smoothing, peaks, debounce -----------------------------------------------------------------------------------------
__global__ void novelty_smooth_kernel(const double* nov, double* curve, int T, int64_t count, int f)
{
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count * T) return;
  const int t = (int) (i % T);
  const double* row = nov + (i - t);
  double s = 0.0;
  for (int j = f - 1; j >= 0; j--) s += (t - j >= 0) ? row[t - j] : 0.0; // oldest first, like the filter buffer
  curve[i] = s / (double) f;
}

void launch_novelty_smooth(const double* nov, double* curve, int T, int64_t count, int f, hipStream_t s)
{
  const int64_t n = count * T;
  if (n < 1) return;
  hipLaunchKernelGGL(novelty_smooth_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, nov, curve, T, count, f);
}

// One wavefront per buffer.  The three-point test is frame-parallel (the peak buffer holds s[t - 2], s[t - 1], s[t], zeros
// before the start); the debounce counter only matters at candidates: a detection at t0 sets it to minSlice, it is back at 0
// when frame t0 + minSlice + 1 is tested, so a candidate is a detection when it lies more than minSlice frames behind the
// last one.  The wavefront walks 64 frames at a time and, wave-uniformly, the set bits of their candidate mask.
__global__ __launch_bounds__(64) void novelty_peaks_kernel(const double* curve, int T, double threshold, int minSlice,
                                                           unsigned char* det, int64_t* counts)
{
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const double* c = curve + b * T;
  unsigned char* out = det + b * T;
  int64_t last = 0, cnt = 0;
  bool have = false;
  for (int base = 0; base < T; base += 64)
  {
    const int t = base + lane;
    bool cand = false;
    if (t < T)
    {
      const double s2 = c[t], s1 = t >= 1 ? c[t - 1] : 0.0, s0 = t >= 2 ? c[t - 2] : 0.0;
      cand = s1 > s0 && s1 > s2 && s1 > threshold;
    }
    unsigned long long mask = __ballot(cand);
    unsigned char flag = 0;
    while (mask)
    {
      const int bit = __ffsll((long long) mask) - 1;
      mask &= mask - 1;
      const int64_t tt = base + bit;
      if (!have || tt - last > minSlice)
      {
        have = true;
        last = tt;
        cnt++;
        if (lane == bit) flag = 1;
      }
    }
    if (t < T) out[t] = flag;
  }
  if (lane == 0) counts[b] = cnt;
}

void launch_novelty_peaks(const double* curve, int T, int64_t count, double threshold, int minSlice, unsigned char* det,
                          int64_t* counts, hipStream_t s)
{
  if (count < 1) return;
  hipLaunchKernelGGL(novelty_peaks_kernel, dim3((unsigned) count), dim3(64), 0, s, curve, T, threshold, minSlice, det, counts);
}

__global__ void mono_sum_kernel(const float* in, int channels, int64_t n, int64_t count, float* out)
{
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count * n) return;
  const int64_t b = i / n, j = i % n;
  float s = 0.0f;
  for (int c = 0; c < channels; c++) s += in[(b * channels + c) * n + j];
  out[i] = s;
}

void launch_mono_sum_f32(const float* in, int channels, int64_t n, int64_t count, float* out, hipStream_t s)
{
  const int64_t total = count * n;
  if (total < 1) return;
  hipLaunchKernelGGL(mono_sum_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, s, in, channels, n, count, out);
}

__global__ void curve_to_f32_kernel(const double* curve, int T, int t0, int keep, int64_t count, float* out)
{
  const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count * keep) return;
  const int64_t b = i / keep;
  const int t = (int) (i % keep);
  out[i] = (float) curve[b * T + t0 + t];
}

void launch_curve_to_f32(const double* curve, int T, int t0, int keep, int64_t count, float* out, hipStream_t s)
{
  const int64_t total = count * keep;
  if (total < 1) return;
  hipLaunchKernelGGL(curve_to_f32_kernel, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, s, curve, T, t0, keep, count, out);
}

} // namespace fluhip
