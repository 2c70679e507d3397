// fluhip_novelty.h -- launch interface of kernels_novelty.hip (BufNoveltySlice / BufNoveltyFeature: Foote's novelty curve,
// its smoothing and the peak picking).  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {

enum : int
{
  kNoveltyFormMfma = 0,  // band on chip, Gram blocks on the FP64 matrix pipe (D >= kNoveltyValuDims)
  kNoveltyFormValu = 1,  // band on chip, Gram entries by plain FMAs (small D)
  kNoveltyFormTiled = 2  // kernel sizes above kNoveltyOnChipKernel: the band goes through a workspace in memory
};
constexpr int kNoveltyOnChipKernel = 65; // largest kernel size whose window of rows is held in the LDS
constexpr int kNoveltyValuDims = 32;     // feature rows shorter than this do not fill an MFMA's contraction

// how one (T, D, kernel size) is computed; nothing in it depends on the number of buffers but the workspace size
struct NoveltyPlan
{
  int form = kNoveltyFormMfma;
  int rows = 0;            // feature rows a workgroup holds (on-chip forms), 16 for the tiled form's row blocks
  int frames = 0;          // curve values a workgroup writes: rows - k + 1
  int64_t workDoubles = 0; // tiled form: [count][T][k] band + [count][T] norms
};
NoveltyPlan novelty_plan(int64_t count, int64_t T, int64_t D, int64_t k);

struct NoveltyArgs
{
  const double* X; // [count][T][ldx] feature rows
  int64_t ldx, strideX;
  int T, D, k;
  int64_t count;
  double norm;     // sum of the squared checkerboard kernel (Novelty.hpp createKernel)
  double* nov;     // [count][T] raw novelty (Novelty::processFrame)
  double* work;    // NoveltyPlan::workDoubles
};
// sigma = k / 3 in integers (WindowFuncs.hpp kGaussian); the kernel's gaussian and its squared sum
double novelty_sigma(int k);
double novelty_kernel_norm(int k);
void launch_novelty_raw(const NoveltyArgs& a, const NoveltyPlan& p, hipStream_t s);
// curve[b][t] = mean of nov[b][t - f + 1 .. t], zeros before the start (NoveltyFeature::processFrame)
void launch_novelty_smooth(const double* nov, double* curve, int T, int64_t count, int f, hipStream_t s);
// NoveltySegmentation::processFrame over all frames: det [count][T] 0 / 1, counts [count]
void launch_novelty_peaks(const double* curve, int T, int64_t count, double threshold, int minSlice, unsigned char* det,
                          int64_t* counts, hipStream_t s);
// out[b][i] = ((0 + in[b][0][i]) + in[b][1][i]) + ... in float (the offline wrapper's mono sum)
void launch_mono_sum_f32(const float* in, int channels, int64_t n, int64_t count, float* out, hipStream_t s);
// out[b][t] = (float) curve[b][t0 + t], t < keep
void launch_curve_to_f32(const double* curve, int T, int t0, int keep, int64_t count, float* out, hipStream_t s);

} // namespace fluhip
