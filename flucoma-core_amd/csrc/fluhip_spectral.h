// fluhip_spectral.h -- launch interface of kernels_spectral.hip and kernels_spectral_fused.hip (BufSpectralShape: the seven
// descriptors of algorithm::SpectralShape; BufChroma: algorithm::ChromaFilterBank).  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {

enum : int
{
  kSpectralShape = 0,
  kSpectralChroma = 1,
  kSpectralKinds = 2
};
enum : int
{
  kSpectralFormOnChip = 0, // spectral_fused_kernel (kernels_spectral_fused.hip): transform and descriptors in one launch, magnitudes in the LDS
  kSpectralFormTwoPass = 1 // the STFT launch writes the magnitudes of a round to a workspace, the kernels of kernels_spectral.hip read them
};
constexpr int kSpectralRun = 32;      // consecutive frames of one buffer a workgroup of the on-chip form writes
constexpr int kShapeDescriptors = 7;  // centroid, spread, skewness, kurtosis, rolloff, flatness, crest

// how one (fft, win, kind) is computed; nothing in it depends on the number of buffers or frames
struct SpectralPlan
{
  int form = kSpectralFormTwoPass;
  int run = 0;        // on-chip form: frames a workgroup writes (kSpectralRun); 0 in the two-pass form
  int transforms = 1;
  int gemm = 0;       // 1: a contraction with the filter table follows (Chroma)
};
// the sizes the on-chip FFT core (fft_core.h) is built for: fft 1024, 2048, 4096 with an even window
bool spectral_fused_supported(int64_t win, int64_t fft);
SpectralPlan spectral_plan(int64_t fft, int64_t win, int kind);

// frame f of a round is row (f / T) magStride + (f % T) ld of `mag`
struct SpectralFrames
{
  const double* mag;
  int64_t magStride, ld;
  int64_t T, nf; // frames per buffer, frames in all
  int F;
};

// SpectralShape::processFrame (SpectralShape.hpp:32-102) behind its bin arithmetic: the segment is the `size` >= 1 bins from
// `lo` on; axis[i] is the frequency (Hz or MIDI) of bin lo + i, LinSpaced as the reference has it
struct ShapeParams
{
  int lo, size;
  int fold;          // the MIDI axis with minBin 0: lo is 1 and bin 1 takes bin 0's (clamped) magnitude too (:51-55)
  int power;         // 1: the clamped magnitudes are squared
  double percent;    // rolloffPercent
  double miss;       // maxBin - 1: the rolloff when the running sum never crosses (a bin index, :79)
  const double* axis; // device, [size]
};

// out[f][0 .. 6] = the seven descriptors of frame f
void launch_shape_frames(const SpectralFrames& p, const ShapeParams& sp, double* out, hipStream_t s);
// out32[b][c][t] = the selected descriptors (bits 0 .. 6 of `select`, in that order) of frame t of buffer b; res [count T][7]
void launch_shape_select(const double* res, int64_t count, int64_t T, int select, float* out32, hipStream_t s);

// pw[f][j] = mag[f][j]^2 for zlo < j < zhi, else 0, row stride F (ChromaFilterBank.hpp:91-104)
void launch_chroma_power(const SpectralFrames& p, int zlo, int zhi, double* pw, hipStream_t s);
// acc [nf][nChroma]: the contraction with the filter table.  v = acc scale, then divided by max(sum, epsilon) (normalize 1)
// or max(max, epsilon) (normalize 2) of the frame (:109-114).  out64 [nf][nChroma] and / or out32[b][c][t], frame f = b T + t
void launch_chroma_epilogue(const double* acc, int64_t nf, int64_t T, int nChroma, double scale, int normalize, double* out64,
                            float* out32, hipStream_t s);

// The on-chip form: frame t of buffer b is frame f = b T + t.  SpectralShape writes out[f][0 .. 6] and nothing else; Chroma
// writes pw[f][j], row stride F, for the GEMM and the epilogue that follow.
struct StftArgs;
struct SpectralFusedArgs
{
  int kind;
  ShapeParams shape;
  int zlo, zhi;      // Chroma: the bins zlo < j < zhi are kept
  double* out;       // [B T][7], SpectralShape only
  double* pw;        // [B T][F], Chroma only
};
// false: no on-chip form for this shape (nothing was launched)
bool launch_spectral_fused(const StftArgs& a, const SpectralFusedArgs& o, hipStream_t s);

} // namespace fluhip
