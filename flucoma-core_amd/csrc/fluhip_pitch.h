// fluhip_pitch.h -- launch interface of kernels_pitch.hip (BufPitch: YinFFT, the harmonic product spectrum and the
// cepstrum, with the peak search they share).  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {

enum : int
{
  kPitchCepstrum = 0,
  kPitchHPS = 1,
  kPitchYinFFT = 2,
  kPitchAlgorithms = 3
};
enum : int
{
  kPitchFormOnChip = 0, // pitch_fused_kernel (kernels_pitch_fused.hip): transform and pitch in one launch, magnitudes in the LDS
  kPitchFormTwoPass = 1 // the STFT launch writes the magnitudes of a round to a workspace, the kernels here read them
};
constexpr int kPitchRun = 32; // consecutive frames of one buffer a workgroup of the on-chip form writes
constexpr int64_t kPitchCepstrumMaxFft = 8192; // the DCT table is quadratic in the bin count: 4097^2 doubles = 134 MB

// how one (fft, win, algorithm) is computed; nothing in it depends on the number of buffers or frames
struct PitchPlan
{
  int form = kPitchFormTwoPass;
  int run = 0;        // on-chip form: frames a workgroup writes (kPitchRun); 0 in the two-pass form
  int transforms = 1; // 2 for YinFFT (the transform of the squared magnitudes)
};
// the sizes the on-chip FFT core (fft_core.h) is built for: fft 1024, 2048, 4096 with an even window
bool pitch_fused_supported(int64_t win, int64_t fft);
PitchPlan pitch_plan(int64_t fft, int64_t win, int algorithm);

// the bin ranges of the three algorithms (YINFFT.hpp:72-76, HPS.hpp:40-42, CepstrumF0.hpp:57-58), F = nBins
void pitch_bins(int algorithm, int64_t F, double minFreq, double maxFreq, double sampleRate, int64_t* minBin, int64_t* maxBin);

// frame f of a round is row (f / T) magStride + (f % T) ld of `mag`
struct PitchFrames
{
  const double* mag;
  int64_t magStride, ld;
  int64_t T, nf; // frames per buffer, frames in all
  int F;
};

// sym[f][i] = mag[f][i <= fft / 2 ? i : fft - i]^2, i < fft (YINFFT.hpp:48-50)
void launch_pitch_sym(const PitchFrames& p, double* sym, hipStream_t s);
// spec [nf][F] interleaved complex: the transform of sym.  curve[f][i] = the normalised yin (YINFFT.hpp:54-64), row
// stride ldc; aux[f] = the final running sum
void launch_pitch_yin_norm(const PitchFrames& p, const double* spec, double* curve, int64_t ldc, double* aux, hipStream_t s);
// curve[f][j] = mag[j] mag[2 j] mag[3 j] (HPS.hpp:49-56), or nullptr; out[f] = (f0, confidence)
void launch_pitch_hps(const PitchFrames& p, int64_t minBin, int64_t maxBin, double sampleRate, double* curve, int64_t ldc,
                      double* out, hipStream_t s);
// lg[f][j] = log(max(mag[f][j], epsilon)), row stride F
void launch_pitch_log(const PitchFrames& p, double* lg, hipStream_t s);
// table[r][j], r < rows, j < n: row 0 of DCT::init's table, then its rows first .. first + rows - 2
void launch_pitch_dct_table(double* table, int64_t n, int64_t first, int64_t rows, hipStream_t s);
// PeakDetection::process(seg, 1, seg.minCoeff(), true, true) per frame and the algorithm's result from its first peak.
// YinFFT: seg = -curve[f][minBin .. maxBin), valid when aux[f] > 0.  Cepstrum: curve[f] holds the cepstrum's value 0
// and then its values minBin .. maxBin - 1.
void launch_pitch_peak(int algorithm, const double* curve, int64_t ldc, const double* aux, int64_t nf, int64_t minBin,
                       int64_t maxBin, double sampleRate, double* out, hipStream_t s);
// out32[b][c][t] = the selected values of frame t of buffer b, the pitch in Hz or MIDI (PitchClient.hpp:61, 139-147)
void launch_pitch_select(const double* res, int64_t count, int64_t T, int unit, int select, float* out32, hipStream_t s);

// The on-chip form: frame t of buffer b is frame f = b T + t.  YinFFT and HPS write out[f] = (f0, confidence) and nothing
// else; the cepstrum writes lg[f][j] = log(max(|X_j|, epsilon)), row stride F, for the GEMM and the peak search that follow.
struct StftArgs;
struct PitchFusedArgs
{
  int algorithm;
  int lo, hi;        // minBin, maxBin of pitch_bins (HPS: clamped to F)
  double sampleRate;
  double* out;       // [B T][2]
  double* lg;        // [B T][F], the cepstrum only
};
// false: no on-chip form for this shape (nothing was launched)
bool launch_pitch_fused(const StftArgs& a, const PitchFusedArgs& o, hipStream_t s);
void launch_pitch_fill(double* p, int64_t n, double v, hipStream_t s);

} // namespace fluhip
