// fluhip_loudness.h -- launch interface of kernels_loudness.hip (BufLoudness: algorithm::Loudness with its carried
// KWeightingFilter and TruePeak states).  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {

enum : int
{
  kLoudnessFormFrames = 0 // lane = frame: zero-state end states, a scan of 8-value states per buffer, every frame run again
};
constexpr int kLoudnessTaps = 49;        // TruePeak.hpp:147
constexpr int kLoudnessMaxPhases = 4;    // maxFactor, :148
constexpr int kLoudnessMaxPerPhase = 25; // ceil(49 / minFactor)
constexpr int kLoudnessState = 8;        // mX[1..4], mY[0..3]
constexpr int64_t kLoudnessLdsBudget = 64 * 1024; // what one workgroup may take without asking the runtime for more
constexpr int64_t kLoudnessMaxWin = 32768;

// how (win, hop, sample rate) is computed; nothing in it depends on the number of buffers or frames
struct LoudnessPlan
{
  int form = kLoudnessFormFrames;
  int run = 0;     // consecutive frames of one buffer a workgroup owns (one lane each)
  int chunk = 0;   // samples of each of those frames the workgroup stages through the LDS at a time
  int factor = 4;  // the interpolation factor: 4 below 88200 Hz, 2 from there on, 1 = no interpolator (176400 Hz and above)
  int history = 0; // samples of the frame stream in front of a frame the interpolator reads: ring - 1 (0 at factor 1)
  int64_t ldsBytes() const { return (int64_t) run * (chunk + 1) * (int64_t) sizeof(double); }
};
LoudnessPlan loudness_plan(int64_t win, int64_t hop, double sampleRate);

// KWeightingFilter::init (:23-70): mB[0..4], mA[0..4], computed in double on the host
struct KWeighting
{
  double b[5], a[5];
};
KWeighting kweighting_coefficients(double sampleRate);

// M = A^win as an unevaluated sum hi + lo of two doubles per entry, row-major: the state behind a frame of zeros per unit of
// entering state.  Built on the host in double-double arithmetic (kernels_loudness.hip: frame_transition)
struct LoudnessTransition
{
  double hi[kLoudnessState * kLoudnessState], lo[kLoudnessState * kLoudnessState];
};
LoudnessTransition frame_transition(const KWeighting& k, int64_t win);

// impl::Interpolator::init (TruePeak.hpp:48-89): per phase the kept taps (|c| > 1e-6) in tap order
struct InterpolatorTaps
{
  int factor;
  int count[kLoudnessMaxPhases];
  int delay[kLoudnessMaxPhases][kLoudnessMaxPerPhase];
  double coeff[kLoudnessMaxPhases][kLoudnessMaxPerPhase];
};
InterpolatorTaps interpolator_taps(int factor);

// B rows of samples (float or double), `stride` elements apart; frame t of row b is the win samples from t hop on, and lies
// inside its row.  Frame f = b T + t.
struct LoudnessFrames
{
  const float* x32;   // one of the two
  const double* x64;
  int64_t stride;
  int64_t B, T;
  int64_t win, hop;
};

// q[f][0..7] = the filter state behind frame f run from zero state
void launch_loudness_zero_state(const LoudnessFrames& p, const LoudnessPlan& plan, const KWeighting& k, double* q, hipStream_t s);
// st[f][0..7] = the state entering frame f, st[b T] = 0, st[f + 1] = M st[f] + q[f] carried as a double-double pair and rounded
// once, to double, when it is stored
void launch_loudness_scan(const double* q, int64_t B, int64_t T, const LoudnessTransition& M, double* st, hipStream_t s);
// res[f][0] = -0.691 + 10 log10(mean(filtered^2) + epsilon), every frame run from st[f]
void launch_loudness_filtered(const LoudnessFrames& p, const LoudnessPlan& plan, const KWeighting& k, const double* st, double* res,
                              hipStream_t s);
// res[f][1] = 20 log10(peak + epsilon): the interpolated peak over the frame stream (truePeak and plan.factor > 1), else
// max |x|; with unweighted != 0 also res[f][0] = -0.691 + 10 log10(mean(x^2) + epsilon)
void launch_loudness_peak(const LoudnessFrames& p, const InterpolatorTaps& taps, int truePeak, int unweighted, double* res,
                          hipStream_t s);
// out32[b][c][t] = the selected columns (bit 0 loudness, bit 1 peak) of frame drop + t of buffer b, t < keep; res [B T][2]
void launch_loudness_select(const double* res, int64_t B, int64_t T, int64_t drop, int64_t keep, int select, float* out32,
                            hipStream_t s);

} // namespace fluhip
