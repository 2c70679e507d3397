// fluhip_amp.h -- launch interface of kernels_amp.hip (BufAmpSlice / BufAmpFeature: algorithm::Envelope and
// algorithm::EnvelopeSegmentation, sample by sample).  Launch 1 (the front end: hold, high-pass, clipped level) and launch 2
// (the followers, with or without the detector) know nothing of each other but the level workspace, so that a gate
// (EnvelopeGate) can put its own state machine behind the same front end.  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {

enum : int
{
  kAmpFormChunks = 0 // front end: lane = chunk, a scan of 4-value states per signal, every chunk run again; followers: a lane pair per signal
};
constexpr int kAmpChunk = 1024;  // samples of a front-end chunk: a constant of the plan, whatever the call's count and n
constexpr int kAmpTile = 32;     // samples of each of 64 rows a wavefront stages through the LDS at a time
constexpr int kAmpSignals = 32;  // signals per wavefront of the follower kernel (a lane pair each: one follower per lane)
constexpr int kAmpState = 4;     // y1[n-1], y1[n-2], y2[n-1], y2[n-2]: the cascade's outputs; its inputs are known

// ButterworthHPFilter::init (:23-31), computed in double on the host; both sections of the cascade are this one
struct AmpHighPass
{
  double b0, b1, b2, a0, a1;
  int on; // 0: hiPassFreq == 0, the filter is bypassed and the scan launches are skipped
};
AmpHighPass amp_highpass(double hipass);

// M = A^kAmpChunk as an unevaluated sum hi + lo of two doubles per entry, row-major: the state behind a chunk of zero input
// per unit of entering state.  Built on the host in double-double arithmetic
struct AmpTransition
{
  double hi[kAmpState * kAmpState], lo[kAmpState * kAmpState];
};
AmpTransition amp_transition(const AmpHighPass& f);

// `count` rows of n samples (float or double), `stride` elements apart
struct AmpSignals
{
  const float* x32; // one of the two
  const double* x64;
  int64_t stride;
  int64_t count, n;
  int64_t chunks() const { return (n + kAmpChunk - 1) / kAmpChunk; }
};

// workspace of the front end in doubles per signal of n samples: the chunk-end holds [chunks][2], q [chunks][4][2] (hi, lo),
// st [chunks][4]
inline int64_t amp_front_doubles(int64_t n) { return ((n + kAmpChunk - 1) / kAmpChunk) * (2 + 3 * kAmpState); }

// ---- launch 1: level[s][i] (count x n doubles, row-major) = max(20 log10 |highpass(held x)|, floor) -------------------------
// work: count * amp_front_doubles(n) doubles
void launch_amp_level(const AmpSignals& p, const AmpHighPass& f, const AmpTransition& M, double floorDb, double* work, double* level,
                      hipStream_t s);

// ---- launch 2: the two followers and, with detect != 0, EnvelopeSegmentation's detector ------------------------------------
struct AmpFollow
{
  double fastUp, fastDown, slowUp, slowDown; // 1 / ramp (SlideUDFilter::updateCoeffs)
  double floorDb, on, off;
  int64_t minSlice;
  int detect;
  int pair; // 1 = a lane pair per signal (amp_follow_pair_kernel), the production form; 0, in the measurement build only, one lane
};
// env64 / env32 (count x n, either may be null; env64 may be `level` itself): fast - slow; det (count x n bytes, may be
// null) and counts (count, with detect): 1 where a slice starts, and how many
void launch_amp_follow(const double* level, int64_t count, int64_t n, const AmpFollow& f, double* env64, float* env32,
                       unsigned char* det, int64_t* counts, hipStream_t s);

} // namespace fluhip
