// fluhip_onset.h -- launch interface of kernels_onset.hip (BufOnsetSlice / BufOnsetFeature: the ten spectral onset
// detection functions, the running median and the threshold / debounce state machine).  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {

enum : int
{
  kOnsetFormOnChip = 0, // onset_fused_kernel (kernels_onset_fused.hip): transform and reduction in one launch, spectra in the LDS
  kOnsetFormTwoPass = 1 // the STFT launch writes the complex spectra of a round to a workspace, onset_reduce_kernel reads them
};
constexpr int kOnsetFunctions = 10;
constexpr int kOnsetMaxFilter = 101;
constexpr int kOnsetMaxDelta = 8192;
constexpr int kOnsetRun = 32; // consecutive frames of one buffer a workgroup of the on-chip form writes

// frames a value looks back: 0 (energy, HFC, and every frame-delta form), 1 (flux .. cosine), 2 (the phase metrics)
inline int onset_history(int function, int64_t frameDelta)
{
  if (function < 2) return 0;
  if (function < 5) return frameDelta != 0 ? 0 : 1;
  return function == 5 ? 1 : 2;
}
// metrics 2, 3, 4 with a frame delta compare a second transform, frameDelta samples on, with the frame's own
inline bool onset_uses_delta(int function, int64_t frameDelta) { return function >= 2 && function <= 4 && frameDelta != 0; }

// how one (fft, win, function, frameDelta) is computed; nothing in it depends on the number of buffers or frames
struct OnsetPlan
{
  int form = kOnsetFormTwoPass;
  int history = 0;    // spectra before a round's first frame that are recomputed (the halo)
  int transforms = 1; // 2 with a frame delta
  int run = 0;        // on-chip form: frames a workgroup writes (kOnsetRun); 0 in the two-pass form
};
// the sizes the on-chip FFT core (fft_core.h) is built for: fft 1024, 2048, 4096 with an even window
bool onset_fused_supported(int64_t win, int64_t fft);
OnsetPlan onset_plan(int64_t fft, int64_t win, int function, int64_t frameDelta);

struct OnsetReduceArgs
{
  const double* spec;  // [count][rows][F] interleaved complex: row r is frame f0 + r
  const double* spec2; // the second transform of the same frames, or nullptr
  int64_t specStride;  // doubles between buffers
  int F, function;
  int history;         // OnsetPlan::history: rows in front of a frame that the function reads
  int f0;              // global index of row 0; frames below 0 are zero spectra
  int t0, nt;          // frames [t0, t0 + nt) are written
  int T;               // frames per buffer of `raw`
  int64_t count;
  double* raw;         // [count][T]
};
void launch_onset_reduce(const OnsetReduceArgs& a, hipStream_t s);

struct StftArgs;
struct OnsetFusedArgs
{
  int function, history;
  int delta; // samples between the two transforms of a frame-delta form, 0: one transform per frame
  int T;     // frames per buffer
  double* raw; // [B][T]
};
// the on-chip form: `a` describes the frames as for launch_stft (mag / spec unused); false when the shape has none
bool launch_onset_fused(const StftArgs& a, const OnsetFusedArgs& o, hipStream_t s);
// filtered[b][t] = raw[b][t] - median of raw[b][t - f + 1 .. t] (zeros before the start; sorted[f / 2]) for f >= 3, raw below
void launch_onset_filter(const double* raw, double* filtered, int T, int64_t count, int filterSize, hipStream_t s);
// OnsetSegmentation::processFrame over all frames: det [count][T] 0 / 1, counts [count]
void launch_onset_detect(const double* filtered, int T, int64_t count, double threshold, int minSlice, unsigned char* det,
                         int64_t* counts, hipStream_t s);

} // namespace fluhip
