// client_frames.h -- the frame bookkeeping of the reference's offline wrappers (clients/common/FluidNRTClientWrapper.hpp),
// once: how many frames a client analyses over a buffer of n samples, how many of them it keeps, and where a slicer's
// detections land.  Host arithmetic only (no HIP: api_pool.cpp includes it under plain g++); nothing here reports an error --
// the range checks ("signal too long", "too many frames", "batch too large") stay with the callers and their bounds.
#pragma once

#include <cstdint>

namespace fluhip {

// FFTParams::padding (cc/ParameterTypes.hpp:315-323): 0 None, 1 Default (half a window), 2 Full (a window less a hop); the
// input sits that many samples into the padded signal
inline int64_t user_padding(int64_t win, int64_t hop, int paddingMode)
{
  return paddingMode == 0 ? 0 : paddingMode == 1 ? win / 2 : win - hop;
}

// StreamingControl::process (:564-579, 642-656).  The padded signal is userPad, the input, userPad, and the client's
// `latency` samples (win for MelBands / MFCC / Pitch / NMFMatch, hop for OnsetFeature, the novelty latency for
// NoveltyFeature; 0 describes BufSTFT's own framing); Full mode rounds it up to whole hops.  Analysis frame j fires with the
// j-th host vector of hop samples and holds the window that ENDS where that vector begins, i.e. it starts at sample
// j hop - win - userPad of the input; the first latency / hop frames are dropped.
struct ControlFrames
{
  int64_t userPad, paddedLength;
  int64_t T;           // analysis frames; counts nothing when paddedLength < win (the callers that can get there refuse it)
  int64_t latencyHops; // ... of which this many are dropped
  int64_t keep;        // T - latencyHops; below 1: "not enough frames"
};

inline ControlFrames control_frames(int64_t n, int64_t win, int64_t hop, int paddingMode, int64_t latency)
{
  ControlFrames g;
  g.userPad = user_padding(win, hop, paddingMode);
  g.paddedLength = n + latency + 2 * g.userPad;
  if (paddingMode == 2) g.paddedLength = ((g.paddedLength + hop - 1) / hop) * hop;
  g.T = 1 + (g.paddedLength - win) / hop;
  g.latencyHops = latency / hop;
  g.keep = g.T - g.latencyHops;
  return g;
}

// Slicing::process (:675-723): `latency` zeros behind the input, rounded up to whole host vectors of 64; a frame fires at
// every multiple of hop below that length
struct SliceFrames
{
  int64_t padded, T;
};

inline SliceFrames slice_frames(int64_t n, int64_t hop, int64_t latency)
{
  SliceFrames g;
  g.padded = (n + latency + 63) / 64 * 64;
  g.T = (g.padded + hop - 1) / hop;
  return g;
}

// Slicing::process :709-722 + spikesToTimes: the detection of frame i (det[i] != 0, i < T) stands at sample i hop of the
// padded signal; any detection inside the latency moves to the first sample, the rest lose the latency, those at or behind
// n are cut.  Writes at most `capacity` indices (startFrame added) to out and returns how many there are; a lone -1 when
// nothing fires.
inline int64_t detections_to_indices(const unsigned char* det, int64_t T, int64_t hop, int64_t latency, int64_t n,
                                     int64_t startFrame, int64_t* out, int64_t capacity)
{
  int64_t cnt = 0;
  auto put = [&](int64_t v) { if (cnt < capacity) out[cnt] = v; cnt++; };
  bool first = false; // a detection at a sample <= latency
  for (int64_t i = 0; i < T && i * hop <= latency; i++) first = first || det[i];
  if (first && n > 0) put(startFrame);
  for (int64_t i = latency / hop + 1; i < T; i++)
  {
    const int64_t p = i * hop - latency;
    if (p >= n) break;
    if (det[i]) put(p + startFrame);
  }
  if (cnt == 0) put(-1);
  return cnt;
}

} // namespace fluhip
