// frame_window.h -- which samples of an STFT frame lie inside their buffer, and which address is loaded for the others (host
// and device; tests/cpp/frame_window_host.cpp sweeps the rule on the host, loads included, tests/test_frame_window.py runs it).
//
// A frame is `span` consecutive samples that start at sample s0 of a buffer of n samples; s0 may be anywhere -- the control
// clients' latency puts whole frames before sample 0 and behind sample n -- and a sample outside [0, n) reads as zero.  The
// gathers that issue their loads unconditionally (a frame's samples in flight together, the value selected afterwards:
// gather_points of fft_core.h, stft_wave_kernel of kernels_stft.hip) need an address for the offsets they discard.  The rule:
//   * a load is issued only at a sample inside [0, n);
//   * offsets count from the frame's first sample (32 bits per lane on a wave-uniform 64-bit base) only while the frame has a
//     sample inside the buffer; a frame with none counts from the BUFFER's first sample, so the address of a discarded load
//     is never formed from a frame start that may be far outside;
//   * with n == 0 nothing is loaded.
// Whether a frame has a valid offset depends on s0, span and n alone: every choice below is wave-uniform but `i`.
#pragma once

#include <cstdint>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace fluhip {

struct FrameWindow
{
  int lo, hi;       // offsets [lo, hi) of the frame are samples of the buffer (lo == hi: none is)
  int64_t origin;   // the sample of the buffer a load's offset counts from: s0 while hi > lo, else 0
  int fallback;     // the offset loaded in place of one outside [lo, hi): lo while hi > lo, else 0
  bool loads;       // false: an empty buffer, no load may be issued at all
};

__host__ __device__ inline FrameWindow frame_window(int64_t s0, int span, int64_t n)
{
  FrameWindow w;
  w.lo = s0 < 0 ? (int) (-s0 < span ? -s0 : span) : 0;                 // first valid offset
  const int64_t room = n - s0;
  w.hi = room < span ? (int) (room > 0 ? room : 0) : span;             // one past the last valid offset
  if (w.hi < w.lo) w.hi = w.lo;                                        // (n < 0 only: never a range that runs backwards)
  const bool any = w.hi > w.lo;
  w.origin = any ? s0 : 0;
  w.fallback = any ? w.lo : 0;
  w.loads = n > 0;
  return w;
}

// offset i of the frame is a sample of the buffer
__host__ __device__ inline bool frame_ok(const FrameWindow& w, int i) { return i >= w.lo && i < w.hi; }

// the offset from sample w.origin of the buffer that the load for offset i of the frame goes to (only while w.loads)
__host__ __device__ inline int frame_load_offset(const FrameWindow& w, int i) { return frame_ok(w, i) ? i : w.fallback; }

// sample position p of a buffer of n >= 1 samples brought into [0, n - 1] (the gathers that clamp every position on its own;
// they load only while n > 0)
__host__ __device__ inline int64_t frame_clamped_sample(int64_t p, int64_t n) { return p < 0 ? 0 : (p > n - 1 ? n - 1 : p); }
__host__ __device__ inline bool frame_sample_ok(int64_t p, int64_t n) { return p >= 0 && p < n; }

} // namespace fluhip
