// Host build of csrc/frame_window.h (tests/test_frame_window.py): one frame's gather emulated the way the kernels do it --
// every offset i of [0, span), its `ok` flag, the address its load goes to -- over frames anywhere around their buffer:
//   small   span 2 / 4 / 8 / 16 / 64, every n of 0 .. 3 span, every s0 of [-4 span, n + 4 span]
//   real    span 1024 / 2048 / 4096, a handful of n, every s0 within +-3 of -2 span, -span, 0, n - span, n, n + span
//   edge    s0 and n at the int32 bounds the callers allow (api_onset.hip check_onset_range: n <= INT32_MAX / 2, every sample
//           index a launch forms inside int32), and a step beyond them
// For every frame: (a) ok(i) exactly when 0 <= s0 + i < n, (b) every address loaded lies in [0, n), (c) nothing is loaded
// when n == 0; and the same three for the per-position clamp (frame_clamped_sample / frame_sample_ok).
//
//   frame_window_host           the shared rule; prints "ok <frames> small <..> real <..> edge <..>" or the first failure
//   frame_window_host parent    the selection gather_points had before this header (`ok ? i : lo` from the frame's first
//                               sample), kept here as test code: it must FAIL, and prints how many frames load outside
//                               [0, n) by class -- "parent empty <..> before <..> behind <..> other <..>"
//   frame_window_host loads     the small sweep with the loads performed, from heap blocks of exactly n floats and n doubles
//                               (built with -fsanitize=address,undefined: a stray address is a report, not a discarded value)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../flucoma-core_amd/csrc/frame_window.h"

using fluhip::FrameWindow;

namespace {

enum Mode { kShared, kParent, kLoads };

struct Tally
{
  long long frames = 0, small = 0, real = 0, edge = 0;
  long long empty = 0, before = 0, behind = 0, other = 0; // parent mode: frames with a load outside [0, n)
  double sink = 0.0;
};

// the rule gather_points carried before frame_window.h: offsets from the frame's first sample, `lo` for a discarded one
struct ParentWindow { int lo, hi; };
ParentWindow parent_window(int64_t s0, int span, int64_t n)
{
  ParentWindow w;
  w.lo = s0 < 0 ? (int) (-s0 < span ? -s0 : span) : 0;
  const int64_t room = n - s0;
  w.hi = room < span ? (int) (room > 0 ? room : 0) : span;
  return w;
}

bool fail(const char* what, int span, int64_t n, int64_t s0, int i, int64_t addr)
{
  std::printf("fail %s span %d n %lld s0 %lld i %d address %lld\n", what, span, (long long) n, (long long) s0, i, (long long) addr);
  return false;
}

// one frame under the shared rule; fbuf / dbuf: blocks of exactly n floats / doubles to load from, or null
bool shared_frame(int span, int64_t n, int64_t s0, const float* fbuf, const double* dbuf, Tally& t)
{
  const FrameWindow w = fluhip::frame_window(s0, span, n);
  if (w.loads != (n > 0)) return fail("loads", span, n, s0, -1, 0);
  if (w.lo < 0 || w.hi > span || w.hi < w.lo) return fail("range", span, n, s0, -1, 0);
  // the kernels' base pointers: formed once per frame, and only where a load follows
  const float* fp = (fbuf && w.loads) ? fbuf + w.origin : nullptr;
  const double* dp = (dbuf && w.loads) ? dbuf + w.origin : nullptr;
  for (int i = 0; i < span; i++)
  {
    const bool ok = fluhip::frame_ok(w, i);
    const int64_t p = s0 + i;
    if (ok != (p >= 0 && p < n)) return fail("ok", span, n, s0, i, p);
    if (w.loads)
    {
      const int off = fluhip::frame_load_offset(w, i);
      const int64_t addr = w.origin + off;
      if (addr < 0 || addr >= n) return fail("address", span, n, s0, i, addr);
      if (ok && addr != p) return fail("sample", span, n, s0, i, addr);
      if (fp) t.sink += ok ? (double) fp[off] : 0.0;
      if (dp) t.sink += ok ? dp[off] : 0.0;
    }
    // the per-position clamp of the wave kernel's gathers
    if (fluhip::frame_sample_ok(p, n) != (p >= 0 && p < n)) return fail("sample_ok", span, n, s0, i, p);
    if (n > 0)
    {
      const int64_t c = fluhip::frame_clamped_sample(p, n);
      if (c < 0 || c >= n || (p >= 0 && p < n && c != p)) return fail("clamp", span, n, s0, i, c);
      if (fbuf) t.sink += fbuf[c];
      if (dbuf) t.sink += dbuf[c];
    }
  }
  return true;
}

// one frame under the parent's rule: counts it by class when one of its loads leaves [0, n)
void parent_frame(int span, int64_t n, int64_t s0, Tally& t)
{
  const ParentWindow w = parent_window(s0, span, n);
  bool bad = false;
  for (int i = 0; i < span && !bad; i++)
  {
    const bool ok = i >= w.lo && i < w.hi;
    const int64_t addr = s0 + (ok ? i : w.lo);
    bad = addr < 0 || addr >= n;
  }
  if (!bad) return;
  if (n == 0) t.empty++;                 // an empty buffer: any load is outside it
  else if (s0 < -(int64_t) span) t.before++;  // wholly before the buffer, by more than a frame
  else if (s0 >= n) t.behind++;          // wholly behind it
  else t.other++;
}

bool frame(Mode mode, int span, int64_t n, int64_t s0, const float* fbuf, const double* dbuf, Tally& t)
{
  t.frames++;
  if (mode == kParent) { parent_frame(span, n, s0, t); return true; }
  return shared_frame(span, n, s0, fbuf, dbuf, t);
}

} // namespace

int main(int argc, char** argv)
{
  Mode mode = kShared;
  if (argc > 1 && !std::strcmp(argv[1], "parent")) mode = kParent;
  else if (argc > 1 && !std::strcmp(argv[1], "loads")) mode = kLoads;
  else if (argc > 1) { std::printf("usage: frame_window_host [parent | loads]\n"); return 2; }
  Tally t;

  for (int span : {2, 4, 8, 16, 64})
    for (int64_t n = 0; n <= 3 * span; n++)
    {
      // exactly n elements each, so that one element outside is outside the block
      std::vector<float> f;
      std::vector<double> d;
      if (mode == kLoads) { f.assign((size_t) n, 1.0f); d.assign((size_t) n, 1.0); f.shrink_to_fit(); d.shrink_to_fit(); }
      const float* fb = (mode == kLoads && n > 0) ? f.data() : nullptr;
      const double* db = (mode == kLoads && n > 0) ? d.data() : nullptr;
      for (int64_t s0 = -4 * span; s0 <= n + 4 * span; s0++)
      {
        if (!frame(mode, span, n, s0, fb, db, t)) return 1;
        t.small++;
      }
    }

  if (mode != kLoads)
  {
    for (int span : {1024, 2048, 4096})
      for (int64_t n : {(int64_t) 0, (int64_t) 1, (int64_t) span - 1, (int64_t) span, (int64_t) span + 1,
                        (int64_t) span + span / 2 + 5, (int64_t) 3 * span})
        for (int64_t edge : {(int64_t) -2 * span, (int64_t) -span, (int64_t) 0, n - span, n, n + span})
          for (int64_t s0 = edge - 3; s0 <= edge + 3; s0++)
          {
            if (!frame(mode, span, n, s0, nullptr, nullptr, t)) return 1;
            t.real++;
          }

    // the int32 bounds: n up to INT32_MAX / 2, frame starts whose every sample index stays inside int32 -- and a step past
    // either, which the 64-bit frame start must carry all the same
    const int64_t half = INT32_MAX / 2, full = INT32_MAX;
    for (int span : {2, 64, 1024, 4096})
      for (int64_t n : {(int64_t) 0, (int64_t) 1, half - 1, half, half + 1, full, full + 1})
        for (int64_t edge : {-full - 1, -full, -half, -half - span, (int64_t) -span, (int64_t) 0, n - span, n, n + span, half,
                             full - span, full, full + 1, (int64_t) 1 << 40, -((int64_t) 1 << 40)})
          for (int64_t s0 = edge - 2; s0 <= edge + 2; s0++)
          {
            if (!frame(mode, span, n, s0, nullptr, nullptr, t)) return 1;
            t.edge++;
          }
  }

  if (mode == kParent)
    std::printf("parent empty %lld before %lld behind %lld other %lld frames %lld\n", t.empty, t.before, t.behind, t.other, t.frames);
  else
    std::printf("ok %lld small %lld real %lld edge %lld sink %.0f\n", t.frames, t.small, t.real, t.edge, t.sink);
  return 0;
}
