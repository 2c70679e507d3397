// fluhip_hpss.h -- launch interface of kernels_hpss.hip (BufHPSS: the two sliding medians over a magnitude plane and the
// three masks built from them).  Not installed; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fluhip {

enum : int
{
  kHpssFormOnChip = 0, // the filter's window of a workgroup's bins is copied to the LDS once and ranked from there
  kHpssFormMemory = 1  // ... is ranked straight from the magnitude plane in memory (through the caches), by index test
};
constexpr int kHpssBinTile = 256;  // bins (= threads) of a workgroup
constexpr int kHpssMaxOnChip = 63; // the largest filter size, of either filter, whose window is held in the LDS

// how one (hSize, vSize) is computed; nothing in it depends on the number of buffers, frames or bins
struct HpssPlan
{
  int formH = kHpssFormOnChip, formV = kHpssFormOnChip;
  int64_t ldsBytes = 0; // dynamic LDS of a workgroup
  int binTile = kHpssBinTile;
};
HpssPlan hpss_plan(int64_t hSize, int64_t vSize);

struct HpssArgs
{
  const double* mag;   // [count][T][ldMag]: row t is frame m = t + 1
  int64_t magStride, ldMag;
  const double* spec;  // [count][T][F] interleaved complex, or nullptr (planes only)
  int64_t specStride;
  int T, F;
  int64_t count;
  int hSize, vSize, mode;
  const double* thrH;  // [F] HPSS::makeThreshold of harmThresh (modes 1, 2)
  const double* thrP;  // [F] ... of percThresh (mode 2)
  double* out;         // [count][3][T][F] interleaved complex: spec times the harmonic / percussive / residual mask, or nullptr
  int64_t outStride;   // doubles between buffers (the three outputs of one lie T F 2 apart)
  double* hmed;        // [count][T][F] or nullptr
  double* vmed;        // [count][T][F] or nullptr
  double* masks[3];    // each [count][T][F] or nullptr
};
void launch_hpss_masks(const HpssArgs& a, hipStream_t s);

} // namespace fluhip
