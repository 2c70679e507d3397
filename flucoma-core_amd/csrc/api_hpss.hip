// api_hpss.hip -- C ABI of BufHPSS:
//   fluhip_hpss_planes_f64   algorithm::HPSS::processFrame over a whole magnitude plane   algorithms/public/HPSS.hpp:66-174
//   fluhip_bufhpss_f32       NRTHPSSClient   clients/rt/HPSSClient.hpp:37-136 behind Streaming, common/FluidNRTClientWrapper.hpp:466-547
// The kernel is in kernels_hpss.hip (fluhip_hpss.h); the spectra come from launch_stft, the audio from the plain form of
// launch_resynth (no ratio mask).  Every device buffer is a DevBuf of the call; no event, no stream is taken.
#include "api_internal.h"
#include "fluhip_hpss.h"

namespace {

constexpr int64_t kHpssCapDoubles = (int64_t) 1 << 27; // 1 GiB of planes and spectra per round
constexpr int64_t kHpssMaxFilter = 1001;               // the count is O(size^2) per value: a bound on what one launch may cost

int check_hpss_sizes(fluhip_ctx* ctx, int64_t hSize, int64_t vSize)
{
  if (hSize < 3 || hSize > kHpssMaxFilter || (hSize % 2) == 0) return fail(ctx, "harmFilterSize must be odd and in [3, 1001]");
  if (vSize < 3 || vSize > kHpssMaxFilter || (vSize % 2) == 0) return fail(ctx, "percFilterSize must be odd and in [3, 1001]");
  return FLUHIP_OK;
}

int check_hpss_params(fluhip_ctx* ctx, int64_t F, int64_t hSize, int64_t vSize, int mode, const double* hThresh,
                      const double* pThresh)
{
  const int rc = check_hpss_sizes(ctx, hSize, vSize);
  if (rc) return rc;
  if (vSize > F) return fail(ctx, "percFilterSize must not exceed the number of bins (fft / 2 + 1)");
  if (mode < 0 || mode > 2) return fail(ctx, "maskingMode must be 0 (Classic), 1 (Coupled) or 2 (Advanced)");
  if (!hThresh || !pThresh) return fail(ctx, "null buffer");
  const double* th[2] = {hThresh, pThresh};
  for (int i = 0; i < 2; i++)
  {
    const double* p = th[i];
    // (FrequencyAmpPairConstraint clips and swaps in the client; here a pair that would need it is refused.  NaN fails every test.)
    if (!(p[0] >= 0.0 && p[0] <= 1.0 && p[2] >= 0.0 && p[2] <= 1.0 && p[0] <= p[2]) || !std::isfinite(p[1]) || !std::isfinite(p[3]))
      return fail(ctx, i == 0 ? "harmThresh: frequencies must be in [0, 1] and ascending, amplitudes finite"
                              : "percThresh: frequencies must be in [0, 1] and ascending, amplitudes finite");
  }
  return FLUHIP_OK;
}

// Eigen's ArrayXd::LinSpaced(size, low, high): size 1 yields HIGH; the end the larger magnitude sits at is exact
void lin_spaced(int64_t size, double low, double high, double* out)
{
  if (size < 1) return;
  if (size == 1) { out[0] = high; return; }
  const double step = (high - low) / (double) (size - 1);
  const bool flip = std::fabs(high) < std::fabs(low);
  for (int64_t i = 0; i < size; i++)
    out[i] = flip ? (i == 0 ? low : high - (double) (size - 1 - i) * step) : (i == size - 1 ? high : low + (double) i * step);
}

// HPSS::makeThreshold, HPSS.hpp:157-174, in doubles on the host
std::vector<double> make_threshold(int64_t nBins, const double* t)
{
  const double x1 = t[0], y1 = t[1], x2 = t[2], y2 = t[3];
  std::vector<double> thr((size_t) nBins, 1.0);
  const int64_t kneeStart = (int64_t) std::floor(x1 * (double) nBins);
  const int64_t kneeEnd = (int64_t) std::floor(x2 * (double) nBins);
  const int64_t kneeLength = kneeEnd - kneeStart;
  for (int64_t i = 0; i < kneeStart; i++) thr[(size_t) i] = std::pow(10.0, y1 / 20.0);
  std::vector<double> lin((size_t) std::max<int64_t>(kneeLength, 0));
  lin_spaced(kneeLength, y1, y2, lin.data());
  for (int64_t i = 0; i < kneeLength; i++) thr[(size_t) (kneeStart + i)] = std::pow(10.0, lin[(size_t) i] / 20.0);
  for (int64_t i = kneeEnd; i < nBins; i++) thr[(size_t) i] = std::pow(10.0, y2 / 20.0);
  return thr;
}

int upload_thresholds(fluhip_ctx* ctx, int64_t F, const double* hThresh, const double* pThresh, DevBuf& dThr)
{
  std::vector<double> thr = make_threshold(F, hThresh);
  const std::vector<double> p = make_threshold(F, pThresh);
  thr.insert(thr.end(), p.begin(), p.end());
  DEV_ALLOC(ctx, "HPSS", dThr, thr.size() * sizeof(double), false);
  HIPCHK(ctx, hipMemcpyAsync(dThr.p, thr.data(), thr.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (thr is a local)
  return FLUHIP_OK;
}

int hpss_planes_impl(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld, int64_t hSize,
                     int64_t vSize, int mode, const double* hThresh, const double* pThresh, double* hmed, double* vmed,
                     double* const* masks)
{
  if (count < 1) return fail(ctx, "need at least one buffer");
  if (T < 1 || F < 1) return fail(ctx, "need at least one frame and one bin");
  int rc = check_hpss_params(ctx, F, hSize, vSize, mode, hThresh, pThresh);
  if (rc) return rc;
  if (!mag) return fail(ctx, "null buffer");
  if (ld < F) return fail(ctx, "row stride below the number of bins");
  if (T > INT32_MAX / 4 || F > INT32_MAX / 4 || ld > INT32_MAX / 4) return fail(ctx, "too many frames or bins");
  if (T > (INT64_MAX / 64) / ld / count) return fail(ctx, "batch too large");
  double* outs[5] = {hmed, vmed, masks ? masks[0] : nullptr, masks ? masks[1] : nullptr, masks ? masks[2] : nullptr};
  int nOut = 0;
  for (double* o : outs) nOut += o != nullptr;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf dThr, dMag, dOut[5];
  if ((rc = upload_thresholds(ctx, F, hThresh, pThresh, dThr))) return rc;
  const int64_t perBuffer = T * (ld + nOut * F);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(count, kHpssCapDoubles / perBuffer));
  DEV_ALLOC(ctx, "HPSS", dMag, (size_t) (chunk * T * ld) * sizeof(double), false);
  for (int i = 0; i < 5; i++)
    if (outs[i]) DEV_ALLOC(ctx, "HPSS", dOut[i], (size_t) (chunk * T * F) * sizeof(double), false);
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    HIPCHK(ctx, hipMemcpyAsync(dMag.p, mag + b0 * T * ld, (size_t) (nb * T * ld) * sizeof(double), hipMemcpyHostToDevice, s));
    HpssArgs a;
    a.mag = dMag.as<double>(); a.magStride = T * ld; a.ldMag = ld;
    a.spec = nullptr; a.specStride = 0;
    a.T = (int) T; a.F = (int) F; a.count = nb;
    a.hSize = (int) hSize; a.vSize = (int) vSize; a.mode = mode;
    a.thrH = dThr.as<double>(); a.thrP = dThr.as<double>() + F;
    a.out = nullptr; a.outStride = 0;
    a.hmed = outs[0] ? dOut[0].as<double>() : nullptr;
    a.vmed = outs[1] ? dOut[1].as<double>() : nullptr;
    for (int i = 0; i < 3; i++) a.masks[i] = outs[2 + i] ? dOut[2 + i].as<double>() : nullptr;
    launch_hpss_masks(a, s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    const size_t nbytes = (size_t) (nb * T * F) * sizeof(double);
    for (int i = 0; i < 5; i++)
      if (outs[i] && (rc = copy_to_host(ctx, outs[i] + b0 * T * F, nbytes, dOut[i].p, nbytes, nbytes, 1, s))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

int bufhpss_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                 int64_t hSize, int64_t vSize, int mode, const double* hThresh, const double* pThresh, float* out)
{
  if (!audio || !out) return fail(ctx, "null buffer");
  if (count < 1) return fail(ctx, "need at least one buffer");
  int rc = check_shape(ctx, n, win, fft, hop, 1);
  if (rc) return rc;
  if (hop > win) return fail(ctx, "fftSettings: hop sizes above the window size are not supported");
  const int64_t F = fft / 2 + 1;
  if ((rc = check_hpss_params(ctx, F, hSize, vSize, mode, hThresh, pThresh))) return rc;
  // Streaming::process (cc/FluidNRTClientWrapper.hpp:466-547) drops the client's latency (hSize - 1) hop + win: the frame a
  // call masks is the input of hSize - 1 calls ago, so -- as in fluhip_nmffilter_f32 -- frame m = 1, 2, ... covers the audio
  // samples [m hop - win, m hop) and is overlap-added where it came from; window^2 is added for every frame.  Frames
  // 1 .. T are those that touch the buffer; the medians see zeros outside them by index test.
  const int64_t T = (n + win + hop - 1) / hop - 1;
  if (T < 1) return fail(ctx, "not enough frames");
  if (T > 2000000000LL / 16) return fail(ctx, "too many frames");
  if (n > INT32_MAX / 2) return fail(ctx, "signal too long");
  const int64_t ldM = round_up(F, 32);
  if (count > (INT64_MAX / 64) / std::max(T * (ldM + 8 * F), n)) return fail(ctx, "batch too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  StftSetup st;
  if ((rc = stft_setup(ctx, win, fft, hop, &st))) return rc;
  DevBuf dThr, dIn, dMag, dSpec, dMasked, dFrames, dOut;
  if ((rc = upload_thresholds(ctx, F, hThresh, pThresh, dThr))) return rc;
  // buffers per round: magnitudes, the spectrum and the three masked spectra of a round stay below the cap
  const int64_t perBuffer = T * (ldM + 8 * F);
  int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(count, kHpssCapDoubles / perBuffer));
  chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, (2000000000LL / 16) / T));
  DEV_ALLOC(ctx, "HPSS", dIn, (size_t) (chunk * n) * sizeof(float), false);
  DEV_ALLOC(ctx, "HPSS", dMag, (size_t) (chunk * T * ldM) * sizeof(double), false);
  DEV_ALLOC(ctx, "HPSS", dSpec, (size_t) (chunk * T * F * 2) * sizeof(double), false);
  DEV_ALLOC(ctx, "HPSS", dMasked, (size_t) (chunk * 3 * T * F * 2) * sizeof(double), false);
  DEV_ALLOC(ctx, "HPSS", dFrames, (size_t) (T * win) * sizeof(double), false);
  DEV_ALLOC(ctx, "HPSS", dOut, (size_t) (chunk * 3 * n) * sizeof(float), false);
  const int nInverse = mode == 2 ? 3 : 2; // the residual mask is zero in modes 0 and 1: its output is zeros, no transform
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    HIPCHK(ctx, hipMemcpyAsync(dIn.p, audio + b0 * n, (size_t) (nb * n) * sizeof(float), hipMemcpyHostToDevice, s));
    StftArgs sa = st.args(dIn.as<float>(), nullptr, n, n, nb, T, hop - win); // frame t = m - 1 starts at (t + 1) hop - win: every one touches the buffer
    sa.mag = dMag.as<double>(); sa.magStride = T * ldM; sa.ldMag = ldM;
    sa.spec = dSpec.as<double>(); sa.specStride = T * F * 2;
    if ((rc = st.launch(ctx, sa, 0))) return rc;
    HIPCHK(ctx, hipGetLastError());
    HpssArgs a;
    a.mag = dMag.as<double>(); a.magStride = T * ldM; a.ldMag = ldM;
    a.spec = dSpec.as<double>(); a.specStride = T * F * 2;
    a.T = (int) T; a.F = (int) F; a.count = nb;
    a.hSize = (int) hSize; a.vSize = (int) vSize; a.mode = mode;
    a.thrH = dThr.as<double>(); a.thrP = dThr.as<double>() + F;
    a.out = dMasked.as<double>(); a.outStride = 3 * T * F * 2;
    a.hmed = a.vmed = nullptr;
    a.masks[0] = a.masks[1] = a.masks[2] = nullptr;
    {
      ProfScope p(ctx, 5);
      launch_hpss_masks(a, s);
    }
    HIPCHK(ctx, hipGetLastError());
    {
      ProfScope inverse(ctx, 6); // (every inverse launch of the round)
      if (nInverse < 3)
        HIPCHK(ctx, hipMemset2DAsync(dOut.as<float>() + 2 * n, (size_t) (3 * n) * sizeof(float), 0, (size_t) n * sizeof(float), (size_t) nb, s));
      for (int64_t b = 0; b < nb; b++)
        for (int c = 0; c < nInverse; c++)
        {
          // ISTFT::processFrame per frame, overlap-add, division by the overlap-added window^2 (BufferedProcess.hpp:219-239)
          // frame t lies at [t hop - trim, t hop - trim + win) of the output, trim = win - hop
          ResynthArgs ra = st.resynth(dMasked.as<double>() + (b * 3 + c) * T * F * 2, T, dFrames.as<double>(), n, win - hop);
          ra.out32 = dOut.as<float>() + (b * 3 + c) * n; ra.outStride = n;
          if ((rc = st.launch(ctx, ra))) return rc;
        }
    }
    HIPCHK(ctx, hipGetLastError());
    const size_t nbytes = (size_t) (nb * 3 * n) * sizeof(float);
    if ((rc = copy_to_host(ctx, out + b0 * 3 * n, nbytes, dOut.p, nbytes, nbytes, 1, s))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_hpss_plan(fluhip_ctx* ctx, int64_t harm_filter_size, int64_t perc_filter_size, int64_t* out4)
{
  if (!out4) return fail(ctx, "null buffer");
  const int rc = check_hpss_sizes(ctx, harm_filter_size, perc_filter_size);
  if (rc) return rc;
  const HpssPlan p = hpss_plan(harm_filter_size, perc_filter_size);
  out4[0] = p.formH;
  out4[1] = p.formV;
  out4[2] = p.ldsBytes;
  out4[3] = p.binTile;
  return FLUHIP_OK;
}

int fluhip_hpss_planes_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                           int64_t harm_filter_size, int64_t perc_filter_size, int mode, const double* harm_thresh,
                           const double* perc_thresh, double* hmed, double* vmed, double* const* masks)
{
  return guarded(ctx, [&] {
    return hpss_planes_impl(ctx, mag, count, T, F, ld, harm_filter_size, perc_filter_size, mode, harm_thresh, perc_thresh, hmed,
                            vmed, masks);
  });
}

int fluhip_bufhpss_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                       int64_t harm_filter_size, int64_t perc_filter_size, int mode, const double* harm_thresh,
                       const double* perc_thresh, float* out)
{
  return guarded(ctx, [&] {
    return bufhpss_impl(ctx, audio, count, n, win, fft, hop, harm_filter_size, perc_filter_size, mode, harm_thresh, perc_thresh, out);
  });
}

} // extern "C"
