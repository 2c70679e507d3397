// api_onset.hip -- C ABI of BufOnsetSlice / BufOnsetFeature:
//   fluhip_onset_curve_f64      algorithm::OnsetDetectionFunctions::processFrame  algorithms/public/OnsetDetectionFunctions.hpp:70-114
//   fluhip_onset_slices_f64     algorithm::OnsetSegmentation::processFrame        algorithms/public/OnsetSegmentation.hpp:46-66
//   fluhip_bufonsetslice_f32    NRTOnsetSliceClient    clients/rt/OnsetSliceClient.hpp, common/FluidNRTClientWrapper.hpp:665-725
//   fluhip_bufonsetfeature_f32  NRTOnsetFeatureClient  clients/rt/OnsetFeatureClient.hpp, common/FluidNRTClientWrapper.hpp:551-660
// The kernels are in kernels_onset.hip (fluhip_onset.h); the spectra come from launch_stft.  Every device buffer is a
// DevBuf of the call (back in the pool on every way out); no event, no stream is taken.
#include "api_internal.h"
#include "fluhip_novelty.h" // launch_mono_sum_f32, launch_curve_to_f32
#include "fluhip_onset.h"

namespace {

constexpr int64_t kSpecCapDoubles = (int64_t) 1 << 27; // 1 GiB of spectra per round

int check_onset_params(fluhip_ctx* ctx, int function, int64_t filterSize, int64_t frameDelta, int64_t win, int64_t fft,
                       int64_t hop)
{
  if (function < 0 || function >= kOnsetFunctions) return fail(ctx, "function (metric) must be in [0, 9]");
  if (filterSize < 1 || filterSize > kOnsetMaxFilter || (filterSize % 2) == 0)
    return fail(ctx, "filterSize must be odd and in [1, 101]");
  if (frameDelta < 0 || frameDelta > kOnsetMaxDelta) return fail(ctx, "frameDelta must be in [0, 8192]");
  return check_fft_settings(ctx, win, fft, hop);
}

int check_slice_params(fluhip_ctx* ctx, double threshold, int64_t minSlice)
{
  if (!(threshold >= 0.0)) return fail(ctx, "threshold must be >= 0");
  if (minSlice < 0) return fail(ctx, "minSliceLength must be >= 0");
  return FLUHIP_OK;
}

// the frames of `nb` equal-length signals on the device: frame i's window starts at sample base + i hop, the second
// transform of a frame-delta form frameDelta samples on.  The callers lay the signals out with their zeros around them
// (onset_padded_length) so that EVERY frame lies inside its row.  (The layout dates from when the STFT kernels' clamped
// gather loaded one sample outside the row for a frame that lay wholly outside it; the gather's loads now stay inside
// [0, n) for any frame, frame_window.h, and the zeros are kept because the kernels' arithmetic and timing rest on them.)
struct OnsetRun
{
  fluhip_ctx* ctx;
  const float* a32;
  const double* a64;
  int64_t n, stride, base;
  int64_t win, fft, hop, T;
  int function;
  int64_t frameDelta;
};

// samples of a row that holds `lead` zeros, the n samples and every frame [i hop, i hop + lead') of T, lead' = win + d
int64_t onset_padded_length(int64_t lead, int64_t n, int64_t T, int64_t hop, int64_t window)
{
  return std::max(lead + n, (T - 1) * hop + window);
}

int check_onset_range(fluhip_ctx* ctx, int64_t n, int64_t base, int64_t T, int64_t win, int64_t hop, int64_t frameDelta)
{
  if (T > INT32_MAX / 4) return fail(ctx, "too many frames");
  // every sample index a launch forms stays inside int32
  if (n > INT32_MAX / 2 || hop > INT32_MAX / 4 || T > (INT32_MAX / 2 - win - frameDelta - std::llabs(base)) / hop)
    return fail(ctx, "signal too long");
  return FLUHIP_OK;
}

// the spectra of frames f0 .. f0 + rows - 1 of buffers b0 .. b0 + nb - 1, each window `extra` samples on
int onset_stft(const OnsetRun& r, const StftSetup& st, int64_t nb, int64_t b0, int64_t f0, int64_t rows, int64_t extra,
               double* spec)
{
  StftArgs sa = st.args(r.a32 ? r.a32 + b0 * r.stride : nullptr, r.a64 ? r.a64 + b0 * r.stride : nullptr, r.n, r.stride, nb,
                        rows, r.base + f0 * r.hop + extra);
  sa.spec = spec; sa.specStride = rows * st.F * 2;
  return st.launch(r.ctx, sa);
}

// raw [nb][T] (device): OnsetDetectionFunctions::processFrame's function value of every frame
int onset_raw_dev(const OnsetRun& r, int64_t nb, double* raw)
{
  fluhip_ctx* ctx = r.ctx;
  hipStream_t s = ctx->stream;
  const OnsetPlan plan = onset_plan(r.fft, r.win, r.function, r.frameDelta);
  const int64_t F = r.fft / 2 + 1, T = r.T;
  StftSetup st;
  int rc = stft_setup(ctx, r.win, r.fft, r.hop, &st);
  if (rc) return rc;
  if (plan.form == kOnsetFormOnChip)
  {
    // one launch over all buffers, no workspace: the spectra stay in the LDS (kernels_onset_fused.hip, onset_fused_kernel)
    StftArgs sa = st.args(r.a32, r.a64, r.n, r.stride, nb, T, r.base);
    OnsetFusedArgs o;
    o.function = r.function; o.history = plan.history;
    o.delta = plan.transforms == 2 ? (int) r.frameDelta : 0;
    o.T = (int) T;
    const int64_t per = std::max<int64_t>(1, ((int64_t) 1 << 30) / ((T + kOnsetRun - 1) / kOnsetRun)); // workgroups per launch
    for (int64_t b0 = 0; b0 < nb; b0 += per)
    {
      sa.B = (int) std::min(per, nb - b0);
      if (r.a32) sa.audio = r.a32 + b0 * r.stride;
      if (r.a64) sa.audio64 = r.a64 + b0 * r.stride;
      o.raw = raw + b0 * T;
      if (!launch_onset_fused(sa, o, s)) return fail(ctx, "internal error: no on-chip onset form for this shape");
      HIPCHK(ctx, hipGetLastError());
    }
    return FLUHIP_OK;
  }
  // rows of spectra a round holds: whole buffers when one fits, else runs of one buffer's frames behind their halo
  const int64_t perRow = F * 2 * plan.transforms;
  const int64_t rowsCap = std::max<int64_t>(plan.history + 1, kSpecCapDoubles / perRow);
  const bool whole = T <= rowsCap;
  const int64_t per = whole ? std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nb, 65535), rowsCap / T)) : 1;
  const int64_t run = whole ? T : rowsCap - plan.history;
  const int64_t rowsMax = whole ? T : rowsCap;
  DevBuf spec, spec2;
  DEV_ALLOC(ctx, "onset", spec, (size_t) (per * rowsMax * F * 2) * sizeof(double), false);
  if (plan.transforms == 2) DEV_ALLOC(ctx, "onset", spec2, (size_t) (per * rowsMax * F * 2) * sizeof(double), false);
  for (int64_t b0 = 0; b0 < nb; b0 += per)
  {
    const int64_t cb = std::min(per, nb - b0);
    for (int64_t t0 = 0; t0 < T; t0 += run)
    {
      const int64_t nt = std::min(run, T - t0);
      const int64_t f0 = std::max<int64_t>(0, t0 - plan.history);
      const int64_t rows = t0 + nt - f0;
      if ((rc = onset_stft(r, st, cb, b0, f0, rows, 0, spec.as<double>()))) return rc;
      if (plan.transforms == 2 && (rc = onset_stft(r, st, cb, b0, f0, rows, r.frameDelta, spec2.as<double>()))) return rc;
      OnsetReduceArgs a;
      a.spec = spec.as<double>(); a.spec2 = plan.transforms == 2 ? spec2.as<double>() : nullptr;
      a.specStride = rows * F * 2;
      a.F = (int) F; a.function = r.function; a.history = plan.history;
      a.f0 = (int) f0; a.t0 = (int) t0; a.nt = (int) nt; a.T = (int) T;
      a.count = cb; a.raw = raw + b0 * T;
      launch_onset_reduce(a, s);
      HIPCHK(ctx, hipGetLastError());
    }
  }
  return FLUHIP_OK;
}

int onset_f64_impl(fluhip_ctx* ctx, const double* signal, int64_t count, int64_t n, int64_t ld, int64_t T, int64_t win,
                   int64_t fft, int64_t hop, int function, int64_t filterSize, int64_t frameDelta, bool slices,
                   double threshold, int64_t minSlice, double* raw, double* filtered, unsigned char* det, int64_t* counts)
{
  int rc = check_onset_params(ctx, function, filterSize, frameDelta, win, fft, hop);
  if (rc) return rc;
  if (slices && (rc = check_slice_params(ctx, threshold, minSlice))) return rc;
  if (!signal || (slices && (!det || !counts))) return fail(ctx, "null buffer");
  if (count < 1 || n < 1 || T < 1) return fail(ctx, "need at least one signal, one sample and one frame");
  if (ld < n) return fail(ctx, "signal stride below the number of samples");
  if ((rc = check_onset_range(ctx, n, 0, T, win, hop, frameDelta))) return rc;
  const int64_t d = onset_uses_delta(function, frameDelta) ? frameDelta : 0;
  const int64_t np = onset_padded_length(0, n, T, hop, win + d); // zeros behind the signal up to the last frame's end
  if (count > (INT64_MAX / 64) / std::max(T, np)) return fail(ctx, "batch too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // buffers per round: the signals of a round stay below 1 GiB on the device
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(count, kSpecCapDoubles / np));
  DevBuf dSig, dRaw, dFilt, dDet, dCnt;
  DEV_ALLOC(ctx, "onset", dSig, (size_t) (chunk * np) * sizeof(double), true); // (only the first n samples of a row are ever written)
  DEV_ALLOC(ctx, "onset", dRaw, (size_t) (chunk * T) * sizeof(double), false);
  DEV_ALLOC(ctx, "onset", dFilt, (size_t) (chunk * T) * sizeof(double), false);
  if (slices)
  {
    DEV_ALLOC(ctx, "onset", dDet, (size_t) (chunk * T), false);
    DEV_ALLOC(ctx, "onset", dCnt, (size_t) chunk * sizeof(int64_t), false);
  }
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    HIPCHK(ctx, hipMemcpy2DAsync(dSig.p, (size_t) np * sizeof(double), signal + b0 * ld, (size_t) ld * sizeof(double),
                                 (size_t) n * sizeof(double), (size_t) nb, hipMemcpyDefault, s));
    OnsetRun r{ctx, nullptr, dSig.as<double>(), np, np, 0, win, fft, hop, T, function, frameDelta};
    if ((rc = onset_raw_dev(r, nb, dRaw.as<double>()))) return rc;
    launch_onset_filter(dRaw.as<double>(), dFilt.as<double>(), (int) T, nb, (int) filterSize, s);
    if (slices)
      launch_onset_detect(dFilt.as<double>(), (int) T, nb, threshold, (int) std::min<int64_t>(minSlice, INT32_MAX),
                          dDet.as<unsigned char>(), dCnt.as<int64_t>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    const size_t nbytes = (size_t) (nb * T) * sizeof(double);
    if (raw && (rc = copy_to_host(ctx, raw + b0 * T, nbytes, dRaw.p, nbytes, nbytes, 1, s))) return rc;
    if (filtered && (rc = copy_to_host(ctx, filtered + b0 * T, nbytes, dFilt.p, nbytes, nbytes, 1, s))) return rc;
    if (slices)
    {
      HIPCHK(ctx, hipMemcpyAsync(det + b0 * T, dDet.p, (size_t) (nb * T), hipMemcpyDeviceToHost, s));
      HIPCHK(ctx, hipMemcpyAsync(counts + b0, dCnt.p, (size_t) nb * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

int check_client(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n)
{
  if (!audio) return fail(ctx, "null buffer");
  if (count < 1) return fail(ctx, "need at least one buffer");
  if (n < 1) return fail(ctx, "not enough frames");
  return FLUHIP_OK;
}

int bufonsetslice_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t startFrame,
                       int function, double threshold, int64_t minSlice, int64_t filterSize, int64_t frameDelta, int64_t win,
                       int64_t fft, int64_t hop, int64_t* indices, int64_t capacity, int64_t* counts)
{
  int rc = check_onset_params(ctx, function, filterSize, frameDelta, win, fft, hop);
  if (rc) return rc;
  if ((rc = check_slice_params(ctx, threshold, minSlice))) return rc;
  if ((rc = check_client(ctx, audio, count, n))) return rc;
  if (!counts || (!indices && capacity > 0)) return fail(ctx, "null buffer");
  if (channels < 1) return fail(ctx, "need at least one channel");
  if (capacity < 0) return fail(ctx, "negative capacity");
  // Slicing::process (:675-723): the client's latency -- one hop -- of zeros behind the input, rounded up to whole host
  // vectors of 64; a frame fires at every multiple of hop below that length and holds the win + d samples that END there
  const int64_t d = onset_uses_delta(function, frameDelta) ? frameDelta : 0;
  const int64_t latency = hop;
  const int64_t T = slice_frames(n, hop, latency).T;
  if ((rc = check_onset_range(ctx, n, -(win + d), T, win, hop, d))) return rc;
  const int64_t lead = win + d, np = onset_padded_length(lead, n, T, hop, win + d);
  if (count > (INT64_MAX / 64) / std::max(T, np) / channels) return fail(ctx, "batch too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(count, 2 * kSpecCapDoubles / (np * channels)));
  DevBuf dIn, dMono, dPad, dRaw, dFilt, dDet, dCnt;
  DEV_ALLOC(ctx, "onset", dPad, (size_t) (chunk * np) * sizeof(float), true); // rows of [lead zeros][mono sum][zeros]; only the sum is written
  if (channels > 1)
  {
    DEV_ALLOC(ctx, "onset", dIn, (size_t) (chunk * channels * n) * sizeof(float), false);
    DEV_ALLOC(ctx, "onset", dMono, (size_t) (chunk * n) * sizeof(float), false);
  }
  DEV_ALLOC(ctx, "onset", dRaw, (size_t) (chunk * T) * sizeof(double), false);
  DEV_ALLOC(ctx, "onset", dFilt, (size_t) (chunk * T) * sizeof(double), false);
  DEV_ALLOC(ctx, "onset", dDet, (size_t) (chunk * T), false);
  DEV_ALLOC(ctx, "onset", dCnt, (size_t) chunk * sizeof(int64_t), false);
  std::vector<unsigned char> det((size_t) (count * T));
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    const float* mono = audio + b0 * n;
    if (channels > 1)
    {
      HIPCHK(ctx, hipMemcpyAsync(dIn.p, audio + b0 * channels * n, (size_t) (nb * channels * n) * sizeof(float), hipMemcpyDefault, s));
      launch_mono_sum_f32(dIn.as<float>(), (int) channels, n, nb, dMono.as<float>(), s);
      mono = dMono.as<float>();
    }
    HIPCHK(ctx, hipMemcpy2DAsync(dPad.as<float>() + lead, (size_t) np * sizeof(float), mono, (size_t) n * sizeof(float),
                                 (size_t) n * sizeof(float), (size_t) nb, hipMemcpyDefault, s));
    OnsetRun r{ctx, dPad.as<float>(), nullptr, np, np, 0, win, fft, hop, T, function, frameDelta};
    if ((rc = onset_raw_dev(r, nb, dRaw.as<double>()))) return rc;
    launch_onset_filter(dRaw.as<double>(), dFilt.as<double>(), (int) T, nb, (int) filterSize, s);
    launch_onset_detect(dFilt.as<double>(), (int) T, nb, threshold, (int) std::min<int64_t>(minSlice, INT32_MAX),
                        dDet.as<unsigned char>(), dCnt.as<int64_t>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(det.data() + b0 * T, dDet.p, (size_t) (nb * T), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  for (int64_t b = 0; b < count; b++)
    counts[b] = detections_to_indices(det.data() + b * T, T, hop, latency, n, startFrame, indices ? indices + b * capacity : nullptr,
                                      capacity);
  return FLUHIP_OK;
}

int bufonsetfeature_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int function, int64_t filterSize,
                         int64_t frameDelta, int64_t win, int64_t fft, int64_t hop, int paddingMode, float* out,
                         int64_t* framesOut)
{
  int rc = check_onset_params(ctx, function, filterSize, frameDelta, win, fft, hop);
  if (rc) return rc;
  if ((rc = check_client(ctx, audio, count, n))) return rc;
  if (paddingMode < 0 || paddingMode > 2) return fail(ctx, "padding mode must be 0 (None), 1 (Default) or 2 (Full)");
  // StreamingControl::process (:564-579, 642-656): the input sits userPad into the padded signal, whose analysis window is
  // win (OnsetFeatureClient::analysisSettings; the frame delta is not part of it); frame j fires with the j-th host vector
  // of hop samples and holds the win + d samples that END where that vector begins; the first latency / hop = 1 frame is
  // dropped
  const int64_t d = onset_uses_delta(function, frameDelta) ? frameDelta : 0;
  if (hop > INT32_MAX / 4 || n > INT32_MAX / 2) return fail(ctx, "signal too long");
  const ControlFrames g = control_frames(n, win, hop, paddingMode, hop);
  const int64_t userPad = g.userPad, T = g.T, latencyHops = g.latencyHops, keep = g.keep;
  if (g.paddedLength < win || keep < 1) return fail(ctx, "not enough frames");
  if ((rc = check_onset_range(ctx, n, -(win + d + userPad), T, win, hop, d))) return rc;
  const int64_t lead = win + d + userPad, np = onset_padded_length(lead, n, T, hop, win + d);
  if (count > (INT64_MAX / 64) / std::max(T, np)) return fail(ctx, "batch too large");
  if (framesOut) *framesOut = keep;
  if (!out) return FLUHIP_OK; // size query
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(count, 2 * kSpecCapDoubles / np));
  DevBuf dPad, dRaw, dFilt, dOut;
  DEV_ALLOC(ctx, "onset", dPad, (size_t) (chunk * np) * sizeof(float), true); // rows of [lead zeros][input][zeros]; only the input is written
  DEV_ALLOC(ctx, "onset", dRaw, (size_t) (chunk * T) * sizeof(double), false);
  DEV_ALLOC(ctx, "onset", dFilt, (size_t) (chunk * T) * sizeof(double), false);
  DEV_ALLOC(ctx, "onset", dOut, (size_t) (chunk * keep) * sizeof(float), false);
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    HIPCHK(ctx, hipMemcpy2DAsync(dPad.as<float>() + lead, (size_t) np * sizeof(float), audio + b0 * n, (size_t) n * sizeof(float),
                                 (size_t) n * sizeof(float), (size_t) nb, hipMemcpyDefault, s));
    OnsetRun r{ctx, dPad.as<float>(), nullptr, np, np, 0, win, fft, hop, T, function, frameDelta};
    if ((rc = onset_raw_dev(r, nb, dRaw.as<double>()))) return rc;
    launch_onset_filter(dRaw.as<double>(), dFilt.as<double>(), (int) T, nb, (int) filterSize, s);
    launch_curve_to_f32(dFilt.as<double>(), (int) T, (int) latencyHops, (int) keep, nb, dOut.as<float>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out + b0 * keep, dOut.p, (size_t) (nb * keep) * sizeof(float), hipMemcpyDefault, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_onset_plan(fluhip_ctx* ctx, int64_t fft, int64_t win, int function, int64_t frame_delta, int64_t* out4)
{
  if (!ctx) return FLUHIP_ERROR;
  if (!out4) return fail(ctx, "null buffer");
  const int rc = check_onset_params(ctx, function, 1, frame_delta, win, fft, 1);
  if (rc) return rc;
  const OnsetPlan p = onset_plan(fft, win, function, frame_delta);
  out4[0] = p.form;
  out4[1] = p.history;
  out4[2] = p.transforms;
  out4[3] = p.run;
  return FLUHIP_OK;
}

int fluhip_onset_curve_f64(fluhip_ctx* ctx, const double* signal, int64_t count, int64_t n, int64_t ld, int64_t T, int64_t win,
                           int64_t fft, int64_t hop, int function, int64_t filter_size, int64_t frame_delta, double* raw,
                           double* filtered)
{
  return guarded(ctx, [&] {
    return onset_f64_impl(ctx, signal, count, n, ld, T, win, fft, hop, function, filter_size, frame_delta, false, 0.0, 0, raw,
                          filtered, nullptr, nullptr);
  });
}

int fluhip_onset_slices_f64(fluhip_ctx* ctx, const double* signal, int64_t count, int64_t n, int64_t ld, int64_t T, int64_t win,
                            int64_t fft, int64_t hop, int function, int64_t filter_size, int64_t frame_delta, double threshold,
                            int64_t min_slice, unsigned char* det, int64_t* counts, double* filtered)
{
  return guarded(ctx, [&] {
    return onset_f64_impl(ctx, signal, count, n, ld, T, win, fft, hop, function, filter_size, frame_delta, true, threshold,
                          min_slice, nullptr, filtered, det, counts);
  });
}

int fluhip_bufonsetslice_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n,
                             int64_t start_frame, int function, double threshold, int64_t min_slice, int64_t filter_size,
                             int64_t frame_delta, int64_t win, int64_t fft, int64_t hop, int64_t* indices, int64_t capacity,
                             int64_t* counts)
{
  return guarded(ctx, [&] {
    return bufonsetslice_impl(ctx, audio, count, channels, n, start_frame, function, threshold, min_slice, filter_size,
                              frame_delta, win, fft, hop, indices, capacity, counts);
  });
}

int fluhip_bufonsetfeature_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int function,
                               int64_t filter_size, int64_t frame_delta, int64_t win, int64_t fft, int64_t hop,
                               int padding_mode, float* out, int64_t* frames_out)
{
  return guarded(ctx, [&] {
    return bufonsetfeature_impl(ctx, audio, count, n, function, filter_size, frame_delta, win, fft, hop, padding_mode, out,
                                frames_out);
  });
}

} // extern "C"
