// api_amp.hip -- C ABI of BufAmpSlice / BufAmpFeature:
//   fluhip_amp_envelope_f64    algorithm::Envelope::processSample              algorithms/public/Envelope.hpp:36-61
//   fluhip_amp_slices_f64      algorithm::EnvelopeSegmentation::processSample  algorithms/public/EnvelopeSegmentation.hpp:36-60
//   fluhip_bufampslice_f32     NRTAmpSliceClient    clients/rt/AmpSliceClient.hpp, common/FluidNRTClientWrapper.hpp:665-725
//   fluhip_bufampfeature_f32   NRTAmpFeatureClient  clients/rt/AmpFeatureClient.hpp, common/FluidNRTClientWrapper.hpp:466-548
//   fluhip_debug_amp_plan
// The kernels are in kernels_amp.hip (fluhip_amp.h).  What depends on nothing per sample -- the high-pass coefficients, the
// chunk transition M as double-doubles, the followers' coefficients -- is built once per call, on the host, and travels as
// kernel arguments.  Every device buffer is a DevBuf of the call; no event, no stream is taken.
#include "api_internal.h"
#include "client_frames.h"
#include "fluhip_amp.h"
#include "fluhip_env.h"
#include "fluhip_novelty.h" // launch_mono_sum_f32

namespace {

constexpr int64_t kWorkCapBytes = (int64_t) 1 << 30; // 1 GiB of samples and workspace per round

int failn(fluhip_ctx* ctx, const char* msg) { return ctx ? fail(ctx, msg) : (int) FLUHIP_ERROR; }

struct AmpParams
{
  int64_t fastUp, fastDown, slowUp, slowDown;
  double on, off, floorDb;
  int64_t minSlice;
  bool slice; // the thresholds and minSliceLength take part
};

bool in_db_range(double v) { return v >= -144.0 && v <= 144.0; } // (false for NaN)

// the reference's parameter table (AmpSliceClient.hpp:39-48): what it would clamp is refused
int check_amp_params(fluhip_ctx* ctx, const AmpParams& a)
{
  if (a.fastUp < 1) return failn(ctx, "fastRampUp must be at least 1");
  if (a.fastDown < 1) return failn(ctx, "fastRampDown must be at least 1");
  if (a.slowUp < 1) return failn(ctx, "slowRampUp must be at least 1");
  if (a.slowDown < 1) return failn(ctx, "slowRampDown must be at least 1");
  if (!in_db_range(a.floorDb)) return failn(ctx, "floor must be in [-144, 144]");
  if (!a.slice) return FLUHIP_OK;
  if (!in_db_range(a.on)) return failn(ctx, "onThreshold must be in [-144, 144]");
  if (!in_db_range(a.off)) return failn(ctx, "offThreshold must be in [-144, 144]");
  if (a.minSlice < 0) return failn(ctx, "minSliceLength must be >= 0");
  return FLUHIP_OK;
}

int check_hipass(fluhip_ctx* ctx, double hipass)
{
  if (!(hipass >= 0.0 && hipass <= 0.5)) return failn(ctx, "hipass (the cutoff as a fraction of the sample rate) must be in [0, 0.5]");
  return FLUHIP_OK;
}

// AmpSliceClient::process :84: min(highPassFreq / sampleRate, 0.5)
int client_hipass(fluhip_ctx* ctx, double highPassFreq, double sampleRate, double* hipass)
{
  if (!(highPassFreq >= 0.0) || !std::isfinite(highPassFreq)) return fail(ctx, "highPassFreq must be finite and >= 0");
  if (!(sampleRate > 0.0) || !std::isfinite(sampleRate)) return fail(ctx, "sample rate must be positive and finite");
  *hipass = std::min(highPassFreq / sampleRate, 0.5);
  return FLUHIP_OK;
}

// what one call builds on the host, and the workspaces of its rounds
struct AmpWork
{
  AmpHighPass hp;
  AmpTransition M;
  AmpFollow follow;
  DevBuf front, level;
};

int amp_work_init(AmpWork& w, fluhip_ctx* ctx, const AmpParams& a, double hipass, int64_t signals, int64_t n)
{
  w.hp = amp_highpass(hipass);
  if (w.hp.on) w.M = amp_transition(w.hp);
  // SlideUDFilter::updateCoeffs :19-23
  w.follow.fastUp = 1.0 / (double) a.fastUp;
  w.follow.fastDown = 1.0 / (double) a.fastDown;
  w.follow.slowUp = 1.0 / (double) a.slowUp;
  w.follow.slowDown = 1.0 / (double) a.slowDown;
  w.follow.floorDb = a.floorDb;
  w.follow.on = a.on;
  w.follow.off = a.off;
  w.follow.minSlice = a.minSlice;
  w.follow.detect = a.slice ? 1 : 0;
  static const int pair = ab_int("FLUHIP_AMP_PAIR", 1); // (always 1 in the production library)
  w.follow.pair = pair;
  DEV_ALLOC(ctx, "amp", w.front, (size_t) (signals * amp_front_doubles(n)) * sizeof(double), false);
  DEV_ALLOC(ctx, "amp", w.level, (size_t) (signals * n) * sizeof(double), false);
  return FLUHIP_OK;
}

// the envelope of the signals p stays in w.level (double); env32 / det / counts (device, may be null) as launch_amp_follow
int amp_round(AmpWork& w, fluhip_ctx* ctx, const AmpSignals& p, float* env32, unsigned char* det, int64_t* counts)
{
  hipStream_t s = ctx->stream;
  {
    ProfScope ps(ctx, 2); // (the feature kernels' class: one record per round, uploads and the copy back outside it)
    launch_amp_level(p, w.hp, w.M, w.follow.floorDb, w.front.as<double>(), w.level.as<double>(), s);
    launch_amp_follow(w.level.as<double>(), p.count, p.n, w.follow, w.level.as<double>(), env32, det, counts, s);
  }
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

// signals a round holds: `perSignal` bytes of samples, workspace and results each within the cap, at least one; whole groups of
// the follower kernel's 32 when there are that many (a round is never cut inside a signal)
int64_t signals_per_round(int64_t signals, int64_t perSignal)
{
  int64_t nb = std::min(signals, std::max<int64_t>(1, kWorkCapBytes / perSignal));
  if (nb >= kAmpSignals) nb -= nb % kAmpSignals;
  return nb;
}

int check_shape(fluhip_ctx* ctx, int64_t count, int64_t channels, int64_t n)
{
  if (count < 1) return fail(ctx, "count: need at least one buffer");
  if (channels < 1) return fail(ctx, "channels: need at least one channel");
  if (n < 1) return fail(ctx, "n: need at least one sample");
  if (n > INT64_MAX / 64 / count / channels) return fail(ctx, "batch too large");
  return FLUHIP_OK;
}

int amp_f64_impl(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t ld, const AmpParams& a, double hipass,
                 unsigned char* det, int64_t* counts, double* envelope)
{
  int rc = check_amp_params(ctx, a);
  if (rc) return rc;
  if ((rc = check_hipass(ctx, hipass))) return rc;
  if ((rc = check_shape(ctx, count, 1, n))) return rc;
  if (!x || (a.slice ? !counts : !envelope)) return fail(ctx, "null buffer");
  if (ld < n) return fail(ctx, "signal stride below the number of samples");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const bool wantDet = a.slice && det;
  const int64_t perSignal = n * (2 * (int64_t) sizeof(double) + (wantDet ? 1 : 0)) + amp_front_doubles(n) * (int64_t) sizeof(double);
  const int64_t perB = signals_per_round(count, perSignal);
  AmpWork w;
  if ((rc = amp_work_init(w, ctx, a, hipass, perB, n))) return rc;
  DevBuf dX, dDet, dCnt;
  DEV_ALLOC(ctx, "amp", dX, (size_t) (perB * n) * sizeof(double), false);
  if (wantDet) DEV_ALLOC(ctx, "amp", dDet, (size_t) (perB * n), false);
  if (a.slice) DEV_ALLOC(ctx, "amp", dCnt, (size_t) perB * sizeof(int64_t), false);
  for (int64_t b0 = 0; b0 < count; b0 += perB)
  {
    const int64_t nb = std::min(perB, count - b0);
    HIPCHK(ctx, hipMemcpy2DAsync(dX.p, (size_t) n * sizeof(double), x + b0 * ld, (size_t) ld * sizeof(double),
                                 (size_t) n * sizeof(double), (size_t) nb, hipMemcpyDefault, s));
    const AmpSignals p{nullptr, dX.as<double>(), n, nb, n};
    if ((rc = amp_round(w, ctx, p, nullptr, wantDet ? dDet.as<unsigned char>() : nullptr, a.slice ? dCnt.as<int64_t>() : nullptr)))
      return rc;
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    const size_t bytes = (size_t) (nb * n) * sizeof(double);
    if (envelope && (rc = copy_to_host(ctx, envelope + b0 * n, bytes, w.level.p, bytes, bytes, 1, s))) return rc;
    if (wantDet) HIPCHK(ctx, hipMemcpyAsync(det + b0 * n, dDet.p, (size_t) (nb * n), hipMemcpyDeviceToHost, s));
    if (a.slice) HIPCHK(ctx, hipMemcpyAsync(counts + b0, dCnt.p, (size_t) nb * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

int bufampslice_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t startFrame,
                     const AmpParams& a, double highPassFreq, double sampleRate, int64_t* indices, int64_t capacity, int64_t* counts)
{
  int rc = check_amp_params(ctx, a);
  if (rc) return rc;
  double hipass = 0;
  if ((rc = client_hipass(ctx, highPassFreq, sampleRate, &hipass))) return rc;
  if ((rc = check_shape(ctx, count, channels, n))) return rc;
  if (!audio || !counts || (!indices && capacity > 0)) return fail(ctx, "null buffer");
  if (capacity < 0) return fail(ctx, "negative capacity");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // Slicing::process (:675-723): the channels summed in float; the client's latency is 0, so no detection is moved or
  // merged at the front, and the zeros that fill the last host vector of 64 lie past n and never reach the output
  const int64_t perSignal = n * ((channels > 1 ? channels + 1 : 1) * (int64_t) sizeof(float) + (int64_t) sizeof(double) + 1) +
                            amp_front_doubles(n) * (int64_t) sizeof(double);
  const int64_t perB = signals_per_round(count, perSignal);
  AmpWork w;
  if ((rc = amp_work_init(w, ctx, a, hipass, perB, n))) return rc;
  DevBuf dIn, dMono, dDet;
  DEV_ALLOC(ctx, "amp", dIn, (size_t) (perB * channels * n) * sizeof(float), false);
  if (channels > 1) DEV_ALLOC(ctx, "amp", dMono, (size_t) (perB * n) * sizeof(float), false);
  DEV_ALLOC(ctx, "amp", dDet, (size_t) (perB * n), false);
  std::vector<unsigned char> det((size_t) (perB * n));
  for (int64_t b0 = 0; b0 < count; b0 += perB)
  {
    const int64_t nb = std::min(perB, count - b0);
    HIPCHK(ctx, hipMemcpyAsync(dIn.p, audio + b0 * channels * n, (size_t) (nb * channels * n) * sizeof(float), hipMemcpyDefault, s));
    const float* mono = dIn.as<float>();
    if (channels > 1)
    {
      launch_mono_sum_f32(dIn.as<float>(), (int) channels, n, nb, dMono.as<float>(), s);
      mono = dMono.as<float>();
    }
    const AmpSignals p{mono, nullptr, n, nb, n};
    if ((rc = amp_round(w, ctx, p, nullptr, dDet.as<unsigned char>(), nullptr))) return rc;
    HIPCHK(ctx, hipMemcpyAsync(det.data(), dDet.p, (size_t) (nb * n), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    for (int64_t b = 0; b < nb; b++) // spikesToTimes: hop 1, latency 0
      counts[b0 + b] = detections_to_indices(det.data() + b * n, n, 1, 0, n, startFrame,
                                             indices ? indices + (b0 + b) * capacity : nullptr, capacity);
  }
  return FLUHIP_OK;
}

int bufampfeature_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, const AmpParams& a,
                       double highPassFreq, double sampleRate, float* out)
{
  int rc = check_amp_params(ctx, a);
  if (rc) return rc;
  double hipass = 0;
  if ((rc = client_hipass(ctx, highPassFreq, sampleRate, &hipass))) return rc;
  if ((rc = check_shape(ctx, count, channels, n))) return rc;
  if (!audio || !out) return fail(ctx, "null buffer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // Streaming::process (:480-544): every channel on its own through a reset client, latency 0, numFrames x numChans out
  const int64_t signals = count * channels;
  const int64_t perSignal = n * (2 * (int64_t) sizeof(float) + (int64_t) sizeof(double)) + amp_front_doubles(n) * (int64_t) sizeof(double);
  const int64_t perB = signals_per_round(signals, perSignal);
  AmpWork w;
  if ((rc = amp_work_init(w, ctx, a, hipass, perB, n))) return rc;
  DevBuf dIn, dOut;
  DEV_ALLOC(ctx, "amp", dIn, (size_t) (perB * n) * sizeof(float), false);
  DEV_ALLOC(ctx, "amp", dOut, (size_t) (perB * n) * sizeof(float), false);
  for (int64_t b0 = 0; b0 < signals; b0 += perB)
  {
    const int64_t nb = std::min(perB, signals - b0);
    HIPCHK(ctx, hipMemcpyAsync(dIn.p, audio + b0 * n, (size_t) (nb * n) * sizeof(float), hipMemcpyDefault, s));
    const AmpSignals p{dIn.as<float>(), nullptr, n, nb, n};
    if ((rc = amp_round(w, ctx, p, dOut.as<float>(), nullptr, nullptr))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    const size_t bytes = (size_t) (nb * n) * sizeof(float);
    if ((rc = copy_to_host(ctx, out + b0 * n, bytes, dOut.p, bytes, bytes, 1, s))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_amp_plan(fluhip_ctx* ctx, double hipass, int64_t* out4)
{
  if (!out4) return failn(ctx, "null buffer");
  const int rc = check_hipass(ctx, hipass);
  if (rc) return rc;
  out4[0] = kAmpFormChunks;
  out4[1] = kAmpChunk;
  out4[2] = kAmpSignals;
  out4[3] = hipass > 0 ? 1 : 0;
  return FLUHIP_OK;
}

int fluhip_amp_envelope_f64(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t ld, int64_t fast_up,
                            int64_t fast_down, int64_t slow_up, int64_t slow_down, double floor_db, double hipass, double* out)
{
  return guarded(ctx, [&] {
    const AmpParams a{fast_up, fast_down, slow_up, slow_down, 0.0, 0.0, floor_db, 0, false};
    return amp_f64_impl(ctx, x, count, n, ld, a, hipass, nullptr, nullptr, out);
  });
}

int fluhip_amp_slices_f64(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t ld, int64_t fast_up, int64_t fast_down,
                          int64_t slow_up, int64_t slow_down, double on, double off, double floor_db, int64_t min_slice,
                          double hipass, unsigned char* det, int64_t* counts, double* envelope)
{
  return guarded(ctx, [&] {
    const AmpParams a{fast_up, fast_down, slow_up, slow_down, on, off, floor_db, min_slice, true};
    return amp_f64_impl(ctx, x, count, n, ld, a, hipass, det, counts, envelope);
  });
}

int fluhip_bufampslice_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t start_frame,
                           int64_t fast_up, int64_t fast_down, int64_t slow_up, int64_t slow_down, double on, double off,
                           double floor_db, int64_t min_slice, double high_pass_freq, double sample_rate, int64_t* indices,
                           int64_t capacity, int64_t* counts)
{
  return guarded(ctx, [&] {
    const AmpParams a{fast_up, fast_down, slow_up, slow_down, on, off, floor_db, min_slice, true};
    return bufampslice_impl(ctx, audio, count, channels, n, start_frame, a, high_pass_freq, sample_rate, indices, capacity, counts);
  });
}

int fluhip_bufampfeature_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t fast_up,
                             int64_t fast_down, int64_t slow_up, int64_t slow_down, double floor_db, double high_pass_freq,
                             double sample_rate, float* out)
{
  return guarded(ctx, [&] {
    const AmpParams a{fast_up, fast_down, slow_up, slow_down, 0.0, 0.0, floor_db, 0, false};
    return bufampfeature_impl(ctx, audio, count, channels, n, a, high_pass_freq, sample_rate, out);
  });
}

} // extern "C"
