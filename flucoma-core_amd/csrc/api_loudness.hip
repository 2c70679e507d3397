// api_loudness.hip -- C ABI of BufLoudness:
//   fluhip_loudness_frames_f64   algorithm::Loudness::processFrame on the frames of given signals, the filter and the
//                                interpolator carried from frame 0 (algorithms/public/Loudness.hpp:43-61)
//   fluhip_bufloudness_f32       NRTLoudnessClient  clients/rt/LoudnessClient.hpp, common/FluidNRTClientWrapper.hpp:551-660
//   fluhip_debug_loudness_plan
// The kernels are in kernels_loudness.hip (fluhip_loudness.h).  What depends on nothing per frame -- the filter's
// coefficients, the frame-length transition M as double-doubles, the interpolator's taps -- is built once per call, on the host,
// and travels as kernel arguments.  Every device buffer is a DevBuf of the call; no event, no stream is taken.
#include "api_internal.h"
#include "client_frames.h"
#include "fluhip_loudness.h"

namespace {

constexpr int64_t kWorkCapBytes = (int64_t) 1 << 30;  // 1 GiB of samples and workspace per round
constexpr int64_t kRoundMaxFrames = (int64_t) 1 << 24; // (the filter launches' grid: frames / run workgroups)
constexpr int64_t kFrameBytes = (2 * kLoudnessState + 2) * (int64_t) sizeof(double); // q, entering state, result

int failn(fluhip_ctx* ctx, const char* msg) { return ctx ? fail(ctx, msg) : (int) FLUHIP_ERROR; }

int check_loudness_params(fluhip_ctx* ctx, int64_t win, int64_t hop, int kWeighting, int truePeak, double sampleRate)
{
  if (win < 1 || win > kLoudnessMaxWin) return failn(ctx, "windowSize must be in [1, 32768]");
  if (hop < 1) return failn(ctx, "hopSize must be at least 1");
  if (kWeighting < 0 || kWeighting > 1) return failn(ctx, "kWeighting must be 0 (Off) or 1 (On)");
  if (truePeak < 0 || truePeak > 1) return failn(ctx, "truePeak must be 0 (Off) or 1 (On)");
  if (!(sampleRate > 0.0) || !std::isfinite(sampleRate)) return failn(ctx, "sample rate must be positive");
  return FLUHIP_OK;
}

// what one call builds on the host
struct LoudnessWork
{
  LoudnessPlan plan;
  KWeighting k;
  LoudnessTransition M;
  InterpolatorTaps taps;
  int kWeighting = 1, truePeak = 1;
  DevBuf q, st, res;
};

int loudness_work_init(LoudnessWork& w, fluhip_ctx* ctx, int64_t win, int64_t hop, int kWeighting, int truePeak, double sampleRate,
                       int64_t framesMax)
{
  w.plan = loudness_plan(win, hop, sampleRate);
  if (w.plan.run < 1 || w.plan.ldsBytes() > kLoudnessLdsBudget) return fail(ctx, "internal error: the loudness plan needs more LDS than a workgroup may have");
  w.kWeighting = kWeighting;
  w.truePeak = truePeak;
  w.k = kweighting_coefficients(sampleRate);
  if (kWeighting) w.M = frame_transition(w.k, win);
  w.taps = interpolator_taps(truePeak ? w.plan.factor : 1);
  if (kWeighting)
  {
    DEV_ALLOC(ctx, "loudness", w.q, (size_t) (framesMax * kLoudnessState) * sizeof(double), false);
    DEV_ALLOC(ctx, "loudness", w.st, (size_t) (framesMax * kLoudnessState) * sizeof(double), false);
  }
  DEV_ALLOC(ctx, "loudness", w.res, (size_t) (framesMax * 2) * sizeof(double), false);
  return FLUHIP_OK;
}

// res [B T][2] (device) of every frame of the rows `p`
int loudness_round(LoudnessWork& w, fluhip_ctx* ctx, const LoudnessFrames& p)
{
  hipStream_t s = ctx->stream;
  double* res = w.res.as<double>();
  {
    ProfScope ps(ctx, 2); // (the feature kernels' class: one record per round, uploads and the copy back outside it)
    if (w.kWeighting)
    {
      launch_loudness_zero_state(p, w.plan, w.k, w.q.as<double>(), s);
      launch_loudness_scan(w.q.as<double>(), p.B, p.T, w.M, w.st.as<double>(), s);
      launch_loudness_filtered(p, w.plan, w.k, w.st.as<double>(), res, s);
    }
    launch_loudness_peak(p, w.taps, w.truePeak, !w.kWeighting, res, s);
  }
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

// buffers a round holds: their samples and the per-frame workspace within the cap, at least one
int64_t buffers_per_round(int64_t count, int64_t rowBytes, int64_t T)
{
  const int64_t per = rowBytes + T * kFrameBytes;
  int64_t nb = std::min(count, std::max<int64_t>(1, kWorkCapBytes / per));
  nb = std::min(nb, std::max<int64_t>(1, kRoundMaxFrames / T));
  return nb;
}

int loudness_frames_impl(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t win, int64_t hop, int kWeighting,
                         int truePeak, double sampleRate, double* out)
{
  int rc = check_loudness_params(ctx, win, hop, kWeighting, truePeak, sampleRate);
  if (rc) return rc;
  if (!x || !out) return fail(ctx, "null buffer");
  if (count < 1) return fail(ctx, "need at least one buffer");
  if (n < win) return fail(ctx, "not enough frames");
  const int64_t T = 1 + (n - win) / hop;
  if (n > INT64_MAX / 256 / count || T > kRoundMaxFrames) return fail(ctx, "signal too long");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t perB = buffers_per_round(count, n * (int64_t) sizeof(double), T);
  LoudnessWork w;
  if ((rc = loudness_work_init(w, ctx, win, hop, kWeighting, truePeak, sampleRate, perB * T))) return rc;
  DevBuf dX;
  DEV_ALLOC(ctx, "loudness", dX, (size_t) (perB * n) * sizeof(double), false);
  for (int64_t b0 = 0; b0 < count; b0 += perB)
  {
    const int64_t nb = std::min(perB, count - b0);
    HIPCHK(ctx, hipMemcpyAsync(dX.p, x + b0 * n, (size_t) (nb * n) * sizeof(double), hipMemcpyDefault, s));
    const LoudnessFrames p{nullptr, dX.as<double>(), n, nb, T, win, hop};
    if ((rc = loudness_round(w, ctx, p))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    const size_t bytes = (size_t) (nb * T * 2) * sizeof(double);
    if ((rc = copy_to_host(ctx, out + b0 * T * 2, bytes, w.res.p, bytes, bytes, 1, s))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

int bufloudness_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t hop, int paddingMode,
                     int select, int kWeighting, int truePeak, double sampleRate, float* out, int64_t* framesOut)
{
  int rc = check_loudness_params(ctx, win, hop, kWeighting, truePeak, sampleRate);
  if (rc) return rc;
  if (select < 1 || select > 3)
    return fail(ctx, select == 0 ? "select is empty: choose among loudness (1) and peak (2)" : "select must be in [1, 3]");
  if (paddingMode < 0 || paddingMode > 2) return fail(ctx, "padding mode must be 0 (None), 1 (Default) or 2 (Full)");
  if (!audio) return fail(ctx, "null buffer");
  if (count < 1) return fail(ctx, "need at least one buffer");
  if (n < 1) return fail(ctx, "not enough frames");
  if (n > INT32_MAX / 2 || hop > INT32_MAX / 4) return fail(ctx, "signal too long");
  // StreamingControl::process (cc/FluidNRTClientWrapper.hpp:564-579, 604-656): the input sits userPad into the padded signal,
  // the client's latency (= windowSize, LoudnessClient.hpp:120) behind it.  The host vector is one hop and the buffered
  // process fires one frame per vector, the window that ends where the vector begins: analysis frame j holds the win samples
  // from j hop - win of the padded signal.  client.reset runs once per channel; EVERY frame goes through the filter and the
  // interpolator, and the first latency / hop results are dropped afterwards
  // (Full padding is win - hop samples: with hop > win the reference copies its input to a negative offset; refused)
  if (paddingMode == 2 && hop > win) return fail(ctx, "padding mode 2 (Full) needs hopSize <= windowSize");
  const ControlFrames g = control_frames(n, win, hop, paddingMode, win);
  const int64_t T = g.T, keep = g.keep;
  if (keep < 1) return fail(ctx, "not enough frames");
  if (T > kRoundMaxFrames) return fail(ctx, "signal too long");
  // rows of [win zeros][userPad zeros][input][zeros] so that every frame lies inside its row: frame j starts at sample j hop
  const int64_t lead = win + g.userPad;
  const int64_t np = std::max(lead + n, (T - 1) * hop + win);
  const int nsel = (select & 1) + (select >> 1 & 1);
  if (count > (INT64_MAX / 256) / std::max(T, np)) return fail(ctx, "batch too large");
  if (framesOut) *framesOut = keep;
  if (!out) return FLUHIP_OK; // size query
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t perB = buffers_per_round(count, np * (int64_t) sizeof(float), T);
  LoudnessWork w;
  if ((rc = loudness_work_init(w, ctx, win, hop, kWeighting, truePeak, sampleRate, perB * T))) return rc;
  DevBuf dPad, dOut;
  DEV_ALLOC(ctx, "loudness", dPad, (size_t) (perB * np) * sizeof(float), true); // only the input is ever written
  DEV_ALLOC(ctx, "loudness", dOut, (size_t) (perB * nsel * keep) * sizeof(float), false);
  for (int64_t b0 = 0; b0 < count; b0 += perB)
  {
    const int64_t nb = std::min(perB, count - b0);
    HIPCHK(ctx, hipMemcpy2DAsync(dPad.as<float>() + lead, (size_t) np * sizeof(float), audio + b0 * n, (size_t) n * sizeof(float),
                                 (size_t) n * sizeof(float), (size_t) nb, hipMemcpyDefault, s));
    const LoudnessFrames p{dPad.as<float>(), nullptr, np, nb, T, win, hop};
    if ((rc = loudness_round(w, ctx, p))) return rc;
    launch_loudness_select(w.res.as<double>(), nb, T, g.latencyHops, keep, select, dOut.as<float>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out + b0 * nsel * keep, dOut.p, (size_t) (nb * nsel * keep) * sizeof(float), hipMemcpyDefault, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_loudness_plan(fluhip_ctx* ctx, int64_t win, int64_t hop, double sample_rate, int64_t* out4)
{
  if (!out4) return failn(ctx, "null buffer");
  const int rc = check_loudness_params(ctx, win, hop, 1, 1, sample_rate);
  if (rc) return rc;
  const LoudnessPlan p = loudness_plan(win, hop, sample_rate);
  out4[0] = p.form;
  out4[1] = p.run;
  out4[2] = p.factor;
  out4[3] = p.history;
  return FLUHIP_OK;
}

int fluhip_loudness_frames_f64(fluhip_ctx* ctx, const double* x, int64_t count, int64_t n, int64_t win, int64_t hop, int k_weighting,
                               int true_peak, double sample_rate, double* out)
{
  return guarded(ctx, [&] { return loudness_frames_impl(ctx, x, count, n, win, hop, k_weighting, true_peak, sample_rate, out); });
}

int fluhip_bufloudness_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t hop, int padding_mode,
                           int select, int k_weighting, int true_peak, double sample_rate, float* out, int64_t* frames_out)
{
  return guarded(ctx, [&] {
    return bufloudness_impl(ctx, audio, count, n, win, hop, padding_mode, select, k_weighting, true_peak, sample_rate, out, frames_out);
  });
}

} // extern "C"
