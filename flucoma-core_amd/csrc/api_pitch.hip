// api_pitch.hip -- C ABI of BufPitch:
//   fluhip_pitch_frames_f64       algorithm::YINFFT / HPS / CepstrumF0 ::processFrame on given magnitudes
//   fluhip_debug_pitch_curve_f64  the curve each of them searches (normalised yin, harmonic product, cepstrum)
//   fluhip_bufpitch_f32           NRTPitchClient  clients/rt/PitchClient.hpp, common/FluidNRTClientWrapper.hpp:551-660
//   fluhip_debug_pitch_plan
// fft 1024 / 2048 / 4096 with an even window run the on-chip form (pitch_fused_kernel, kernels_pitch_fused.hip): one launch from
// the samples to (f0, confidence), or to the log-magnitudes of the cepstrum.  Everything else, and the two entry points
// that are given magnitudes, run the two-pass form: the kernels are in kernels_pitch.hip (fluhip_pitch.h); the magnitudes
// come from launch_stft, YinFFT's second transform is the same launch over the symmetric squared magnitudes (window = hop
// = fft, a table of ones as the window).  In both forms the cepstrum is cross_gemm_kernel (fluhip_cross.h) over the rows
// of the DCT table that are read.  Every device buffer is a DevBuf of the call; no event, no stream is taken.
#include "api_internal.h"
#include "fluhip_cross.h"
#include "fluhip_env.h"
#include "fluhip_pitch.h"

namespace {

constexpr int64_t kWorkCapDoubles = (int64_t) 1 << 27; // 1 GiB of workspace per round
constexpr int64_t kRoundMaxFrames = (int64_t) 1 << 21; // (the GEMM's grid: frames / 64 workgroup rows)

int check_pitch_params(fluhip_ctx* ctx, int algorithm, double minFreq, double maxFreq, double sampleRate, int64_t fft)
{
  if (algorithm < 0 || algorithm >= kPitchAlgorithms)
    return fail(ctx, "algorithm must be 0 (Cepstrum), 1 (Harmonic Product Spectrum) or 2 (YinFFT)");
  if (!(minFreq >= 0.0 && minFreq <= 10000.0)) return fail(ctx, "minFreq must be in [0, 10000]");
  if (!(maxFreq >= 1.0 && maxFreq <= 20000.0)) return fail(ctx, "maxFreq must be in [1, 20000]");
  if (minFreq > maxFreq) return fail(ctx, "minFreq must not exceed maxFreq");
  if (!(sampleRate > 0.0) || !std::isfinite(sampleRate)) return fail(ctx, "sample rate must be positive");
  if (fft < 4 || (fft & (fft - 1)) || fft > 65536) return fail(ctx, "fft size must be a power of two from 4 to 65536");
  if (algorithm == kPitchCepstrum && fft > kPitchCepstrumMaxFft)
    return fail(ctx, "Cepstrum is limited to fft sizes up to 8192: its DCT table is quadratic in the number of bins");
  return FLUHIP_OK;
}

// the workspaces of one call, sized for its largest round
struct PitchWork
{
  fluhip_ctx* ctx = nullptr;
  int algorithm = 0;
  int64_t F = 0, fft = 0, lo = 0, hi = 0, rows = 0, cap = 0;
  double sampleRate = 0;
  bool fullCurve = false; // (debug) the cepstrum of every bin
  bool chip = false;      // the on-chip form: YinFFT and HPS need no workspace, the cepstrum none for magnitudes
  const double* ttab = nullptr;
  DevBuf sym, spec, curve, aux, ones, lg, table, cep;
};

// doubles a frame needs beside its magnitudes
int64_t pitch_frame_doubles(int algorithm, int64_t F, int64_t rows, bool wantCurve)
{
  if (algorithm == kPitchYinFFT) return 2 * (F - 1) + 2 * F + F + 1;
  if (algorithm == kPitchCepstrum) return F + rows;
  return wantCurve ? F : 0;
}

int pitch_work_init(PitchWork& w, fluhip_ctx* ctx, int algorithm, int64_t F, double minFreq, double maxFreq, double sampleRate,
                    bool fullCurve)
{
  w.ctx = ctx; w.algorithm = algorithm; w.F = F; w.fft = 2 * (F - 1); w.sampleRate = sampleRate; w.fullCurve = fullCurve;
  pitch_bins(algorithm, F, minFreq, maxFreq, sampleRate, &w.lo, &w.hi);
  if (algorithm == kPitchCepstrum)
  {
    if (fullCurve) { w.lo = 0; w.hi = F; }
    w.rows = 1 + std::max<int64_t>(0, w.hi - w.lo);
  }
  return FLUHIP_OK;
}

int pitch_work_alloc(PitchWork& w, int64_t nfMax)
{
  fluhip_ctx* ctx = w.ctx;
  hipStream_t s = ctx->stream;
  w.cap = nfMax;
  if (w.algorithm == kPitchYinFFT && !w.chip) // (on chip the second transform and the curve stay in the LDS)
  {
    int rc = get_twiddle(ctx, w.fft, &w.ttab);
    if (rc) return rc;
    DEV_ALLOC(ctx, "pitch", w.sym, (size_t) (nfMax * w.fft) * sizeof(double), false);
    DEV_ALLOC(ctx, "pitch", w.spec, (size_t) (nfMax * w.F * 2) * sizeof(double), false);
    DEV_ALLOC(ctx, "pitch", w.curve, (size_t) (nfMax * w.F) * sizeof(double), false);
    DEV_ALLOC(ctx, "pitch", w.aux, (size_t) nfMax * sizeof(double), false);
    DEV_ALLOC(ctx, "pitch", w.ones, (size_t) w.fft * sizeof(double), false);
    launch_pitch_fill(w.ones.as<double>(), w.fft, 1.0, s);
  }
  else if (w.algorithm == kPitchCepstrum)
  {
    DEV_ALLOC(ctx, "pitch", w.lg, (size_t) (nfMax * w.F) * sizeof(double), false);
    DEV_ALLOC(ctx, "pitch", w.table, (size_t) (w.rows * w.F) * sizeof(double), false);
    DEV_ALLOC(ctx, "pitch", w.cep, (size_t) (nfMax * w.rows) * sizeof(double), false);
    launch_pitch_dct_table(w.table.as<double>(), w.F, w.lo, w.rows, s); // once per call
  }
  else if (w.algorithm == kPitchHPS && w.fullCurve)
    DEV_ALLOC(ctx, "pitch", w.curve, (size_t) (nfMax * w.F) * sizeof(double), false);
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

// the cepstrum of the nf frames whose log-magnitudes are in w.lg, and its peak search: out [nf][2]
void pitch_cepstrum(PitchWork& w, int64_t nf, double* out)
{
  hipStream_t s = w.ctx->stream;
  // cep[f][r] = sum_j lg[f][j] table[r][j]: one contraction per element whatever the number of frames (no split), so a
  // frame's bits do not depend on the round it falls in
  CrossGemm g;
  g.A = w.lg.as<double>(); g.lda = w.F;
  g.B = w.table.as<double>(); g.ldb = w.F;
  g.C = w.cep.as<double>(); g.ldc = w.rows;
  g.M = nf; g.N = w.rows; g.Kd = w.F;
  CrossGemmPlan plan;
  plan.big = false; // one tile form whatever the number of frames in the round
  plan.nsplit = 1;
  plan.kChunk = round_up(g.Kd, 16);
  launch_cross_gemm(g, 0, 0, kCrossEpiStore, plan, nullptr, s);
  // (the debug curve call widens the rows to every bin and takes the cepstrum itself: no peak search)
  if (!w.fullCurve) launch_pitch_peak(kPitchCepstrum, w.cep.as<double>(), w.rows, nullptr, nf, w.lo, w.hi, w.sampleRate, out, s);
}

// out [nf][2] (device) of the frames `p`; the curve stays in w.curve ([nf][F]) or w.cep ([nf][rows])
int pitch_round(PitchWork& w, const PitchFrames& p, double* out)
{
  fluhip_ctx* ctx = w.ctx;
  hipStream_t s = ctx->stream;
  if (p.nf > w.cap) return fail(ctx, "internal error: pitch round larger than its workspace");
  if (w.algorithm == kPitchHPS)
    launch_pitch_hps(p, w.lo, w.hi, w.sampleRate, w.fullCurve ? w.curve.as<double>() : nullptr, w.F, out, s);
  else if (w.algorithm == kPitchYinFFT)
  {
    launch_pitch_sym(p, w.sym.as<double>(), s);
    // the second transform: window = hop = fft over the rows of sym, a table of ones as the window
    const StftSetup sym{w.fft, w.fft, w.fft, w.F, w.ones.as<double>(), w.ttab};
    StftArgs sa = sym.args(nullptr, w.sym.as<double>(), p.nf * w.fft, p.nf * w.fft, 1, p.nf, 0);
    sa.spec = w.spec.as<double>(); sa.specStride = p.nf * w.F * 2;
    if (const int rc = sym.launch(ctx, sa)) return rc;
    launch_pitch_yin_norm(p, w.spec.as<double>(), w.curve.as<double>(), w.F, w.aux.as<double>(), s);
    launch_pitch_peak(kPitchYinFFT, w.curve.as<double>(), w.F, w.aux.as<double>(), p.nf, w.lo, w.hi, w.sampleRate, out, s);
  }
  else
  {
    launch_pitch_log(p, w.lg.as<double>(), s);
    pitch_cepstrum(w, p.nf, out);
  }
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

// the on-chip form of one round: the frames of `sa` (B buffers of T frames) from the samples to out [B T][2]
int pitch_round_fused(PitchWork& w, const StftArgs& sa, double* out)
{
  fluhip_ctx* ctx = w.ctx;
  hipStream_t s = ctx->stream;
  const int64_t nf = (int64_t) sa.B * sa.T;
  if (nf > w.cap) return fail(ctx, "internal error: pitch round larger than its workspace");
  const bool cep = w.algorithm == kPitchCepstrum;
  PitchFusedArgs o;
  o.algorithm = w.algorithm;
  o.lo = cep ? 0 : (int) std::min(w.lo, w.F); // (HPS: the reference reads past the array above F, clamped here)
  o.hi = cep ? 0 : (int) std::min(w.hi, w.F);
  o.sampleRate = w.sampleRate;
  o.out = out;
  o.lg = cep ? w.lg.as<double>() : nullptr;
  {
    ProfScope ps(ctx, 0);
    if (!launch_pitch_fused(sa, o, s)) return fail(ctx, "internal error: no on-chip pitch form for this shape");
  }
  if (cep) pitch_cepstrum(w, nf, out);
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

int pitch_frames_impl(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld, int algorithm,
                      double minFreq, double maxFreq, double sampleRate, double* out, double* curve)
{
  if (F < 3) return fail(ctx, "need at least 3 bins");
  int rc = check_pitch_params(ctx, algorithm, minFreq, maxFreq, sampleRate, 2 * (F - 1));
  if (rc) return rc;
  if (!mag || (!out && !curve)) return fail(ctx, "null buffer");
  if (count < 1 || T < 1) return fail(ctx, "need at least one buffer and one frame");
  if (ld < F) return fail(ctx, "row stride below the number of bins");
  if (count > (INT64_MAX / 64) / T / ld) return fail(ctx, "batch too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  PitchWork w;
  if ((rc = pitch_work_init(w, ctx, algorithm, F, minFreq, maxFreq, sampleRate, curve != nullptr))) return rc;
  const int64_t nfAll = count * T; // the rows of [count][T][ld] are one run of frames
  const int64_t per = ld + pitch_frame_doubles(algorithm, F, w.rows, curve != nullptr) + 2;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min(nfAll, kRoundMaxFrames), kWorkCapDoubles / per));
  if ((rc = pitch_work_alloc(w, chunk))) return rc;
  DevBuf dMag, dOut;
  DEV_ALLOC(ctx, "pitch", dMag, (size_t) (chunk * ld) * sizeof(double), false);
  DEV_ALLOC(ctx, "pitch", dOut, (size_t) (chunk * 2) * sizeof(double), false);
  for (int64_t f0 = 0; f0 < nfAll; f0 += chunk)
  {
    const int64_t nf = std::min(chunk, nfAll - f0);
    HIPCHK(ctx, hipMemcpyAsync(dMag.p, mag + f0 * ld, (size_t) (nf * ld) * sizeof(double), hipMemcpyDefault, s));
    PitchFrames p{dMag.as<double>(), nf * ld, ld, nf, nf, (int) F};
    if ((rc = pitch_round(w, p, dOut.as<double>()))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    if (out)
    {
      const size_t nb = (size_t) (nf * 2) * sizeof(double);
      if ((rc = copy_to_host(ctx, out + f0 * 2, nb, dOut.p, nb, nb, 1, s))) return rc;
    }
    if (curve)
    {
      const bool cep = algorithm == kPitchCepstrum;
      const double* src = cep ? w.cep.as<double>() + 1 : w.curve.as<double>();
      const size_t spitch = (size_t) (cep ? w.rows : F) * sizeof(double), width = (size_t) F * sizeof(double);
      if ((rc = copy_to_host(ctx, curve + f0 * F, width, src, spitch, width, (size_t) nf, s))) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

int bufpitch_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                  int paddingMode, int algorithm, double minFreq, double maxFreq, int unit, int select, double sampleRate,
                  float* out, int64_t* framesOut)
{
  int rc = check_fft_settings(ctx, win, fft, hop);
  if (rc) return rc;
  if ((rc = check_pitch_params(ctx, algorithm, minFreq, maxFreq, sampleRate, fft))) return rc;
  if (select < 1 || select > 3)
    return fail(ctx, select == 0 ? "select is empty: choose pitch (1), confidence (2) or both (3)" : "select must be in [1, 3]");
  if (unit < 0 || unit > 1) return fail(ctx, "unit must be 0 (Hz) or 1 (MIDI)");
  if (paddingMode < 0 || paddingMode > 2) return fail(ctx, "padding mode must be 0 (None), 1 (Default) or 2 (Full)");
  if (!audio) return fail(ctx, "null buffer");
  if (count < 1) return fail(ctx, "need at least one buffer");
  if (n < 1) return fail(ctx, "not enough frames");
  if (hop > INT32_MAX / 4 || n > INT32_MAX / 2) return fail(ctx, "signal too long");
  // StreamingControl::process (cc/FluidNRTClientWrapper.hpp:564-579, 642-656): the input sits userPad into the padded
  // signal, the client's latency (= win, PitchClient.hpp:151) in front of it; analysis frame j holds the win samples from
  // j hop - win - userPad of the input on; the first latency / hop frames are dropped
  const ControlFrames g = control_frames(n, win, hop, paddingMode, win);
  const int64_t latencyHops = g.latencyHops, userPad = g.userPad, T = g.keep; // (only the kept frames are computed)
  if (T < 1) return fail(ctx, "not enough frames");
  if (T > INT32_MAX / 4 || T + latencyHops > (INT32_MAX / 2 - 2 * win - userPad) / hop) return fail(ctx, "signal too long");
  // rows of [lead zeros][input][zeros] so that every frame lies inside its row: frame j starts at sample j hop
  const int64_t lead = win + userPad;
  const int64_t np = std::max(lead + n, (latencyHops + T - 1) * hop + win);
  const int nsel = (select & 1) + ((select >> 1) & 1);
  if (count > (INT64_MAX / 64) / std::max(T, np)) return fail(ctx, "batch too large");
  if (framesOut) *framesOut = T;
  if (!out) return FLUHIP_OK; // size query
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t F = fft / 2 + 1, Fp = round_up(F, 32);
  StftSetup st;
  if ((rc = stft_setup(ctx, win, fft, hop, &st))) return rc;
  PitchWork w;
  if ((rc = pitch_work_init(w, ctx, algorithm, F, minFreq, maxFreq, sampleRate, false))) return rc;
  // frames a round holds: whole buffers when one fits, else runs of one buffer's frames
  w.chip = pitch_plan(fft, win, algorithm).form == kPitchFormOnChip;
  if (const char* e = fluhip::ab_getenv("FLUHIP_PITCH_FORM")) w.chip = w.chip && std::atoi(e) != kPitchFormTwoPass; // tests: the two-pass form at the on-chip sizes
  const bool chip = w.chip;
  const int64_t per = chip ? (algorithm == kPitchCepstrum ? F + w.rows : 0) + 2 : Fp + pitch_frame_doubles(algorithm, F, w.rows, false) + 2;
  int64_t rowsCap = std::max<int64_t>(1, std::min(kRoundMaxFrames, kWorkCapDoubles / per));
  if (const char* e = fluhip::ab_getenv("FLUHIP_PITCH_ROUND_FRAMES")) rowsCap = std::max<int64_t>(1, std::atoll(e)); // tests: force several rounds
  const bool whole = T <= rowsCap;
  const int64_t perB = whole ? std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(count, 65535), rowsCap / T)) : 1;
  const int64_t run = whole ? T : rowsCap;
  if ((rc = pitch_work_alloc(w, perB * run))) return rc;
  DevBuf dPad, dMag, dRes, dOut;
  DEV_ALLOC(ctx, "pitch", dPad, (size_t) (perB * np) * sizeof(float), true); // only the input is ever written
  if (!chip) DEV_ALLOC(ctx, "pitch", dMag, (size_t) (perB * run * Fp) * sizeof(double), false);
  DEV_ALLOC(ctx, "pitch", dRes, (size_t) (perB * T * 2) * sizeof(double), false);
  DEV_ALLOC(ctx, "pitch", dOut, (size_t) (perB * nsel * T) * sizeof(float), false);
  for (int64_t b0 = 0; b0 < count; b0 += perB)
  {
    const int64_t nb = std::min(perB, count - b0);
    HIPCHK(ctx, hipMemcpy2DAsync(dPad.as<float>() + lead, (size_t) np * sizeof(float), audio + b0 * n, (size_t) n * sizeof(float),
                                 (size_t) n * sizeof(float), (size_t) nb, hipMemcpyDefault, s));
    for (int64_t t0 = 0; t0 < T; t0 += run)
    {
      const int64_t nt = std::min(run, T - t0);
      StftArgs sa = st.args(dPad.as<float>(), nullptr, np, np, nb, nt, (latencyHops + t0) * hop); // (analysis frame j starts at j hop of a row)
      sa.mag = chip ? nullptr : dMag.as<double>(); sa.magStride = nt * Fp; sa.ldMag = Fp;
      // (one buffer per round when its frames come in runs: the results of run t0 go behind those before it)
      double* res = dRes.as<double>() + (whole ? 0 : t0 * 2);
      if (chip)
      {
        if ((rc = pitch_round_fused(w, sa, res))) return rc;
        continue;
      }
      if ((rc = st.launch(ctx, sa, 0))) return rc;
      HIPCHK(ctx, hipGetLastError());
      PitchFrames p{dMag.as<double>(), nt * Fp, Fp, nt, nb * nt, (int) F};
      if ((rc = pitch_round(w, p, res))) return rc;
    }
    launch_pitch_select(dRes.as<double>(), nb, T, unit, select, dOut.as<float>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out + b0 * nsel * T, dOut.p, (size_t) (nb * nsel * T) * sizeof(float), hipMemcpyDefault, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_pitch_plan(fluhip_ctx* ctx, int64_t fft, int64_t win, int algorithm, int64_t* out4)
{
  if (!ctx) return FLUHIP_ERROR;
  if (!out4) return fail(ctx, "null buffer");
  if (win < 1 || fft < win) return fail(ctx, "fftSettings: fft size must be a power of two >= window size, from 4 to 65536");
  const int rc = check_pitch_params(ctx, algorithm, 20.0, 10000.0, 44100.0, fft);
  if (rc) return rc;
  const PitchPlan p = pitch_plan(fft, win, algorithm);
  int64_t lo = 0, hi = 0;
  pitch_bins(algorithm, fft / 2 + 1, 20.0, 10000.0, 44100.0, &lo, &hi);
  out4[0] = p.form;
  out4[1] = p.run;
  out4[2] = p.transforms;
  out4[3] = algorithm == kPitchCepstrum ? 1 + std::max<int64_t>(0, hi - lo) : 0; // (at the default bounds and 44.1 kHz)
  return FLUHIP_OK;
}

int fluhip_pitch_frames_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld, int algorithm,
                            double min_freq, double max_freq, double sample_rate, double* out)
{
  return guarded(ctx, [&] {
    if (!out) return fail(ctx, "null buffer");
    return pitch_frames_impl(ctx, mag, count, T, F, ld, algorithm, min_freq, max_freq, sample_rate, out, nullptr);
  });
}

int fluhip_debug_pitch_curve_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                                 int algorithm, double min_freq, double max_freq, double sample_rate, double* curve)
{
  return guarded(ctx, [&] {
    if (!curve) return fail(ctx, "null buffer");
    return pitch_frames_impl(ctx, mag, count, T, F, ld, algorithm, min_freq, max_freq, sample_rate, nullptr, curve);
  });
}

int fluhip_bufpitch_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                        int padding_mode, int algorithm, double min_freq, double max_freq, int unit, int select,
                        double sample_rate, float* out, int64_t* frames_out)
{
  return guarded(ctx, [&] {
    return bufpitch_impl(ctx, audio, count, n, win, fft, hop, padding_mode, algorithm, min_freq, max_freq, unit, select,
                         sample_rate, out, frames_out);
  });
}

} // extern "C"
