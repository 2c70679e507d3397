// api_spectral.hip -- C ABI of BufSpectralShape and BufChroma:
//   fluhip_spectralshape_frames_f64   algorithm::SpectralShape::processFrame on given magnitudes
//   fluhip_bufspectralshape_f32       NRTSpectralShapeClient  clients/rt/SpectralShapeClient.hpp, common/FluidNRTClientWrapper.hpp:551-660
//   fluhip_debug_chroma_filters_f64   the table of algorithm::ChromaFilterBank::init
//   fluhip_chroma_frames_f64          algorithm::ChromaFilterBank::processFrame on given magnitudes
//   fluhip_bufchroma_f32              NRTChromaClient  clients/rt/ChromaClient.hpp
//   fluhip_debug_spectral_plan
// fft 1024 / 2048 / 4096 with an even window run the on-chip form (spectral_fused_kernel, kernels_spectral_fused.hip): one
// launch from the samples to the seven descriptors, or to the squared magnitudes of Chroma's contraction.  Everything else,
// and the two entry points that are given magnitudes, run the two-pass form: the kernels are in kernels_spectral.hip
// (fluhip_spectral.h); the magnitudes come from launch_stft.  In both forms Chroma's contraction is cross_gemm_kernel
// (fluhip_cross.h) over the filter table.  The frequency axis and the filter table depend on nothing per frame: both are
// built once per call, on the host, with the reference's own sequence of double operations.  Every device buffer is a DevBuf
// of the call; no event, no stream is taken.
#include "api_internal.h"
#include "fluhip_cross.h"
#include "fluhip_env.h"
#include "fluhip_spectral.h"

namespace {

constexpr int64_t kWorkCapDoubles = (int64_t) 1 << 27; // 1 GiB of workspace per round
constexpr int64_t kRoundMaxFrames = (int64_t) 1 << 21; // (the GEMM's grid: frames / 64 workgroup rows)
constexpr double kLog2E = 1.44269504088896340736;      // util/AlgorithmUtils.hpp:24, ChromaFilterBank.hpp:38

struct ShapeSettings
{
  double minFreq, maxFreq, percent;
  int unit, power;
};
struct ChromaSettings
{
  int64_t nChroma;
  double ref;
  int normalize;
  double minFreq, maxFreq;
};

int check_sample_rate_and_bins(fluhip_ctx* ctx, double sampleRate, int64_t fft)
{
  if (!(sampleRate > 0.0) || !std::isfinite(sampleRate)) return fail(ctx, "sample rate must be positive");
  if (fft < 4 || (fft & (fft - 1)) || fft > 65536) return fail(ctx, "fft size must be a power of two from 4 to 65536");
  return FLUHIP_OK;
}

int check_shape_params(fluhip_ctx* ctx, const ShapeSettings& p, double sampleRate, int64_t fft)
{
  if (!(p.minFreq >= 0.0)) return fail(ctx, "minFreq must be at least 0");
  if (!(p.maxFreq >= -1.0)) return fail(ctx, "maxFreq must be at least -1 (-1: half the sample rate)");
  if (!(p.percent >= 0.0 && p.percent <= 100.0)) return fail(ctx, "rolloffPercent must be in [0, 100]");
  if (p.unit < 0 || p.unit > 1) return fail(ctx, "unit must be 0 (Hz) or 1 (Midi Cents)");
  if (p.power < 0 || p.power > 1) return fail(ctx, "power must be 0 (No) or 1 (Yes)");
  return check_sample_rate_and_bins(ctx, sampleRate, fft);
}

int check_chroma_params(fluhip_ctx* ctx, const ChromaSettings& p, double sampleRate, int64_t fft)
{
  if (p.nChroma < 2 || p.nChroma > 128) return fail(ctx, "numChroma must be in [2, 128]");
  if (!(p.ref > 0.0 && p.ref <= 22000.0)) return fail(ctx, "ref must be in (0, 22000]");
  if (p.normalize < 0 || p.normalize > 2) return fail(ctx, "normalize must be 0 (None), 1 (Sum) or 2 (Max)");
  if (!(p.minFreq >= 0.0)) return fail(ctx, "minFreq must be at least 0");
  if (!(p.maxFreq == -1.0 || p.maxFreq >= 0.0)) return fail(ctx, "maxFreq must be -1 (half the sample rate) or at least 0");
  return check_sample_rate_and_bins(ctx, sampleRate, fft);
}

// an index from a quotient; at or beyond the bin count it counts as the bin count (the cast of a huge value is undefined)
int64_t bin_of(double q, int64_t F, bool up) { return !(q < (double) F) ? F : (int64_t) (up ? std::ceil(q) : std::floor(q)); }

// Eigen's ArrayXd::LinSpaced(size, low, high), 0 <= low <= high: size 1 yields high, the last element is exactly high
double lin_spaced(int64_t i, int64_t size, double low, double high)
{
  if (size == 1 || i == size - 1) return high;
  const double step = (high - low) / (double) (size - 1);
  return low + (double) i * step;
}

// SpectralShape.hpp:37-69: false = an empty range (seven zeros per frame).  axis: the host image of ShapeParams::axis
bool shape_setup(const ShapeSettings& p, int64_t F, double sampleRate, ShapeParams& sp, std::vector<double>& axis)
{
  const double maxFreq = p.maxFreq == -1.0 ? sampleRate / 2 : std::min(p.maxFreq, sampleRate / 2);
  const double binHz = sampleRate / ((double) (F - 1) * 2.0);
  int64_t minBin = bin_of(p.minFreq / binHz, F, true);
  const int64_t maxBin = std::min(bin_of(maxFreq / binHz, F, false), F - 1);
  if (maxBin <= minBin) return false;
  sp.fold = 0;
  if (p.unit == 1 && minBin == 0)
  {
    minBin = 1;
    sp.fold = 1;
  }
  const int64_t size = maxBin - minBin; // bin maxBin is never read
  if (size < 1) return false;           // (defined here: the reference reads an empty array)
  sp.lo = (int) minBin;
  sp.size = (int) size;
  sp.power = p.power;
  sp.percent = p.percent;
  sp.miss = (double) (maxBin - 1);
  axis.resize((size_t) size);
  for (int64_t i = 0; i < size; i++)
  {
    // the step is (maxBin - minBin) binHz / (size - 1), not binHz
    const double f = lin_spaced(i, size, (double) minBin * binHz, (double) maxBin * binHz);
    axis[(size_t) i] = p.unit == 1 ? 69 + (12 * std::log(f / 440) * kLog2E) : f;
  }
  return true;
}

// ChromaFilterBank::init (:35-81): filters [nChroma][F]
void chroma_table(int64_t nChroma, int64_t F, double ref, double sampleRate, std::vector<double>& filters)
{
  const int64_t fft = 2 * (F - 1);
  // LinSpaced(fftSize, 0, sampleRate): the step is sr / (fftSize - 1); points 0 .. F are read
  std::vector<double> freqs((size_t) F + 1);
  for (int64_t j = 0; j <= F && j < fft; j++)
    freqs[(size_t) j] = (double) nChroma * std::log(lin_spaced(j, fft, 0.0, sampleRate) / (ref / 16)) * kLog2E;
  freqs[0] = freqs[1] - 1.5 * (double) nChroma;
  const int64_t half = nChroma / 2; // lrint of an integer quotient
  filters.assign((size_t) (nChroma * F), 0.0);
  for (int64_t j = 0; j < F; j++)
  {
    const double width = std::max(freqs[(size_t) j + 1] - freqs[(size_t) j], 1.0); // (j + 1 <= F <= fftSize - 1)
    double sq = 0.0;
    for (int64_t c = 0; c < nChroma; c++)
    {
      const double d = freqs[(size_t) j] - (double) c;
      const double r = std::fmod(d + (double) (10 * nChroma) + (double) half, (double) nChroma) - (double) half;
      const double q = 2 * r / width;
      const double w = std::exp(-0.5 * (q * q));
      filters[(size_t) (c * F + j)] = w;
      sq += w * w;
    }
    const double norm = std::sqrt(sq);
    for (int64_t c = 0; c < nChroma; c++) filters[(size_t) (c * F + j)] /= norm;
  }
}

// ChromaFilterBank::processFrame :91-103: the bins zlo < j < zhi survive
void chroma_range(const ChromaSettings& p, int64_t F, double sampleRate, int* zlo, int* zhi)
{
  *zlo = -1;
  *zhi = (int) F;
  if (p.minFreq == 0.0 && p.maxFreq == -1.0) return;
  const double maxFreq = p.maxFreq == -1.0 ? sampleRate / 2 : std::min(p.maxFreq, sampleRate / 2);
  const double binHz = sampleRate / ((double) (F - 1) * 2.0);
  const int64_t minBin = p.minFreq == 0.0 ? 0 : bin_of(p.minFreq / binHz, F, true);
  const int64_t maxBin = std::min(bin_of(maxFreq / binHz, F, false), F - 1);
  *zlo = (int) std::min(minBin, F - 1); // bins 0 .. minBin inclusive are zeroed (clamped to the frame)
  *zhi = (int) maxBin;
}

// the tables and workspaces of one call, sized for its largest round
struct SpectralWork
{
  fluhip_ctx* ctx = nullptr;
  int kind = 0;
  int64_t F = 0, cap = 0;
  bool empty = false; // SpectralShape with an empty range: seven zeros per frame, nothing is transformed
  bool chip = false;
  ShapeParams shape{};
  int64_t nChroma = 0;
  int normalize = 0, zlo = -1, zhi = 0;
  double scale = 0;
  DevBuf axis, filters, pw;
  int64_t width() const { return kind == kSpectralShape ? kShapeDescriptors : nChroma; } // doubles a frame's result takes
};

int spectral_work_init(SpectralWork& w, fluhip_ctx* ctx, int kind, int64_t F, double sampleRate, const ShapeSettings* sh,
                       const ChromaSettings* ch)
{
  w.ctx = ctx; w.kind = kind; w.F = F;
  hipStream_t s = ctx->stream;
  if (kind == kSpectralShape)
  {
    std::vector<double> axis;
    w.empty = !shape_setup(*sh, F, sampleRate, w.shape, axis);
    if (w.empty) return FLUHIP_OK;
    DEV_ALLOC(ctx, "spectral shape", w.axis, axis.size() * sizeof(double), false);
    HIPCHK(ctx, hipMemcpyAsync(w.axis.p, axis.data(), axis.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s)); // (the host image leaves scope)
    w.shape.axis = w.axis.as<double>();
    return FLUHIP_OK;
  }
  w.nChroma = ch->nChroma; w.normalize = ch->normalize;
  w.scale = 2.0 / (double) (2 * (F - 1) * ch->nChroma);
  chroma_range(*ch, F, sampleRate, &w.zlo, &w.zhi);
  std::vector<double> filters;
  chroma_table(ch->nChroma, F, ch->ref, sampleRate, filters);
  DEV_ALLOC(ctx, "chroma", w.filters, filters.size() * sizeof(double), false);
  HIPCHK(ctx, hipMemcpyAsync(w.filters.p, filters.data(), filters.size() * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

int spectral_work_alloc(SpectralWork& w, int64_t nfMax)
{
  w.cap = nfMax;
  if (w.kind == kSpectralChroma) DEV_ALLOC(w.ctx, "chroma", w.pw, (size_t) (nfMax * w.F) * sizeof(double), false);
  return FLUHIP_OK;
}

// acc[f][c] = sum_j pw[f][j] filters[c][j]: one contraction per element whatever the number of frames (no split, one tile
// form), so a frame's bits do not depend on the round it falls in
void chroma_contract(SpectralWork& w, int64_t nf, double* acc)
{
  CrossGemm g;
  g.A = w.pw.as<double>(); g.lda = w.F;
  g.B = w.filters.as<double>(); g.ldb = w.F;
  g.C = acc; g.ldc = w.nChroma;
  g.M = nf; g.N = w.nChroma; g.Kd = w.F;
  CrossGemmPlan plan;
  plan.big = false;
  plan.nsplit = 1;
  plan.kChunk = round_up(g.Kd, 16);
  launch_cross_gemm(g, 0, 0, kCrossEpiStore, plan, nullptr, w.ctx->stream);
}

// res [nf][width] (device) of the frames `p`: the descriptors, or Chroma's raw contraction (scale and normalize follow)
int spectral_round(SpectralWork& w, const SpectralFrames& p, double* res)
{
  fluhip_ctx* ctx = w.ctx;
  hipStream_t s = ctx->stream;
  if (p.nf > w.cap) return fail(ctx, "internal error: spectral round larger than its workspace");
  if (w.kind == kSpectralShape)
    launch_shape_frames(p, w.shape, res, s);
  else
  {
    launch_chroma_power(p, w.zlo, w.zhi, w.pw.as<double>(), s);
    chroma_contract(w, p.nf, res);
  }
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

// the on-chip form of one round: the frames of `sa` (B buffers of T frames) from the samples to res [B T][width]
int spectral_round_fused(SpectralWork& w, const StftArgs& sa, double* res)
{
  fluhip_ctx* ctx = w.ctx;
  hipStream_t s = ctx->stream;
  const int64_t nf = (int64_t) sa.B * sa.T;
  if (nf > w.cap) return fail(ctx, "internal error: spectral round larger than its workspace");
  const bool chroma = w.kind == kSpectralChroma;
  SpectralFusedArgs o{};
  o.kind = w.kind;
  o.shape = w.shape;
  o.zlo = w.zlo; o.zhi = w.zhi;
  o.out = chroma ? nullptr : res;
  o.pw = chroma ? w.pw.as<double>() : nullptr;
  {
    ProfScope ps(ctx, 0);
    if (!launch_spectral_fused(sa, o, s)) return fail(ctx, "internal error: no on-chip spectral form for this shape");
  }
  if (chroma) chroma_contract(w, nf, res);
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

int spectral_frames_impl(fluhip_ctx* ctx, int kind, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                         const ShapeSettings* sh, const ChromaSettings* ch, double sampleRate, double* out)
{
  if (F < 3) return fail(ctx, "need at least 3 bins");
  int rc = kind == kSpectralShape ? check_shape_params(ctx, *sh, sampleRate, 2 * (F - 1)) : check_chroma_params(ctx, *ch, sampleRate, 2 * (F - 1));
  if (rc) return rc;
  if (!mag || !out) return fail(ctx, "null buffer");
  if (count < 1 || T < 1) return fail(ctx, "need at least one buffer and one frame");
  if (ld < F) return fail(ctx, "row stride below the number of bins");
  if (count > (INT64_MAX / 256) / T / ld) return fail(ctx, "batch too large");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  SpectralWork w;
  if ((rc = spectral_work_init(w, ctx, kind, F, sampleRate, sh, ch))) return rc;
  const int64_t nfAll = count * T; // the rows of [count][T][ld] are one run of frames
  const int64_t width = w.width();
  if (w.empty)
  {
    std::fill(out, out + nfAll * width, 0.0);
    return FLUHIP_OK;
  }
  const int64_t per = ld + (kind == kSpectralChroma ? F : 0) + 2 * width;
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min(nfAll, kRoundMaxFrames), kWorkCapDoubles / per));
  if ((rc = spectral_work_alloc(w, chunk))) return rc;
  DevBuf dMag, dRes, dOut;
  DEV_ALLOC(ctx, "spectral", dMag, (size_t) (chunk * ld) * sizeof(double), false);
  DEV_ALLOC(ctx, "spectral", dRes, (size_t) (chunk * width) * sizeof(double), false);
  if (kind == kSpectralChroma) DEV_ALLOC(ctx, "spectral", dOut, (size_t) (chunk * width) * sizeof(double), false);
  for (int64_t f0 = 0; f0 < nfAll; f0 += chunk)
  {
    const int64_t nf = std::min(chunk, nfAll - f0);
    HIPCHK(ctx, hipMemcpyAsync(dMag.p, mag + f0 * ld, (size_t) (nf * ld) * sizeof(double), hipMemcpyDefault, s));
    SpectralFrames p{dMag.as<double>(), nf * ld, ld, nf, nf, (int) F};
    if ((rc = spectral_round(w, p, dRes.as<double>()))) return rc;
    const double* src = dRes.as<double>();
    if (kind == kSpectralChroma)
    {
      launch_chroma_epilogue(dRes.as<double>(), nf, nf, (int) w.nChroma, w.scale, w.normalize, dOut.as<double>(), nullptr, s);
      HIPCHK(ctx, hipGetLastError());
      src = dOut.as<double>();
    }
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    const size_t nb = (size_t) (nf * width) * sizeof(double);
    if ((rc = copy_to_host(ctx, out + f0 * width, nb, src, nb, nb, 1, s))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

int spectral_buf_impl(fluhip_ctx* ctx, int kind, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                      int64_t hop, int paddingMode, int select, const ShapeSettings* sh, const ChromaSettings* ch,
                      double sampleRate, float* out, int64_t* framesOut)
{
  int rc = check_fft_settings(ctx, win, fft, hop);
  if (rc) return rc;
  if ((rc = kind == kSpectralShape ? check_shape_params(ctx, *sh, sampleRate, fft) : check_chroma_params(ctx, *ch, sampleRate, fft))) return rc;
  if (kind == kSpectralShape && (select < 1 || select > 127))
    return fail(ctx, select == 0 ? "select is empty: choose among centroid (1), spread (2), skew (4), kurtosis (8), rolloff (16), flatness (32), crest (64)"
                                 : "select must be in [1, 127]");
  if (paddingMode < 0 || paddingMode > 2) return fail(ctx, "padding mode must be 0 (None), 1 (Default) or 2 (Full)");
  if (!audio) return fail(ctx, "null buffer");
  if (count < 1) return fail(ctx, "need at least one buffer");
  if (n < 1) return fail(ctx, "not enough frames");
  if (hop > INT32_MAX / 4 || n > INT32_MAX / 2) return fail(ctx, "signal too long");
  // StreamingControl::process (cc/FluidNRTClientWrapper.hpp:564-579, 642-656): the input sits userPad into the padded
  // signal, the client's latency (= win, SpectralShapeClient.hpp:129, ChromaClient.hpp:111) in front of it; analysis frame
  // j holds the win samples from j hop - win - userPad of the input on; the first latency / hop frames are dropped
  const ControlFrames g = control_frames(n, win, hop, paddingMode, win);
  const int64_t latencyHops = g.latencyHops, userPad = g.userPad, T = g.keep; // (only the kept frames are computed)
  if (T < 1) return fail(ctx, "not enough frames");
  if (T > INT32_MAX / 4 || T + latencyHops > (INT32_MAX / 2 - 2 * win - userPad) / hop) return fail(ctx, "signal too long");
  // rows of [lead zeros][input][zeros] so that every frame lies inside its row: frame j starts at sample j hop
  const int64_t lead = win + userPad;
  const int64_t np = std::max(lead + n, (latencyHops + T - 1) * hop + win);
  const int64_t F = fft / 2 + 1, Fp = round_up(F, 32);
  int nsel = 0;
  for (int i = 0; i < kShapeDescriptors; i++) nsel += (select >> i) & 1;
  if (kind == kSpectralChroma) nsel = (int) ch->nChroma;
  if (count > (INT64_MAX / 256) / std::max(T, np)) return fail(ctx, "batch too large");
  if (framesOut) *framesOut = T;
  if (!out) return FLUHIP_OK; // size query
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  SpectralWork w;
  if ((rc = spectral_work_init(w, ctx, kind, F, sampleRate, sh, ch))) return rc;
  if (w.empty)
  {
    std::fill(out, out + count * nsel * T, 0.0f);
    return FLUHIP_OK;
  }
  StftSetup st;
  if ((rc = stft_setup(ctx, win, fft, hop, &st))) return rc;
  const int64_t width = w.width();
  // frames a round holds: whole buffers when one fits, else runs of one buffer's frames
  w.chip = spectral_plan(fft, win, kind).form == kSpectralFormOnChip;
  if (const char* e = fluhip::ab_getenv("FLUHIP_SPECTRAL_FORM")) w.chip = w.chip && std::atoi(e) != kSpectralFormTwoPass; // tests: the two-pass form at the on-chip sizes
  const bool chip = w.chip;
  const int64_t per = (chip ? 0 : Fp) + (kind == kSpectralChroma ? F : 0) + width + nsel;
  int64_t rowsCap = std::max<int64_t>(1, std::min(kRoundMaxFrames, kWorkCapDoubles / per));
  if (const char* e = fluhip::ab_getenv("FLUHIP_SPECTRAL_ROUND_FRAMES")) rowsCap = std::max<int64_t>(1, std::atoll(e)); // tests: force several rounds
  const bool whole = T <= rowsCap;
  const int64_t perB = whole ? std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(count, 65535), rowsCap / T)) : 1;
  const int64_t run = whole ? T : rowsCap;
  if ((rc = spectral_work_alloc(w, perB * run))) return rc;
  DevBuf dPad, dMag, dRes, dOut;
  DEV_ALLOC(ctx, "spectral", dPad, (size_t) (perB * np) * sizeof(float), true); // only the input is ever written
  if (!chip) DEV_ALLOC(ctx, "spectral", dMag, (size_t) (perB * run * Fp) * sizeof(double), false);
  DEV_ALLOC(ctx, "spectral", dRes, (size_t) (perB * T * width) * sizeof(double), false);
  DEV_ALLOC(ctx, "spectral", dOut, (size_t) (perB * nsel * T) * sizeof(float), false);
  for (int64_t b0 = 0; b0 < count; b0 += perB)
  {
    const int64_t nb = std::min(perB, count - b0);
    HIPCHK(ctx, hipMemcpy2DAsync(dPad.as<float>() + lead, (size_t) np * sizeof(float), audio + b0 * n, (size_t) n * sizeof(float),
                                 (size_t) n * sizeof(float), (size_t) nb, hipMemcpyDefault, s));
    for (int64_t t0 = 0; t0 < T; t0 += run)
    {
      const int64_t nt = std::min(run, T - t0);
      // (analysis frame j starts at j hop of a row; the latency frames in front are never transformed)
      StftArgs sa = st.args(dPad.as<float>(), nullptr, np, np, nb, nt, (latencyHops + t0) * hop);
      sa.mag = chip ? nullptr : dMag.as<double>(); sa.magStride = nt * Fp; sa.ldMag = Fp;
      // (one buffer per round when its frames come in runs: the results of run t0 go behind those before it)
      double* res = dRes.as<double>() + (whole ? 0 : t0 * width);
      if (chip)
      {
        if ((rc = spectral_round_fused(w, sa, res))) return rc;
        continue;
      }
      if ((rc = st.launch(ctx, sa, 0))) return rc;
      HIPCHK(ctx, hipGetLastError());
      SpectralFrames p{dMag.as<double>(), nt * Fp, Fp, nt, nb * nt, (int) F};
      if ((rc = spectral_round(w, p, res))) return rc;
    }
    if (kind == kSpectralShape)
      launch_shape_select(dRes.as<double>(), nb, T, select, dOut.as<float>(), s);
    else
      launch_chroma_epilogue(dRes.as<double>(), nb * T, T, (int) w.nChroma, w.scale, w.normalize, nullptr, dOut.as<float>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out + b0 * nsel * T, dOut.p, (size_t) (nb * nsel * T) * sizeof(float), hipMemcpyDefault, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_spectral_plan(fluhip_ctx* ctx, int64_t fft, int64_t win, int kind, int64_t* out4)
{
  if (!ctx) return FLUHIP_ERROR;
  if (!out4) return fail(ctx, "null buffer");
  if (win < 1 || fft < win) return fail(ctx, "fftSettings: fft size must be a power of two >= window size, from 4 to 65536");
  if (kind < 0 || kind >= kSpectralKinds) return fail(ctx, "kind must be 0 (SpectralShape) or 1 (Chroma)");
  const int rc = check_sample_rate_and_bins(ctx, 44100.0, fft);
  if (rc) return rc;
  const SpectralPlan p = spectral_plan(fft, win, kind);
  out4[0] = p.form;
  out4[1] = p.run;
  out4[2] = p.transforms;
  out4[3] = p.gemm;
  return FLUHIP_OK;
}

int fluhip_spectralshape_frames_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                                    double min_freq, double max_freq, double rolloff_percent, int unit, int power,
                                    double sample_rate, double* out)
{
  return guarded(ctx, [&] {
    const ShapeSettings sh{min_freq, max_freq, rolloff_percent, unit, power};
    return spectral_frames_impl(ctx, kSpectralShape, mag, count, T, F, ld, &sh, nullptr, sample_rate, out);
  });
}

int fluhip_bufspectralshape_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                                int64_t hop, int padding_mode, int select, double min_freq, double max_freq,
                                double rolloff_percent, int unit, int power, double sample_rate, float* out, int64_t* frames_out)
{
  return guarded(ctx, [&] {
    const ShapeSettings sh{min_freq, max_freq, rolloff_percent, unit, power};
    return spectral_buf_impl(ctx, kSpectralShape, audio, count, n, win, fft, hop, padding_mode, select, &sh, nullptr, sample_rate,
                             out, frames_out);
  });
}

int fluhip_debug_chroma_filters_f64(fluhip_ctx* ctx, int64_t num_chroma, int64_t F, double ref, double sample_rate, double* out)
{
  return guarded(ctx, [&] {
    if (F < 3) return fail(ctx, "need at least 3 bins");
    const ChromaSettings ch{num_chroma, ref, 0, 0.0, -1.0};
    const int rc = check_chroma_params(ctx, ch, sample_rate, 2 * (F - 1));
    if (rc) return rc;
    if (!out) return fail(ctx, "null buffer");
    std::vector<double> filters;
    chroma_table(num_chroma, F, ref, sample_rate, filters);
    std::copy(filters.begin(), filters.end(), out);
    return (int) FLUHIP_OK;
  });
}

int fluhip_chroma_frames_f64(fluhip_ctx* ctx, const double* mag, int64_t count, int64_t T, int64_t F, int64_t ld,
                             int64_t num_chroma, double ref, int normalize, double min_freq, double max_freq, double sample_rate,
                             double* out)
{
  return guarded(ctx, [&] {
    const ChromaSettings ch{num_chroma, ref, normalize, min_freq, max_freq};
    return spectral_frames_impl(ctx, kSpectralChroma, mag, count, T, F, ld, nullptr, &ch, sample_rate, out);
  });
}

int fluhip_bufchroma_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft, int64_t hop,
                         int padding_mode, int64_t num_chroma, double ref, int normalize, double min_freq, double max_freq,
                         double sample_rate, float* out, int64_t* frames_out)
{
  return guarded(ctx, [&] {
    const ChromaSettings ch{num_chroma, ref, normalize, min_freq, max_freq};
    return spectral_buf_impl(ctx, kSpectralChroma, audio, count, n, win, fft, hop, padding_mode, 0, nullptr, &ch, sample_rate, out,
                             frames_out);
  });
}

} // extern "C"
