// api_novelty.hip -- C ABI of BufNoveltySlice / BufNoveltyFeature:
//   fluhip_novelty_curve_f64      algorithm::NoveltyFeature::processFrame       algorithms/public/NoveltyFeature.hpp:44-62
//   fluhip_novelty_slices_f64     algorithm::NoveltySegmentation::processFrame  algorithms/public/NoveltySegmentation.hpp:44-63
//   fluhip_bufnoveltyslice_f32    NRTNoveltySliceClient    clients/rt/NoveltySliceClient.hpp, cc/FluidNRTClientWrapper.hpp:665-725
//   fluhip_bufnoveltyfeature_f32  NRTNoveltyFeatureClient  clients/rt/NoveltyFeatureClient.hpp, cc/FluidNRTClientWrapper.hpp:551-660
// The kernels are in kernels_novelty.hip (fluhip_novelty.h); the feature rows come from launch_stft / launch_features.
// Every device buffer is a DevBuf of the call (back in the pool on every way out); no event, no stream is taken.
#include "api_internal.h"
#include "fluhip_novelty.h"

namespace {

constexpr int64_t kMaxFilterSize = (int64_t) 1 << 20; // the moving mean is O(filterSize) per value; the latency stays far inside int64

int check_novelty_params(fluhip_ctx* ctx, int64_t k, int64_t f, double threshold, int64_t minSlice)
{
  if (k < 3 || (k % 2) == 0) return fail(ctx, "kernelSize must be odd and >= 3");
  if (k > 32767) return fail(ctx, "kernelSize is too large");
  if (f < 1) return fail(ctx, "filterSize must be >= 1");
  if (f > kMaxFilterSize) return fail(ctx, "filterSize above 1048576 is not supported");
  if (!(threshold >= 0.0)) return fail(ctx, "threshold must be >= 0");
  if (minSlice < 0) return fail(ctx, "minSliceLength must be >= 0");
  return FLUHIP_OK;
}

int check_novelty_algorithm(fluhip_ctx* ctx, int algorithm)
{
  static const char* names[] = {"Spectrum", "MFCC", "Chroma", "Pitch", "Loudness"};
  if (algorithm < 0 || algorithm > 4) return fail(ctx, "algorithm must be in [0, 4]");
  if (algorithm >= 2)
    return fail(ctx, std::string("algorithm ") + std::to_string(algorithm) + " (" + names[algorithm] +
                         ") is not available: only Spectrum (0) and MFCC (1) are built");
  return FLUHIP_OK;
}

// raw novelty + smoothing of `count` buffers of device feature rows; curve [count][T] (device)
int novelty_curve_dev(fluhip_ctx* ctx, const double* X, int64_t ldx, int64_t strideX, int64_t count, int64_t T, int64_t D,
                      int64_t k, int64_t f, double* curve)
{
  hipStream_t s = ctx->stream;
  const NoveltyPlan one = novelty_plan(1, T, D, k);
  // buffers per round: the launches' grids stay below 2^31 workgroups and the tiled form's workspace below 2 GiB
  int64_t per = one.form == kNoveltyFormTiled ? T * (k + 1) : (T + one.frames - 1) / one.frames;
  const int64_t cap = one.form == kNoveltyFormTiled ? ((int64_t) 1 << 28) : ((int64_t) 1 << 30);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(count, cap / std::max<int64_t>(per, 1)));
  DevBuf nov, work;
  DEV_ALLOC(ctx, "novelty", nov, (size_t) (chunk * T) * sizeof(double), false);
  const NoveltyPlan full = novelty_plan(chunk, T, D, k);
  if (full.workDoubles) DEV_ALLOC(ctx, "novelty", work, (size_t) full.workDoubles * sizeof(double), false);
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    NoveltyArgs a;
    a.X = X + b0 * strideX; a.ldx = ldx; a.strideX = strideX;
    a.T = (int) T; a.D = (int) D; a.k = (int) k; a.count = nb;
    a.norm = novelty_kernel_norm((int) k);
    a.nov = nov.as<double>(); a.work = work.as<double>();
    launch_novelty_raw(a, full, s);
    launch_novelty_smooth(nov.as<double>(), curve + b0 * T, (int) T, nb, (int) f, s);
    HIPCHK(ctx, hipGetLastError());
  }
  return FLUHIP_OK;
}

int check_curve_shape(fluhip_ctx* ctx, const double* feat, int64_t count, int64_t T, int64_t D, int64_t ld)
{
  if (!feat) return fail(ctx, "null buffer");
  if (count < 1 || T < 1 || D < 1) return fail(ctx, "empty feature matrix");
  if (ld < D) return fail(ctx, "row stride below the number of dimensions");
  if (T > INT32_MAX / 4 || D > INT32_MAX / 4) return fail(ctx, "too many frames");
  if (count > (INT64_MAX / 16) / T / ld) return fail(ctx, "feature matrix too large"); // count T ld doubles, in bytes, fit int64
  return FLUHIP_OK;
}

int novelty_slices_impl(fluhip_ctx* ctx, const double* feat, int64_t count, int64_t T, int64_t D, int64_t ld, int64_t k,
                        int64_t f, double threshold, int64_t minSlice, bool slices, unsigned char* det, int64_t* counts,
                        double* curve)
{
  int rc = check_novelty_params(ctx, k, f, slices ? threshold : 0.0, slices ? minSlice : 0);
  if (rc) return rc;
  if ((rc = check_curve_shape(ctx, feat, count, T, D, ld))) return rc;
  if (slices ? (!det || !counts) : !curve) return fail(ctx, "null buffer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf dX, dCurve, dDet, dCnt;
  // feature rows and a curve that are already resident are used in place (a corpus described on the device skips PCIe)
  hipPointerAttribute_t pa;
  const bool featDev = hipPointerGetAttributes(&pa, feat) == hipSuccess && pa.type == hipMemoryTypeDevice;
  const bool curveDev = !slices && hipPointerGetAttributes(&pa, curve) == hipSuccess && pa.type == hipMemoryTypeDevice;
  (void) hipGetLastError();
  if (featDev && curveDev)
  {
    if ((rc = novelty_curve_dev(ctx, feat, ld, T * ld, count, T, D, k, f, curve))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(s));
    return FLUHIP_OK;
  }
  DEV_ALLOC(ctx, "novelty", dX, (size_t) (count * T * D) * sizeof(double), false);
  DEV_ALLOC(ctx, "novelty", dCurve, (size_t) (count * T) * sizeof(double), false);
  HIPCHK(ctx, hipMemcpy2DAsync(dX.p, (size_t) D * sizeof(double), feat, (size_t) ld * sizeof(double), (size_t) D * sizeof(double),
                               (size_t) (count * T), hipMemcpyDefault, s));
  if ((rc = novelty_curve_dev(ctx, dX.as<double>(), D, T * D, count, T, D, k, f, dCurve.as<double>()))) return rc;
  if (slices)
  {
    DEV_ALLOC(ctx, "novelty", dDet, (size_t) (count * T), false);
    DEV_ALLOC(ctx, "novelty", dCnt, (size_t) count * sizeof(int64_t), false);
    launch_novelty_peaks(dCurve.as<double>(), (int) T, count, threshold, (int) std::min<int64_t>(minSlice, INT32_MAX), dDet.as<unsigned char>(),
                         dCnt.as<int64_t>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(s)); // nothing is written to the caller's buffers before the device work has succeeded
    HIPCHK(ctx, hipMemcpyAsync(det, dDet.p, (size_t) (count * T), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipMemcpyAsync(counts, dCnt.p, (size_t) count * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  }
  if (curve)
  {
    const size_t nb = (size_t) (count * T) * sizeof(double);
    if ((rc = copy_to_host(ctx, curve, nb, dCurve.p, nb, nb, 1, s))) return rc;
  }
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

// the feature rows of `nb` mono float buffers on the device under the clients' framing: frame i holds the samples
// [i hop - win - shift, i hop - shift) (FluidSource::pull after BufferedProcess::push: the window ENDS where the host
// vector that fired the frame begins).  rows / ldx / strideX describe the result inside `mag` (Spectrum) or `coef` (MFCC).
struct NoveltyFeatures
{
  fluhip_ctx* ctx;
  int algorithm;
  int64_t n, win, fft, hop, T, F, Tp, Fp, shift;
  double sampleRate;
  StftSetup st;
  DevBuf mag, coef, dLo, dPack, dFilt, dDct;
  MelTables mel;
  int64_t chunk = 1; // buffers per round
  static constexpr int64_t kBands = 40, kCoefs = 13, kBandsPad = 64;

  int64_t dims() const { return algorithm == 0 ? F : kCoefs; }

  int prepare(int64_t count)
  {
    hipStream_t s = ctx->stream;
    F = fft / 2 + 1; Tp = round_up(T, 32); Fp = round_up(F, 32);
    const int rc = stft_setup(ctx, win, fft, hop, &st);
    if (rc) return rc;
    const int64_t perBuf = Tp * Fp * (int64_t) sizeof(double);
    chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(count, 65535), ((int64_t) 2 << 30) / perBuf));
    DEV_ALLOC(ctx, "novelty", mag, (size_t) (chunk * perBuf), true);
    if (algorithm == 1)
    {
      // mMelBands.init(20, 20e3, 40, frameSize, sampleRate, winSize); mDCT.init(40, 13) (rt/NoveltySliceClient.hpp:112-116)
      mel.build(true, F, kBands, kBandsPad, kCoefs, 0, 20.0, 20e3, sampleRate);
      DEV_ALLOC(ctx, "novelty", coef, (size_t) (chunk * T * kCoefs) * sizeof(double), false);
      DEV_ALLOC(ctx, "novelty", dLo, mel.bandLo.size() * sizeof(int), false);
      DEV_ALLOC(ctx, "novelty", dPack, mel.wpack.size() * sizeof(double), false);
      DEV_ALLOC(ctx, "novelty", dFilt, mel.filtT.size() * sizeof(double), false);
      DEV_ALLOC(ctx, "novelty", dDct, mel.dct.size() * sizeof(double), false);
      HIPCHK(ctx, hipMemcpyAsync(dLo.p, mel.bandLo.data(), mel.bandLo.size() * sizeof(int), hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dPack.p, mel.wpack.data(), mel.wpack.size() * sizeof(double), hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dFilt.p, mel.filtT.data(), mel.filtT.size() * sizeof(double), hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dDct.p, mel.dct.data(), mel.dct.size() * sizeof(double), hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipStreamSynchronize(s)); // (the tables are host temporaries of this object; kept simple)
    }
    return FLUHIP_OK;
  }

  int run(const float* audioDev, int64_t nb, const double** rows, int64_t* ldx, int64_t* strideX)
  {
    hipStream_t s = ctx->stream;
    StftArgs sa = st.args(audioDev, nullptr, n, n, nb, T, -win - shift);
    sa.mag = mag.as<double>(); sa.magStride = Tp * Fp; sa.ldMag = Fp;
    if (const int rc = st.launch(ctx, sa)) return rc;
    *rows = mag.as<double>(); *ldx = Fp; *strideX = Tp * Fp;
    if (algorithm == 1)
    {
      FeatArgs fa;
      fa.mag = mag.as<double>(); fa.magStride = Tp * Fp; fa.ldMag = Fp;
      fa.T = (int) T; fa.F = (int) F; fa.B = (int) nb; fa.win = (int) win;
      fa.filtT = dFilt.as<double>(); fa.nBands = (int) kBands; fa.bandsPad = (int) kBandsPad;
      fa.bandLo = dLo.as<int>(); fa.wpack = dPack.as<double>(); fa.maxLen = (int) mel.maxLen;
      fa.magNorm = 0; fa.usePower = 0; fa.logOutput = 1; // processFrame(magnitude, bands, false, false, true) (:157-158)
      fa.dct = dDct.as<double>(); fa.nDct = (int) mel.nDct; fa.startCoeff = 0;
      fa.nOut = (int) kCoefs; fa.out = nullptr; fa.out64 = coef.as<double>();
      if (!launch_features(fa, s)) return fail(ctx, "internal: the mel kernel has no layout for the MFCC algorithm's 40 bands");
      *rows = coef.as<double>(); *ldx = kCoefs; *strideX = T * kCoefs;
    }
    HIPCHK(ctx, hipGetLastError());
    return FLUHIP_OK;
  }
};

int64_t novelty_latency(int64_t hop, int64_t k, int64_t f)
{
  if (f % 2) f++;
  return hop * (1 + ((k + 1) >> 1) + (f >> 1)); // rt/NoveltySliceClient.hpp:200-206
}

int check_client_shape(fluhip_ctx* ctx, int algorithm, int64_t n, int64_t win, int64_t fft, int64_t hop)
{
  int rc = check_shape(ctx, n, win, fft, hop, 1);
  if (rc) return rc;
  if (hop > INT32_MAX / 2 || n > INT64_MAX / 4) return fail(ctx, "hop size or buffer too large"); // (the latency is hop times at most 2^20)
  if (algorithm == 1 && fft / 2 + 1 < NoveltyFeatures::kBands) return fail(ctx, "the MFCC algorithm needs at least 40 bins");
  return FLUHIP_OK;
}

int bufnoveltyslice_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n, int64_t startFrame,
                         int algorithm, int64_t k, double threshold, int64_t f, int64_t minSlice, int64_t win, int64_t fft,
                         int64_t hop, double sampleRate, int64_t* indices, int64_t capacity, int64_t* counts)
{
  int rc = check_novelty_algorithm(ctx, algorithm);
  if (rc) return rc;
  if ((rc = check_novelty_params(ctx, k, f, threshold, minSlice))) return rc;
  if (!audio || !counts || (!indices && capacity > 0)) return fail(ctx, "null buffer");
  if (count < 1 || channels < 1) return fail(ctx, "need at least one buffer and one channel");
  if (capacity < 0) return fail(ctx, "negative capacity");
  if ((rc = check_client_shape(ctx, algorithm, n, win, fft, hop))) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // Slicing::process (:675-723): latency zeros behind the input, rounded up to whole host vectors of 64; a frame fires at
  // every multiple of hop below that length
  const int64_t latency = novelty_latency(hop, k, f);
  const int64_t T = slice_frames(n, hop, latency).T;
  if (T > INT32_MAX / 4) return fail(ctx, "too many frames");
  NoveltyFeatures nf{ctx, algorithm, n, win, fft, hop, T, 0, 0, 0, 0, sampleRate};
  if ((rc = nf.prepare(count))) return rc;
  const int64_t chunk = nf.chunk;
  DevBuf dIn, dMono, dCurve, dDet, dCnt;
  DEV_ALLOC(ctx, "novelty", dIn, (size_t) (chunk * channels * n) * sizeof(float), false);
  if (channels > 1) DEV_ALLOC(ctx, "novelty", dMono, (size_t) (chunk * n) * sizeof(float), false);
  DEV_ALLOC(ctx, "novelty", dCurve, (size_t) (chunk * T) * sizeof(double), false);
  DEV_ALLOC(ctx, "novelty", dDet, (size_t) (chunk * T), false);
  DEV_ALLOC(ctx, "novelty", dCnt, (size_t) chunk * sizeof(int64_t), false);
  std::vector<unsigned char> det((size_t) (count * T));
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    HIPCHK(ctx, hipMemcpyAsync(dIn.p, audio + b0 * channels * n, (size_t) (nb * channels * n) * sizeof(float), hipMemcpyDefault, s));
    const float* mono = dIn.as<float>();
    if (channels > 1)
    {
      launch_mono_sum_f32(dIn.as<float>(), (int) channels, n, nb, dMono.as<float>(), s);
      mono = dMono.as<float>();
    }
    const double* rows = nullptr;
    int64_t ldx = 0, strideX = 0;
    if ((rc = nf.run(mono, nb, &rows, &ldx, &strideX))) return rc;
    if ((rc = novelty_curve_dev(ctx, rows, ldx, strideX, nb, T, nf.dims(), k, f, dCurve.as<double>()))) return rc;
    launch_novelty_peaks(dCurve.as<double>(), (int) T, nb, threshold, (int) std::min<int64_t>(minSlice, INT32_MAX), dDet.as<unsigned char>(),
                         dCnt.as<int64_t>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(det.data() + b0 * T, dDet.p, (size_t) (nb * T), hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  for (int64_t b = 0; b < count; b++)
    counts[b] = detections_to_indices(det.data() + b * T, T, hop, latency, n, startFrame, indices ? indices + b * capacity : nullptr,
                                      capacity);
  return FLUHIP_OK;
}

int bufnoveltyfeature_impl(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int algorithm, int64_t k, int64_t f,
                           int64_t win, int64_t fft, int64_t hop, double sampleRate, int paddingMode, float* out,
                           int64_t* framesOut)
{
  int rc = check_novelty_algorithm(ctx, algorithm);
  if (rc) return rc;
  if ((rc = check_novelty_params(ctx, k, f, 0.0, 0))) return rc;
  if (!audio) return fail(ctx, "null buffer");
  if (paddingMode < 0 || paddingMode > 2) return fail(ctx, "padding mode must be 0 (None), 1 (Default) or 2 (Full)");
  if (count < 1) return fail(ctx, "need at least one buffer");
  if ((rc = check_client_shape(ctx, algorithm, n, win, fft, hop))) return rc;
  // StreamingControl::process (:564-579, 642-656): the input sits userPad into the padded signal, frame j fires with the
  // j-th host vector of hop samples, the first latency / hop frames are dropped
  const ControlFrames g = control_frames(n, win, hop, paddingMode, novelty_latency(hop, k, f));
  const int64_t userPad = g.userPad, T = g.T, latencyHops = g.latencyHops, keep = g.keep;
  if (g.paddedLength < win || keep < 1) return fail(ctx, "not enough frames");
  if (T > INT32_MAX / 4) return fail(ctx, "too many frames");
  if (framesOut) *framesOut = keep;
  if (!out) return FLUHIP_OK; // size query
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  NoveltyFeatures nf{ctx, algorithm, n, win, fft, hop, T, 0, 0, 0, userPad, sampleRate};
  if ((rc = nf.prepare(count))) return rc;
  const int64_t chunk = nf.chunk;
  DevBuf dIn, dCurve, dOut;
  DEV_ALLOC(ctx, "novelty", dIn, (size_t) (chunk * n) * sizeof(float), false);
  DEV_ALLOC(ctx, "novelty", dCurve, (size_t) (chunk * T) * sizeof(double), false);
  DEV_ALLOC(ctx, "novelty", dOut, (size_t) (chunk * keep) * sizeof(float), false);
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    HIPCHK(ctx, hipMemcpyAsync(dIn.p, audio + b0 * n, (size_t) (nb * n) * sizeof(float), hipMemcpyDefault, s));
    const double* rows = nullptr;
    int64_t ldx = 0, strideX = 0;
    if ((rc = nf.run(dIn.as<float>(), nb, &rows, &ldx, &strideX))) return rc;
    if ((rc = novelty_curve_dev(ctx, rows, ldx, strideX, nb, T, nf.dims(), k, f, dCurve.as<double>()))) return rc;
    launch_curve_to_f32(dCurve.as<double>(), (int) T, (int) latencyHops, (int) keep, nb, dOut.as<float>(), s);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out + b0 * keep, dOut.p, (size_t) (nb * keep) * sizeof(float), hipMemcpyDefault, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_novelty_plan(fluhip_ctx* ctx, int64_t T, int64_t D, int64_t kernel_size, int64_t* out3)
{
  if (!ctx || !out3 || T < 1 || D < 1 || kernel_size < 3 || (kernel_size % 2) == 0) return FLUHIP_ERROR;
  const NoveltyPlan p = novelty_plan(1, T, D, kernel_size);
  out3[0] = p.form;
  out3[1] = p.rows;
  out3[2] = p.frames;
  return FLUHIP_OK;
}

int fluhip_novelty_curve_f64(fluhip_ctx* ctx, const double* feat, int64_t count, int64_t T, int64_t D, int64_t ld,
                             int64_t kernel_size, int64_t filter_size, double* curve)
{
  return guarded(ctx, [&] {
    return novelty_slices_impl(ctx, feat, count, T, D, ld, kernel_size, filter_size, 0.0, 0, false, nullptr, nullptr, curve);
  });
}

int fluhip_novelty_slices_f64(fluhip_ctx* ctx, const double* feat, int64_t count, int64_t T, int64_t D, int64_t ld,
                              int64_t kernel_size, int64_t filter_size, double threshold, int64_t min_slice,
                              unsigned char* det, int64_t* counts, double* curve)
{
  return guarded(ctx, [&] {
    return novelty_slices_impl(ctx, feat, count, T, D, ld, kernel_size, filter_size, threshold, min_slice, true, det, counts,
                               curve);
  });
}

int fluhip_bufnoveltyslice_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t channels, int64_t n,
                               int64_t start_frame, int algorithm, int64_t kernel_size, double threshold,
                               int64_t filter_size, int64_t min_slice, int64_t win, int64_t fft, int64_t hop,
                               double sample_rate, int64_t* indices, int64_t capacity, int64_t* counts)
{
  return guarded(ctx, [&] {
    return bufnoveltyslice_impl(ctx, audio, count, channels, n, start_frame, algorithm, kernel_size, threshold, filter_size,
                                min_slice, win, fft, hop, sample_rate, indices, capacity, counts);
  });
}

int fluhip_bufnoveltyfeature_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int algorithm,
                                 int64_t kernel_size, int64_t filter_size, int64_t win, int64_t fft, int64_t hop,
                                 double sample_rate, int padding_mode, float* out, int64_t* frames_out)
{
  return guarded(ctx, [&] {
    return bufnoveltyfeature_impl(ctx, audio, count, n, algorithm, kernel_size, filter_size, win, fft, hop, sample_rate,
                                  padding_mode, out, frames_out);
  });
}

} // extern "C"
