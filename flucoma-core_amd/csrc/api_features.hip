// api_features.hip -- BufSTFT (clients/nrt/BufSTFTClient.hpp:81-276) and the feature pipeline BufMelBands / BufMFCC
// (algorithms/public/MelBands.hpp, DCT.hpp; clients/rt/MFCCClient.hpp, MelBandsClient.hpp behind StreamingControl) of the C ABI.
#include "api_internal.h"

// the host-side tables of the mel / DCT kernels: dense bin-major filter bank, the same packed over each band's support, DCT rows
void MelTables::build(bool mfcc, int64_t F, int64_t nBands, int64_t bandsPad, int64_t nCoefs, int64_t startCoeff, double minFreq,
                      double maxFreq, double sampleRate)
{
  // mel filter bank (alg/MelBands.hpp:53-73), bin-major and zero padded; f64 on the host like the reference
  filtT.assign((size_t) F * bandsPad, 0.0);
  {
    auto hz2mel = [](double x) { return 1127.01048 * std::log(x / 700.0 + 1.0); };
    const int64_t nc = nBands + 2;
    std::vector<double> centres((size_t) nc);
    const double mlo = hz2mel(minFreq), mhi = hz2mel(maxFreq);
    for (int64_t i = 0; i < nc; i++)
      centres[(size_t) i] = 700.0 * (std::exp((mlo + (double) i * (mhi - mlo) / (double) (nc - 1)) / 1127.01048) - 1.0);
    for (int64_t b = 0; b < nBands; b++)
    {
      const double d0 = std::fabs(centres[(size_t) b] - centres[(size_t) b + 1]);
      const double d1 = std::fabs(centres[(size_t) b + 1] - centres[(size_t) b + 2]);
      for (int64_t f = 0; f < F; f++)
      {
        const double hz = (double) f * (sampleRate / 2.0) / (double) (F - 1);
        const double lower = -(centres[(size_t) b] - hz) / d0, upper = (centres[(size_t) b + 2] - hz) / d1;
        filtT[(size_t) (f * bandsPad + b)] = std::max(0.0, std::min(lower, upper));
      }
    }
  }
  // the filter bank over each band's support only (kernels_feat.hip): first non-zero bin and packed weights
  bandLo.assign((size_t) bandsPad, 0);
  maxLen = 1;
  {
    std::vector<int64_t> hi((size_t) bandsPad, -1);
    for (int64_t b = 0; b < nBands; b++)
    {
      int64_t lo = -1;
      for (int64_t f = 0; f < F; f++)
        if (filtT[(size_t) (f * bandsPad + b)] != 0.0) { if (lo < 0) lo = f; hi[(size_t) b] = f; }
      bandLo[(size_t) b] = (int) std::max<int64_t>(lo, 0);
      if (lo >= 0) maxLen = std::max(maxLen, hi[(size_t) b] - lo + 1);
    }
  }
  wpack.assign((size_t) maxLen * bandsPad, 0.0);
  for (int64_t b = 0; b < nBands; b++)
    for (int64_t j = 0; j < maxLen; j++)
    {
      const int64_t f = bandLo[(size_t) b] + j;
      if (f < F) wpack[(size_t) (j * bandsPad + b)] = filtT[(size_t) (f * bandsPad + b)];
    }
  nDct = mfcc ? std::min(nCoefs + startCoeff, nBands) : 0; // rt/MFCCClient.hpp:104-105
  dct.assign((size_t) std::max<int64_t>(1, nDct * nBands), 0.0);
  for (int64_t i = 0; i < nDct; i++) // alg/DCT.hpp:53-61
  {
    const double scale = i == 0 ? 1.0 / std::sqrt((double) nBands) : std::sqrt(2.0 / (double) nBands);
    for (int64_t j = 0; j < nBands; j++)
      dct[(size_t) (i * nBands + j)] = std::cos((M_PI / (double) nBands) * (double) i * (0.5 + (double) j)) * scale;
  }
}

// ---- which form a feature call takes (features_common runs by it, fluhip_debug_features_plan reports it) ----------
static int check_feature_params(fluhip_ctx* ctx, bool mfcc, int64_t fft, int64_t nBands, int64_t nCoefs, int64_t startCoeff,
                                double minFreq, double maxFreq)
{
  if (nBands < 2 || nBands > fft / 2 + 1) return fail(ctx, "numBands must be in [2, fft/2 + 1]");
  if (!(maxFreq > minFreq)) return fail(ctx, "maxFreq must be above minFreq");
  if (mfcc && (nCoefs < 2 || nCoefs > nBands || startCoeff < 0 || startCoeff > 1))
    return fail(ctx, "numCoeffs must be in [2, numBands] and startCoeff in [0, 1]");
  return FLUHIP_OK;
}

// fused form (kernels_stft_feat.hip stft_feat_kernel): the magnitudes never leave the chip.
// Every bin must lie on the rising edge of at most one band and the falling edge of the band below it, with the
// bins of each edge contiguous: then band b = (sum of up[f] m[f] over interval b) + (sum of dn[f] m[f] over interval
// b + 1), interval s = the bins between centres s and s + 1.  True of any filter bank whose triangles are wider than
// a bin; checked here against the dense matrix, coefficient by coefficient, and anything else takes the two-kernel path.
// Returns whether the shape runs fused and, if so, leaves the kernel's boundary tables in up / dn / slot.
static bool fused_features_tables(bool mfcc, int64_t win, int64_t fft, int64_t nBands, int64_t bandsPad, const MelTables& mel,
                                  std::vector<double>& up, std::vector<double>& dn, std::vector<short>& slot)
{
  const int64_t F = fft / 2 + 1, nDct = mel.nDct;
  const std::vector<double>& filtT = mel.filtT;
  const int CH = stft_features_bins_per_lane((int) fft);
  up.assign((size_t) 64 * CH, 0.0);
  dn.assign((size_t) 64 * CH, 0.0);
  slot.assign((size_t) 64 * CH, (short) -1);
  std::vector<int64_t> interval((size_t) F, -1); // interval of bin f, -1: no band touches it
  // (nDct * nBands <= 4096 bounds the table; the kernel's LDS must also hold its padded rows: stft_features_fits)
  bool ok = nBands <= 64 && (!mfcc || nDct * nBands <= 4096) && !stft_needs_scratch(win, fft) && (fft == 1024 || fft == 2048) &&
            (win % 2) == 0 && stft_features_fits((int) fft, (int) nBands, mfcc ? (int) nDct : 0);
  if (const char* e = fluhip::ab_getenv("FLUHIP_FEAT_FUSED")) // A/B and tests: 0 forces the two-kernel form
    if (std::atoi(e) == 0) ok = false;
  std::vector<int64_t> peak((size_t) nBands, 0);
  for (int64_t b = 0; ok && b < nBands; b++)
  {
    double best = -1.0;
    for (int64_t f = 0; f < F; f++)
      if (filtT[(size_t) (f * bandsPad + b)] > best) { best = filtT[(size_t) (f * bandsPad + b)]; peak[(size_t) b] = f; }
    if (best <= 0.0) ok = false; // a band no bin falls into
  }
  for (int64_t f = 0; ok && f < F; f++)
  {
    int64_t b1 = -1, b2 = -1, cnt = 0;
    for (int64_t b = 0; b < nBands; b++)
      if (filtT[(size_t) (f * bandsPad + b)] != 0.0) { if (cnt == 0) b1 = b; else b2 = b; cnt++; }
    if (cnt == 0) continue;
    if (cnt > 2 || (cnt == 2 && b2 != b1 + 1)) { ok = false; break; }
    if (cnt == 2)
    {
      interval[(size_t) f] = b2;
      up[(size_t) f] = filtT[(size_t) (f * bandsPad + b2)];
      dn[(size_t) f] = filtT[(size_t) (f * bandsPad + b1)];
    }
    else if (f <= peak[(size_t) b1]) { interval[(size_t) f] = b1; up[(size_t) f] = filtT[(size_t) (f * bandsPad + b1)]; }
    else { interval[(size_t) f] = b1 + 1; dn[(size_t) f] = filtT[(size_t) (f * bandsPad + b1)]; }
  }
  // interval s starts at bin g[s].  The touched bins must be one contiguous run whose intervals ascend one at a time
  // from some i0 up to nBands (the falling edge of the last band); intervals below i0 are empty and the running
  // sums are still 0 at their boundaries, which therefore publish nothing.
  std::vector<int64_t> g((size_t) nBands + 2, -1);
  if (ok)
  {
    int64_t prev = -1, first = -1, last = -1;
    bool ended = false;
    for (int64_t f = 0; f < F && ok; f++)
    {
      const int64_t iv = interval[(size_t) f];
      if (iv < 0) { if (first >= 0) ended = true; continue; }
      if (ended) { ok = false; break; }              // touched bins are not one contiguous run
      if (first < 0) first = f;
      else if (iv != prev && iv != prev + 1) { ok = false; break; }
      if (iv != prev) g[(size_t) iv] = f;
      prev = iv;
      last = f;
    }
    if (first < 0 || prev != nBands) ok = false;
    if (ok)
    {
      int64_t i0 = 0;
      while (g[(size_t) i0] < 0) i0++;
      for (int64_t sI = 0; sI < i0; sI++) g[(size_t) sI] = first;
      g[(size_t) nBands + 1] = last + 1;
      for (int64_t sI = i0 + 1; sI <= nBands + 1; sI++) slot[(size_t) (g[(size_t) sI] - 1)] = (short) sI;
    }
    // reconstruction: the segment sums must give back the dense matrix exactly
    for (int64_t b = 0; ok && b < nBands; b++)
      for (int64_t f = 0; f < F; f++)
      {
        double w = 0.0;
        if (f >= g[(size_t) b] && f < g[(size_t) b + 1]) w += up[(size_t) f];
        if (f >= g[(size_t) b + 1] && f < g[(size_t) b + 2]) w += dn[(size_t) f];
        if (w != filtT[(size_t) (f * bandsPad + b)]) { ok = false; break; }
      }
  }
  return ok;
}

// ---- BufSTFT ------------------------------------------------------------------
static int bufstft_forward(fluhip_ctx* ctx, const float* audio, int64_t n, int64_t stride, int64_t win, int64_t fft, int64_t hop,
                           int padding_mode, float* mag, float* phase, int64_t* hops_out)
{
  if (!audio) return fail(ctx, "No input buffer supplied");
  if (!mag && !phase) return fail(ctx, "Neither magnitude nor phase buffer supplied");
  if (padding_mode < 0 || padding_mode > 2) return fail(ctx, "padding mode must be 0, 1 or 2");
  if (stride < 1) return fail(ctx, "stride must be >= 1");
  int rc = check_shape(ctx, n, win, fft, hop, 1);
  if (rc) return rc;
  if (fft / 2 + 1 >= 65536) // nrt/BufSTFTClient.hpp:135-138
    return fail(ctx, "Can produce up to 65536 channels. Split your data up and try again");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const ControlFrames g = control_frames(n, win, hop, padding_mode, 0); // :121-130: no latency, every frame kept
  const int64_t F = fft / 2 + 1, T = g.T;
  if (g.paddedLength < win) return fail(ctx, "not enough frames");
  if (hops_out) *hops_out = T;
  StftSetup st;
  if ((rc = stft_setup(ctx, win, fft, hop, &st))) return rc;
  DevBuf in, spec, dm, dp;
  HIPCHK(ctx, in.alloc((size_t) n * sizeof(float), false, s));
  HIPCHK(ctx, upload_strided(in.p, audio, (size_t) n, (size_t) stride, sizeof(float), s));
  HIPCHK(ctx, spec.alloc((size_t) T * F * 2 * sizeof(double), false, s));
  if (mag) HIPCHK(ctx, dm.alloc((size_t) T * F * sizeof(float), false, s));
  if (phase) HIPCHK(ctx, dp.alloc((size_t) T * F * sizeof(float), false, s));
  StftArgs sa = st.args(in.as<float>(), nullptr, n, n, 1, T, -g.userPad); // frame i starts at sample i*hop - padding (:151-162)
  sa.spec = spec.as<double>();
  if ((rc = st.launch(ctx, sa))) return rc;
  launch_spec_to_magphase(spec.as<double>(), (int) T, (int) F, mag ? dm.as<float>() : nullptr,
                          phase ? dp.as<float>() : nullptr, s);
  HIPCHK(ctx, hipGetLastError());
  if (mag) HIPCHK(ctx, hipMemcpyAsync(mag, dm.p, (size_t) T * F * sizeof(float), hipMemcpyDeviceToHost, s));
  if (phase) HIPCHK(ctx, hipMemcpyAsync(phase, dp.p, (size_t) T * F * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

static int bufstft_inverse(fluhip_ctx* ctx, const float* mag, const float* phase, int64_t hops, int64_t win, int64_t fft,
                           int64_t hop, int padding_mode, float* out, int64_t* n_out)
{
  if (!mag || !phase) return fail(ctx, "Need both magnutude and phase buffers for inverse transform");
  if (padding_mode < 0 || padding_mode > 2) return fail(ctx, "padding mode must be 0, 1 or 2");
  if (hops < 1) return fail(ctx, "not enough frames");
  int rc = check_shape(ctx, 1, win, fft, hop, 1);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t F = fft / 2 + 1, T = hops, pad = user_padding(win, hop, padding_mode);
  const int64_t paddedOut = (T - 1) * hop + win; // nrt/BufSTFTClient.hpp:233
  const int64_t finalOut = paddedOut - pad;      // :234
  if (n_out) *n_out = finalOut;
  if (!out) return FLUHIP_OK;                    // size query
  StftSetup st;
  if ((rc = stft_setup(ctx, win, fft, hop, &st))) return rc;
  DevBuf dm, dp, spec, frames, dout;
  HIPCHK(ctx, dm.alloc((size_t) T * F * sizeof(float), false, s));
  HIPCHK(ctx, dp.alloc((size_t) T * F * sizeof(float), false, s));
  HIPCHK(ctx, spec.alloc((size_t) T * F * 2 * sizeof(double), false, s));
  HIPCHK(ctx, frames.alloc((size_t) T * win * sizeof(double), false, s));
  HIPCHK(ctx, dout.alloc((size_t) finalOut * sizeof(float), false, s));
  HIPCHK(ctx, hipMemcpyAsync(dm.p, mag, (size_t) T * F * sizeof(float), hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(dp.p, phase, (size_t) T * F * sizeof(float), hipMemcpyHostToDevice, s));
  launch_polar_to_spec(dm.as<float>(), dp.as<float>(), (int) T, (int) F, spec.as<double>(), s);
  ResynthArgs ra = st.resynth(spec.as<double>(), T, frames.as<double>(), finalOut, pad);
  ra.out32 = dout.as<float>();
  if ((rc = st.launch(ctx, ra))) return rc;
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, dout.p, (size_t) finalOut * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

// ---- feature pipeline -------------------------------------------------------
static int features_common(fluhip_ctx* ctx, bool mfcc, const float* audio, int64_t count, int64_t n, int64_t win,
                           int64_t fft, int64_t hop, int64_t nBands, int64_t nCoefs, int64_t startCoeff,
                           double minFreq, double maxFreq, double sampleRate, int normalize, int scaleDb,
                           int paddingMode, float* out, int64_t* frames_out)
{
  if (!audio || !out) return fail(ctx, "null buffer");
  if (paddingMode < 0 || paddingMode > 2) return fail(ctx, "padding mode must be 0 (None), 1 (Default) or 2 (Full)");
  if (count < 1) return fail(ctx, "need at least one buffer");
  int rc = check_shape(ctx, n, win, fft, hop, 1);
  if (rc) return rc;
  if ((rc = check_feature_params(ctx, mfcc, fft, nBands, nCoefs, startCoeff, minFreq, maxFreq))) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t F = fft / 2 + 1;
  // StreamingControl bookkeeping with the client's latency = win; only the kept frames are computed
  const ControlFrames g = control_frames(n, win, hop, paddingMode, win);
  const int64_t T = g.keep;
  const int64_t frame0 = g.latencyHops * hop - win - g.userPad; // where kept frame 0 (analysis frame latencyHops) starts
  if (T < 1) return fail(ctx, "not enough frames");
  if (frames_out) *frames_out = T;
  const int64_t Tp = round_up(T, 32), Fp = round_up(F, 32);
  const int64_t bandsPad = round_up(nBands, 64);
  // (more than 64 bands never run fused: refused before tables of gigabytes are built for them)
  if (nBands > 64 && !features_layout(F, bandsPad).fits)
    return fail(ctx, "too many bands for this fft size: the band energies of a frame do not fit on chip");
  MelTables mel;
  mel.build(mfcc, F, nBands, bandsPad, nCoefs, startCoeff, minFreq, maxFreq, sampleRate);
  const std::vector<double>&filtT = mel.filtT, &wpack = mel.wpack, &dct = mel.dct;
  const std::vector<int>& bandLo = mel.bandLo;
  const int64_t maxLen = mel.maxLen, nDct = mel.nDct;
  const int64_t nOut = mfcc ? nCoefs : nBands;
  StftSetup st;
  if ((rc = stft_setup(ctx, win, fft, hop, &st))) return rc;
  DevBuf dFilt, dDct, dAudio, dMag, dOut, dLo, dPack;
  HIPCHK(ctx, dLo.alloc(bandLo.size() * sizeof(int), false, s));
  HIPCHK(ctx, dPack.alloc(wpack.size() * sizeof(double), false, s));
  HIPCHK(ctx, hipMemcpyAsync(dLo.p, bandLo.data(), bandLo.size() * sizeof(int), hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(dPack.p, wpack.data(), wpack.size() * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(ctx, dFilt.alloc(filtT.size() * sizeof(double), false, s));
  HIPCHK(ctx, dDct.alloc(dct.size() * sizeof(double), false, s));
  HIPCHK(ctx, hipMemcpyAsync(dFilt.p, filtT.data(), filtT.size() * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpyAsync(dDct.p, dct.data(), dct.size() * sizeof(double), hipMemcpyHostToDevice, s));
  // ---- fused form (kernels_stft_feat.hip stft_feat_kernel): the magnitudes never leave the chip --------------------------
  {
    std::vector<double> up, dn;
    std::vector<short> slot;
    bool ok = fused_features_tables(mfcc, win, fft, nBands, bandsPad, mel, up, dn, slot);
    if (ok)
    {
      DevBuf dUp, dDn, dSlot, dDct2, dAud, dOutF;
      HIPCHK(ctx, dUp.alloc(up.size() * sizeof(double), false, s));
      HIPCHK(ctx, dDn.alloc(dn.size() * sizeof(double), false, s));
      HIPCHK(ctx, dSlot.alloc(slot.size() * sizeof(short), false, s));
      HIPCHK(ctx, dDct2.alloc(dct.size() * sizeof(double), false, s));
      HIPCHK(ctx, hipMemcpyAsync(dUp.p, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dDn.p, dn.data(), dn.size() * sizeof(double), hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dSlot.p, slot.data(), slot.size() * sizeof(short), hipMemcpyHostToDevice, s));
      HIPCHK(ctx, hipMemcpyAsync(dDct2.p, dct.data(), dct.size() * sizeof(double), hipMemcpyHostToDevice, s));
      // device-resident audio / output are used in place; host buffers go through staging chunks of bounded size
      hipPointerAttribute_t pa;
      const bool audDev = hipPointerGetAttributes(&pa, audio) == hipSuccess && pa.type == hipMemoryTypeDevice;
      const bool outDev = hipPointerGetAttributes(&pa, out) == hipSuccess && pa.type == hipMemoryTypeDevice;
      (void) hipGetLastError();
      int64_t chunkBytes = (int64_t) 1 << 31;
      if (const char* e = fluhip::ab_getenv("FLUHIP_FEAT_CHUNK_BYTES")) chunkBytes = std::max<int64_t>(1, std::atoll(e)); // tests: force several chunks
      const int64_t chunkB = (audDev && outDev) ? count
                                                : std::max<int64_t>(1, std::min<int64_t>(count, chunkBytes / (n * (int64_t) sizeof(float))));
      if (!audDev) HIPCHK(ctx, dAud.alloc((size_t) chunkB * n * sizeof(float), false, s));
      if (!outDev) HIPCHK(ctx, dOutF.alloc((size_t) chunkB * nOut * T * sizeof(float), false, s));
      for (int64_t b0 = 0; b0 < count; b0 += chunkB)
      {
        const int64_t nb = std::min(chunkB, count - b0);
        const float* aPtr = audio + b0 * n;
        if (!audDev)
        {
          HIPCHK(ctx, hipMemcpyAsync(dAud.p, aPtr, (size_t) nb * n * sizeof(float), hipMemcpyDefault, s));
          aPtr = dAud.as<float>();
        }
        float* oPtr = outDev ? out + b0 * nOut * T : dOutF.as<float>();
        const StftArgs sa = st.args(aPtr, nullptr, n, n, nb, T, frame0);
        FeatArgs fa;
        fa.mag = nullptr; fa.magStride = 0; fa.ldMag = 0;
        fa.T = (int) T; fa.F = (int) F; fa.B = (int) nb; fa.win = (int) win;
        fa.filtT = nullptr; fa.nBands = (int) nBands; fa.bandsPad = (int) bandsPad;
        fa.bandLo = nullptr; fa.wpack = nullptr; fa.maxLen = 0;
        fa.magNorm = mfcc ? 0 : (normalize ? 1 : 0); fa.usePower = 0; fa.logOutput = mfcc ? 1 : (scaleDb ? 1 : 0);
        fa.dct = mfcc ? dDct2.as<double>() : nullptr; fa.nDct = (int) nDct; fa.startCoeff = (int) startCoeff;
        fa.nOut = (int) nOut; fa.out = oPtr;
        bool launched;
        {
          ProfScope p(ctx, 2);
          launched = launch_stft_features(sa, fa, dUp.as<double>(), dDn.as<double>(), dSlot.as<short>(), s);
        }
        if (!launched) { ok = false; break; }
        HIPCHK(ctx, hipGetLastError());
        if (!outDev)
          HIPCHK(ctx, hipMemcpyAsync(out + b0 * nOut * T, oPtr, (size_t) nb * nOut * T * sizeof(float), hipMemcpyDefault, s));
        if (!audDev || !outDev) HIPCHK(ctx, hipStreamSynchronize(s));   // the staging buffers are reused by the next chunk
      }
      if (ok)
      {
        HIPCHK(ctx, hipStreamSynchronize(s));
        return FLUHIP_OK;
      }
    }
  }
  // ---- two-kernel form: magnitudes through HBM, any filter bank / fft size -------------------------------------------
  if (!features_layout(F, bandsPad).fits)
    return fail(ctx, "too many bands for this fft size: the band energies of a frame do not fit on chip");
  // buffers are processed in chunks that keep the magnitude scratch around 2 GiB
  const int64_t perBuf = Tp * Fp * (int64_t) sizeof(double);
  int64_t scratchBytes = 2LL << 30;
  if (const char* e = fluhip::ab_getenv("FLUHIP_FEAT_CHUNK_BYTES")) scratchBytes = std::max<int64_t>(1, std::atoll(e)); // tests: force several chunks
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(count, 65535), scratchBytes / perBuf));
  HIPCHK(ctx, dAudio.alloc((size_t) chunk * n * sizeof(float), false, s));
  HIPCHK(ctx, dMag.alloc((size_t) chunk * perBuf, true, s));
  HIPCHK(ctx, dOut.alloc((size_t) chunk * nOut * T * sizeof(float), false, s));
  for (int64_t b0 = 0; b0 < count; b0 += chunk)
  {
    const int64_t nb = std::min(chunk, count - b0);
    // hipMemcpyDefault: `audio` and `out` may be host or device pointers (a corpus already resident in HBM skips PCIe)
    HIPCHK(ctx, hipMemcpyAsync(dAudio.p, audio + b0 * n, (size_t) nb * n * sizeof(float), hipMemcpyDefault, s));
    StftArgs sa = st.args(dAudio.as<float>(), nullptr, n, n, nb, T, frame0);
    sa.mag = dMag.as<double>(); sa.magStride = Tp * Fp; sa.ldMag = Fp;
    if ((rc = st.launch(ctx, sa, 0))) return rc;
    FeatArgs fa;
    fa.mag = dMag.as<double>(); fa.magStride = Tp * Fp; fa.ldMag = Fp;
    fa.T = (int) T; fa.F = (int) F; fa.B = (int) nb; fa.win = (int) win;
    fa.filtT = dFilt.as<double>(); fa.nBands = (int) nBands; fa.bandsPad = (int) bandsPad;
    fa.bandLo = dLo.as<int>(); fa.wpack = dPack.as<double>(); fa.maxLen = (int) maxLen;
    // rt/MFCCClient.hpp:123-124 (false, false, true); rt/MelBandsClient.hpp:106-108 (normalize, false, scale == dB)
    fa.magNorm = mfcc ? 0 : (normalize ? 1 : 0); fa.usePower = 0; fa.logOutput = mfcc ? 1 : (scaleDb ? 1 : 0);
    fa.dct = mfcc ? dDct.as<double>() : nullptr; fa.nDct = (int) nDct; fa.startCoeff = (int) startCoeff;
    fa.nOut = (int) nOut; fa.out = dOut.as<float>();
    {
      ProfScope p(ctx, 2);
      if (!launch_features(fa, s)) return fail(ctx, "internal: the mel kernel has no layout for a shape that was planned");
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out + b0 * nOut * T, dOut.p, (size_t) nb * nOut * T * sizeof(float),
                               hipMemcpyDefault, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  return FLUHIP_OK;
}

static int features_plan(fluhip_ctx* ctx, int mfcc, int64_t win, int64_t fft, int64_t n_bands, int64_t n_coefs,
                         int64_t start_coeff, double min_freq, double max_freq, double sample_rate, int64_t* out5)
{
  if (!out5) return fail(ctx, "null buffer");
  int rc = check_shape(ctx, 1, win, fft, 1, 1);
  if (rc) return rc;
  if ((rc = check_feature_params(ctx, mfcc != 0, fft, n_bands, n_coefs, start_coeff, min_freq, max_freq))) return rc;
  const int64_t F = fft / 2 + 1, bandsPad = round_up(n_bands, 64);
  for (int i = 0; i < 5; i++) out5[i] = 0;
  if (n_bands <= 64) // (the fused form's first condition; the filter bank of thousands of bands is not built to learn that)
  {
    MelTables mel;
    mel.build(mfcc != 0, F, n_bands, bandsPad, n_coefs, start_coeff, min_freq, max_freq, sample_rate);
    std::vector<double> up, dn;
    std::vector<short> slot;
    if (fused_features_tables(mfcc != 0, win, fft, n_bands, bandsPad, mel, up, dn, slot)) return FLUHIP_OK;
  }
  const FeatLayout p = features_layout(F, bandsPad);
  if (!p.fits) return fail(ctx, "too many bands for this fft size: the band energies of a frame do not fit on chip");
  out5[0] = 1; out5[1] = p.nw; out5[2] = p.ft; out5[3] = (int64_t) p.lds; out5[4] = p.rowsInLds ? 1 : 0;
  return FLUHIP_OK;
}

extern "C" {

int fluhip_bufstft_forward_f32(fluhip_ctx* ctx, const float* audio, int64_t n, int64_t stride, int64_t win,
                               int64_t fft, int64_t hop, int padding_mode, float* mag, float* phase,
                               int64_t* hops_out)
{
  return guarded(ctx, [&] { return bufstft_forward(ctx, audio, n, stride, win, fft, hop, padding_mode, mag, phase, hops_out); });
}

int fluhip_bufstft_inverse_f32(fluhip_ctx* ctx, const float* mag, const float* phase, int64_t hops, int64_t win,
                               int64_t fft, int64_t hop, int padding_mode, float* out, int64_t* n_out)
{
  return guarded(ctx, [&] { return bufstft_inverse(ctx, mag, phase, hops, win, fft, hop, padding_mode, out, n_out); });
}

int fluhip_debug_features_plan(fluhip_ctx* ctx, int mfcc, int64_t win, int64_t fft, int64_t n_bands, int64_t n_coefs,
                               int64_t start_coeff, double min_freq, double max_freq, double sample_rate, int64_t* out5)
{
  fluhip_ctx host; // pure host arithmetic: a null context is accepted (an error then has no text to leave)
  return guarded(ctx ? ctx : &host, [&] {
    return features_plan(ctx, mfcc, win, fft, n_bands, n_coefs, start_coeff, min_freq, max_freq, sample_rate, out5);
  });
}

int fluhip_bufmelbands_padded_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win,
                                  int64_t fft, int64_t hop, int64_t n_bands, double min_freq, double max_freq,
                                  double sample_rate, int normalize, int scale_db, int padding_mode, float* out,
                                  int64_t* frames_out)
{
  return guarded(ctx, [&] {
    return features_common(ctx, false, audio, count, n, win, fft, hop, n_bands, 0, 0, min_freq, max_freq, sample_rate,
                           normalize, scale_db, padding_mode, out, frames_out);
  });
}
int fluhip_bufmelbands_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win,
                           int64_t fft, int64_t hop, int64_t n_bands, double min_freq, double max_freq,
                           double sample_rate, int normalize, int scale_db, float* out, int64_t* frames_out)
{
  return fluhip_bufmelbands_padded_f32(ctx, audio, count, n, win, fft, hop, n_bands, min_freq, max_freq, sample_rate,
                                       normalize, scale_db, 1, out, frames_out);
}

int fluhip_bufmfcc_padded_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                              int64_t hop, int64_t n_bands, int64_t n_coefs, int64_t start_coeff, double min_freq,
                              double max_freq, double sample_rate, int padding_mode, float* out, int64_t* frames_out)
{
  return guarded(ctx, [&] {
    return features_common(ctx, true, audio, count, n, win, fft, hop, n_bands, n_coefs, start_coeff, min_freq, max_freq,
                           sample_rate, 0, 0, padding_mode, out, frames_out);
  });
}
int fluhip_bufmfcc_f32(fluhip_ctx* ctx, const float* audio, int64_t count, int64_t n, int64_t win, int64_t fft,
                       int64_t hop, int64_t n_bands, int64_t n_coefs, int64_t start_coeff, double min_freq,
                       double max_freq, double sample_rate, float* out, int64_t* frames_out)
{
  return fluhip_bufmfcc_padded_f32(ctx, audio, count, n, win, fft, hop, n_bands, n_coefs, start_coeff, min_freq,
                                   max_freq, sample_rate, 1, out, frames_out);
}

} // extern "C"
