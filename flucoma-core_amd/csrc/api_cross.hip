// api_cross.hip -- C ABI of BufNMFCross (audio mosaicing):
//   fluhip_nmfcross_process_f64  algorithm::NMFCross::process          algorithms/public/NMFCross.hpp:59-78, 156-186
//   fluhip_griffinlim_f64        algorithm::GriffinLim::process        algorithms/public/GriffinLim.hpp:26-52
//   fluhip_bufnmfcross_f32       client::nmfcross::NMFCrossClient      clients/nrt/NMFCrossClient.hpp:84-184
// The kernels are in kernels_nmfcross.hip (fluhip_cross.h); the STFT / ISTFT steps reuse launch_stft / launch_resynth.
#include "api_internal.h"
#include "fluhip_cross.h"

namespace {

// The H-update loop of NMFCross::multiplicativeUpdates (:156-186) on device data: X [T][F] (ld F), W [K][F] (ld F,
// clamped to eps in place), H [T][ldh] out (ldh = K).  progress(1..iters) with the context's run-ahead bound.
struct CrossLoop
{
  fluhip_ctx* ctx;
  const double* X;
  double* W;
  int64_t T, F, K;
  int64_t r, p, c, iters, seed;
  double* Hout; // device [T][K]
};

int cross_loop(const CrossLoop& L, fluhip_progress_fn progress, void* user)
{
  fluhip_ctx* ctx = L.ctx;
  hipStream_t s = ctx->stream;
  const int64_t T = L.T, F = L.F, K = L.K, ldh = K;
  DevBuf dsum, denergy, Hc, Hs, Q, part;
  DEV_ALLOC(ctx, "NMFCross", dsum, (size_t) K * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", denergy, (size_t) K * sizeof(double), false);
  launch_cross_dict(L.W, F, (int) K, (int) F, dsum.as<double>(), denergy.as<double>(), s);
  // H = EigenRandom<MatrixXd>(K, T, seed, [0, 1)) (:70-71): column-major K x T, one draw per value -- entry (k, t) is draw
  // t K + k, which is H1[t][k] of the T x K layout here
  {
    std::vector<double> h0;
    draw_uniform(L.seed, (size_t) (T * K), h0);
    HIPCHK(ctx, hipMemcpyAsync(L.Hout, h0.data(), h0.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipStreamSynchronize(s)); // (h0 is a host temporary)
  }
  const int cus = std::max(1, ctx->props.multiProcessorCount);
  const CrossGemmPlan p1 = cross_gemm_plan(T, F, K, cus), p2 = cross_gemm_plan(T, K, F, cus);
  DEV_ALLOC(ctx, "NMFCross", Hc, (size_t) (T * ldh) * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", Hs, (size_t) (T * ldh) * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", Q, (size_t) (T * F) * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", part, (size_t) std::max<int64_t>(std::max(p1.partDoubles, p2.partDoubles), 1) * sizeof(double), false);
  double* H = L.Hout;
  // measurement builds only (fluhip_env.h): FLUHIP_CROSS_WIDE=1 runs the same H update on the any-rank path of the plain NMF
  // (kernels_nmf_wide.hip: dgemm_tile_kernel, the ratio and apply launches) -- the A/B baseline of tools/nmfcross_bench.py
  const char* wideEnv = ab_getenv("FLUHIP_CROSS_WIDE");
  const bool wide = wideEnv && std::atoi(wideEnv) != 0;
  const int64_t Kp = round_up(K, 16);
  DevBuf WT, XT, HW, wideScr;
  if (wide)
  {
    DEV_ALLOC(ctx, "NMFCross", WT, (size_t) (round_up(F, 32) * Kp) * sizeof(double), true);
    DEV_ALLOC(ctx, "NMFCross", XT, (size_t) (F * T) * sizeof(double), false);
    DEV_ALLOC(ctx, "NMFCross", HW, (size_t) (round_up(T, 32) * Kp) * sizeof(double), true);
    DEV_ALLOC(ctx, "NMFCross", wideScr, (size_t) nmf_update_wide_scratch_doubles((int) F, (int) T, (int) Kp, 1) * sizeof(double), false);
    launch_transpose(L.W, F, 0, WT.as<double>(), Kp, 0, (int) K, (int) F, 1, s);
    launch_transpose(L.X, F, 0, XT.as<double>(), T, 0, (int) T, (int) F, 1, s);
  }
  auto enqueue = [&](int64_t i) {
    // the factor 1 - ((i + 1) / iters) of :132 / :150 is 1 (identity) but on the last iteration, where it is 0
    const double* src = H;
    if ((i + 1) / L.iters == 1)
    {
      launch_cross_sparsity(H, Hs.as<double>(), ldh, (int) T, (int) K, (int) L.r, s);
      launch_cross_polyphony(Hs.as<double>(), ldh, (int) T, (int) K, denergy.as<double>(), (int) L.p, s);
      src = Hs.as<double>();
    }
    launch_cross_continuity(src, Hc.as<double>(), ldh, (int) T, (int) K, (int) L.c, s);
    if (wide)
    {
      launch_pad_copy(Hc.as<double>(), ldh, 0, HW.as<double>(), Kp, 0, (int) T, (int) K, 1, s);
      UpdateArgs a{};
      a.V = XT.as<double>(); a.ldv = T; a.strideV = 0;
      a.Mv = WT.as<double>(); a.strideM = 0;
      a.S = HW.as<double>(); a.strideS = 0;
      a.R = (int) F; a.C = (int) T; a.B = 1; a.Kp = (int) Kp; a.nsplit = 1;
      launch_nmf_update_wide(a, wideScr.as<double>(), s);
      launch_pad_copy(HW.as<double>(), Kp, 0, H, ldh, 0, (int) T, (int) K, 1, s);
      return;
    }
    CrossGemm g1;
    g1.A = Hc.as<double>(); g1.lda = ldh; g1.B = L.W; g1.ldb = F; g1.C = Q.as<double>(); g1.ldc = F;
    g1.M = T; g1.N = F; g1.Kd = K; g1.V = L.X; g1.ldv = F;
    launch_cross_gemm(g1, 0, 1, kCrossEpiRatio, p1, part.as<double>(), s);
    CrossGemm g2;
    g2.A = Q.as<double>(); g2.lda = F; g2.B = L.W; g2.ldb = F; g2.C = H; g2.ldc = ldh;
    g2.M = T; g2.N = K; g2.Kd = F; g2.Hc = Hc.as<double>(); g2.ldh = ldh; g2.den = dsum.as<double>();
    launch_cross_gemm(g2, 0, 0, kCrossEpiHUpdate, p2, part.as<double>(), s);
  };
  if (!progress)
  {
    for (int64_t i = 0; i < L.iters; i++) enqueue(i);
    HIPCHK(ctx, hipGetLastError());
    return FLUHIP_OK;
  }
  // one event per iteration, taken once for the call and given back on every way out (no per-call leak)
  constexpr int kMaxLag = 64;
  const int kLag = std::max(1, std::min(kMaxLag, ctx->progressLag));
  hipEvent_t ev[kMaxLag];
  for (int i = 0; i < kLag; i++) ev[i] = take_event(ctx);
  struct GiveBack
  {
    fluhip_ctx* ctx;
    hipEvent_t* ev;
    int n;
    ~GiveBack() { for (int i = 0; i < n; i++) if (ev[i]) ctx->eventPool.push_back(ev[i]); }
  } giveBack{ctx, ev, kLag};
  int64_t reported = 0;
  for (int64_t i = 0; i < L.iters; i++)
  {
    enqueue(i);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[i % kLag], s));
    const int64_t enq = i + 1;
    while (reported < enq)
    {
      const bool mustWait = enq - reported >= kLag || enq == L.iters;
      const hipError_t q = mustWait ? hipEventSynchronize(ev[reported % kLag]) : hipEventQuery(ev[reported % kLag]);
      if (q == hipErrorNotReady) break;
      if (q != hipSuccess) return fail_hip(ctx, q, "the NMFCross iteration loop");
      reported++;
      if (!progress(reported, user))
      {
        (void) hipStreamSynchronize(s);
        return fail(ctx, "cancelled", FLUHIP_CANCELLED);
      }
    }
  }
  return FLUHIP_OK;
}

// GriffinLim::process on a device spectrum [T][F] (in and out); the random phase is drawn on the host
int griffinlim_dev(fluhip_ctx* ctx, double* spec, int64_t T, int64_t F, int64_t nSamples, int64_t iters, int64_t win,
                   int64_t fft, int64_t hop, int64_t seed)
{
  hipStream_t s = ctx->stream;
  StftSetup st;
  int rc = stft_setup(ctx, win, fft, hop, &st);
  if (rc) return rc;
  const int64_t n = T * F;
  DevBuf mag, phase, est, prev, tmp, frames;
  DEV_ALLOC(ctx, "NMFCross", mag, (size_t) n * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", phase, (size_t) n * 2 * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", est, (size_t) n * 2 * sizeof(double), true);  // estimate = 0 (:39)
  DEV_ALLOC(ctx, "NMFCross", prev, (size_t) n * 2 * sizeof(double), true);
  DEV_ALLOC(ctx, "NMFCross", tmp, (size_t) nSamples * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", frames, (size_t) (T * win) * sizeof(double), false);
  // magnitude = |in| (:37)
  launch_mag_hypot(spec, (int) T, (int) F, mag.as<double>(), F, s);
  // phase = EigenRandomPhase<ArrayXXcd>(T, F, seed) (:38, util/EigenRandom.hpp:147-160): column-major, entry (t, f) is draw
  // f T + t of uniform_real_distribution(0, 2 pi) = 2 pi u + 0, then std::polar(1, theta)
  {
    std::vector<double> u, ph((size_t) n * 2);
    draw_uniform(seed, (size_t) n, u);
    const double twopi = 2 * M_PI;
    for (int64_t f = 0; f < F; f++)
      for (int64_t t = 0; t < T; t++)
      {
        const double th = twopi * u[(size_t) (f * T + t)] + 0.0;
        ph[(size_t) (2 * (t * F + f))] = std::cos(th);
        ph[(size_t) (2 * (t * F + f) + 1)] = std::sin(th);
      }
    HIPCHK(ctx, hipMemcpyAsync(phase.p, ph.data(), ph.size() * sizeof(double), hipMemcpyHostToDevice, s));
    launch_gl_apply(mag.as<double>(), phase.as<double>(), spec, n, s);
    HIPCHK(ctx, hipStreamSynchronize(s));
  }
  ResynthArgs ra = st.resynth(spec, T, frames.as<double>(), nSamples, win / 2); // ISTFT::process
  ra.out = tmp.as<double>();
  StftArgs sa = st.args(nullptr, tmp.as<double>(), nSamples, nSamples, 1, T, -(win / 2)); // STFT::process
  sa.specStride = n * 2;
  double* e = est.as<double>();
  double* pv = prev.as<double>();
  for (int64_t i = 0; i < iters; i++)
  {
    std::swap(e, pv);                 // prev = estimate (:41)
    if ((rc = st.launch(ctx, ra))) return rc; // istft(magnitude * phase) (:42-43)
    sa.spec = e;
    if ((rc = st.launch(ctx, sa))) return rc; // estimate = stft(tmp) (:44)
    launch_gl_update(mag.as<double>(), e, pv, spec, n, s); // phase update (:45-46); spec = magnitude * phase
    HIPCHK(ctx, hipGetLastError());
  }
  return FLUHIP_OK;
}

int nmfcross_process_impl(fluhip_ctx* ctx, const double* X, int64_t T, int64_t F, int64_t ldx, const double* W0, int64_t K,
                          int64_t ldw, int64_t r, int64_t p, int64_t c, int64_t iters, int64_t seed, double* H1,
                          fluhip_progress_fn progress, void* user)
{
  if (!X || !W0 || !H1) return fail(ctx, "null buffer");
  if (T < 1 || F < 1 || K < 1) return fail(ctx, "empty matrix");
  if (ldx < F || ldw < F) return fail(ctx, "row stride below the number of bins");
  if (r < 1 || c < 1) return fail(ctx, "time sparsity and continuity must be >= 1");
  if (p < 1 || p > K) return fail(ctx, "polyphony must be in [1, rank]");
  if (iters < 0) return fail(ctx, "negative iteration count");
  if (T > INT32_MAX || K > INT32_MAX) return fail(ctx, "too many frames");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf dX, dW, dH;
  DEV_ALLOC(ctx, "NMFCross", dX, (size_t) (T * F) * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", dW, (size_t) (K * F) * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", dH, (size_t) (T * K) * sizeof(double), false);
  HIPCHK(ctx, hipMemcpy2DAsync(dX.p, (size_t) F * sizeof(double), X, (size_t) ldx * sizeof(double), (size_t) F * sizeof(double),
                               (size_t) T, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipMemcpy2DAsync(dW.p, (size_t) F * sizeof(double), W0, (size_t) ldw * sizeof(double), (size_t) F * sizeof(double),
                               (size_t) K, hipMemcpyHostToDevice, s));
  CrossLoop L{ctx, dX.as<double>(), dW.as<double>(), T, F, K, r, p, c, iters, seed, dH.as<double>()};
  int rc = cross_loop(L, progress, user);
  if (rc) return rc;
  // (the reference's closing V = W H, :185, is never read: not computed)
  const size_t nb = (size_t) (T * K) * sizeof(double);
  if ((rc = copy_to_host(ctx, H1, nb, dH.p, nb, nb, 1, s))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

int griffinlim_impl(fluhip_ctx* ctx, double* spec, int64_t T, int64_t F, int64_t nSamples, int64_t iters, int64_t win,
                    int64_t fft, int64_t hop, int64_t seed)
{
  if (!spec) return fail(ctx, "null buffer");
  if (iters < 0) return fail(ctx, "negative iteration count");
  int rc = check_shape(ctx, nSamples, win, fft, hop, 1);
  if (rc) return rc;
  if (F != fft / 2 + 1) return fail(ctx, "bins must be fft / 2 + 1");
  if (T != (nSamples + hop) / hop) return fail(ctx, "frames must be (n_samples + hop) / hop");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf d;
  const size_t nb = (size_t) (T * F) * 2 * sizeof(double);
  DEV_ALLOC(ctx, "NMFCross", d, nb, false);
  HIPCHK(ctx, hipMemcpyAsync(d.p, spec, nb, hipMemcpyHostToDevice, s));
  if ((rc = griffinlim_dev(ctx, d.as<double>(), T, F, nSamples, iters, win, fft, hop, seed))) return rc;
  if ((rc = copy_to_host(ctx, spec, nb, d.p, nb, nb, 1, s))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

// STFT::process of a strided float channel: spectrum [T][F] interleaved, magnitudes [T][F] by hypot (STFT::magnitude)
int cross_stft(fluhip_ctx* ctx, const float* audio, int64_t n, int64_t stride, int64_t win, int64_t fft, int64_t hop,
               DevBuf& spec, DevBuf& mag)
{
  hipStream_t s = ctx->stream;
  const int64_t T = (n + hop) / hop, F = fft / 2 + 1;
  StftSetup st;
  int rc = stft_setup(ctx, win, fft, hop, &st);
  if (rc) return rc;
  DevBuf in;
  DEV_ALLOC(ctx, "NMFCross", in, (size_t) n * sizeof(float), false);
  HIPCHK(ctx, upload_strided(in.p, audio, (size_t) n, (size_t) stride, sizeof(float), s));
  DEV_ALLOC(ctx, "NMFCross", spec, (size_t) (T * F) * 2 * sizeof(double), false);
  DEV_ALLOC(ctx, "NMFCross", mag, (size_t) (T * F) * sizeof(double), false);
  StftArgs a = st.args(in.as<float>(), nullptr, n, n, 1, T, -(win / 2));
  a.spec = spec.as<double>(); a.specStride = T * F * 2;
  if ((rc = st.launch(ctx, a))) return rc;
  launch_mag_hypot(spec.as<double>(), (int) T, (int) F, mag.as<double>(), F, s);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(s)); // (`in` is released behind the launches)
  return FLUHIP_OK;
}

int bufnmfcross_impl(fluhip_ctx* ctx, const float* source, int64_t nSrc, int64_t srcStride, const float* target, int64_t nTgt,
                     int64_t tgtStride, int64_t win, int64_t fft, int64_t hop, int64_t r, int64_t p, int64_t c, int64_t iters,
                     int64_t seed, float* out, fluhip_progress_fn progress, void* user)
{
  if (!source || !target || !out) return fail(ctx, "null buffer");
  if (srcStride < 1 || tgtStride < 1) return fail(ctx, "stride must be >= 1");
  if (win < 1 || hop < 1) return fail(ctx, "window and hop sizes must be positive");
  const int64_t srcWindows = (nSrc + hop) / hop, tgtWindows = (nTgt + hop) / hop; // NMFCrossClient.hpp:104-109
  // :111-118, in the reference's order
  if (nSrc <= 0) return fail(ctx, "Empty source buffer");
  if (nTgt <= 0) return fail(ctx, "Empty target buffer");
  if (r > tgtWindows) return fail(ctx, "Time Sparsity is larger than target frames");
  if (c > tgtWindows) return fail(ctx, "Continuity is larger than target frames");
  if (r < 1 || c < 1 || p < 1) return fail(ctx, "time sparsity, polyphony and continuity must be >= 1");
  if (iters < 1) return fail(ctx, "iterations must be >= 1");
  int rc = check_shape(ctx, nSrc, win, fft, hop, 1);
  if (rc) return rc;
  if ((rc = check_shape(ctx, nTgt, win, fft, hop, 1))) return rc;
  const int64_t F = fft / 2 + 1, K = srcWindows, T = tgtWindows;
  if (T > INT32_MAX || K > INT32_MAX) return fail(ctx, "too many frames");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf srcSpec, srcMag, tgtSpec, tgtMag, H, result, dout;
  if ((rc = cross_stft(ctx, source, nSrc, srcStride, win, fft, hop, srcSpec, srcMag))) return rc;
  if ((rc = cross_stft(ctx, target, nTgt, tgtStride, win, fft, hop, tgtSpec, tgtMag))) return rc;
  tgtSpec.release();
  DEV_ALLOC(ctx, "NMFCross", H, (size_t) (T * K) * sizeof(double), false);
  // nmf.process(tgtMag, outputEnvelopes, W, r, min(srcWindows, p), c, seed) (:157-159)
  CrossLoop L{ctx, tgtMag.as<double>(), srcMag.as<double>(), T, F, K, r, std::min(srcWindows, p), c, iters, seed, H.as<double>()};
  if ((rc = cross_loop(L, progress, user))) return rc;
  tgtMag.release();
  srcMag.release();
  auto step = [&](int64_t k) -> int {
    if (!progress) return FLUHIP_OK;
    HIPCHK(ctx, hipStreamSynchronize(s));
    return progress(k, user) ? FLUHIP_OK : fail(ctx, "cancelled", FLUHIP_CANCELLED);
  };
  // NMFCross::synthesize (:49-57): result [T][2F] = H1 [T][K] . srcSpectrum [K][2F] -- one real GEMM over the interleaved
  // complex matrix
  DEV_ALLOC(ctx, "NMFCross", result, (size_t) (T * F) * 2 * sizeof(double), false);
  {
    const int cus = std::max(1, ctx->props.multiProcessorCount);
    const CrossGemmPlan ps = cross_gemm_plan(T, 2 * F, K, cus);
    DevBuf part;
    DEV_ALLOC(ctx, "NMFCross", part, (size_t) std::max<int64_t>(ps.partDoubles, 1) * sizeof(double), false);
    CrossGemm g;
    g.A = H.as<double>(); g.lda = K; g.B = srcSpec.as<double>(); g.ldb = 2 * F; g.C = result.as<double>(); g.ldc = 2 * F;
    g.M = T; g.N = 2 * F; g.Kd = K;
    launch_cross_gemm(g, 0, 1, kCrossEpiStore, ps, part.as<double>(), s);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = step(iters + 1))) return rc;
  }
  H.release();
  srcSpec.release();
  // gl.process(result, tgtFrames, 50, win, fft, hop, seed) (:168-170)
  if ((rc = griffinlim_dev(ctx, result.as<double>(), T, F, nTgt, 50, win, fft, hop, seed))) return rc;
  if ((rc = step(iters + 2))) return rc;
  // istft.process(result, resultAudio) (:175): tgtFrames samples, to float
  {
    StftSetup st;
    if ((rc = stft_setup(ctx, win, fft, hop, &st))) return rc;
    DevBuf frames;
    DEV_ALLOC(ctx, "NMFCross", frames, (size_t) (T * win) * sizeof(double), false);
    DEV_ALLOC(ctx, "NMFCross", dout, (size_t) nTgt * sizeof(float), false);
    ResynthArgs ra = st.resynth(result.as<double>(), T, frames.as<double>(), nTgt, win / 2);
    ra.out32 = dout.as<float>();
    if ((rc = st.launch(ctx, ra))) return rc;
    HIPCHK(ctx, hipGetLastError());
    if ((rc = step(iters + 3))) return rc;
  }
  const size_t nb = (size_t) nTgt * sizeof(float);
  if ((rc = copy_to_host(ctx, out, nb, dout.p, nb, nb, 1, s))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

// Diagnostic: one constraint stencil of the H loop -- the launch the clients share -- on the caller's own doubles.
// H, out [T][K]; which 0: continuity (size = c), 1: temporal sparsity on its zeroing iteration (size = r), 2: polyphony
// on its zeroing iteration (size = p, energy [K]; the kernel works in place, so it runs on the device copy of H)
int debug_cross_stencil_impl(fluhip_ctx* ctx, const double* H, int64_t T, int64_t K, int which, int64_t size,
                             const double* energy, double* out)
{
  const char* me = "fluhip_debug_cross_stencil_f64: ";
  if (!H || !out) return fail(ctx, std::string(me) + "null H or out");
  if (which < 0 || which > 2) return fail(ctx, std::string(me) + "which must be 0 (continuity), 1 (sparsity) or 2 (polyphony)");
  if (which == 2 && !energy) return fail(ctx, std::string(me) + "polyphony needs energy");
  if (T < 1 || K < 1) return fail(ctx, std::string(me) + "T and K must be >= 1");
  if (T > INT32_MAX || K > INT32_MAX) return fail(ctx, std::string(me) + "too many frames");
  if (size < 1 || size > (1 << 20)) return fail(ctx, std::string(me) + "size must be from 1 to 1048576");
  if (which == 2 && size > K) return fail(ctx, std::string(me) + "polyphony must be in [1, K]");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const size_t nb = (size_t) (T * K) * sizeof(double);
  DevBuf dH, dOut, dE;
  DEV_ALLOC(ctx, "NMFCross", dH, nb, false);
  HIPCHK(ctx, hipMemcpyAsync(dH.p, H, nb, hipMemcpyHostToDevice, s));
  const double* res = dH.as<double>();
  if (which == 2)
  {
    DEV_ALLOC(ctx, "NMFCross", dE, (size_t) K * sizeof(double), false);
    HIPCHK(ctx, hipMemcpyAsync(dE.p, energy, (size_t) K * sizeof(double), hipMemcpyHostToDevice, s));
    launch_cross_polyphony(dH.as<double>(), K, (int) T, (int) K, dE.as<double>(), (int) size, s);
  }
  else
  {
    DEV_ALLOC(ctx, "NMFCross", dOut, nb, false);
    if (which == 0) launch_cross_continuity(dH.as<double>(), dOut.as<double>(), K, (int) T, (int) K, (int) size, s);
    else launch_cross_sparsity(dH.as<double>(), dOut.as<double>(), K, (int) T, (int) K, (int) size, s);
    res = dOut.as<double>();
  }
  HIPCHK(ctx, hipGetLastError());
  int rc = copy_to_host(ctx, out, nb, res, nb, nb, 1, s);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

} // namespace

extern "C" {

int fluhip_debug_cross_stencil_f64(fluhip_ctx* ctx, const double* H, int64_t T, int64_t K, int which, int64_t size,
                                   const double* energy, double* out)
{
  return guarded(ctx, [&] { return debug_cross_stencil_impl(ctx, H, T, K, which, size, energy, out); });
}

int fluhip_debug_cross_plan(fluhip_ctx* ctx, int64_t M, int64_t N, int64_t Kd, int64_t* out3)
{
  if (!ctx || !out3 || M < 1 || N < 1 || Kd < 1) return FLUHIP_ERROR;
  const CrossGemmPlan p = cross_gemm_plan(M, N, Kd, std::max(1, ctx->props.multiProcessorCount));
  out3[0] = p.big ? 1 : 0;
  out3[1] = p.nsplit;
  out3[2] = p.kChunk;
  return FLUHIP_OK;
}

int fluhip_nmfcross_process_f64(fluhip_ctx* ctx, const double* X, int64_t T, int64_t F, int64_t ldx, const double* W0,
                                int64_t K, int64_t ldw, int64_t time_sparsity, int64_t polyphony, int64_t continuity,
                                int64_t iters, int64_t seed, double* H1, fluhip_progress_fn progress, void* user)
{
  return guarded(ctx, [&] {
    return nmfcross_process_impl(ctx, X, T, F, ldx, W0, K, ldw, time_sparsity, polyphony, continuity, iters, seed, H1,
                                 progress, user);
  });
}

int fluhip_griffinlim_f64(fluhip_ctx* ctx, double* spec, int64_t T, int64_t F, int64_t n_samples, int64_t iters,
                          int64_t win, int64_t fft, int64_t hop, int64_t seed)
{
  return guarded(ctx, [&] { return griffinlim_impl(ctx, spec, T, F, n_samples, iters, win, fft, hop, seed); });
}

int fluhip_bufnmfcross_f32(fluhip_ctx* ctx, const float* source, int64_t n_src, int64_t src_stride, const float* target,
                           int64_t n_tgt, int64_t tgt_stride, int64_t win, int64_t fft, int64_t hop,
                           int64_t time_sparsity, int64_t polyphony, int64_t continuity, int64_t iters, int64_t seed,
                           float* out, fluhip_progress_fn progress, void* user)
{
  return guarded(ctx, [&] {
    return bufnmfcross_impl(ctx, source, n_src, src_stride, target, n_tgt, tgt_stride, win, fft, hop, time_sparsity,
                            polyphony, continuity, iters, seed, out, progress, user);
  });
}

} // extern "C"
