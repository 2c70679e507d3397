// api_corpus.hip -- the corpus level of the C ABI: B equal-shape (or ragged) buffers resident in HBM, their workspaces as the
// plan sizes them (corpus_plan.hip), the STFT and factor initialisation, and the fluhip_corpus_* entry points around the
// iteration loop (corpus_loop.hip).
//   NMF::multiplicativeUpdates             include/flucoma/algorithms/public/NMF.hpp:144-183
//   bufnmf::NMFClient::process write-back  include/flucoma/clients/nrt/NMFClient.hpp:277-300
#include "corpus_internal.h"

// the two work lists of a list plan onto the device
static int plan_lists(fluhip_ctx* ctx, fluhip_corpus* c, const ListPlanHost& plan)
{
  auto upload = [&](DevBuf& dst, const void* src, size_t bytes) -> int {
    HIPCHK(ctx, dst.alloc(bytes, false, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // the host image may go out of scope
    return FLUHIP_OK;
  };
  auto take = [&](fluhip_corpus::WorkList& dst, const ListSide& src) -> int {
    dst.wgs = src.wgs; dst.ng = src.ng; dst.partial = src.partial; dst.maxSplit = src.maxSplit;
    if (int rc = upload(dst.list, src.list.data(), src.list.size() * sizeof(WaveDesc))) return rc;
    return upload(dst.splitTab, src.splitTab.data(), src.splitTab.size() * sizeof(int));
  };
  if (int rc = take(c->listW, plan.W)) return rc;
  return take(c->listH, plan.H);
}

// the plan of the corpus's shape onto the corpus + its workspaces; needs B, T, F, Tp, Fp, K, Kp (ragged: tOf)
int plan_updates(fluhip_ctx* ctx, fluhip_corpus* c)
{
  hipStream_t s = ctx->stream;
  UpdatePlan& p = c->plan;
  ListPlanHost lists;
  if (c->ragged) decide_list_plan(c->tOf, c->T, c->F, c->K, p, lists);
  else decide_update_plan(c->B, c->T, c->F, c->K, p, &lists);
  if (p.Kp != c->Kp) return fail(ctx, "internal error: the plan's padded rank is not the corpus's");
  if (p.useLists)
    if (int rc = plan_lists(ctx, c, lists)) return rc;
  auto bytes = [](int64_t doubles) { return (size_t) doubles * sizeof(double); };
  if (p.wideDoubles) HIPCHK(ctx, c->wideScratch.alloc(bytes(p.wideDoubles), false, s));
  // (stripPart zeroed once: with the Nyquist bin as a side column only 16 values of its partial blocks are ever written, and the
  //  reduce launch adds the whole blocks before it masks the bins that do not exist)
  if (p.stripPartDoubles) HIPCHK(ctx, c->stripPart.alloc(bytes(p.stripPartDoubles), true, s));
#ifdef FLUHIP_AB_SWITCHES
  if (p.stripBin)
    HIPCHK(ctx, c->binWork.alloc((size_t) nmf_binstrip_doubles((int) c->F, (int) c->T, (int) c->B) * sizeof(double), true, s));
  if (p.stripTile)
    HIPCHK(ctx, c->tileWork.alloc((size_t) nmf_bintile_doubles((int) c->F, (int) c->B, nmf_strip_workgroups((int) c->T)) * sizeof(double), true, s));
#endif
  if (p.variant != 0)
  {
    if (p.partDoubles) HIPCHK(ctx, c->part.alloc(bytes(p.partDoubles), true, s));
    HIPCHK(ctx, c->dpart.alloc(bytes(p.dpartDoubles), true, s));
    if (p.csumDoubles) HIPCHK(ctx, c->csumScratch.alloc(bytes(p.csumDoubles), false, s));
  }
  HIPCHK(ctx, c->clk.alloc(8 * sizeof(long long), true, s));
  if (p.lazy && p.variant != 0)
  {
    HIPCHK(ctx, c->wnorm.alloc((size_t) c->B * c->Kp * sizeof(double), false, s));
    launch_fill_ones(c->wnorm.as<double>(), (int64_t) (c->B * c->Kp), s);
    HIPCHK(ctx, c->wscratch.alloc(bytes(p.wscratchDoubles), true, s));
    if (p.colPartDoubles) HIPCHK(ctx, c->colPart.alloc(bytes(p.colPartDoubles), true, s));
  }
  return FLUHIP_OK;
}

int corpus_alloc(fluhip_ctx* ctx, fluhip_corpus* c)
{
  hipStream_t s = ctx->stream;
  c->T = (c->n + c->hop) / c->hop; // alg/STFT.hpp:98-99; nrt/NMFClient.hpp:111-112
  c->F = c->fft / 2 + 1;
  c->Tp = round_up(c->T, 32);
  c->Fp = round_up(c->F, 32);
  c->Kp = padded_rank(c->K);
  const size_t B = (size_t) c->B;
  HIPCHK(ctx, c->mag.alloc(B * c->Tp * c->Fp * sizeof(double), true, s));
  // (a corpus that only ever transforms -- algorithm::STFT::process / magnitude at the algorithm level, fluhip_stft_* -- has one
  //  layout of the magnitudes and no factor workspaces: the bin-major copy exists for the H update alone)
  if (c->stftOnly) return FLUHIP_OK;
  HIPCHK(ctx, c->magT.alloc(B * c->Fp * c->Tp * sizeof(double), true, s));
  HIPCHK(ctx, c->Wf.alloc(B * c->Fp * c->Kp * sizeof(double), true, s));
  HIPCHK(ctx, c->H1.alloc(B * c->Tp * c->Kp * sizeof(double), true, s));
  HIPCHK(ctx, c->hmax.alloc(B * sizeof(double), true, s));
  if (c->ragged)
  {
    HIPCHK(ctx, c->nTab.alloc(B * sizeof(int64_t), false, s));
    HIPCHK(ctx, c->tTab.alloc(B * sizeof(int), false, s));
    HIPCHK(ctx, hipMemcpyAsync(c->nTab.p, c->nOf.data(), B * sizeof(int64_t), hipMemcpyHostToDevice, s));
    HIPCHK(ctx, hipMemcpyAsync(c->tTab.p, c->tOf.data(), B * sizeof(int), hipMemcpyHostToDevice, s));
  }
  return plan_updates(ctx, c);
}

// launch-geometry limits of the factor-update paths, refused up front with a message instead of surfacing as an
// "invalid configuration" launch error: the normalisation kernels put the padded rank in one workgroup (<= 1024
// threads), and the any-rank path (rank above 128, kernels_nmf_wide.hip) puts frames / bins in gridDim.y (<= 65535)
int check_rank(fluhip_ctx* ctx, int64_t T, int64_t F, int64_t K)
{
  if (padded_rank(K) > 1024) return fail(ctx, "ranks above 1024 are not supported");
  if (padded_rank(K) > 128 && std::max(T, F) > 65535)
    return fail(ctx, "ranks above 128 are limited to 65535 frames and bins");
  return FLUHIP_OK;
}

int check_shape(fluhip_ctx* ctx, int64_t n, int64_t win, int64_t fft, int64_t hop, int64_t K)
{
  if (n <= 0) return fail(ctx, "not enough frames");
  if (win < 1 || hop < 1) return fail(ctx, "window and hop sizes must be positive");
  if (fft < 4 || (fft & (fft - 1)) || fft < win)
    return fail(ctx, "fft size must be a power of two >= window size");
  if (!stft_supported(win, fft))
    return fail(ctx, "fft sizes above 65536 are not supported");
  if (K < 1) return fail(ctx, "rank must be >= 1");
  if ((n + hop) / hop > 2000000000LL / 16) return fail(ctx, "too many frames");
  return check_rank(ctx, (n + hop) / hop, fft / 2 + 1, K);
}

int corpus_stft(fluhip_corpus* c, const float* a32, const double* a64, int64_t audioStride, bool magOnly)
{
  // magOnly: the frame-major magnitudes alone (what STFT::process + STFT::magnitude compute, alg/STFT.hpp:90-108, 61-66);
  // the bin-major copy is written for the factor updates only -- half the kernel's store traffic
  fluhip_ctx* ctx = c->ctx;
  StftSetup st;
  const int rc = stft_setup(ctx, c->win, c->fft, c->hop, &st, c->windowType);
  if (rc) return rc;
  if (c->keepSpec && !c->spec.p)
    HIPCHK(ctx, c->spec.alloc((size_t) c->B * c->T * c->F * 2 * sizeof(double), false, ctx->stream));
  StftArgs a = st.args(a32, a64, c->n, audioStride, c->B, c->T, -(c->win / 2)); // STFT::process
  a.mag = c->mag.as<double>(); a.magStride = c->Tp * c->Fp; a.ldMag = c->Fp;
  a.spec = c->keepSpec ? c->spec.as<double>() : nullptr; a.specStride = c->T * c->F * 2;
  a.nTab = c->ragged ? c->nTab.as<int64_t>() : nullptr;
  a.bigScratch = big_fft_scratch(ctx, c->win, c->fft, c->B * c->T);
  if (stft_needs_scratch(c->win, c->fft) && !a.bigScratch) return FLUHIP_ERROR;
  // V is kept in both layouts (frame-major for the W update, bin-major for the H update).  The block form of K1
  // writes both in one pass; shapes it does not cover take the wave / generic kernel and a transposing copy.
  bool both = false;
  {
    ProfScope p(ctx, 0);
    if (!stft_needs_scratch(c->win, c->fft))
      both = launch_stft_block(a, magOnly ? nullptr : c->magT.as<double>(), c->Fp * c->Tp, c->Tp, ctx->stream);
    if (!both && c->ragged) return fail(ctx, "ragged corpora need an STFT shape with a block form (fft 1024 / 2048 / 4096, even window)");
    if (!both) launch_stft(a, ctx->stream);
  }
  if (!both && !magOnly)
  {
    ProfScope p(ctx, 4);
    launch_transpose(c->mag.as<double>(), c->Fp, c->Tp * c->Fp, c->magT.as<double>(), c->Tp,
                     c->Fp * c->Tp, (int) c->T, (int) c->F, (int) c->B, ctx->stream);
  }
  HIPCHK(ctx, hipGetLastError());
  c->haveMag = !magOnly;   // (the factor updates need both layouts)
  c->touched = true;
  return FLUHIP_OK;
}

// util/EigenRandom.hpp:73-101: std::mt19937_64 g{seed ? *seed : rd()} +
// std::uniform_real_distribution<double>{0, 1}; one draw per coefficient in Eigen's column-major
// linear order.  libstdc++'s <random> is used verbatim, exactly as the reference does.
void draw_uniform(int64_t seed, size_t count, std::vector<double>& out)
{
  std::random_device rd;
  std::mt19937_64 g{seed >= 0 ? (size_t) seed : (size_t) rd()};
  std::uniform_real_distribution<double> d{0.0, 1.0};
  out.resize(count);
  for (size_t i = 0; i < count; i++) out[i] = d(g);
}

// The source of one factor (`count` = F K or T K coefficients per buffer) onto the device, in `stage`: the float seeds [B][count],
// else doubles -- the caller's host image (one shared, or one per buffer), or uniform draws (one shared seed, or per-buffer
// seeds, equal seeds drawn once).  *nsrc: images staged (1: every buffer takes the same).  `host` keeps what was drawn.
static int stage_factor(fluhip_corpus* c, const float* f32, const double* src, bool shared, int64_t seed, const int64_t* seeds,
                        size_t count, std::vector<double>& host, DevBuf& stage, int* nsrc)
{
  fluhip_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  const int B = (int) c->B;
  if (f32)
  {
    HIPCHK(ctx, stage.alloc((size_t) B * count * sizeof(float), false, s));
    HIPCHK(ctx, hipMemcpyAsync(stage.p, f32, (size_t) B * count * sizeof(float), hipMemcpyHostToDevice, s));
    return FLUHIP_OK;
  }
  *nsrc = src ? (shared ? 1 : B) : 1;
  if (!src)
  {
    if (seeds)
    {
      *nsrc = B;
      host.resize((size_t) B * count);
      std::vector<double> tmp;
      std::map<int64_t, int> seen;
      for (int b = 0; b < B; b++)
      {
        auto it = seeds[b] >= 0 ? seen.find(seeds[b]) : seen.end();
        if (it != seen.end())
          std::memcpy(&host[(size_t) b * count], &host[(size_t) it->second * count], count * sizeof(double));
        else
        {
          draw_uniform(seeds[b], count, tmp);
          std::memcpy(&host[(size_t) b * count], tmp.data(), count * sizeof(double));
          if (seeds[b] >= 0) seen[seeds[b]] = b;
        }
      }
    }
    else
      draw_uniform(seed, count, host); // alg/NMF.hpp:104-105, 116-117 (each factor: a fresh generator from the same seed)
    src = host.data();
  }
  HIPCHK(ctx, stage.alloc((size_t) *nsrc * count * sizeof(double), false, s));
  HIPCHK(ctx, hipMemcpyAsync(stage.p, src, (size_t) *nsrc * count * sizeof(double), hipMemcpyHostToDevice, s));
  return FLUHIP_OK;
}

int corpus_init_factors(fluhip_corpus* c, int64_t seed, const int64_t* seeds,
                               const FactorInit& fi)
{
  fluhip_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  const size_t FK = (size_t) c->F * c->K, TK = (size_t) c->T * c->K;
  const int B = (int) c->B;
  // The draws run on the calling thread while the device is still busy with whatever was enqueued before (the STFT
  // of this job); the host images stay alive to the single synchronisation at the end, so the two uploads and the
  // scatter kernels queue up behind each other without a host round trip in between.
  std::vector<double> hostW, hostH;
  DevBuf stageH;
  int nsrc = 1;
  // --- W ---
  if (int rc = stage_factor(c, fi.W0f32, fi.W0host, fi.sharedW, seed, seeds, FK, hostW, c->stage, &nsrc)) return rc;
  if (fi.W0f32)
    launch_scatter_factor_f32(c->stage.as<float>(), (int64_t) FK, c->Wf.as<double>(), c->Fp * c->Kp,
                              (int) c->F, (int) c->K, (int) c->Kp, B, s);
  else
    // K x F row-major source (random: column-major F x K fill; seeded: W0 transposed, :102-112)
    launch_scatter_factor(c->stage.as<double>(), nsrc == 1 ? 0 : (int64_t) FK, c->Wf.as<double>(),
                          c->Fp * c->Kp, (int) c->F, (int) c->K, (int) c->Kp, B, true, s);
  // --- H ---
  if (int rc = stage_factor(c, fi.H0f32, fi.H0host, fi.sharedH, seed, seeds, TK, hostH, stageH, &nsrc)) return rc;
  if (fi.H0f32)
    launch_scatter_factor_f32(stageH.as<float>(), (int64_t) TK, c->H1.as<double>(), c->Tp * c->Kp,
                              (int) c->T, (int) c->K, (int) c->Kp, B, s, c->ragged ? c->tTab.as<int>() : nullptr);
  else
    // T x K row-major source (random: column-major K x T fill; seeded: H0 transposed, :113-124)
    launch_scatter_factor(stageH.as<double>(), nsrc == 1 ? 0 : (int64_t) TK, c->H1.as<double>(),
                          c->Tp * c->Kp, (int) c->T, (int) c->K, (int) c->Kp, B, false, s,
                          c->ragged ? c->tTab.as<int>() : nullptr); // (K x T_b column-major = the first T_b K draws)
  // alg/NMF.hpp:150-153: clamp both to eps, normalise columns of W and rows of H (= columns of H1)
  if (!c->normScratch.p)
  {
    const size_t nd = (size_t) colnorm_scratch_doubles((int) std::max(c->T, c->F), (int) c->Kp, B);
    HIPCHK(ctx, c->normScratch.alloc(nd * sizeof(double), false, s));
  }
  launch_colnorm(c->H1.as<double>(), c->Tp * c->Kp, (int) c->T, (int) c->K, (int) c->Kp, B, true, false,
                 c->normScratch.as<double>(), s, c->ragged ? c->tTab.as<int>() : nullptr);
  launch_colnorm(c->Wf.as<double>(), c->Fp * c->Kp, (int) c->F, (int) c->K, (int) c->Kp, B, true, false,
                 c->normScratch.as<double>(), s);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(s)); // the host images and the second staging buffer go out of scope
  c->haveFactors = true;
  c->run.stripStatsValid = false;
  return FLUHIP_OK;
}

// ---------------------------------------------------------------------------------------
// C ABI
// Host allocations inside the library (std::vector images of seeds, plans, staging) can throw: nothing may cross the C ABI.
// std::bad_alloc is classified like a device out-of-memory (fluhip_last_error_is_out_of_memory), anything else is an error.
// (The corpus entry points keep this guard of their own: its texts differ from api_internal.h's `guarded`.)
template <typename Fn> static int guarded_corpus(fluhip_ctx* ctx, Fn&& fn)
{
  try { return fn(); }
  catch (const std::bad_alloc&) { return fail_oom(ctx, "out of host memory inside libflucoma_hip"); }
  catch (const std::exception& e) { return fail(ctx, std::string("internal error: ") + e.what()); }
}

extern "C" {

static int fluhip_corpus_create_impl(fluhip_ctx* ctx, int64_t count, int64_t n, int64_t win, int64_t fft,
                         int64_t hop, int64_t K, fluhip_corpus** out)
{
  if (!ctx || !out) return FLUHIP_ERROR;
  *out = nullptr;
  if (count < 1) return fail(ctx, "corpus must hold at least one buffer");
  if (count > 65535) return fail(ctx, "a corpus holds at most 65535 buffers (split larger corpora into several)");
  int rc = check_shape(ctx, n, win, fft, hop, K);
  if (rc) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<fluhip_corpus> c(new fluhip_corpus);
  c->ctx = ctx; c->B = count; c->n = n; c->win = win; c->fft = fft; c->hop = hop; c->K = K;
  rc = corpus_alloc(ctx, c.get());
  if (rc) return rc;
  *out = c.release();
  return FLUHIP_OK;
}

int fluhip_corpus_create_ragged(fluhip_ctx* ctx, int64_t count, const int64_t* n, int64_t win, int64_t fft, int64_t hop,
                                int64_t K, fluhip_corpus** out)
{
  if (!ctx || !out) return FLUHIP_ERROR;
  *out = nullptr;
  if (!n || count < 1) return fail(ctx, "corpus must hold at least one buffer");
  if (count > 65535) return fail(ctx, "a corpus holds at most 65535 buffers (split larger corpora into several)");
  int64_t nmax = 0;
  for (int64_t i = 0; i < count; i++)
  {
    if (n[i] < 1) return fail(ctx, "buffer " + std::to_string(i) + ": not enough frames");
    nmax = std::max(nmax, n[i]);
  }
  int rc = check_shape(ctx, nmax, win, fft, hop, K);
  if (rc) return rc;
  // one set of launches over buffers of different lengths needs the work-list form of the factor-update kernel (padded
  // rank 16 / 32 / 64 / 128) and the block form of the STFT (it takes per-buffer lengths)
  if (update_variant((int) padded_rank(K)) != 5) return fail(ctx, "ragged corpora support ranks up to 128");
  if (!(fft == 1024 || fft == 2048 || fft == 4096) || (win % 2) != 0 || win > fft)
    return fail(ctx, "ragged corpora need an STFT shape with a block form (fft 1024 / 2048 / 4096, even window)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<fluhip_corpus> c(new fluhip_corpus);
  c->ctx = ctx; c->B = count; c->n = nmax; c->win = win; c->fft = fft; c->hop = hop; c->K = K;
  c->ragged = true;
  c->nOf.assign(n, n + count);
  c->tOf.resize((size_t) count);
  for (int64_t i = 0; i < count; i++) c->tOf[(size_t) i] = (int) ((n[i] + hop) / hop); // alg/STFT.hpp:98-99 per buffer
  rc = corpus_alloc(ctx, c.get());
  if (rc) return rc;
  *out = c.release();
  return FLUHIP_OK;
}

int64_t fluhip_corpus_frames_of(const fluhip_corpus* c, int64_t i)
{
  if (!c || i < 0 || i >= c->B) return 0;
  return c->ragged ? c->tOf[(size_t) i] : c->T;
}

int fluhip_corpus_set_audio_ragged_host(fluhip_corpus* c, const float* const* audio)
{
  if (!c || !audio) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  if (!c->ragged) return fail(ctx, "not a ragged corpus");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t) c->B * c->n * sizeof(float);
  if (c->audioOwn.bytes < bytes) HIPCHK(ctx, c->audioOwn.alloc(bytes, false, ctx->stream));
  // every buffer at its slot of the longest buffer's stride; the kernel never reads past a buffer's own length
  for (int64_t i = 0; i < c->B; i++)
  {
    if (!audio[i]) return fail(ctx, "buffer " + std::to_string(i) + ": null audio");
    HIPCHK(ctx, hipMemcpyAsync(c->audioOwn.as<float>() + i * c->n, audio[i], (size_t) c->nOf[(size_t) i] * sizeof(float),
                               hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  c->audioDev = c->audioOwn.as<float>();
  return FLUHIP_OK;
}

int fluhip_corpus_writeback_ragged_host(fluhip_corpus* c, float* const* bases, float* const* acts)
{
  if (!c) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf db, da;
  const size_t nb = (size_t) c->B * c->K * c->F * sizeof(float), na = (size_t) c->B * c->K * c->T * sizeof(float);
  if (bases) HIPCHK(ctx, db.alloc(nb, false, ctx->stream));
  if (acts) HIPCHK(ctx, da.alloc(na, false, ctx->stream));
  int rc = fluhip_corpus_writeback_dev(c, bases ? db.as<float>() : nullptr, acts ? da.as<float>() : nullptr);
  if (rc) return rc;
  for (int64_t i = 0; i < c->B; i++)
  {
    const int64_t Ti = fluhip_corpus_frames_of(c, i);
    if (bases && bases[i])
      HIPCHK(ctx, hipMemcpyAsync(bases[i], db.as<float>() + i * c->K * c->F, (size_t) c->K * c->F * sizeof(float),
                                 hipMemcpyDeviceToHost, ctx->stream));
    if (acts && acts[i]) // K rows of the buffer's own T_i frames out of rows of the longest buffer's length
      HIPCHK(ctx, hipMemcpy2DAsync(acts[i], (size_t) Ti * sizeof(float), da.as<float>() + i * c->K * c->T,
                                   (size_t) c->T * sizeof(float), (size_t) Ti * sizeof(float), (size_t) c->K,
                                   hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FLUHIP_OK;
}

void fluhip_corpus_destroy(fluhip_corpus* c)
{
  if (!c) return;
  (void) hipSetDevice(c->ctx->device);
  (void) hipStreamSynchronize(c->ctx->stream);
  delete c;
}

int64_t fluhip_corpus_frames(const fluhip_corpus* c) { return c ? c->T : 0; }
int64_t fluhip_corpus_bins(const fluhip_corpus* c) { return c ? c->F : 0; }
int64_t fluhip_corpus_device_bytes(const fluhip_corpus* c) { return c ? c->device_bytes() : 0; }

static int fluhip_corpus_set_audio_host_impl(fluhip_corpus* c, const float* audio)
{
  if (!c || !audio) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t bytes = (size_t) c->B * c->n * sizeof(float);
  if (c->audioOwn.bytes < bytes) HIPCHK(ctx, c->audioOwn.alloc(bytes, false, ctx->stream));
  // The copy runs on the context's COPY stream: whatever another corpus of this context has in flight on the compute stream
  // (the previous slice of a pool job: its iterations) goes on beside it -- SURVEY section 7 step 5's double-buffered upload.
  // A corpus whose own audio may still be read by enqueued work drains the compute stream first.
  if (c->touched) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (!ctx->copyStream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copyStream, hipStreamNonBlocking));
  HIPCHK(ctx, hipMemcpyAsync(c->audioOwn.p, audio, bytes, hipMemcpyHostToDevice, ctx->copyStream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->copyStream)); // the caller's buffer is free again; the device copy is complete
  c->audioDev = c->audioOwn.as<float>();
  return FLUHIP_OK;
}

int fluhip_corpus_set_audio_dev(fluhip_corpus* c, const float* audio_dev)
{
  if (!c || !audio_dev) return FLUHIP_ERROR;
  c->audioDev = audio_dev;
  return FLUHIP_OK;
}

// the STFT phase with the frame-major magnitudes alone (every buffer's STFT::process + magnitude, nothing for the factor
// updates): what a spectrogram-only caller -- BufSTFT, the algorithm-level fluhip_stft_* -- pays per frame.  The corpus has no
// spectrogram for fluhip_corpus_nmf afterwards until fluhip_corpus_stft runs again.
int fluhip_corpus_stft_mag_only(fluhip_corpus* c)
{
  if (!c) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  if (!c->audioDev) return fail(ctx, "corpus has no audio: call fluhip_corpus_set_audio_* first");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  return corpus_stft(c, c->audioDev, nullptr, c->n, true);
}

static int fluhip_corpus_stft_impl(fluhip_corpus* c)
{
  if (!c) return FLUHIP_ERROR;
  if (!c->audioDev) return fail(c->ctx, "corpus has no audio");
  HIPCHK(c->ctx, hipSetDevice(c->ctx->device));
  return corpus_stft(c, c->audioDev, nullptr, c->n);
}

static int fluhip_corpus_nmf_impl(fluhip_corpus* c, int64_t iters, int update_w, int update_h, int64_t seed,
                      const int64_t* seeds, fluhip_progress_fn progress, void* user)
{
  if (!c) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  if (!c->haveMag) return fail(ctx, "corpus has no spectrogram: call fluhip_corpus_stft first");
  if (iters < 0) return fail(ctx, "negative iteration count");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  FactorInit fi;
  if (!c->seedW32.empty()) fi.W0f32 = c->seedW32.data(); // nrt/NMFClient.hpp:246-258 -> alg/NMF.hpp:102-112
  if (!c->seedH32.empty()) fi.H0f32 = c->seedH32.data(); // :113-124
  int rc = corpus_init_factors(c, seed, seeds, fi);
  if (rc) return rc;
  return corpus_iterate(c, iters, update_w != 0, update_h != 0, progress, user);
}

static int fluhip_corpus_set_factors_impl(fluhip_corpus* c, const float* bases_seed, const float* acts_seed)
{
  if (!c) return FLUHIP_ERROR;
  const size_t nw = (size_t) c->B * c->K * c->F, nh = (size_t) c->B * c->K * c->T;
  if (bases_seed) c->seedW32.assign(bases_seed, bases_seed + nw);
  else std::vector<float>().swap(c->seedW32);
  if (acts_seed) c->seedH32.assign(acts_seed, acts_seed + nh);
  else std::vector<float>().swap(c->seedH32);
  return FLUHIP_OK;
}

int fluhip_corpus_writeback_dev(fluhip_corpus* c, float* bases_dev, float* acts_dev)
{
  if (!c) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  if (!c->haveFactors) return fail(ctx, "corpus has no factors: call fluhip_corpus_nmf first");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (bases_dev) // clients/nrt/NMFClient.hpp:277-283
    launch_gather_w_f32(c->Wf.as<double>(), c->Fp * c->Kp, bases_dev, c->K * c->F, (int) c->F,
                        (int) c->K, (int) c->Kp, (int) c->B, s);
  if (acts_dev) // :286-300
    launch_acts_f32(c->H1.as<double>(), c->Tp * c->Kp, acts_dev, c->K * c->T, (int) c->T, (int) c->K,
                    (int) c->Kp, (int) c->B, c->hmax.as<double>(), s);
  HIPCHK(ctx, hipGetLastError());
  return FLUHIP_OK;
}

// clients/nrt/NMFClient.hpp:302-334 for every buffer of the corpus: estimate -> ratio mask -> ISTFT per component
static int fluhip_corpus_keep_spectrum_impl(fluhip_corpus* c, int on)
{
  if (!c) return FLUHIP_ERROR;
  c->keepSpec = on != 0;
  if (!c->keepSpec) c->spec.release();
  c->haveMag = c->haveMag && !(c->keepSpec && !c->spec.p); // a later resynthesis needs the STFT to run again
  return FLUHIP_OK;
}

int fluhip_corpus_resynth_dev(fluhip_corpus* c, float* out_dev)
{
  if (!c || !out_dev) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  if (!c->haveFactors) return fail(ctx, "corpus has no factors: call fluhip_corpus_nmf first");
  if (!c->keepSpec || !c->spec.p)
    return fail(ctx, "resynthesis needs the complex spectrogram: fluhip_corpus_keep_spectrum(c, 1) before fluhip_corpus_stft");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const double *wtab = nullptr, *ttab = nullptr;
  int rc = get_window(ctx, c->win, c->fft, c->windowType, &wtab);
  if (rc) return rc;
  rc = get_twiddle(ctx, c->fft, &ttab);
  if (rc) return rc;
  // Batched form (kernels_resynth_batch.hip resynth_seq_kernel): every component of a group of buffers in one launch, the
  // overlap-add in registers -- no windowed frames in memory (the per-buffer path below writes and re-reads K T win doubles
  // per buffer: 58 GB each way on the bench shard, 85 ms against 113 ms for 200 iterations).  FLUHIP_RESYNTH_BATCH=0 off.
  static const int batchEnv = fluhip::ab_int("FLUHIP_RESYNTH_BATCH", 1);
  if (batchEnv != 0 && resynth_batch_supported((int) c->win, (int) c->fft, (int) c->hop))
  {
    // buffers per launch: the reciprocal V-hat of a group within ~1 GiB
    const int64_t perBuf = c->T * c->F * (int64_t) sizeof(double);
    const int64_t group = std::max<int64_t>(1, std::min<int64_t>(c->B, ((int64_t) 1 << 30) / perBuf));
    DevBuf mult, wt, nrm;
    HIPCHK(ctx, mult.alloc((size_t) (group * perBuf), false, s));
    HIPCHK(ctx, wt.alloc((size_t) (group * c->Kp * c->F) * sizeof(double), false, s));
    HIPCHK(ctx, nrm.alloc((size_t) c->hop * sizeof(double), false, s));
    launch_resynth_normaliser(wtab, (int) c->win, (int) c->hop, nrm.as<double>(), s);
    for (int64_t b0 = 0; b0 < c->B; b0 += group)
    {
      const int nb = (int) std::min(group, c->B - b0);
      const double* Wb = c->Wf.as<double>() + b0 * c->Fp * c->Kp;
      const double* Hb = c->H1.as<double>() + b0 * c->Tp * c->Kp;
      launch_resynth_mult(Wb, c->Fp * c->Kp, Hb, c->Tp * c->Kp, wt.as<double>(), mult.as<double>(), (int) c->T, (int) c->F,
                          (int) c->K, (int) c->Kp, nb, s);
      ResynthBatchArgs ra;
      ra.spec = c->spec.as<double>() + b0 * c->T * c->F * 2; ra.specStride = c->T * c->F * 2;
      ra.mult = mult.as<double>(); ra.multStride = c->T * c->F;
      ra.Wt = wt.as<double>(); ra.wtStride = c->Kp * c->F;
      ra.H1 = Hb; ra.hStride = c->Tp * c->Kp;
      ra.Kp = (int) c->Kp; ra.K = (int) c->K;
      ra.win = (int) c->win; ra.fft = (int) c->fft; ra.hop = (int) c->hop; ra.T = (int) c->T; ra.F = (int) c->F; ra.B = nb;
      ra.window = wtab; ra.twiddle = ttab; ra.nrmTab = nrm.as<double>();
      ra.out32 = out_dev + b0 * c->K * c->n; ra.n = c->n; ra.outStride = c->n; ra.trim = c->win / 2;
      ra.nTab = c->ragged ? c->nTab.as<int64_t>() + b0 : nullptr;
      if (!launch_resynth_batch(ra, s)) return fail(ctx, "batched resynthesis refused a shape it had accepted");
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(s)); // the workspaces go out of scope
    return FLUHIP_OK;
  }
  DevBuf vhat, frames;
  HIPCHK(ctx, vhat.alloc((size_t) c->T * c->F * sizeof(double), false, s));
  const int64_t compsPerLaunch = std::max<int64_t>(1, std::min<int64_t>(c->K, ((int64_t) 1 << 30) / (c->T * c->win * 8)));
  HIPCHK(ctx, frames.alloc((size_t) compsPerLaunch * c->T * c->win * sizeof(double), false, s));
  for (int64_t b = 0; b < c->B; b++)
  {
    const double* Wb = c->Wf.as<double>() + b * c->Fp * c->Kp;
    const double* Hb = c->H1.as<double>() + b * c->Tp * c->Kp;
    // a ragged corpus: the buffer's own frames and samples (arrays are strided by the longest buffer's)
    const int Tb = c->ragged ? c->tOf[(size_t) b] : (int) c->T;
    const int64_t nb = c->ragged ? c->nOf[(size_t) b] : c->n;
    launch_vhat(Wb, 0, Hb, 0, vhat.as<double>(), c->F, 0, Tb, (int) c->F, (int) c->Kp, 1, s);
    ResynthArgs ra;
    ra.spec = c->spec.as<double>() + b * c->T * c->F * 2; ra.Wf = Wb; ra.H1 = Hb;
    ra.Vhat = vhat.as<double>(); ra.ldV = c->F; ra.Kp = (int) c->Kp;
    ra.win = (int) c->win; ra.fft = (int) c->fft; ra.hop = (int) c->hop; ra.T = Tb; ra.F = (int) c->F;
    ra.window = wtab; ra.twiddle = ttab; ra.frames = frames.as<double>(); ra.out = nullptr; ra.n = nb; ra.outStride = c->n;
    ra.trim = c->win / 2;
    for (int64_t k = 0; k < c->K; k += compsPerLaunch)
    {
      ra.k = (int) k;
      ra.nComp = (int) std::min(compsPerLaunch, c->K - k);
      ra.out32 = out_dev + (b * c->K + k) * c->n;
      ra.bigScratch = big_fft_scratch(ctx, ra.win, ra.fft, ra.T);
      if (stft_needs_scratch(ra.win, ra.fft) && !ra.bigScratch) return FLUHIP_ERROR;
      launch_resynth(ra, s);
    }
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(s)); // vhat / frames go out of scope
  return FLUHIP_OK;
}

static int fluhip_corpus_resynth_host_impl(fluhip_corpus* c, float* out)
{
  if (!c || !out) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf d;
  const size_t nb = (size_t) c->B * c->K * c->n * sizeof(float);
  HIPCHK(ctx, d.alloc(nb, false, ctx->stream));
  int rc = fluhip_corpus_resynth_dev(c, d.as<float>());
  if (rc) return rc;
  return copy_to_host(ctx, out, nb, d.p, nb, nb, 1, ctx->stream);
}

// The same, written the way an interleaved host buffer holds it (MemoryBufferAdaptor, SuperCollider and Max buffers:
// frames x channels): out[t * frame_stride + b * K + k] = component k of buffer b at sample t -- the layout of
// resynth.samps(i * rank + j) in clients/nrt/NMFClient.hpp:321-326 when the buffer's channels are interleaved.  The
// transposition happens on the device; the host sees one streaming copy instead of count x K strided passes over its buffer.
static int fluhip_corpus_resynth_interleaved_host_impl(fluhip_corpus* c, float* out, int64_t frame_stride)
{
  if (!c || !out) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  if (c->ragged) return fail(ctx, "interleaved resynthesis needs equal-length buffers");
  const int64_t chans = c->B * c->K;
  if (frame_stride < chans) return fail(ctx, "frame stride below count x K");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf d, dt;
  const size_t nb = (size_t) chans * c->n * sizeof(float);
  HIPCHK(ctx, d.alloc(nb, false, s));
  HIPCHK(ctx, dt.alloc(nb, false, s));
  int rc = fluhip_corpus_resynth_dev(c, d.as<float>());
  if (rc) return rc;
  launch_transpose_f32(d.as<float>(), c->n, dt.as<float>(), chans, (int) chans, c->n, s); // [chans][n] -> [n][chans]
  HIPCHK(ctx, hipGetLastError());
  const size_t width = (size_t) chans * sizeof(float);
  if (frame_stride == chans) return copy_to_host(ctx, out, nb, dt.p, nb, nb, 1, s);
  return copy_to_host(ctx, out, (size_t) frame_stride * sizeof(float), dt.p, width, width, (size_t) c->n, s);
}

int fluhip_corpus_resynth_ragged_host(fluhip_corpus* c, float* const* out)
{
  if (!c || !out) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf d;
  const size_t nb = (size_t) c->B * c->K * c->n * sizeof(float);
  HIPCHK(ctx, d.alloc(nb, true, ctx->stream));
  int rc = fluhip_corpus_resynth_dev(c, d.as<float>());
  if (rc) return rc;
  for (int64_t i = 0; i < c->B; i++)
  {
    if (!out[i]) continue;
    const int64_t ni = c->ragged ? c->nOf[(size_t) i] : c->n; // K rows of the buffer's own samples out of rows of the longest
    HIPCHK(ctx, hipMemcpy2DAsync(out[i], (size_t) ni * sizeof(float), d.as<float>() + i * c->K * c->n, (size_t) c->n * sizeof(float),
                                 (size_t) ni * sizeof(float), (size_t) c->K, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FLUHIP_OK;
}

static int fluhip_corpus_writeback_host_impl(fluhip_corpus* c, float* bases, float* acts)
{
  if (!c) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf db, da;
  const size_t nb = (size_t) c->B * c->K * c->F * sizeof(float), na = (size_t) c->B * c->K * c->T * sizeof(float);
  if (bases) HIPCHK(ctx, db.alloc(nb, false, ctx->stream));
  if (acts) HIPCHK(ctx, da.alloc(na, false, ctx->stream));
  int rc = fluhip_corpus_writeback_dev(c, bases ? db.as<float>() : nullptr, acts ? da.as<float>() : nullptr);
  if (rc) return rc;
  // (large corpora: through the pinned staging blocks, copy_to_host)
  if (bases && (rc = copy_to_host(ctx, bases, nb, db.p, nb, nb, 1, ctx->stream))) return rc;
  if (acts && (rc = copy_to_host(ctx, acts, na, da.p, na, na, 1, ctx->stream))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FLUHIP_OK;
}

int fluhip_corpus_read_f64(fluhip_corpus* c, double* mag, double* W1, double* H1)
{
  if (!c) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (mag)
  {
    if (!c->haveMag) return fail(ctx, "corpus has no spectrogram");
    for (int64_t b = 0; b < c->B; b++)
      HIPCHK(ctx, hipMemcpy2DAsync(mag + b * c->T * c->F, (size_t) c->F * sizeof(double),
                                   c->mag.as<double>() + b * c->Tp * c->Fp, (size_t) c->Fp * sizeof(double),
                                   (size_t) c->F * sizeof(double), (size_t) c->T, hipMemcpyDeviceToHost, s));
  }
  DevBuf dw, dh;
  if (W1 || H1)
    if (!c->haveFactors) return fail(ctx, "corpus has no factors");
  if (W1)
  {
    const size_t bytes = (size_t) c->B * c->K * c->F * sizeof(double);
    HIPCHK(ctx, dw.alloc(bytes, false, s));
    launch_gather_w_f64(c->Wf.as<double>(), c->Fp * c->Kp, dw.as<double>(), c->K * c->F, (int) c->F,
                        (int) c->K, (int) c->Kp, (int) c->B, s);
    HIPCHK(ctx, hipMemcpyAsync(W1, dw.p, bytes, hipMemcpyDeviceToHost, s));
  }
  if (H1)
  {
    const size_t bytes = (size_t) c->B * c->T * c->K * sizeof(double);
    HIPCHK(ctx, dh.alloc(bytes, false, s));
    launch_gather_h_f64(c->H1.as<double>(), c->Tp * c->Kp, dh.as<double>(), c->T * c->K, (int) c->T,
                        (int) c->K, (int) c->Kp, (int) c->B, s);
    HIPCHK(ctx, hipMemcpyAsync(H1, dh.p, bytes, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

// Diagnostic: the corpus's layouts as they lie on the device, padding included -- the frame-major magnitudes
// [count][Tp][Fp] (readable after fluhip_corpus_stft_mag_only too, where fluhip_corpus_read_f64 refuses), the bin-major copy
// the H update streams, [count][Fp][Tp], and (with keep_spectrum on) the complex spectrum [count][T][F][2].
// dims5 = {count, Fp, Tp, T, F}; any array may be null (dims5 alone sizes the caller's arrays).
int fluhip_debug_corpus_read_layouts_f64(fluhip_corpus* c, int64_t* dims5, double* mag, double* magT, double* spec)
{
  if (!c) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  if (dims5) { dims5[0] = c->B; dims5[1] = c->Fp; dims5[2] = c->Tp; dims5[3] = c->T; dims5[4] = c->F; }
  if (!mag && !magT && !spec) return FLUHIP_OK;
  if (!c->touched) return fail(ctx, "corpus has no spectrogram: no transform has run on it");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (mag) HIPCHK(ctx, hipMemcpyAsync(mag, c->mag.p, (size_t) c->B * c->Tp * c->Fp * sizeof(double), hipMemcpyDeviceToHost, s));
  if (magT)
  {
    if (!c->haveMag || !c->magT.p) return fail(ctx, "corpus has no bin-major magnitudes: call fluhip_corpus_stft first");
    HIPCHK(ctx, hipMemcpyAsync(magT, c->magT.p, (size_t) c->B * c->Fp * c->Tp * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (spec)
  {
    if (!c->keepSpec || !c->spec.p)
      return fail(ctx, "corpus has no spectrum: fluhip_corpus_keep_spectrum(c, 1) before the transform");
    HIPCHK(ctx, hipMemcpyAsync(spec, c->spec.p, (size_t) c->B * c->T * c->F * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(ctx, hipStreamSynchronize(s));
  return FLUHIP_OK;
}

int fluhip_corpus_plan(const fluhip_corpus* c, int64_t* out8)
{
  if (!c || !out8) return FLUHIP_ERROR;
  out8[0] = c->plan.variant;
  out8[1] = c->plan.nsplitW;
  out8[2] = c->plan.nsplitH | ((int64_t) c->plan.tailSplitH << 16); // (tail split of the two-launch H update in the high half)
  out8[3] = c->plan.lazy ? 1 : 0;
  out8[4] = c->plan.sideW ? 1 : 0;
  out8[5] = c->plan.stripsW;
  out8[6] = c->Kp | ((int64_t) (c->plan.Kc > 0 ? c->plan.Kc : c->Kp) << 16); // (the rank the factor updates compute in the high half)
  out8[7] = c->plan.strip ? (c->plan.stripTile ? 3 : (c->plan.stripBin ? 2 : 1)) : 0; // 2: the W update as a bin-strip launch (A/B); 3: as the bin-tiled launch
  return FLUHIP_OK;
}

// ---- profiling ------------------------------------------------------------------------
// debugging aid for FLUHIP_K5_INSTR: first 8 words of the split-denominator scratch
int fluhip_corpus_debug_words(fluhip_corpus* c, int64_t* out32)
{
  if (!c || !out32 || !c->dpart.p) return FLUHIP_ERROR;
  HIPCHK(c->ctx, hipStreamSynchronize(c->ctx->stream));
  if (c->plan.strip)
  {
    // FLUHIP_STRIP_INSTR: the 32 words behind the partials (kernels_nmf_strip.hip STRIP_STAMP)
    std::memset(out32, 0, 32 * sizeof(int64_t));
    const int64_t off = nmf_strip_part_doubles((int) c->F, (int) c->T, (int) c->B) - 32;
    HIPCHK(c->ctx, hipMemcpy(out32, c->stripPart.as<double>() + off, 32 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return FLUHIP_OK;
  }
  HIPCHK(c->ctx, hipMemcpy(out32, c->dpart.p, 32 * sizeof(int64_t), hipMemcpyDeviceToHost));
  return FLUHIP_OK;
}

int fluhip_corpus_last_loop_ms(fluhip_corpus* c, double* ms)
{
  if (!c || !ms) return FLUHIP_ERROR;
  if (!c->loopTimed) return fail(c->ctx, "no iteration loop has been timed on this corpus");
  float t = 0.f;
  HIPCHK(c->ctx, hipEventSynchronize(c->loopEv1));
  HIPCHK(c->ctx, hipEventElapsedTime(&t, c->loopEv0, c->loopEv1));
  *ms = (double) t;
  return FLUHIP_OK;
}

int fluhip_corpus_update_clocks(fluhip_corpus* c, int64_t* out8, int reset)
{
  if (!c || !c->clk.p) return FLUHIP_ERROR;
  fluhip_ctx* ctx = c->ctx;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (out8) HIPCHK(ctx, hipMemcpy(out8, c->clk.p, 8 * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (reset) HIPCHK(ctx, hipMemset(c->clk.p, 0, 8 * sizeof(int64_t)));
  return FLUHIP_OK;
}

// the entry points of the clients' batched block (NMFClient.hpp), exception-tight
int fluhip_corpus_create(fluhip_ctx* ctx, int64_t count, int64_t n, int64_t win, int64_t fft,
                         int64_t hop, int64_t K, fluhip_corpus** out)
{
  return guarded_corpus(ctx, [&] { return fluhip_corpus_create_impl(ctx, count, n, win, fft, hop, K, out); });
}

int fluhip_corpus_set_audio_host(fluhip_corpus* c, const float* audio)
{
  return guarded_corpus((c ? c->ctx : nullptr), [&] { return fluhip_corpus_set_audio_host_impl(c, audio); });
}

int fluhip_corpus_stft(fluhip_corpus* c)
{
  return guarded_corpus((c ? c->ctx : nullptr), [&] { return fluhip_corpus_stft_impl(c); });
}

int fluhip_corpus_set_factors(fluhip_corpus* c, const float* bases_seed, const float* acts_seed)
{
  return guarded_corpus((c ? c->ctx : nullptr), [&] { return fluhip_corpus_set_factors_impl(c, bases_seed, acts_seed); });
}

int fluhip_corpus_nmf(fluhip_corpus* c, int64_t iters, int update_w, int update_h, int64_t seed,
                      const int64_t* seeds, fluhip_progress_fn progress, void* user)
{
  return guarded_corpus((c ? c->ctx : nullptr), [&] { return fluhip_corpus_nmf_impl(c, iters, update_w, update_h, seed, seeds, progress, user); });
}

int fluhip_corpus_writeback_host(fluhip_corpus* c, float* bases, float* acts)
{
  return guarded_corpus((c ? c->ctx : nullptr), [&] { return fluhip_corpus_writeback_host_impl(c, bases, acts); });
}

int fluhip_corpus_resynth_host(fluhip_corpus* c, float* out)
{
  return guarded_corpus((c ? c->ctx : nullptr), [&] { return fluhip_corpus_resynth_host_impl(c, out); });
}

int fluhip_corpus_resynth_interleaved_host(fluhip_corpus* c, float* out, int64_t frame_stride)
{
  return guarded_corpus((c ? c->ctx : nullptr), [&] { return fluhip_corpus_resynth_interleaved_host_impl(c, out, frame_stride); });
}

int fluhip_corpus_keep_spectrum(fluhip_corpus* c, int on)
{
  return guarded_corpus((c ? c->ctx : nullptr), [&] { return fluhip_corpus_keep_spectrum_impl(c, on); });
}

} // extern "C"
