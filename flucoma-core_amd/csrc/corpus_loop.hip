// corpus_loop.hip -- the iteration loop of the corpus layer: the launch sequence of one iteration for the frame-strip schedule
// and for the uniform / split / work-list / any-rank schedules, and the loop around them.  Reads the corpus's plan, writes its
// run state.
//   NMF::multiplicativeUpdates             include/flucoma/algorithms/public/NMF.hpp:144-183
#include "corpus_internal.h"

// the second stream and the fork / join events of the W update's side column (created on first use; false: stay on one stream)
constexpr bool kSideBesideDefault = false;
constexpr bool kSideFirstCorpora = false;
static bool side_stream_ready(fluhip_ctx* ctx)
{
  if (ctx->sideStream) return ctx->sideEv[7] != nullptr;
  if (hipStreamCreateWithFlags(&ctx->sideStream, hipStreamNonBlocking) != hipSuccess) { ctx->sideStream = nullptr; return false; }
  for (auto& e : ctx->sideEv)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
  return true;
}

// the frame-strip kernel's arguments over the whole corpus; doH / doW and the generation are the launch's own
static StripArgs strip_args(const fluhip_corpus* c)
{
  StripArgs a;
  a.V = c->mag.as<double>(); a.strideV = c->Tp * c->Fp; a.ldv = c->Fp;
  a.W = c->Wf.as<double>(); a.strideW = c->Fp * c->Kp;
  a.H = c->H1.as<double>(); a.strideH = c->Tp * c->Kp;
  a.part = c->stripPart.as<double>(); a.nrm = c->wnorm.as<double>();
  a.F = (int) c->F; a.T = (int) c->T; a.K = (int) c->K; a.B = (int) c->B;
  a.doH = a.doW = 0; a.wPend = c->run.wPending ? 1 : 0;
  return a;
}

// one iteration of the frame-strip schedule (plan.strip: a single buffer of rank <= 16)
static void enqueue_strip_iteration(fluhip_corpus* c, bool updateW, bool updateH, bool last)
{
  fluhip_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  StripArgs a = strip_args(c);
#ifdef FLUHIP_AB_SWITCHES
  BinTileArgs bt{};
  if (c->plan.stripTile)
  {
    bt.VT = c->magT.as<double>(); bt.strideVT = c->Fp * c->Tp; bt.ldT = c->Tp;
    bt.W = a.W; bt.strideW = a.strideW; bt.H = a.H; bt.strideH = a.strideH;
    bt.work = c->tileWork.as<double>(); bt.nSideWG = nmf_strip_workgroups((int) c->T);
    bt.F = a.F; bt.K = a.K; bt.B = a.B;
    a.nRec = nmf_bintile_records(a.F); a.sideOut = nmf_bintile_side_area(bt);
  }
  // (the strip launches of the tiled form read the tile records of the generation current at their launch)
  auto tile_gen = [&]() { if (c->plan.stripTile) a.tileStat = nmf_bintile_records_ptr(bt, c->run.stripGen); };
#else
  auto tile_gen = [] {};
#endif
  if (!c->run.stripStatsValid)
  {
    // W was written by something else (initialisation, the normalisation at the end of the last call)
    a.statGen = c->run.stripGen;
#ifdef FLUHIP_AB_SWITCHES
    if (c->plan.stripTile) { bt.statGen = c->run.stripGen; bt.wPend = 0; launch_nmf_bintile_wstats(bt, s); }
    else
#endif
    launch_nmf_strip_wstats(a, s);
    c->run.stripStatsValid = true;
  }
#ifdef FLUHIP_AB_SWITCHES
  if (updateW && c->plan.stripTile)
  {
    // alg/NMF.hpp:158-161 as ONE launch over tiles of four bins; :162 stays deferred (tile records of the other generation)
    if (!c->run.stripSideReady)
    {
      // the Nyquist bin's numerator partials from the H in memory (first iteration of a call, W-only iterations)
      a.doH = 0; a.doW = 2; a.wPend = c->run.wPending ? 1 : 0; a.statGen = c->run.stripGen; tile_gen();
      ProfScope p(ctx, 3);
      launch_nmf_strip(a, s);
    }
    bt.sidePart = a.sideOut; bt.statGen = c->run.stripGen; bt.wPend = c->run.wPending ? 1 : 0;
    {
      ProfScope p(ctx, 1);
      launch_nmf_bintile(bt, s);
    }
    c->run.stripGen ^= 1;
    c->run.wPending = true;
    c->run.stripSideReady = false;
    c->run.stripReady = false;
    c->run.stripNormFresh = false;
  }
  else
#endif
  if (updateW && c->plan.stripBin)
  {
    // alg/NMF.hpp:158-161 as one launch over bin strips: reads W', its records and the H in memory, leaves the new W' and
    // its records (other generation); :162 stays deferred as in the fused form
    a.wPend = c->run.wPending ? 1 : 0; a.statGen = c->run.stripGen;
    {
      ProfScope p(ctx, 1);
#ifdef FLUHIP_AB_SWITCHES
      launch_nmf_binstrip(a, c->binWork.as<double>(), s);
#endif
    }
    c->run.stripGen ^= 1;
    c->run.wPending = true;
    c->run.stripReady = false;
    c->run.stripNormFresh = false;
  }
  else if (updateW)
  {
    // alg/NMF.hpp:158-161; :162 is implicit in the next staging of W'
    if (!c->run.stripReady)
    {
      a.doH = 0; a.doW = 1; a.wPend = c->run.wPending ? 1 : 0; a.statGen = c->run.stripGen;
      ProfScope p(ctx, 1);
      launch_nmf_strip(a, s);
    }
    {
      a.wPend = c->run.wPending ? 1 : 0; a.statGen = c->run.stripGen;
      ProfScope p(ctx, 3);
      launch_nmf_strip_reduce(a, s);
      c->run.stripGen ^= 1;
    }
    c->run.wPending = true;
    c->run.stripReady = false;
    c->run.stripNormFresh = false;
  }
  if (updateH)
  {
    // :165-170, and behind it the numerator of the next iteration's W update while the new H is at hand
    a.doH = 1; a.doW = (updateW && !last && !c->plan.stripBin) ? (c->plan.stripTile ? 2 : 1) : 0; a.wPend = c->run.wPending ? 1 : 0; a.statGen = c->run.stripGen;
    tile_gen();
    ProfScope p(ctx, 1);
    launch_nmf_strip(a, s);
    c->run.stripReady = a.doW == 1;
    c->run.stripSideReady = a.doW == 2;
    c->run.stripNormFresh = true;
  }
}

// one iteration of the uniform / split / work-list / any-rank schedules
static void enqueue_mfma_iteration(fluhip_corpus* c, bool updateW, bool updateH, bool last)
{
  fluhip_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  // (a window of the corpus: every per-buffer array starts b0 buffers in; the scratch of the small kernels is reused)
  const int64_t b0 = c->run.winB ? c->run.winB0 : 0;
  const int Bw = (int) (c->run.winB ? c->run.winB : c->B);
  double* const magW = c->mag.as<double>() + b0 * c->Tp * c->Fp;
  double* const magTW = c->magT.as<double>() + b0 * c->Fp * c->Tp;
  double* const WfW = c->Wf.as<double>() + b0 * c->Fp * c->Kp;
  double* const H1W = c->H1.as<double>() + b0 * c->Tp * c->Kp;
  double* const wnormW = c->wnorm.p ? c->wnorm.as<double>() + b0 * c->Kp : nullptr;
  // the H update's arguments (alg/NMF.hpp:165-170; V2 is formed from the already updated W) -- also wanted by the W update's
  // step, which asks what the H launch behind it will take over (dryRun)
  auto h_args = [&]() {
    UpdateArgs a;
    a.V = magTW; a.ldv = c->Tp; a.strideV = c->Fp * c->Tp;
    a.Mv = WfW; a.strideM = c->Fp * c->Kp;
    a.S = H1W; a.strideS = c->Tp * c->Kp;
    a.R = (int) c->F; a.C = (int) c->T; a.B = Bw; a.Kp = (int) c->Kp; a.Kc = c->plan.Kc;
    if (c->run.winB) a.stripsOverride = c->run.winStripsH;
    a.nsplit = c->plan.nsplitH; a.part = c->part.as<double>(); a.dpart = c->dpart.as<double>();
    a.Cp = c->plan.useLists ? std::max(c->Fp, c->Tp) : c->Tp; a.colsumScratch = c->csumScratch.as<double>();
    a.clk = c->clk.as<long long>() + 4;
    if (c->plan.useLists)
    {
      a.list = c->listH.list.as<WaveDesc>(); a.listWGs = c->listH.wgs; a.listNG = c->listH.ng; a.listPartial = c->listH.partial;
    }
    return a;
  };
  // the W update's (alg/NMF.hpp:158-161), before what the deferred normalisation adds
  auto w_args = [&]() {
    UpdateArgs a;
    a.V = magW; a.ldv = c->Fp; a.strideV = c->Tp * c->Fp;
    a.Mv = H1W; a.strideM = c->Tp * c->Kp;
    a.S = WfW; a.strideS = c->Fp * c->Kp;
    a.R = (int) c->T; a.C = (int) c->F - (c->plan.sideW ? 1 : 0); a.B = Bw; a.Kp = (int) c->Kp; a.Kc = c->plan.Kc;
    if (c->run.winB) a.stripsOverride = c->run.winStripsW;
    a.nsplit = c->plan.nsplitW; a.part = c->part.as<double>(); a.dpart = c->dpart.as<double>();
    a.Cp = c->plan.useLists ? std::max(c->Fp, c->Tp) : c->Fp; a.colsumScratch = c->csumScratch.as<double>();
    a.clk = c->clk.as<long long>();
    if (c->plan.useLists)
    {
      a.list = c->listW.list.as<WaveDesc>(); a.listWGs = c->listW.wgs; a.listNG = c->listW.ng; a.listPartial = c->listW.partial;
    }
    return a;
  };
  // an update launch, and behind it the finalize launch when its work list leaves partials in memory
  auto launch_update = [&](const UpdateArgs& a, const fluhip_corpus::WorkList& wl, double* statPart) {
    const int did = launch_nmf_update5(a, s);
    if (wl.partial)
      launch_update_finalize(a.S, a.strideS, a.part, a.dpart, a.C, a.Kp, a.Cp, wl.maxSplit, a.B, s, a.nrm, a.nrmMode, statPart,
                             wl.splitTab.as<int>());
    return did;
  };
  // the norm-combine launch of this window's W (launch_wnorm_combine: what `side` and the phase select)
  auto wnorm_combine = [&](const SideColumn* side, hipStream_t st, int sidePhase, int sideSlices = 0, int sideGen = -1,
                           const WnormColsum* colsum = nullptr) {
    return launch_wnorm_combine(WfW, c->Fp * c->Kp, (int) c->F, (int) c->K, (int) c->Kp, Bw, c->plan.stripsW,
                                c->wscratch.as<double>(), wnormW, side, st, sidePhase, sideSlices, sideGen, colsum);
  };
  const int uvH = c->plan.variant;
  // (the plain one-launch form of the H update: no work lists, no second launch for a poorly filled last round)
  const bool hPlain = !c->plan.useLists && uvH == 5 && !(c->plan.tailSplitH > 1 && !c->run.winB);
  // FLUHIP_SIDE_FROM_H=0 (A/B build): side-column launch and norm-combine launch between the updates, as before round 4
  static const bool fromH = fluhip::ab_int("FLUHIP_SIDE_FROM_H", 1) != 0;
  static const bool normInH = fluhip::ab_int("FLUHIP_NORM_IN_H", 1) != 0;
  auto side_io = [&](UpdateArgs& a, bool wantNorm) {
    double* scr = c->wscratch.as<double>();
    const int outGen = c->run.sideGen ^ 1;
    a.sideOut = wnorm_side_part(scr, (int) c->Kp, Bw, c->plan.stripsW, outGen);
    a.sideWold = wnorm_side_wold(scr, (int) c->Kp, Bw, c->plan.stripsW, outGen);
    if (wantNorm)
    {
      a.cmbStat = scr; a.cmbParts = c->plan.stripsW;
      a.cmbSide = wnorm_side_part(scr, (int) c->Kp, Bw, c->plan.stripsW, c->run.sideGen);
      a.cmbWold = wnorm_side_wold(scr, (int) c->Kp, Bw, c->plan.stripsW, c->run.sideGen);
      a.cmbSlices = c->run.sideFromHSlices; a.cmbK = (int) c->K;
      a.cmbNrmOut = wnormW; a.cmbRowOut = WfW;
    }
  };
  if (updateW)
  {
    UpdateArgs a = w_args();
    if (c->plan.lazy)
    {
      // W' = W diag(wnorm) in memory: the kernel divides its stationary rows by wnorm, writes the new W'
      // and its per-wavefront column statistics; [side column ->] new wnorm.  alg/NMF.hpp:162 is then
      // implicit in every later use of (W', wnorm).
      a.nrm = wnormW; a.nrmMode = 1; a.statPart = c->wscratch.as<double>();
      SideColumn sc{magTW + (c->F - 1) * c->Tp, c->Fp * c->Tp, H1W, c->Tp * c->Kp, (int) c->T};
      // The side column (bin F-1 of W, scalar FMAs) reads H, V, the old W row and the old norms -- nothing the update launch
      // writes -- so it runs BESIDE that launch on a second stream: forked behind the H update in front, joined before the norm
      // combine.  The update launch is enqueued first; its wavefronts are the older ones on every SIMD and are served first.
      static const bool sideBeside = fluhip::ab_int("FLUHIP_SIDE_STREAM", kSideBesideDefault) != 0;
      const bool sideReady = c->run.sideFromH;
      c->run.sideFromH = false;
      hipEvent_t join = nullptr;
      if (c->plan.sideW && !sideReady && sideBeside && side_stream_ready(ctx))
      {
        hipEvent_t fork = ctx->sideEv[(ctx->sideTurn * 2) % 8];
        join = ctx->sideEv[(ctx->sideTurn * 2 + 1) % 8];
        ctx->sideTurn++;
        if (hipEventRecord(fork, s) != hipSuccess || hipStreamWaitEvent(ctx->sideStream, fork, 0) != hipSuccess) join = nullptr;
      }
      // Arrays of rank 128 at compute ranks above 104 take the update's column sums of H from a pre-pass -- and the side
      // column's denominator is that same sum.  There the side-column launch goes IN FRONT of the update (it reads H, V, the old
      // side row and the old norms: nothing the update writes) and its slices' denominators are added into the update's
      // denominator slots: one sweep over H instead of two (config 3: colsum_part_kernel's 11 - 16 us per iteration gone).
      // FLUHIP_COLSUM_FROM_SIDE=0 (A/B build): the pre-pass as before.
      static const bool csFromSide = fluhip::ab_int("FLUHIP_COLSUM_FROM_SIDE", 1) != 0;
      static const bool sideFused = fluhip::ab_int("FLUHIP_SIDE_FUSED", 0) == 1;   // (A/B: the combine rides in the side-column launch, which must then follow the update)
      // FLUHIP_SIDE_FIRST_CORPORA=0|1 (A/B build): whether corpora whose side column and norm combine are ONE launch behind the
      // update (side_norm_kernel) give that up for the side-first order
      static const bool sideFirstCorpora = fluhip::ab_int("FLUHIP_SIDE_FIRST_CORPORA", kSideFirstCorpora) != 0;
      const bool sideFirst = csFromSide && !sideFused && c->plan.sideW && !sideReady && !join && !c->plan.useLists && c->Kp == 128 &&
                             (c->plan.Kc <= 0 || c->plan.Kc > 104) && a.colsumScratch && c->plan.variant == 5 &&
                             (sideFirstCorpora || !wnorm_side_norm_shape(Bw, c->plan.stripsW, sc.R, (int) c->Kp));
      if (sideFirst)
      {
        ProfScope p(ctx, 3);
        wnorm_combine(&sc, s, 1);
        const int ns = a.nsplit < 1 ? 1 : a.nsplit;
        launch_colsum_from_side(c->wscratch.as<double>(), (int) c->Kp, Bw, c->plan.stripsW, wnorm_side_slices(sc.R, (int) c->Kp),
                                a.dpart, (int64_t) ns * c->Kp, ns - 1, s);
        a.colsumInPlace = true;
      }
      // rank 32, steady state of the two-launch iteration: the H update in front left the side column's partials, whose
      // denominators are the column sums of H this update divides by -- no accumulators in its loop; it leaves the column sums
      // of its rows for the H update behind (the launcher decides whether the form exists for these arguments: bit 2)
      if (sideReady && c->plan.sideW && !c->plan.useLists && c->colPart.p && c->run.sideFromHSlices > 0 && c->plan.variant == 5)
      {
        a.colIn = wnorm_side_part(c->wscratch.as<double>(), (int) c->Kp, Bw, c->plan.stripsW, c->run.sideGen);
        a.colInN = c->run.sideFromHSlices;
        a.colOut = c->colPart.as<double>();
      }
      {
        ProfScope p(ctx, 1);
        c->run.colPartValid = (launch_update(a, c->listW, a.statPart) & 4) != 0;
      }
      if (join)
      {
        wnorm_combine(&sc, ctx->sideStream, 1);
        (void) hipEventRecord(join, ctx->sideStream);
        (void) hipStreamWaitEvent(s, join, 0);
      }
      c->run.normDue = false;
      if (c->plan.sideW && sideReady && updateH && hPlain && normInH && c->plan.stripsW <= 16 && c->run.sideFromHSlices <= 16)
      {
        // ... and the norm combine too can wait for the H update behind this launch, whose wavefronts then do it in their
        // prologue -- if the form that launch will take does that (dryRun: nothing is launched)
        c->run.normDue = (plain_h_update_takes(h_args(), true, 0) & 2) != 0;
      }
      if (!c->run.normDue)   // (nothing between the updates otherwise: no event pair of the profiling aid there either)
      {
        ProfScope p(ctx, 3);
        if (c->plan.sideW && sideReady)   // the H update in front left the side column's partials: the norm combine is all that is due
          wnorm_combine(&sc, s, 2, c->run.sideFromHSlices, c->run.sideGen);
        else
        {
          // ... and where the H update behind takes ITS column sums (of the new W') from a pre-pass, the combine launch leaves
          // them in that update's denominator slots (long factors: launch_wnorm_combine says whether it did)
          WnormColsum wc;
          if (csFromSide && updateH && !c->plan.useLists && uvH == 5 && c->Kp == 128 && (c->plan.Kc <= 0 || c->plan.Kc > 104) && c->csumScratch.p)
          {
            double* dp = c->dpart.as<double>();
            if (c->plan.tailSplitH > 1 && !c->run.winB)
            {
              wc.out1 = dp; wc.stride1 = c->Kp; wc.zero1 = 0;
              wc.out2 = dp + (int64_t) Bw * c->Kp; wc.stride2 = (int64_t) c->plan.tailSplitH * c->Kp; wc.zero2 = c->plan.tailSplitH - 1;
            }
            else
            {
              const int nsH = c->plan.nsplitH < 1 ? 1 : c->plan.nsplitH;
              wc.out1 = dp; wc.stride1 = (int64_t) nsH * c->Kp; wc.zero1 = nsH - 1;
            }
          }
          c->run.colsumWInPlace = wnorm_combine(c->plan.sideW ? &sc : nullptr, s, (join || sideFirst) ? 2 : 0, 0, -1, wc.out1 ? &wc : nullptr);
        }
      }
      c->run.wPending = true;
    }
    else
    {
      {
        ProfScope p(ctx, 1);
        if (c->plan.variant == 5) launch_nmf_update5(a, s);
        else launch_nmf_update_wide(a, c->wideScratch.as<double>(), s);
      }
      // :162  if (W.maxCoeff() > epsilon) W.colwise().normalize()
      launch_colnorm(WfW, c->Fp * c->Kp, (int) c->F, (int) c->K, (int) c->Kp, Bw, false, true,
                     c->normScratch.as<double>(), s);
    }
  }
  if (updateH)
  {
    UpdateArgs a = h_args();
    const bool colValid = c->run.colPartValid;
    c->run.colPartValid = false;
    if (c->run.wPending) { a.nrm = wnormW; a.nrmMode = 2; }
    const bool csIn = c->run.colsumWInPlace;   // (the column sums of W' are in this update's denominator slots already)
    c->run.colsumWInPlace = false;
    ProfScope p(ctx, 1);
    if (c->plan.useLists) launch_update(a, c->listH, nullptr);
    else if (uvH == 5 && c->plan.tailSplitH > 1 && !c->run.winB)
    {
      // two launches (plan_tail): whole contractions for the frames that fill whole rounds, split ones for the rest
      UpdateArgs a1 = a;
      a1.C = c->plan.tailColsH; a1.stripsOverride = c->plan.tailStripsH; a1.nsplit = 1;
      a1.colsumInPlace = csIn;
      launch_nmf_update5(a1, s);
      UpdateArgs a2 = a;
      a2.V = a.V + c->plan.tailColsH; a2.S = a.S + (int64_t) c->plan.tailColsH * c->Kp; a2.C = a.C - c->plan.tailColsH;
      a2.stripsOverride = c->plan.tailRestH; a2.nsplit = c->plan.tailSplitH; a2.Cp = round_up(a2.C, 32);
      a2.dpart = a.dpart + (int64_t) Bw * c->Kp;
      if (csIn) a2.colsumInPlace = true;
      else if (c->Kp > 64) a2.colsumGiven = a.dpart; // (the first launch's pre-pass left the column sums of W there)
      a2.clk = nullptr;                         // the clock stamps stay those of the whole-contraction wavefront
      launch_nmf_update5(a2, s);
    }
    else if (uvH == 5)
    {
      // a W update follows (same call, same window) and keeps bin F - 1 as a side column: this launch, which holds the new H
      // in registers at its end, leaves that side column's contraction as per-wavefront partials (UpdateArgs::sideOut) and the
      // side-column launch -- a second pass over H, 10 us per iteration of the bench shard -- is not needed.
      // FLUHIP_SIDE_FROM_H=0 (A/B build): the side-column launch as before.
      // (the norm combine of the W update in front, if that was left to this launch: c->run.normDue)
      const bool wantNorm = c->run.normDue;
      a.colsumInPlace = csIn;
      if (wantNorm && updateW && colValid) { a.colIn = c->colPart.as<double>(); a.colInN = c->plan.stripsW; }
      if (wantNorm || (fromH && updateW && !last && c->plan.lazy && c->plan.sideW && c->run.wPending && c->plan.nsplitH == 1)) side_io(a, wantNorm);
      const int did = launch_nmf_update5(a, s);
      if (wantNorm && !(did & 2)) c->run.planError = true; // (cannot happen: the dry run in the W update's step took the same arguments)
      c->run.normDue = false;
      c->run.sideFromH = (did & 1) != 0 && updateW && !last;
      if (did & 1)
      {
        const int G = ((int) c->T + 15) / 16;
        c->run.sideGen ^= 1;
        c->run.sideFromHSlices = a.stripsOverride > 0 ? std::min(a.stripsOverride, G) : nmf_update5_strips((int) c->T, (int) c->Kp, Bw);
      }
    }
    else launch_nmf_update_wide(a, c->wideScratch.as<double>(), s);
  }
}

static void enqueue_iteration(fluhip_corpus* c, bool updateW, bool updateH, bool last)
{
  if (c->plan.strip) enqueue_strip_iteration(c, updateW, updateH, last);
  else enqueue_mfma_iteration(c, updateW, updateH, last);
}

// alg/NMF.hpp:154-181 loop + :175-176 callbacks.  Iterations are enqueued back to back; with a progress callback
// every iteration is followed by an event and the callback is invoked once per completed iteration, in order, on
// the calling thread, with a bounded run-ahead.
static int corpus_iterate_loop(fluhip_corpus* c, int64_t iters, bool updateW, bool updateH,
                               fluhip_progress_fn progress, void* user)
{
  fluhip_ctx* ctx = c->ctx;
  c->run.begin_call();
  if (!progress)
  {
    // Corpora of several rounds of wavefronts (more than 1024 / strips buffers) run ROUND-MAJOR: all iterations of the
    // first 128 buffers (at 8 strips), then of the next 128, ...  Buffers are independent jobs (nrt/NMFClient.hpp:233),
    // so the order is free, and a round's factor matrices (63 MB at the bench shape) stay in the 256 MB last-level cache
    // from launch to launch, which the whole corpus's (500 MB at 1024 buffers) do not: 8-round launches measured 0.304 -
    // 0.319 ms per round against 0.271 - 0.278 for one-round launches (profiles/r03/bench_v*_1024_buffers_one_gpu.json).
    // With a progress callback the iterations stay outermost: "iteration i" means every buffer has passed it.
    // FLUHIP_ROUND_MAJOR=0: iteration-major as before.
    static const int roundEnv = fluhip::ab_int("FLUHIP_ROUND_MAJOR", 1);
    int64_t chunk = 0;
    if (roundEnv && !c->plan.strip && !c->plan.useLists && c->plan.lazy && c->plan.nsplitW == 1 && c->plan.nsplitH == 1 && c->plan.variant == 5)
    {
      const int CW = (int) c->F - (c->plan.sideW ? 1 : 0);
      const int wW = nmf_update5_strips(CW, (int) c->Kp, (int) c->B), wH = nmf_update5_strips((int) c->T, (int) c->Kp, (int) c->B);
      const int64_t per = 1024 / std::max(wW, wH);
      if (per >= 8 && c->B >= 2 * per)
      {
        // the schedule of ONE round of `per` buffers, kept for every window (the update kernel would otherwise deal its
        // strips from the number of buffers it is launched on); the W update's strips also fix the layout of its column
        // statistics, which was planned for the whole corpus
        const int wWc = nmf_update5_strips(CW, (int) c->Kp, (int) per), wHc = nmf_update5_strips((int) c->T, (int) c->Kp, (int) per);
        // (both updates must fill most of a round at that window: short buffers at a wide rank -- 128 x 1.6 s, rank 128: 32
        //  strips over the bins, 5 over the frames -- ran H updates of 160 wavefronts per window: 1 510 us per iteration against
        //  608 iteration-major, tools/wide_list_ab.sh)
        if (wWc == wW && per * std::max(wWc, wHc) <= 1024 && per * std::min(wWc, wHc) >= 768)
        {
          chunk = per; c->run.winStripsW = wWc; c->run.winStripsH = wHc;
        }
      }
    }
    if (chunk > 0)
    {
      for (int64_t b0 = 0; b0 < c->B; b0 += chunk)
      {
        c->run.winB0 = b0;
        c->run.winB = std::min(chunk, c->B - b0);
        c->run.sideFromH = false;
        for (int64_t i = 0; i < iters; i++) enqueue_iteration(c, updateW, updateH, i + 1 == iters);
      }
      c->run.winB0 = c->run.winB = 0;
    }
    else
    {
      // FLUHIP_GRAPH_ITERS=n (experiment, default off -- DESIGN.md "hipGraph"): after the first iteration, runs of n iterations
      // are captured once as a hipGraph and replayed; the last iterations (fewer than n + 1) are enqueued as usual.  n even: the
      // frame-strip schedule alternates two statistics buffers.  Not with the profiler's events in the stream.
      static const int graphN = fluhip::ab_int("FLUHIP_GRAPH_ITERS", 0) & ~1;
      int64_t i = 0;
      if (graphN >= 2 && !ctx->prof && iters >= 2 * (int64_t) graphN + 2)
      {
        enqueue_iteration(c, updateW, updateH, false);
        i = 1;
        // whatever fails in here, the stream leaves capture mode and the graph objects are released (an early
        // return between Begin- and EndCapture left the context's stream capturing, and every later call on it failed)
        struct Capture
        {
          hipStream_t s;
          hipGraph_t graph = nullptr;
          hipGraphExec_t exec = nullptr;
          bool capturing = false;
          ~Capture()
          {
            if (capturing) (void) hipStreamEndCapture(s, &graph);
            if (exec) (void) hipGraphExecDestroy(exec);
            if (graph) (void) hipGraphDestroy(graph);
          }
        } cap{ctx->stream};
        HIPCHK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        cap.capturing = true;
        for (int g = 0; g < graphN; g++) enqueue_iteration(c, updateW, updateH, false);
        cap.capturing = false;
        HIPCHK(ctx, hipStreamEndCapture(ctx->stream, &cap.graph));
        HIPCHK(ctx, hipGraphInstantiate(&cap.exec, cap.graph, nullptr, nullptr, 0));
        for (; i + graphN < iters; i += graphN) HIPCHK(ctx, hipGraphLaunch(cap.exec, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // (experiment: the graph is dropped right away)
      }
      for (; i < iters; i++) enqueue_iteration(c, updateW, updateH, i + 1 == iters);
    }
    HIPCHK(ctx, hipGetLastError());
    if (c->run.planError) return fail(ctx, "internal error: an update launch did not take the form its dry run announced");
    return FLUHIP_OK;
  }
  // One event per iteration; callbacks are delivered in order as the events complete, and the host never runs more
  // than kLag iterations ahead of the last one it has reported: a cancel at iteration i stops the device after at
  // most kLag - 1 further iterations (alg/NMF.hpp:175-176 stops at i exactly; the client above never looks at the
  // factors of a cancelled job, clients/nrt/NMFClient.hpp:273-274).
  constexpr int kMaxLag = 64;
  const int kLag = std::max(1, std::min(kMaxLag, ctx->progressLag));
  hipEvent_t ev[kMaxLag];
  for (int i = 0; i < kLag; i++) ev[i] = take_event(ctx);
  auto give_back = [&] { for (int i = 0; i < kLag; i++) ctx->eventPool.push_back(ev[i]); };
  int64_t reported = 0;
  for (int64_t i = 0; i < iters; i++)
  {
    enqueue_iteration(c, updateW, updateH, i + 1 == iters);
    if (hipEventRecord(ev[i % kLag], ctx->stream) != hipSuccess) { give_back(); return fail(ctx, "HIP error: hipEventRecord"); }
    const int64_t enq = i + 1;
    while (reported < enq)
    {
      hipEvent_t e = ev[reported % kLag];
      const bool mustWait = enq - reported >= kLag || enq == iters;
      hipError_t q = mustWait ? hipEventSynchronize(e) : hipEventQuery(e);
      if (q == hipErrorNotReady) break;
      if (q != hipSuccess) { give_back(); return fail(ctx, std::string("HIP error: ") + hipGetErrorString(q) + " in the iteration loop"); }
      reported++;
      if (!progress(reported, user))
      {
        (void) hipStreamSynchronize(ctx->stream);
        give_back();
        return fail(ctx, "cancelled", FLUHIP_CANCELLED);
      }
    }
  }
  give_back();
  if (c->run.planError) return fail(ctx, "internal error: an update launch did not take the form its dry run announced");
  return FLUHIP_OK;
}

int corpus_iterate(fluhip_corpus* c, int64_t iters, bool updateW, bool updateH,
                          fluhip_progress_fn progress, void* user)
{
  c->loopTimed = false;
  if (!c->loopEv0) { c->loopEv0 = take_event(c->ctx); c->loopEv1 = take_event(c->ctx); }
  const bool ev0 = c->loopEv0 && c->loopEv1 && hipEventRecord(c->loopEv0, c->ctx->stream) == hipSuccess;
  const int rc = corpus_iterate_loop(c, iters, updateW, updateH, progress, user);
  c->loopTimed = ev0 && hipEventRecord(c->loopEv1, c->ctx->stream) == hipSuccess;
  if (c->plan.strip)
  {
    c->run.stripReady = false; // H may change before the next call
    c->run.stripSideReady = false;
    if (c->run.wPending && !c->run.stripNormFresh)
    {
      // the last launch was a reduce: one workgroup per buffer recomputes the column norms of W'
      StripArgs a = strip_args(c); // (wPend = 1)
      a.statGen = c->run.stripGen;
#ifdef FLUHIP_AB_SWITCHES
      if (c->plan.stripTile)
      {
        BinTileArgs bt{};
        bt.work = c->tileWork.as<double>(); bt.F = a.F; bt.B = a.B;
        a.nRec = nmf_bintile_records(a.F); a.tileStat = nmf_bintile_records_ptr(bt, c->run.stripGen);
      }
#endif
      launch_nmf_strip(a, c->ctx->stream);
      c->run.stripNormFresh = true;
    }
    if (c->run.wPending) c->run.stripStatsValid = false; // the normalisation below rewrites W
  }
  if (c->run.wPending)
  {
    // leave the deferred form on every exit (also a cancelled run hands back W, alg/NMF.hpp:175-176)
    launch_wnorm_apply(c->Wf.as<double>(), c->Fp * c->Kp, (int) c->F, (int) c->Kp, (int) c->B, c->wnorm.as<double>(),
                       c->ctx->stream);
    c->run.wPending = false;
  }
  return rc;
}
