// corpus_plan.hip -- the planner of the corpus layer: which schedule the factor updates of a shape take (UpdatePlan), the work
// lists of ragged and small corpora, and the fluhip_debug_plan_* entry points that report both.  Pure host code: no device, no
// context, nothing read from a corpus -- api_corpus.hip allocates what a plan sizes, corpus_loop.hip launches what it says.
//   NMF::multiplicativeUpdates             include/flucoma/algorithms/public/NMF.hpp:144-183
#include "corpus_internal.h"

// which factor-update path runs:
//   5 = v_mfma_f64_4x4x4_4b + LDS-DMA operand streaming (kernels_nmf5.hip): every rank up to 128, padded to 16 / 32 / 64 / 128
//   0 = un-fused, over a materialised ratio matrix (kernels_nmf_wide.hip): any rank, used above 128
//       (FLUHIP_NMF_KERNEL=-1 forces it: an independent second implementation for the tests)
int update_variant(int Kp)
{
  if (Kp > 128) return 0;
  static const int forced = fluhip::ab_int("FLUHIP_NMF_KERNEL", 0);
  if (forced == -1) return 0;
  return 5;
}
// padded rank: the 4x4x4 kernel is built for 16 / 32 / 64 / 128 (components up to the padded rank are zero and stay zero);
// above 128 the any-rank path takes multiples of 16
int64_t padded_rank(int64_t K)
{
  if (K <= 16) return 16;
  if (K <= 32) return 32;
  if (K <= 64) return 64;
  if (K <= 128) return 128;
  return round_up(K, 16);
}

static int choose_split4(int64_t B, int C, int R, int Kp)
{
  static const int forceS = fluhip::ab_int("FLUHIP_PLAN_SPLIT", 0);
  const int64_t nSteps = (R + 3) / 4;
  const int64_t smax = std::max<int64_t>(1, std::min<int64_t>(64, nSteps / 12)); // >= 12 steps per wavefront
  if (forceS > 0) return (int) std::min<int64_t>(std::min<int64_t>(forceS, 64), std::max<int64_t>(1, nSteps / 2)); // the finalize kernel sums at most 64 splits
  const int64_t waves = B * nmf_update5_waves_per_buffer(C, Kp, (int) B);
  if (waves >= 768) return 1;
  // one wavefront per SIMD (the kernel's register footprint allows no more): never exceed 1024 in
  // total, a 1025th wavefront would wait for a whole pass of the others
  const int64_t s = 1024 / waves;
  return (int) std::max<int64_t>(1, std::min(s, smax));
}

// A whole-contraction update whose wavefronts need a last, poorly filled round of the 1024 SIMDs (config 3's H update: 2 x 808
// strips = 1.58 rounds, paid as 2) goes out as TWO launches: the strips that fill whole rounds as before, then the remaining
// strips with their contraction cut into `split` pieces (uniform split schedule: partials + finalize), which deals the tail
// over the chip in short rounds -- 513 + 2 x 171 steps instead of 2 x 513.  Costs in 4-row steps of this strip width:
// ~20 k cycles of prologue + epilogue per wavefront, partials written and read back at ~3 TB/s plus the finalize launch.
// Returns the split (0: one launch pays) and the strips per buffer of the first launch.  FLUHIP_TAIL_SPLIT: 0 off, n forces n
// pieces; FLUHIP_TAIL_SLOTS: the wavefronts of a round (tests: small corpora take the path).
static int plan_tail(int64_t B, int C, int R, int Kp, int* stripsA)
{
  static const int forceS = fluhip::ab_int("FLUHIP_TAIL_SPLIT", -1);
  static const int slotsEnv = fluhip::ab_int("FLUHIP_TAIL_SLOTS", 0);
  *stripsA = 0;
  if (forceS == 0) return 0;
  const int64_t slots = slotsEnv > 0 ? slotsEnv : 1024;
  const int G = (C + 15) / 16;
  const int w = nmf_update5_strips(C, Kp, (int) B);
  const int ng = (G + w - 1) / w;
  const int64_t total = B * w;
  const int64_t roundsA = total / slots;
  if (roundsA < 1 || roundsA > 3 || total % slots == 0) return 0;
  // (a workgroup is four wavefronts of ONE buffer and one workgroup fills a CU: strips are dealt in fours, and a launch
  //  occupies round_up(strips, 4) slots per buffer -- 200 buffers x 5 strips are 400 workgroups, two rounds, not 1000 slots)
  int wA = (int) std::min<int64_t>(w - 1, roundsA * slots / B);
  wA -= wA % 4;
  if (wA < 4) return 0;
  const int64_t nRest = B * round_up(w - wA, 4);
  const int64_t nSteps = (R + 3) / 4;
  const double cycles = 400.0 + 270.0 * ng * (Kp / 32.0); // per step (measured: rank 32 400 + 270 NG; rank 128, 2 groups 2 376)
  const double ovh = 20000.0 / cycles, stepUs = cycles / 2300.0;
  const double cur = (double) ((B * round_up(w, 4) + slots - 1) / slots) * (nSteps + ovh);
  const int64_t restCols = C - (int64_t) wA * ng * 16;
  int best = 0;
  double bestCost = 0.93 * cur; // a clear win only
  const int smax = (int) std::min<int64_t>(8, nSteps / 12);
  for (int sp = 2; sp <= smax; sp++)
  {
    if (forceS > 0 && sp != std::min(forceS, smax)) continue;
    const double finUs = 2.0 * sp * B * restCols * Kp * 8.0 / 3.0e6 + 8.0;
    const double cost = (double) ((B * wA + slots - 1) / slots) * (nSteps + ovh) +
                        (double) ((nRest * sp + slots - 1) / slots) * ((nSteps + sp - 1) / sp + ovh) + finUs / stepUs;
    // (more pieces only for a clear gain: they cost memory, and config 3 measures the same with 3 and 5)
    if ((best == 0 ? cost < bestCost : cost < 0.97 * bestCost) || (forceS > 0 && best == 0)) { best = sp; bestCost = cost; }
  }
  if (best) *stripsA = wA;
  return best;
}

static bool offsize_enabled()
{
  static const int offEnv = fluhip::ab_int("FLUHIP_OFFSIZE", 1);
  return offEnv != 0;
}
// where the work-list form beats the uniform split schedule for equal-length corpora (tools/batch_timing.py with
// FLUHIP_LIST_PLAN=0|1, profiles/r03/small_batches_*.jsonl)
struct PlanShape { int64_t B, T, F, Kp; }; // what the choice of schedule depends on (also reachable without a corpus: fluhip_debug_plan_kind)
static bool list_plan_pays(const PlanShape* c)
{
  // measured at rank 32, 10 s buffers (us per iteration, uniform schedule -> lists): 1 buffer 47 -> 51, 2: 53 -> 57, 4: 73 -> 65,
  // 8: 92 -> 73, 16: 135 -> 109, 24: 196 -> 168, 32: 250 -> 202, 48: 346 -> 289, 64: 370 -> 345, 96: 758 -> 511, 112: 878 -> 564,
  // 128: 619 = 621 (the same schedule either way); ranks 16 / 64 / 128 at 4 and 16 buffers likewise (49 -> 49, 89 -> 76;
  // 130 -> 98, 227 -> 193; 211 -> 160, 486 -> 476).  Between one and two rounds (profiles/r03/midsize_ab.txt, two rounds of
  // the uniform schedule = ~1 250 us): 144 buffers 729, 176: 854, 200: 1 007, 232: 1 102, 250: 1 153.  So: from three buffers on,
  // while whole contractions at the widest strips do not fill the chip in whole rounds.
  const int maxNG = nmf_update5_max_groups((int) c->Kp);
  const int G = ((int) c->F - 1 + 15) / 16;
  const int64_t w0 = c->B * ((G + maxNG - 1) / maxNG);
  // Beyond one round the lists win as well, whole rounds or not (profiles/r03/midsize_ab.txt parts 3 - 4, uniform schedule in
  // round-major windows -> lists: 288 buffers 1 723 -> 1 475 us, 400: 2 300 -> 2 015, 520: 2 864 -> 2 589, 900: 4 568 -> 4 320,
  // 1000: 4 586 -> 4 424; exact multiples of a round 256: 1 222 -> 1 206, 512: 2 346 -> 2 285, 1024: 4 611 -> 4 485, and with a
  // progress callback -- iteration-major launches of several rounds -- 512: 2 427 -> 2 234, 1024: 5 157 -> 4 452): several
  // thousand workgroups handed out as CUs free up keep the chip busy across what the uniform launch runs as lock-step rounds.
  // Exactly one round (the bench shard: 128 buffers) is the same schedule either way and stays on the uniform kernel.
  // (Rank 128 apart: the list kernel's instantiation there -- grouped refill, column sums in the kernel -- runs 3 580 cycles per
  //  step against the uniform one's 2 376.)
  // Rank 128 (profiles/r03/plan_regimes.txt): 4 buffers 211 -> 160 on the lists, but 16: 452 -> 500, 24: 581 -> 820, 32: 639 -> 818,
  // 40: 902 (uniform, two-launch H update) -> 1 330 -- lists only while whole contractions fill less than half a round.
  // (few buffers, 10 s each: 3: 177 -> 167, 4: 168 -> 163, 8: 240 -> 273, 12: 516 -> 405; long ones lose: 4 x 60 s 558 -> 753)
  if (c->Kp > 64) return c->B >= 3 && w0 < 512 && c->T <= 2048;
  // Rank 64 follows rank 32 (100 x 10 s 1 333 -> 1 043, 300: 2 999 -> 2 771, 128 x 2 s 330 -> 317, 1 x 60 s 131 -> 106, 1 x 300 s
  // 417 -> 263, 2 x 300 s 800 -> 614; 40 x 10 s 456 -> 473 the one loss).
  // One or two buffers (rank <= 64; a single buffer of rank <= 16 that fits the frame-strip schedule never gets here): the
  // uniform split schedule up to ~45 s of frames in all (1 x 30 s 62.5 us per iteration against 66.7, 2 x 10 s 53 against 57),
  // lists beyond (1 x 60 s 80.5 -> 72.8, 1 x 300 s 253 -> 163, 2 x 30 s 79.3 -> 71.3, 2 x 300 s 454 -> 340).
  if (c->B <= 2) return c->B * c->T * c->F >= 4200000;
  return w0 != 1024;
}

// ---------------------------------------------------------------------------------------
// ragged corpora: work lists of the two factor updates
// ---------------------------------------------------------------------------------------
namespace {
// up to four wavefronts that share a strip and split its contraction (WaveDesc::grp); they stay together in one workgroup
struct WaveGroup
{
  std::vector<WaveDesc> waves; // waves[0] is the leader; grp holds (rank << 4 | size << 8) until the packing
  int64_t work;                // what the group takes: its longest member
  int buf;
};

// groups -> workgroups of 4 wavefronts: longest first (the hardware hands the next workgroup to whichever CU frees up),
// first fit (a later, shorter group fills the slots an earlier workgroup has left).  Workgroup i runs on XCD i & 7 and a
// launch of up to 256 workgroups is ONE round only if every XCD gets at most 32 of them, so the workgroups are numbered
// in list order -- 8 consecutive ones on 8 different XCDs -- rather than by buffer.
void pack_groups(std::vector<WaveGroup>& groups, std::vector<WaveDesc>& out, int* wgs)
{
  std::stable_sort(groups.begin(), groups.end(), [](const WaveGroup& a, const WaveGroup& b) { return a.work > b.work; });
  std::vector<std::vector<WaveDesc>> q; // workgroups of up to 4 descriptors
  size_t firstOpen = 0;
  for (const auto& g : groups)
  {
    bool placed = false;
    while (firstOpen < q.size() && q[firstOpen].size() >= 4) firstOpen++;
    for (size_t i = std::max(firstOpen, q.size() > 256 ? q.size() - 256 : 0); i < q.size(); i++) // (a bounded look-back: linear time)
      if (q[i].size() + g.waves.size() <= 4) { q[i].insert(q[i].end(), g.waves.begin(), g.waves.end()); placed = true; break; }
    if (!placed) q.push_back(g.waves);
  }
  out.assign(q.size() * 4, WaveDesc{0, 0, 0, 0, 0, -1, 0, -1, 0, 0, 0, 0});
  for (size_t i = 0; i < q.size(); i++)
  {
    auto& wgp = q[i];
    bool barrier = false;
    for (const auto& d : wgp) barrier = barrier || ((d.grp >> 8) & 15) > 1;
    size_t leaderAt = 0; // the leader's wavefront index is known only now
    for (size_t w = 0; w < wgp.size(); w++)
    {
      WaveDesc d = wgp[w];
      const int rank = (d.grp >> 4) & 15, size = (d.grp >> 8) & 15;
      if (rank == 0) leaderAt = w;
      d.grp = (int) leaderAt | (rank << 4) | (size << 8) | (barrier ? (1 << 16) : 0);
      out[i * 4 + w] = d;
    }
  }
  *wgs = (int) q.size();
}

} // namespace

// Work lists of the two factor updates over buffers with their own frame counts tOf[b]: ragged corpora, and equal-length
// corpora too small to fill the chip with whole contractions (the intra-workgroup reduction is what this form has over the
// uniform split schedule: fewer or no partials in memory, no finalize launch).
// pure host code (no device, no context): also reachable through fluhip_debug_plan_lists for the CPU tests
static void build_list_plan(const std::vector<int>& tOf, int Tmax, int F, int Kp, ListPlanHost& out)
{
  const int B = (int) tOf.size();
  const int maxNG = nmf_update5_max_groups(Kp);
  // ---- W update: strips over the bins (the same for every buffer), the contraction over a buffer's own frames ------------
  {
    std::vector<int> steps((size_t) B);
    for (int b = 0; b < B; b++) steps[(size_t) b] = (tOf[(size_t) b] + 3) / 4;
    // the Nyquist bin as a side column (fluhip_kernels.h SideColumn): every power-of-two transform has 16 m + 1 bins, and a
    // wavefront runs the loop of the widest strip of the launch -- 65 column groups never deal evenly
    static const int sideOff = fluhip::ab_int("FLUHIP_NO_SIDE", 0);
    out.sideW = !sideOff && nmf_side_column_supported(Tmax, F, Kp);
    const int C = F - (out.sideW ? 1 : 0);
    const int G = (C + 15) / 16;
    // One candidate schedule per strip width.  Contractions are cut into pieces when one round of wavefronts (1024 SIMDs, one
    // workgroup of four per CU) would stay part empty: the wavefront budget goes to whichever buffer has the longest pieces
    // (down to 12 steps); the pieces of one strip go to up to four wavefronts of one workgroup (added up through the LDS:
    // WaveDesc::grp) and only what is left beyond four becomes partials in memory for the finalize launch.  Cost model as
    // for the H update below: ~400 + 270 NG cycles per step of a strip of NG column groups, ~40 k per round, ~60 k per
    // finalize launch -- narrow strips cost little per group, so few buffers take many narrow strips and few partials.
    struct Cand
    {
      std::vector<WaveDesc> list;
      std::vector<int> splitTab;
      bool anyPartial = false;
      int64_t pbase = 0;
      int maxSplit = 1, maxPieces = 1, wgs = 0, wW = 0, ngW = 0;
      double cost = 1e300;
    };
    auto build = [&](int wW, int forcedBudget) -> Cand {
      Cand r;
      r.wW = wW;
      r.ngW = (G + wW - 1) / wW;
      r.splitTab.assign((size_t) B * 2, 0);
      const int gmax = std::min(fluhip::ab_int("FLUHIP_RG_GMAX", 4), nmf_update5_groups_fit(Kp, r.ngW) ? 4 : 1);
      const int64_t waves0 = (int64_t) B * wW;
      const int64_t wgs0 = (waves0 + 3) / 4;
      const int64_t roundsWanted = wgs0 <= 384 ? std::max<int64_t>(1, (wgs0 + 255) / 256) : 0; // 0: many rounds, no cutting
      std::vector<int> nsOf((size_t) B, 1);
      for (int64_t budgetWaves = forcedBudget > 0 ? forcedBudget : 1024 * std::max<int64_t>(roundsWanted, 1);; budgetWaves -= 32)
      {
        std::fill(nsOf.begin(), nsOf.end(), 1);
        if (roundsWanted > 0 && budgetWaves > waves0)
        {
          const int64_t budget = budgetWaves / wW;
          auto piece = [&](int b) { return (steps[(size_t) b] + nsOf[(size_t) b] - 1) / nsOf[(size_t) b]; };
          std::vector<std::pair<int, int>> heap; // (piece, buffer)
          for (int b = 0; b < B; b++) heap.emplace_back(piece(b), b);
          std::make_heap(heap.begin(), heap.end());
          for (int64_t units = B; units < budget; units++)
          {
            std::pop_heap(heap.begin(), heap.end());
            const int b = heap.back().second;
            if (heap.back().first <= 12 || nsOf[(size_t) b] >= 64) break; // the longest piece cannot get shorter
            nsOf[(size_t) b]++;
            heap.back() = std::make_pair(piece(b), b);
            std::push_heap(heap.begin(), heap.end());
          }
        }
        r.anyPartial = false;
        for (int b = 0; b < B; b++) r.anyPartial = r.anyPartial || nsOf[(size_t) b] > gmax;
        std::vector<WaveGroup> groups;
        r.pbase = 0;
        r.maxSplit = 1;
        r.maxPieces = 1;
        int64_t longest = 0;
        for (int b = 0; b < B; b++)
        {
          const int ns = nsOf[(size_t) b];
          const int per = (steps[(size_t) b] + ns - 1) / ns;
          const int np = (ns + gmax - 1) / gmax; // partials in memory
          r.splitTab[(size_t) b * 2] = (int) r.pbase;
          r.splitTab[(size_t) b * 2 + 1] = np;
          r.maxSplit = std::max(r.maxSplit, np);
          r.maxPieces = std::max(r.maxPieces, ns);
          longest = std::max<int64_t>(longest, per);
          int piece = 0;
          for (int q = 0; q < np; q++)
          {
            const int size = ns / np + (q < ns % np ? 1 : 0);
            const int base = G / wW, rem = G % wW;
            int g0 = 0;
            for (int st = 0; st < wW; st++)
            {
              const int ng = base + (st < rem ? 1 : 0);
              WaveGroup grp;
              grp.buf = b; grp.work = 0;
              for (int rk = 0; rk < size; rk++)
              {
                const int s0 = std::min(steps[(size_t) b], (piece + rk) * per), s1 = std::min(steps[(size_t) b], s0 + per); // (an empty tail piece: no steps, zeros)
                WaveDesc d{};
                d.buf = b; d.g0 = g0; d.ng = ng; d.s0 = s0; d.s1 = std::max(s0, s1);
                d.partIdx = (r.anyPartial && rk == 0) ? (int) r.pbase + q : -1;
                d.statIdx = b * wW + st;
                d.dIdx = (r.anyPartial && st == 0 && rk == 0) ? d.partIdx : -1;
                d.grp = (rk << 4) | (size << 8);
                grp.work = std::max<int64_t>(grp.work, d.s1 - d.s0);
                grp.waves.push_back(d);
              }
              if (ng > 0) groups.push_back(std::move(grp));
              g0 += ng;
            }
            piece += size;
          }
          r.pbase += np;
        }
        pack_groups(groups, r.list, &r.wgs);
        const double rounds = roundsWanted == 0 ? (double) r.wgs / 256.0 : (double) ((r.wgs + 255) / 256);
        r.cost = rounds * ((double) longest * (400.0 + 270.0 * r.ngW) + 40000.0) + (r.maxPieces > 1 ? 6000.0 : 0.0) +
                 (r.anyPartial ? 60000.0 + 3000.0 * r.maxSplit : 0.0);
        if (roundsWanted == 0 || r.wgs <= 256 * roundsWanted || budgetWaves <= waves0 || forcedBudget > 0) break;
      }
      return r;
    };
    Cand best;
    const int forcedNG = fluhip::ab_int("FLUHIP_RG_WNG", 0), forcedBudget = fluhip::ab_int("FLUHIP_RG_WBUDGET", 0);
    int lastW = -1;
    for (int ngc = maxNG; ngc >= 1; ngc--)
    {
      if (forcedNG > 0 && ngc != std::min(forcedNG, maxNG)) continue;
      const int wW = (G + ngc - 1) / ngc;
      if (wW == lastW) continue; // the same strips as the wider candidate
      lastW = wW;
      // wide strips re-use the moving factor's rows over more columns: with enough buffers to fill the chip without cutting
      // anything the widest form is what the batched kernel was tuned for -- narrower candidates only while the chip is not full
      if (forcedNG == 0 && (int64_t) B * ((G + maxNG - 1) / maxNG) >= 1536 && ngc < maxNG) break;
      Cand cnd = build(wW, forcedBudget);
      if (cnd.cost < best.cost - 1.0) best = std::move(cnd);
    }
    out.W.wgs = best.wgs;
    out.W.ng = best.ngW; out.W.partial = best.anyPartial ? 1 : 0; out.W.maxSplit = best.maxSplit;
    out.W.nPartials = best.anyPartial ? best.pbase : 0;
    out.W.statParts = best.anyPartial ? update_finalize_parts(C, Kp) : best.wW;
    out.W.pieces = best.maxPieces;
    out.W.list = std::move(best.list);
    out.W.splitTab = std::move(best.splitTab);
  }
  // ---- H update: strips over a buffer's own frames, the contraction over the bins (the same for every buffer) ------------
  {
    std::vector<int> groupsOf((size_t) B);
    for (int b = 0; b < B; b++) groupsOf[(size_t) b] = (tOf[(size_t) b] + 15) / 16;
    // Strip width NG, pieces of the bin contraction that share a workgroup (gsz: added up through the LDS) and partials in
    // memory (ns: a finalize launch) by a small cost model in shader cycles, fitted to tools/ragged_sweep.sh
    // and tools/batch_timing.py: a wavefront runs the loop of the launch's widest strip at ~400 + 270 NG cycles per 4-row step
    // (measured: 1 group 695, 4: 1 370, 6: 1 780, 7: 2 250, 8: 2 620, 9: 2 775), a round of up to 256 workgroups pays ~40 k
    // cycles of prologue, epilogue and launch, a finalize launch ~60 k.
    const int steps = (F + 3) / 4;
    int NG = maxNG, gsz = 1, ns = 1;
    double bestCost = 1e300;
    for (int cand = maxNG; cand >= 1; cand--)
    {
      int64_t strips = 0;
      int widestStrip = 1;
      for (int b = 0; b < B; b++)
      {
        const int w = (groupsOf[(size_t) b] + cand - 1) / cand;
        strips += w;
        widestStrip = std::max(widestStrip, (groupsOf[(size_t) b] + w - 1) / std::max(w, 1));
      }
      const bool fit = nmf_update5_groups_fit(Kp, widestStrip);
      for (int g : {1, 2, 4})
      {
        if (g > 1 && !fit) continue;
        for (int m : {1, 2, 3, 4, 6, 8, 12, 16})
        {
          const int pieces = g * m;
          if (pieces > 1 && steps / pieces < 12) continue;
          const int64_t wgs = (strips * m + (4 / g) - 1) / (4 / g);
          const double rounds = (double) ((wgs + 255) / 256);
          const double perWave = (double) ((steps + pieces - 1) / pieces) * (400.0 + 270.0 * widestStrip) + 40000.0;
          const double cost = rounds * perWave + (g > 1 ? 6000.0 : 0.0) + (m > 1 ? 60000.0 + 3000.0 * m : 0.0);
          if (cost < bestCost - 1.0) { bestCost = cost; NG = cand; gsz = g; ns = m; }
        }
      }
    }
    NG = std::max(1, std::min(maxNG, fluhip::ab_int("FLUHIP_RG_HNG", NG)));
    gsz = fluhip::ab_int("FLUHIP_RG_HG", gsz);
    ns = fluhip::ab_int("FLUHIP_RG_HM", ns);
    int ngH = 1;
    for (int b = 0; b < B; b++)
    {
      const int w = (groupsOf[(size_t) b] + NG - 1) / NG;
      ngH = std::max(ngH, (groupsOf[(size_t) b] + w - 1) / std::max(w, 1));
    }
    if (!nmf_update5_groups_fit(Kp, ngH)) gsz = 1;
    const int pieces = gsz * ns;
    const int per = (steps + pieces - 1) / pieces;
    std::vector<WaveGroup> groups;
    std::vector<int> splitTab((size_t) B * 2);
    for (int b = 0; b < B; b++) { splitTab[(size_t) b * 2] = b * ns; splitTab[(size_t) b * 2 + 1] = ns; }
    for (int b = 0; b < B; b++)
    {
      const int G = groupsOf[(size_t) b];
      const int w = (G + NG - 1) / NG;
      for (int j = 0; j < ns; j++)
      {
        const int base = G / w, rem = G % w;
        int g0 = 0;
        for (int st = 0; st < w; st++)
        {
          const int ng = base + (st < rem ? 1 : 0);
          WaveGroup grp;
          grp.buf = b; grp.work = 0;
          for (int r = 0; r < gsz; r++)
          {
            WaveDesc d{};
            d.buf = b; d.g0 = g0; d.ng = ng;
            d.s0 = std::min(steps, (j * gsz + r) * per); d.s1 = std::max(d.s0, std::min(steps, d.s0 + per));
            d.partIdx = (ns > 1 && r == 0) ? b * ns + j : -1;
            d.statIdx = 0;
            d.dIdx = (ns > 1 && st == 0 && r == 0) ? d.partIdx : -1;
            d.grp = (r << 4) | (gsz << 8);
            grp.work = std::max<int64_t>(grp.work, (int64_t) (d.s1 - d.s0) * ng);
            grp.waves.push_back(d);
          }
          if (ng > 0) groups.push_back(std::move(grp));
          g0 += ng;
        }
      }
    }
    pack_groups(groups, out.H.list, &out.H.wgs);
    out.H.ng = ngH; out.H.partial = ns > 1 ? 1 : 0; out.H.maxSplit = ns; out.H.nPartials = ns > 1 ? (int64_t) B * ns : 0;
    out.H.pieces = pieces;
    out.H.splitTab = std::move(splitTab);
  }
}

// Off-size ranks (round 5): a rank between two array ranks keeps the ARRAYS of the padded rank (32 / 64 / 128) -- every
// helper kernel runs its form of that rank on zero columns -- and the factor updates compute fewer MFMAs per product
// (kernels_nmf5.hip KPM, nmf_update5_compute_rank): 6 of 8 for ranks 17 .. 24; 10 / 12 / 14 of 16 for 33 .. 40 / 48 / 56; 18, 20 .. 28
// of 32 for 65 .. 72, .. 80, .. 112.  The plain and the split-contraction schedules and the work lists; the strip schedule
// (rank <= 16) has no off-size rank.  FLUHIP_OFFSIZE=0 (A/B build): the padded forms, for the comparison.
static int compute_rank(int64_t B, int64_t T, int64_t F, int64_t K, int Kp)
{
  const int Kc = offsize_enabled() ? nmf_update5_compute_rank((int) K, Kp) : Kp;
  // (the launcher deals its strips by the COMPUTE rank, everything planned here -- statistics records, side
  //  slices, the tail launch, the scratch sizes -- by the padded rank.  The two agree because the group limits are the same
  //  within an off-size class; should a future form break that, the shape keeps the padded rank rather than a layout mismatch)
  if (Kc != Kp && (nmf_update5_strips((int) F, Kc, (int) B) != nmf_update5_strips((int) F, Kp, (int) B) ||
                   nmf_update5_strips((int) F - 1, Kc, (int) B) != nmf_update5_strips((int) F - 1, Kp, (int) B) ||
                   nmf_update5_strips((int) T, Kc, (int) B) != nmf_update5_strips((int) T, Kp, (int) B)))
    return Kp;
  return Kc;
}

// What the plain one-launch H update with arguments `a` (shape, ranks, split, strips) takes over from the launches around it:
// bit 0 the side partials of the next W update, bit 1 (wantNorm) the norm combine of the W update in front, bit 2 (colInN
// records per buffer) its column sums from that W update.  The launcher's own answer -- nothing is launched, no device is
// touched (UpdateArgs::dryRun) -- asked the same way by the iteration loop and by the planner's debug entry points.
int plain_h_update_takes(UpdateArgs a, bool wantNorm, int colInN)
{
  static double dummy = 0.0;
  a.nrm = &dummy; a.nrmMode = 2;
  a.sideOut = &dummy; a.sideWold = &dummy;
  if (wantNorm) { a.cmbStat = &dummy; a.cmbSide = &dummy; a.cmbWold = &dummy; a.cmbNrmOut = &dummy; a.cmbRowOut = &dummy; }
  if (colInN > 0) { a.colIn = &dummy; a.colInN = colInN; }
  a.dryRun = true;
  return launch_nmf_update5(a, nullptr);
}

// The plan of a work-list corpus from its frame counts tOf[b] (T: the longest): equal-length shapes come here from
// decide_update_plan, ragged corpora straight from plan_updates.  The lists themselves are built (and checked descriptor by
// descriptor: tests/test_list_plan.py) by build_list_plan and handed back for the upload.
void decide_list_plan(const std::vector<int>& tOf, int64_t T, int64_t F, int64_t K, UpdatePlan& p, ListPlanHost& lp)
{
  const int64_t B = (int64_t) tOf.size(), Tp = round_up(T, 32), Fp = round_up(F, 32);
  p = UpdatePlan{};
  p.Kp = padded_rank(K);
  const int Kp = (int) p.Kp;
  p.lazy = p.useLists = true;
  p.Kc = compute_rank(B, T, F, K, Kp);
  build_list_plan(tOf, (int) T, (int) F, Kp, lp);
  p.sideW = lp.sideW;
  p.stripsW = lp.W.statParts;
  p.nsplitW = lp.W.pieces;
  p.nsplitH = lp.H.pieces;
  const int64_t nPart = std::max(lp.W.nPartials, lp.H.nPartials);
  p.partDoubles = nPart * std::max(Fp, Tp) * Kp;
  p.dpartDoubles = std::max<int64_t>(32, std::max<int64_t>(nPart, B) * Kp);
  p.wscratchDoubles = wnorm_scratch_doubles(Kp, (int) B, p.stripsW);
}

// ---------------------------------------------------------------------------------------
// The schedule of the factor updates of a shape as DATA (round 6).  decide_update_plan() is a pure function
// of (B, T, F, K): no device, no allocation, nothing read from a corpus -- every choice between the uniform / split / work-list /
// frame-strip / two-launch / any-rank forms, the side column, the off-size compute rank, and the size in doubles of every
// workspace the launches of that plan index.  plan_updates() keeps it on the corpus and allocates exactly those sizes;
// fluhip_debug_plan_shape() reports it without a device; tests/test_plan_table.py holds it to its invariants over a grid of
// shapes and to the pinned plans of the BASELINE and perf-matrix shapes.
void decide_update_plan(int64_t B, int64_t T, int64_t F, int64_t K, UpdatePlan& p, ListPlanHost* lists)
{
  p = UpdatePlan{};
  const int64_t Tp = round_up(T, 32), Fp = round_up(F, 32);
  p.Kp = padded_rank(K);
  p.variant = update_variant((int) p.Kp);
  p.Kc = (int) p.Kp;
  p.nsplitW = p.nsplitH = 1;
  if (p.variant == 0)
  {
    p.wideDoubles = std::max(nmf_update_wide_scratch_doubles((int) T, (int) F, (int) p.Kp, (int) B),
                             nmf_update_wide_scratch_doubles((int) F, (int) T, (int) p.Kp, (int) B));
  }
  else
  {
    const int Kp = (int) p.Kp;
    p.nsplitW = choose_split4(B, (int) F, (int) T, Kp);
    p.nsplitH = choose_split4(B, (int) T, (int) F, Kp);
    // Fast path: W stays un-normalised in memory during the loop (UpdateArgs::nrm), the column statistics
    // come out of the update kernel's epilogue and the Nyquist bin is a side column when that shortens the
    // widest strip of the MFMA kernel (fluhip_kernels.h SideColumn).
    static const int lazyOff = fluhip::ab_int("FLUHIP_NO_LAZY", 0);
    static const int sideOff = fluhip::ab_int("FLUHIP_NO_SIDE", 0);
    p.lazy = !lazyOff;
    if (p.lazy && !sideOff && p.nsplitW == 1 && nmf_side_column_supported((int) T, (int) F, Kp) &&
        choose_split4(B, (int) F - 1, (int) T, Kp) == 1)
    {
      const int G = ((int) F + 15) / 16, G1 = G - 1;
      const int w = nmf_update5_strips((int) F, Kp, (int) B);
      const int w1 = nmf_update5_strips((int) F - 1, Kp, (int) B);
      // worth it when the widest strip gets shorter, or when the launch needs fewer passes over the 1024 SIMDs
      const int64_t passes = (B * w + 1023) / 1024, passes1 = (B * w1 + 1023) / 1024;
      p.sideW = w1 <= w && ((G1 + w1 - 1) / w1 < (G + w - 1) / w || passes1 < passes);
    }
    else if (p.lazy && !sideOff && p.nsplitW > 1 && nmf_side_column_supported((int) T, (int) F, Kp))
    {
      // Split contraction (few buffers): without the 16 m + 1-th bin the strips deal evenly and the pieces get shorter --
      // config 3 (2 x 2049 bins, rank 128): 130 strips x 7 pieces of 923 steps (910 wavefronts) -> 128 strips x 8 pieces
      // of 808 steps (1024 wavefronts).  Taken when the longest piece shrinks.
      const int s1 = choose_split4(B, (int) F - 1, (int) T, Kp);
      const int64_t nSteps = (T + 3) / 4;
      const int64_t w = B * nmf_update5_waves_per_buffer((int) F, Kp, (int) B);
      const int64_t w1 = B * nmf_update5_waves_per_buffer((int) F - 1, Kp, (int) B);
      if (s1 > 1 && w1 * s1 <= 1024 && w * p.nsplitW <= 1024 && (nSteps + s1 - 1) / s1 < (nSteps + p.nsplitW - 1) / p.nsplitW)
      {
        p.sideW = true;
        p.nsplitW = s1;
      }
    }
    // A single buffer of rank <= 16 runs the frame-strip schedule while one round of workgroups covers it (at most 6 frame
    // quads per CU: 71 s at hop 512): two launches per iteration instead of five and V read once.  Longer buffers and
    // batches stay with the split / batched kernels, which win there (tools/strip_vs_split.py).  FLUHIP_STRIP=0 off,
    // =1 wherever the kernel supports the shape.
    static const int stripEnv = fluhip::ab_int("FLUHIP_STRIP", -1);
    p.strip = p.lazy && stripEnv != 0 && nmf_strip_supported((int) F, (int) T, Kp) &&
              (stripEnv == 1 || (B == 1 && nmf_strip_workgroups((int) T) <= 512));
    if (p.strip)
    {
      p.sideW = false;
      p.stripPartDoubles = nmf_strip_part_doubles((int) F, (int) T, (int) B);
      // FLUHIP_STRIP_BIN=1 (A/B build only): the W update as its own launch over bin strips instead of the fused form (W
      // partials behind the H phase + the reduce launch).  Built and measured in round 4 (profiles/r04/c2_forms.md): 45.1 us
      // per iteration against 40.3 at config 2 -- a tenth of the partial bytes, but the last arriver's chain of cross-XCD
      // round trips (ticket, partials in two rounds, update) costs what the reduce launch cost.  Not adopted.
      static const int binEnv = fluhip::ab_int("FLUHIP_STRIP_BIN", 0);
      p.stripBin = kAbSwitches && binEnv != 0;
      // Round 5: the W update as the BIN-TILED launch (kernels_nmf_bintile.hip: four bins and ALL frames per workgroup, no
      // numerator partials in memory, no reduce launch, no ticket), the strip kernel doing the H update and the Nyquist bin's
      // partials.  Built to the review's specification, parity-green at full size, and measured at config 2
      // (profiles/r05/c2_bintile.md): 20.3 us for the launch in three layouts against the review's 13 us kill line.  Not
      // adopted: A/B build only (the kernel is not part of the production library), FLUHIP_STRIP_TILE=1.
#ifdef FLUHIP_AB_SWITCHES
      static const int tileEnv = fluhip::ab_int("FLUHIP_STRIP_TILE", 0);
      p.stripTile = !p.stripBin && tileEnv == 1 && nmf_bintile_supported((int) F, (int) T, Kp) &&
                    nmf_strip_tile_supported((int) F, (int) T, Kp);
#endif
    }
    // Equal-length corpora too small to fill the chip with whole contractions: the work-list form (decide_list_plan) instead of
    // the uniform split schedule -- narrow strips, the pieces of a contraction added up inside a workgroup, few or no
    // partials in memory.  FLUHIP_LIST_PLAN=0 keeps the uniform split schedule, =1 takes the lists whenever something is split.
    static const int listEnv = fluhip::ab_int("FLUHIP_LIST_PLAN", -1);
    const PlanShape ps{B, T, F, Kp};
    p.useLists = !p.strip && p.lazy && listEnv != 0 && (listEnv == 1 || list_plan_pays(&ps));
    if (p.useLists)
    {
      ListPlanHost lp;
      decide_list_plan(std::vector<int>((size_t) B, (int) T), T, F, K, p, lists ? *lists : lp);
      return;
    }
    p.Kc = (p.lazy && !p.strip) ? compute_rank(B, T, F, K, Kp) : Kp;
    // statistics partials of the W update: one per wavefront of a buffer, or one per 64-row chunk from the
    // finalize kernel when the contraction is split
    p.stripsW = p.nsplitW > 1 ? update_finalize_parts((int) F - (p.sideW ? 1 : 0), Kp)
                              : nmf_update5_strips((int) F - (p.sideW ? 1 : 0), Kp, (int) B);
    if (!p.strip && p.lazy && p.nsplitH == 1)
    {
      int wA = 0;
      const int sp = plan_tail(B, (int) T, (int) F, Kp, &wA);
      if (sp > 1)
      {
        const int G = ((int) T + 15) / 16, w = nmf_update5_strips((int) T, Kp, (int) B);
        p.tailSplitH = sp;
        p.tailStripsH = wA;
        p.tailRestH = w - wA;
        p.tailColsH = wA * ((G + w - 1) / w) * 16;
      }
    }
    if (!p.strip) p.stripsH = nmf_update5_strips((int) T, p.Kc, (int) B);
    // workspaces of the factor updates: split-contraction partials, denominators, column-sum pre-pass
    const int ns = std::max(std::max(p.nsplitW, p.nsplitH), p.tailSplitH);
    if (ns > 1 && !p.strip)
    {
      // partial numerators [B][pieces][rows][Kp]: the W update's rows are the bins, the H update's the frames (of the tail launch:
      // the frames behind the whole-contraction ones); the launches set UpdateArgs::Cp to their own row count
      const int64_t rowsW = p.nsplitW > 1 ? (int64_t) p.nsplitW * Fp : 0;
      const int64_t rowsH = p.nsplitH > 1 ? (int64_t) p.nsplitH * Tp : 0;
      const int64_t rowsT = p.tailSplitH > 1 ? (int64_t) p.tailSplitH * round_up(T - p.tailColsH, 32) : 0;
      p.partDoubles = B * std::max(std::max(rowsW, rowsH), rowsT) * Kp;
    }
    // (the tail launch keeps its denominator slots behind the first launch's B x Kp)
    p.dpartDoubles = std::max<int64_t>(32, B * std::max(ns, 1 + p.tailSplitH) * Kp);
    if (Kp > 64) p.csumDoubles = colsum_scratch_doubles((int) std::max(T, F), Kp, (int) B);
    if (p.lazy)
    {
      p.wscratchDoubles = wnorm_scratch_doubles(Kp, (int) B, p.stripsW);
      // column sums of the rows of W' every wavefront of a W update writes (UpdateArgs::colOut; rank 32, the two-launch iteration)
      if (Kp == 32 && !p.strip && p.stripsW > 0) p.colPartDoubles = B * p.stripsW * Kp;
    }
  }
}

extern "C" {

// ---- the planner without a device: debug entry points of the CPU tests and the tools ----
int64_t fluhip_debug_plan_lists(int64_t count, const int64_t* frames, int64_t bins, int64_t K, int which, int32_t* desc,
                                int64_t cap, int32_t* info8)
{
  if (!frames || count < 1 || bins < 1 || K < 1 || K > 128) return -1;
  std::vector<int> tOf((size_t) count);
  int tmax = 1;
  for (int64_t i = 0; i < count; i++)
  {
    if (frames[i] < 1) return -1;
    tOf[(size_t) i] = (int) frames[i];
    tmax = std::max(tmax, tOf[(size_t) i]);
  }
  ListPlanHost plan;
  build_list_plan(tOf, tmax, (int) bins, (int) padded_rank(K), plan);
  const ListSide& sd = which ? plan.H : plan.W;
  if (info8)
  {
    info8[0] = sd.wgs; info8[1] = sd.ng; info8[2] = sd.partial; info8[3] = sd.maxSplit; info8[4] = sd.pieces;
    info8[5] = (int32_t) sd.nPartials; info8[6] = plan.sideW ? 1 : 0; info8[7] = sd.statParts;
  }
  const int64_t n = (int64_t) sd.list.size();
  static_assert(sizeof(WaveDesc) == 12 * sizeof(int32_t), "descriptor layout");
  if (desc) std::memcpy(desc, sd.list.data(), (size_t) std::min(n, cap) * sizeof(WaveDesc));
  return n;
}

int fluhip_debug_plan_kind(int64_t count, int64_t frames, int64_t bins, int64_t K)
{
  if (count < 1 || frames < 1 || bins < 1 || K < 1) return -1;
  const int Kp = (int) padded_rank(K);
  if (update_variant(Kp) != 5) return 0;
  const PlanShape ps{count, frames, bins, Kp};
  return list_plan_pays(&ps) ? 1 : 0;
}

int fluhip_debug_plan_h_update(int64_t count, int64_t frames, int64_t bins, int64_t K)
{
  if (count < 1 || frames < 1 || bins < 1 || K < 1) return -1;
  const int Kp = (int) padded_rank(K);
  if (update_variant(Kp) != 5) return 0;
  const PlanShape ps{count, frames, bins, Kp};
  int wA = 0;
  if (list_plan_pays(&ps) || plan_tail(count, (int) frames, (int) bins, Kp, &wA) > 1) return 0; // (work lists, two-launch H update: the plain forms only)
  if (!nmf_side_column_supported((int) frames, (int) bins, Kp)) return 0;                       // no side column, nothing to take over
  UpdateArgs a;
  a.R = (int) bins; a.C = (int) frames; a.B = (int) count; a.Kp = Kp;
  a.nsplit = 1;
  return plain_h_update_takes(a, true, 0);
}

int fluhip_debug_plan_tail(int64_t count, int64_t frames, int64_t bins, int64_t K, int64_t* out4)
{
  if (count < 1 || frames < 1 || bins < 1 || K < 1 || !out4) return FLUHIP_ERROR;
  const int Kp = (int) padded_rank(K);
  out4[0] = out4[1] = out4[2] = out4[3] = 0;
  if (update_variant(Kp) != 5) return FLUHIP_OK;
  int wA = 0;
  const int sp = plan_tail(count, (int) frames, (int) bins, Kp, &wA);
  if (sp > 1)
  {
    const int G = ((int) frames + 15) / 16, w = nmf_update5_strips((int) frames, Kp, (int) count);
    out4[0] = sp; out4[1] = wA; out4[2] = w - wA; out4[3] = (int64_t) wA * ((G + w - 1) / w) * 16;
  }
  return FLUHIP_OK;
}

// The whole plan of a shape without a device (decide_update_plan), for tests/test_plan_table.py and tools: out32 =
//  0 variant   1 nsplitW   2 nsplitH   3 lazy   4 sideW   5 stripsW   6 Kp   7 Kc   8 strip (0 no, 1 fused, 2 bin strips, 3 bin tiles)
//  9 work lists   10 tailSplitH   11 tailStripsH   12 tailRestH   13 tailColsH   14 stripsH
//  15 .. 21 workspaces in doubles: part, dpart, csum, wscratch, colPart, stripPart, wide
//  22 what the plain H update takes over (bit 0 side partials, bit 1 norm combine, bit 2 column sums from the W update; 0 when
//     the schedule has no such launch)   23 form of the norm-combine launch between the updates in the steady state (WnormForm;
//     -1: none, the H update does it)   24 slices of the side-column launch (0: no side column)
//  25 kSideFromHSlots   26 the first word of wscratch behind the statistics records (B stripsW 2 Kp)
int fluhip_debug_plan_shape(int64_t count, int64_t frames, int64_t bins, int64_t K, int64_t* out32)
{
  if (count < 1 || frames < 1 || bins < 1 || K < 1 || !out32) return FLUHIP_ERROR;
  UpdatePlan p;
  decide_update_plan(count, frames, bins, K, p);
  std::memset(out32, 0, 32 * sizeof(int64_t));
  out32[0] = p.variant; out32[1] = p.nsplitW; out32[2] = p.nsplitH; out32[3] = p.lazy; out32[4] = p.sideW; out32[5] = p.stripsW;
  out32[6] = p.Kp; out32[7] = p.Kc; out32[8] = p.strip ? (p.stripTile ? 3 : (p.stripBin ? 2 : 1)) : 0; out32[9] = p.useLists;
  out32[10] = p.tailSplitH; out32[11] = p.tailStripsH; out32[12] = p.tailRestH; out32[13] = p.tailColsH; out32[14] = p.stripsH;
  out32[15] = p.partDoubles; out32[16] = p.dpartDoubles; out32[17] = p.csumDoubles; out32[18] = p.wscratchDoubles;
  out32[19] = p.colPartDoubles; out32[20] = p.stripPartDoubles; out32[21] = p.wideDoubles;
  out32[23] = -1;
  out32[25] = kSideFromHSlots;
  out32[26] = count * p.stripsW * 2 * p.Kp;
  if (p.variant == 5 && p.lazy && !p.strip)
  {
    const int Kp = (int) p.Kp;
    int takes = 0;
    if (!p.useLists && p.sideW && p.nsplitH == 1 && p.tailSplitH <= 1)
    {
      UpdateArgs a;
      a.R = (int) bins; a.C = (int) frames; a.B = (int) count; a.Kp = Kp; a.Kc = p.Kc;
      a.nsplit = 1;
      const bool normInH = p.stripsW <= 16 && p.stripsH <= 16; // (as the iteration loop asks: the combine's records fit the prologue)
      takes = plain_h_update_takes(a, normInH, normInH && p.colPartDoubles ? p.stripsW : 0);
    }
    out32[22] = takes;
    const int nsl = p.sideW ? wnorm_side_slices((int) frames, Kp) : 0;
    out32[24] = (takes & 1) ? 0 : nsl;
    if (!(takes & 2))
      out32[23] = (int) wnorm_combine_form(Kp, (int) count, p.stripsW, (takes & 1) ? p.stripsH : nsl, (int) frames, (takes & 1) ? 2 : 0, false);
  }
  return FLUHIP_OK;
}

int fluhip_debug_wnorm_form(int Kp, int count, int parts, int slices, int side_rows, int side_phase, int want_colsum)
{
  return (int) wnorm_combine_form(Kp, count, parts, slices, side_rows, side_phase, want_colsum != 0);
}
} // extern "C"
