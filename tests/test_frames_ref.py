"""CPU tests of tests/frames_ref.py, and the derivation of every bar tests/test_gpu_frames.py holds the device to:

  FRAMES_BAR   what the device's documented quotient (a Newton-refined reciprocal, relative error <= 2^-46:
               kernels_nmf5.hip, recip_tree.h) may cost in H and V, measured on the reference, times 8;
  MATCH_FLOOR / FILTER_FLOOR   how far two independent double STFTs (numpy's FFT, the C oracle's) put the NMFMatch /
               NMFFilter chains apart on the GPU tests' own inputs; the GPU bars are 64 times these.

The reference itself is held against oracle_np.nmf_process_frame and the C oracle row by row and against its own long double
form, and the shape list against the planner: every regime of the H update is named and reached.
"""
import numpy as np
import pytest

import frames_ref as R
import oracle_np

# 8 x the largest rowrel (over H and V, over every shape the GPU file runs at that iteration count) between the reference and
# the reference with every quotient v0 / v1 times (1 + 2^-46) -- one-sided, the worst case -- or times (1 + 2^-46 u), u
# uniform in [-1, 1]; the factor 8 covers summation order and FMA contraction, which the perturbation does not model.
# Measured by test_the_quotient_cost_stays_under_the_bar (one-sided; the random form stays between 2e-15 and 4.3e-14):
#   10 iterations  1.343e-13 at (65535, 3, 130)   (6.4e-14 .. 1.22e-13 at the other shapes, 1.43e-14 at the single frame)
#    1 iteration   1.597e-14 at (300, 513, 5)
#   25 iterations  3.092e-13 at (4200, 33, 32)
#   50 iterations  6.404e-13 at (4200, 33, 32)
# rounded up to two digits.  With no iteration no quotient is taken: H is held bit for bit, and V = H W, whose summation
# order and normalised dictionary are the device's own, to the bar of one iteration.
FRAMES_BAR = {0: 1.3e-13, 1: 1.3e-13, 10: 1.1e-12, 25: 2.5e-12, 50: 5.2e-12}

# (n, win, fft, hop, K, padding mode, channels, audio) of the NMFMatch tests; audio "synth" is oracle_np.synth_audio(n, 8100 + c),
# "step" frames_ref.level_step_audio: a 60 dB drop halfway through
MATCH_CASES = ([(30000, 1024, 1024, 512, 5, 1, 2, "synth"), (12345, 1000, 1024, 300, 3, 0, 2, "synth"),
                (9000, 512, 1024, 128, 20, 2, 2, "synth"), (5000, 256, 256, 384, 2, 1, 2, "synth"),
                (20000, 2048, 2048, 512, 33, 1, 2, "synth")] +                     # the five of test_nmfmatch_vs_oracle
               # more components than distinct content, on both sides of every padded rank and in the any-rank kernels
               [(9000, 512, 1024, 128, K, 1, 2, "synth") for K in (16, 17, 64, 65, 128, 130)] +
               [(30000, 1024, 1024, 512, 5, 1, 1, "synth"),                         # mono
                (12345, 1000, 1024, 300, 3, 0, 3, "synth"),                         # channel boundaries inside a 32-row block
                (270000, 2048, 2048, 128, 20, 1, 2, "synth"),                       # 2 x 2126 frames x 1025 bins: work lists
                (70000, 16384, 16384, 4096, 4, 1, 1, "synth"),                      # a transform above the LDS limit
                (700, 1024, 1024, 256, 3, 1, 2, "synth"),                           # n smaller than the window
                (30000, 1024, 1024, 512, 5, 1, 2, "step")])
LIST_MATCH_CASE = MATCH_CASES[13]

# (n, win, fft, hop, K, iterations, channels, audio) of the NMFFilter tests (synth_audio(n, 8200 + c))
FILTER_CASES = [(30000, 1024, 1024, 512, 4, 10, 2, "synth"), (12345, 1000, 1024, 300, 3, 5, 2, "synth"),
                (9000, 512, 1024, 128, 9, 12, 2, "synth"), (6000, 256, 256, 256, 2, 3, 2, "synth"),
                (20000, 2048, 2048, 512, 20, 10, 2, "synth"),                       # the five of test_nmffilter_vs_oracle
                (9000, 512, 1024, 128, 9, 0, 2, "synth"),                           # no iteration: the seed's activations
                (30000, 1024, 1024, 512, 4, 10, 2, "step")]
# The chunked resynthesis (api_frames.hip compsPerLaunch): T = (200000 + 4096 + 63) / 64 - 1 = 3188 frames; the inverse frames
# of ONE component are 3188 x 4096 doubles = 104.5 MB, so 2^30 / 104.5 MB = 10 components fit a launch and rank 12 takes two
# launches: components 0-9, then 10 and 11 (ra.k = 10, ra.nComp = 2, the output offset by ten components).
CHUNKED_FILTER_CASE = (200000, 4096, 4096, 64, 12, 10, 1, "synth")

# The largest per-column rowrel between frames_ref.nmfmatch_double on numpy's FFT and on the C oracle's STFT over MATCH_CASES
# (test_the_floor_between_two_double_transforms_nmfmatch: 2.483e-15 at rank 17 of the rank sweep, 3.0e-16 .. 2.2e-15 elsewhere),
# rounded up to one digit
MATCH_FLOOR = 3e-15
MATCH_BAR = 64 * MATCH_FLOOR
# The same for frames_ref.nmffilter_double: max|a - b| / peak over FILTER_CASES and CHUNKED_FILTER_CASE -- of the components, of
# the quiet half on its own peak where the level steps, and of the components' sum against the input
# (test_the_floor_between_two_double_transforms_nmffilter: 2.027e-15 at window = hop = 256, 2.8e-16 .. 8.9e-16 elsewhere),
# rounded up to one digit
FILTER_FLOOR = 3e-15
FILTER_BAR = 64 * FILTER_FLOOR + 2.0 ** -24


def case_audio(case, base):
    n, channels, kind = case[0], case[6], case[7]
    make = R.level_step_audio if kind == "step" else oracle_np.synth_audio
    return np.stack([make(n, base + c) for c in range(channels)]).astype(np.float32)


def match_inputs(case):
    n, win, fft, hop, K = case[:5]
    bases = (np.abs(np.random.RandomState(K).standard_normal((K, fft // 2 + 1))) + 0.01).astype(np.float32)
    return case_audio(case, 8100), bases


def filter_inputs(case):
    n, win, fft, hop, K = case[:5]
    bases = (np.abs(np.random.RandomState(K + n).standard_normal((K, fft // 2 + 1))) + 0.01).astype(np.float32)
    return case_audio(case, 8200), bases


def peak_of(x, want):
    return max(float(np.abs(x).max()), float(np.abs(want).max()))


SMALL = [s for s in R.ALL_SHAPES if s[0] <= 600]


# ---- the bar -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", sorted(FRAMES_BAR))
def test_the_quotient_cost_stays_under_the_bar(iters):
    shapes = R.ALL_SHAPES if iters == 10 else R.ITER_SHAPES
    worst = 0.0
    for s in shapes:
        one, rnd = R.quotient_cost(*s, iters)
        print(f"{R.shape_id(s)} x {iters}: one-sided {one:.3e}, random {rnd:.3e}")
        assert one > 0 or iters == 0
        worst = max(worst, one, rnd)
    print(f"{iters} iterations: worst {worst:.3e}, x 8 = {8 * worst:.3e} (FRAMES_BAR {FRAMES_BAR[iters]:.1e})")
    assert 8 * worst <= FRAMES_BAR[iters] <= 1e-9


def test_every_iteration_count_of_the_gpu_file_has_a_bar():
    assert set(FRAMES_BAR) == set(R.ITER_COUNTS) | {10} and FRAMES_BAR[0] == FRAMES_BAR[1]


# ---- (a) the reference is inside its own bar ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL, ids=R.shape_id)
def test_float64_against_long_double(shape):
    assert np.finfo(np.longdouble).eps < 2e-19
    X, W0 = R.frames_input(*shape)
    for iters in ((10,) if shape not in R.ITER_SHAPES else (10,) + R.ITER_COUNTS):
        H, V = R.reference(*shape, iters)
        Hl, Vl = R.process_frames(X, W0, iters, R.SEED, dtype=np.longdouble)
        eh, ev = R.rowrel(H, Hl), R.rowrel(V, Vl)
        print(f"{R.shape_id(shape)} x {iters}: float64 vs long double H {float(eh):.3e} V {float(ev):.3e}")
        assert max(eh, ev) <= FRAMES_BAR[iters]
        if iters == 0:
            assert np.array_equal(H, Hl.astype(np.float64))


def test_the_input_spans_twelve_decades_and_reaches_both_clamps():
    X, W0 = R.frames_input(300, 513, 5)
    level = X.max(axis=1)
    assert not X[150].any() and not X[0, :7].any() and X[0, 7:].all() and not W0[0, :3].any()
    live = level[level > 0]
    assert live.max() / live.min() > 1e10
    H, V = R.reference(300, 513, 5, 10)
    assert np.isfinite(H).all() and (H > 0).all() and H[150].max() < 1e-12     # the silent row stays at the clamp's scale


# ---- (b) the vectorised reference is the per-frame one -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,iters", [((50, 513, 5), 10), ((7, 33, 3), 25), ((33, 129, 40), 10)],
                         ids=["50x513x5", "7x33x3", "33x129x40"])
def test_against_the_per_frame_restatement_and_the_c_oracle(oracle, shape, iters):
    X, W0 = R.frames_input(*shape)
    H, V = R.process_frames(X, W0, iters, R.SEED)
    rows = [oracle_np.nmf_process_frame(x, W0, iters, R.SEED) for x in X]
    Hn, Vn = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    Hc, Vc = oracle.nmf_process_frames(X, W0, iters, R.SEED)
    errs = (R.rowrel(H, Hn), R.rowrel(V, Vn), R.rowrel(H, Hc), R.rowrel(V, Vc))
    print(f"{R.shape_id(shape)} x {iters}: numpy per frame H {errs[0]:.2e} V {errs[1]:.2e}, C oracle H {errs[2]:.2e} V {errs[3]:.2e}")
    assert max(errs) <= FRAMES_BAR[iters]


def test_the_perturb_hook_sees_every_quotient():
    X, W0 = R.frames_input(31, 513, 32)
    seen = []
    H, _ = R.process_frames(X, W0, 3, R.SEED, perturb=lambda q, it: (seen.append((it, q.shape)), q)[1])
    assert seen == [(0, (31, 513)), (1, (31, 513)), (2, (31, 513))]
    assert np.array_equal(H, R.process_frames(X, W0, 3, R.SEED)[0])
    H2, _ = R.process_frames(X, W0, 1, R.SEED, perturb=lambda q, it: q * 2.0)
    assert np.array_equal(H2, 2.0 * R.process_frames(X, W0, 1, R.SEED)[0])     # one update is linear in the quotients


# ---- (c) the shape list reaches every regime of the planner ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(fluhip_lib_path):
    import fluhip
    return fluhip.load_library(fluhip_lib_path)


def test_the_shapes_reach_every_planner_regime(lib):
    plan = {s: R.plan_shape(lib, *s) for s in R.ALL_SHAPES}
    for s, p in plan.items():
        print(R.shape_id(s), p)
    for s in R.SHAPES["strip"] + R.SHAPES["strip_edge"][:1]:
        assert plan[s]["strip"] == 1 and plan[s]["variant"] == 5, s
    edge = plan[R.SHAPES["strip_edge"][1]]
    assert (edge["strip"], edge["lists"], edge["nsplitH"]) == (0, 0, 1) and edge["stripsH"] == 257
    for s in R.SHAPES["tiny"] + R.SHAPES["uniform_split"]:
        assert (plan[s]["strip"], plan[s]["lists"]) == (0, 0) and plan[s]["nsplitH"] > 1, s
    assert [plan[s]["nsplitH"] for s in R.SHAPES["uniform_split"]] == [21, 29, 8, 3]
    assert plan[(9000, 513, 128)]["stripsH"] == 282
    for s in R.SHAPES["split1_many_strips"]:
        assert (plan[s]["strip"], plan[s]["lists"], plan[s]["nsplitH"]) == (0, 0, 1) and plan[s]["stripsH"] > 64, s
    assert [plan[s]["stripsH"] for s in R.SHAPES["split1_many_strips"]] == [88, 66, 66]
    for s in R.SHAPES["lists"]:
        assert plan[s]["lists"] == 1 and plan[s]["variant"] == 5, s
    for s in R.SHAPES["any_rank"]:
        assert plan[s]["variant"] == 0, s
    # every compute rank class: the padded ranks themselves and the off-size ones between them
    assert {p["Kc"] for p in plan.values() if p["variant"] == 5} == {16, 24, 32, 40, 64, 72, 104, 128}
    assert plan[(4200, 1025, 20)]["Kc"] == 24 and plan[(2100, 2049, 33)]["Kc"] == 40 and plan[(6000, 513, 40)]["Kc"] == 40
    assert plan[(1100, 2049, 72)]["Kc"] == 72 and plan[(2100, 33, 100)]["Kc"] == 104
    # the shapes of the iteration and stride sweeps are one strip, one many-strip and one work-list shape
    assert all(s in R.ALL_SHAPES for s in R.ITER_SHAPES + R.STRIDED_SHAPES)
    # NMFMatch's work-list case and NMFFilter's chunked case, by their total frame counts
    n, win, fft, hop, K, mode, channels, _ = LIST_MATCH_CASE
    T = R.match_geometry(n, win, hop, mode)[0]
    assert T % 32 and R.plan_shape(lib, channels * T, fft // 2 + 1, K)["lists"] == 1
    assert R.plan_shape(lib, T, fft // 2 + 1, K)["lists"] == 0        # ... which one channel alone does not reach
    n, win, fft, hop, K = CHUNKED_FILTER_CASE[:5]
    T = R.filter_geometry(n, win, hop)[0]
    assert T == 3188 and (1 << 30) // (T * win * 8) == 10 < K
    three = MATCH_CASES[12]
    assert three[6] == 3 and R.match_geometry(three[0], three[1], three[3], three[5])[0] % 32


# ---- the closed forms in double are the committed restatements before their float32 rounding ------------------------------
def test_the_double_closed_forms_round_to_the_restatements():
    for case in (MATCH_CASES[1], MATCH_CASES[3], MATCH_CASES[15]):
        n, win, fft, hop, K, mode = case[:6]
        audio, bases = match_inputs(case)
        want = oracle_np.nmfmatch_channel(audio[0], bases, win, fft, hop, R.SEED, mode)
        got = R.nmfmatch_double(audio[0], bases, win, fft, hop, R.SEED, mode)
        assert got.shape == want.shape and np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()
    for case in (FILTER_CASES[1], FILTER_CASES[3]):
        n, win, fft, hop, K, iters = case[:6]
        audio, bases = filter_inputs(case)
        want = oracle_np.nmffilter_channel(audio[0], bases, win, fft, hop, iters, R.SEED)
        got = R.nmffilter_double(audio[0], bases, win, fft, hop, iters, R.SEED)
        assert got.shape == want.shape and np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()


def test_both_transforms_see_the_same_frames(oracle):
    x = oracle_np.synth_audio(3000, 5).astype(np.float64)
    for first, count, win, fft, hop in ((-1024, 7, 1024, 1024, 512), (-300, 9, 1000, 1024, 300), (-128, 20, 256, 256, 384),
                                        (-64, 12, 512, 1024, 128)):
        a = R.spectra_numpy(x, first, count, win, fft, hop)
        b = R.spectra_oracle(oracle, x, first, count, win, fft, hop)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


# ---- the floors of NMFMatch and NMFFilter -----------------------------------------------------------------------------------
def test_the_floor_between_two_double_transforms_nmfmatch(oracle):
    worst = 0.0
    for case in MATCH_CASES:
        n, win, fft, hop, K, mode, channels, kind = case
        audio, bases = match_inputs(case)
        k0 = R.match_geometry(n, win, hop, mode)[2]
        e = 0.0
        for c in range(channels):
            a = R.nmfmatch_double(audio[c], bases, win, fft, hop, R.SEED, mode)
            b = R.nmfmatch_double(audio[c], bases, win, fft, hop, R.SEED, mode,
                                  spectra=lambda *args: R.spectra_oracle(oracle, *args))
            e = max(e, R.rowrel(a.T[k0:], b.T[k0:]))
        worst = max(worst, e)
        print(f"nmfmatch {case}: per-column floor {e:.3e}")
    print(f"nmfmatch floor {worst:.3e} (MATCH_FLOOR {MATCH_FLOOR:.1e}, MATCH_BAR {MATCH_BAR:.2e})")
    assert 0 < worst <= MATCH_FLOOR and MATCH_BAR <= 1e-9


def test_the_floor_between_two_double_transforms_nmffilter(oracle):
    worst = 0.0
    for case in FILTER_CASES + [CHUNKED_FILTER_CASE]:
        n, win, fft, hop, K, iters, channels, kind = case
        audio, bases = filter_inputs(case)
        e = 0.0
        for c in range(channels):
            a = R.nmffilter_double(audio[c], bases, win, fft, hop, iters, R.SEED)
            b = R.nmffilter_double(audio[c], bases, win, fft, hop, iters, R.SEED,
                                   spectra=lambda *args: R.spectra_oracle(oracle, *args))
            peak = peak_of(audio[c], a)
            e = max(e, float(np.abs(a - b).max()) / peak)
            if kind == "step":                       # the quiet half on its own peak, as the GPU test holds it
                q = slice(n // 2 + win, n)
                e = max(e, float(np.abs(a[:, q] - b[:, q]).max()) / peak_of(audio[c][q], a[:, q]))
            if hop < win and win % hop == 0:         # the masks add up to one: the components add up to the input
                e = max(e, float(np.abs(a.sum(axis=0) - audio[c]).max()) / peak)
        worst = max(worst, e)
        print(f"nmffilter {case}: floor {e:.3e} of peak")
    print(f"nmffilter floor {worst:.3e} (FILTER_FLOOR {FILTER_FLOOR:.1e}, FILTER_BAR {FILTER_BAR:.3e})")
    assert 0 < worst <= FILTER_FLOOR
