"""CPU tests of tests/nmf_ref.py, and the derivation of the bars tests/test_gpu_nmf.py holds the device's W and H updates to,
entry by entry:

  NMF_BAR[iters], NMF_BAR_AUDIO[iters]
                   8 x the largest elrel (nmf_ref.elrel: every entry relative to itself), over W and H and over every input
                   of that family the GPU file runs at up to that iteration count, among
                     - the reference with every quotient V / max(W H, eps) times (1 + 2^-46) -- the device's documented
                       quotient, a Newton-refined reciprocal (kernels_nmf5.hip, recip_tree.h), one-sided,
                     - the same with (1 + 2^-46 u), u uniform in [-1, 1],
                     - the float64 reference against its own long double form.
                   The factor 8 is FRAMES_BAR's: summation order and FMA contraction, which a perturbation of the quotients
                   does not model.  One bar per input family: one buffer of doubles (nmf_ref.nmf_input) and corpora of audio,
                   whose sparser factors cost several times more -- a bar set by the audio would let errors through on the
                   doubles.

The bars have teeth by construction, not by measurement: none exceeds 1e-11, and at EVERY input, at every count, the
reference with its quotients times (1 + 2^-40) -- 64 times the documented error -- misses its bar.  A factor common to all
quotients is absorbed by the H update within one iteration, so that costs 1.3 x 2^-40 = 9.1e-13 at any count, while
rounding accumulates: on audio, float64 is 7.2e-13 from long double after 30 iterations (entries that decayed fifteen
decades under their frame's peak) and no bar 8 x above that can refuse 9.1e-13.  So the audio runs up to 10 iterations
(nmf_ref.AUDIO_ITER_COUNTS) and 30 is held on the doubles, where the condition holds.

The restatement is held to oracle_np.nmf_process bit for bit and to the C oracle within the bar, the inputs to what they claim
(levels, the silent frame, the zero bin, the 1e-9 last bin, no subnormal in any reference), and the shape table to the planner:
every regime of the update loop is named and reached.
"""
import functools

import numpy as np
import pytest

import nmf_ref as R
import oracle_np

# How a bar follows from the figures (test_the_bars_cover_the_measured_cost recomputes them and prints every one): 8 x the worst
# elrel of the three measures at that count, made monotone in the count (the larger of it and the bar of the count before:
# the figures of 7, 8 and 9 iterations differ by noise), plus 3 % for another BLAS build's roundings, rounded up to two digits.
HEADROOM = 1.03
# Measured with one BLAS thread, the worst case of each count (one-sided / random quotient error / float64 against long double):
#   doubles   0  0 / 0 / 3.219e-16 at 87x129x3 (no quotient is taken: the normalisation of the seeds alone)
#             1  1.696e-14 / 1.398e-14 / 2.977e-15 at 33x513x32       2  1.533e-14 / 1.489e-14 / 1.219e-15 at 33x33x32
#             7  1.606e-14 / 2.050e-14 / 2.126e-15 at 33x33x32        8  1.651e-14 / 2.777e-14 / 4.008e-15 at 87x129x3
#             9  1.688e-14 / 2.911e-14 / 4.594e-15 at 87x129x3       10  1.857e-14 / 3.940e-14 / 1.038e-14 at 33x513x32 (of 28 inputs)
#            30  3.431e-14 / 8.384e-14 / 2.627e-14 at 87x129x3
#   audio     0  0 / 0 / 9.880e-16        1  1.634e-14 / 1.308e-14 / 3.456e-15        2  1.694e-14 / 1.610e-14 / 4.394e-15
#             7  2.230e-14 / 5.504e-14 / 2.215e-14        8  2.289e-14 / 5.244e-14 / 2.703e-14        9  2.380e-14 / 7.530e-14 / 3.082e-14
#                (all on buffers of 8x173x513x20)        10  2.413e-14 / 8.465e-14 / 2.664e-14 at buffer 0 of 2x87x129x200 (of 36
#                buffers, four spread over each corpus, drawn and seeded factors, the ragged corpus at both ranks)
# Every quotient times (1 + 2^-40) costs 9.10e-13 .. 9.20e-13 on the doubles and 9.12e-13 .. 9.88e-13 on the audio, at every count.
NMF_BAR = {0: 2.7e-15, 1: 1.4e-13, 2: 1.4e-13, 7: 1.7e-13, 8: 2.3e-13, 9: 2.4e-13, 10: 3.3e-13, 30: 7.0e-13}
NMF_BAR_AUDIO = {0: 8.2e-15, 1: 1.4e-13, 2: 1.4e-13, 7: 4.6e-13, 8: 4.6e-13, 9: 6.3e-13, 10: 7.0e-13}
BARS = {"doubles": NMF_BAR, "audio": NMF_BAR_AUDIO}
BAR_CAP = 1e-11


@functools.lru_cache(maxsize=None)
def measured(iters):
    """{(name, family): (one-sided 2^-46, random 2^-46, float64 against long double, one-sided 2^-40)} of every input the GPU
    file runs at this count: computed once, shared by the bar and the 2^-40 tests.  The figures are float64 roundings amplified
    by the iteration and follow the order in which the BLAS behind numpy's matmul adds, which follows its thread count: one
    thread makes them the same on every run."""
    import threadpoolctl
    assert np.finfo(np.longdouble).eps < 2e-19
    with threadpoolctl.threadpool_limits(limits=1):
        return {(name, family): R.measure(X, K, iters, seed, W0, H0) for name, family, X, K, seed, W0, H0 in R.bar_cases(iters)}


def round_up_two_digits(x):
    if x == 0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 1
    return float(f"{np.ceil(x / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e:.1e}")


@pytest.fixture(scope="module")
def lib(fluhip_lib_path):
    import fluhip
    return fluhip.load_library(fluhip_lib_path)


# ---- the bars ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(BARS))
def test_the_bars_cover_the_measured_cost(family):
    bars, envelope = BARS[family], 0.0
    for iters in sorted(bars):
        worst, where = 0.0, None
        for (name, fam), (one, rnd, ld, _) in measured(iters).items():
            if fam != family:
                continue
            print(f"{name} x {iters}: one-sided {one:.3e}, random {rnd:.3e}, float64 vs long double {ld:.3e}")
            assert iters == 0 or (one > 0 and rnd > 0)
            if max(one, rnd, ld) > worst:
                worst, where = max(one, rnd, ld), (name, one, rnd, ld)
        assert where is not None
        envelope = max(envelope, 8 * worst)
        want = round_up_two_digits(envelope * HEADROOM)
        print(f"{family} x {iters}: worst {worst:.3e} at {where}, x 8 = {8 * worst:.3e}, monotone {envelope:.3e}, "
              f"+ 3 % rounded up {want:.1e} (bar {bars[iters]:.1e})")
        assert 8 * worst <= bars[iters] <= 1.1 * want, (family, iters, worst, want)      # covers, and is not looser than the rule


def test_the_bars_have_teeth_the_cap():
    assert set(NMF_BAR) == set(R.ITER_COUNTS) and set(NMF_BAR_AUDIO) == set(R.AUDIO_ITER_COUNTS)
    for bars in BARS.values():
        counts = sorted(bars)
        assert all(0 < bars[i] <= BAR_CAP for i in counts)
        assert all(bars[a] <= bars[b] for a, b in zip(counts, counts[1:]))
    assert min(i for i in NMF_BAR if i >= R.CANCEL_AT) == 7                       # (cancellation at 5 takes the bar of 7)


@pytest.mark.parametrize("iters", sorted(set(NMF_BAR) - {0}))
def test_the_bars_have_teeth_quotients_off_by_2_to_the_minus_40_miss_them(iters):
    """64 times the documented quotient error, every quotient times (1 + 2^-40): at EVERY input of either family the bar of
    that family refuses it"""
    for (name, family), (_, _, _, far) in measured(iters).items():
        print(f"{name} x {iters}: quotients times 1 + 2^-40 cost {far:.3e} (bar {BARS[family][iters]:.1e})")
        assert far > BARS[family][iters], (name, far)


# ---- the restatement against the existing oracles ------------------------------------------------------------------------------
SMALL = [(50, 129, 5), (7, 33, 3), (33, 100, 40)]


@pytest.mark.parametrize("seeded", [False, True], ids=["drawn", "seeded"])
@pytest.mark.parametrize("uw,uh", R.MODES)
@pytest.mark.parametrize("shape", SMALL, ids=R.shape_id)
def test_against_the_numpy_restatement_and_the_c_oracle(oracle, shape, uw, uh, seeded):
    T, F, K = shape
    X = R.nmf_input(T, F, K)
    W0, H0 = (a.astype(np.float64) for a in R.seed_factors(T, F, K)) if seeded else (None, None)
    iters = 10
    got = R.nmf_process(X, K, iters, uw, uh, R.SEED, W0, H0)
    want = oracle_np.nmf_process(X, K, iters, uw, uh, R.SEED, W0, H0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)                                 # the same operations in the same order: the same bits
    cW, cH, cV, _ = oracle.nmf_process(X, K, iters, uw, uh, R.SEED, W0=W0, H0=H0)
    bar = NMF_BAR[iters if (uw or uh) else 0]
    errs = (R.elrel(cW, got[0]), R.elrel(cH, got[1]), R.elrel(cV, got[2]))
    print(f"{R.shape_id(shape)} W {uw} H {uh} seeded {seeded}: C oracle elrel W {errs[0]:.2e} H {errs[1]:.2e} V {errs[2]:.2e}")
    assert max(errs) <= bar


def test_no_iteration_is_the_normalised_seeds():
    X = R.nmf_input(33, 100, 40)
    W, H, V = R.nmf_process(X, 40, 0)
    assert np.abs(np.sqrt((W * W).sum(axis=1)) - 1).max() < 1e-15 and np.abs(np.sqrt((H * H).sum(axis=0)) - 1).max() < 1e-15
    assert R.elrel(V, H @ W) < 1e-15
    for uw, uh in R.MODES:
        for g, w in zip(R.nmf_process(X, 40, 0, uw, uh), (W, H, V)):
            assert np.array_equal(g, w)
    # a factor that is not updated stays the normalised seed
    assert np.array_equal(R.nmf_process(X, 40, 3, False, True)[0], W) and np.array_equal(R.nmf_process(X, 40, 3, True, False)[1], H)


def test_the_perturb_hook_sees_both_quotients_of_an_iteration():
    T, F, K = 31, 100, 5
    X = R.nmf_input(T, F, K)
    for uw, uh, per in ((True, True, ["W", "H"]), (True, False, ["W"]), (False, True, ["H"]), (False, False, [])):
        seen = []
        got = R.nmf_process(X, K, 3, uw, uh, perturb=lambda q, which, it: (seen.append((it, which, q.shape)), q)[1])
        assert seen == [(it, which, (F, T)) for it in range(3) for which in per]
        for g, w in zip(got, R.nmf_process(X, K, 3, uw, uh)):
            assert np.array_equal(g, w)
    # one H update is linear in its quotients
    H2 = R.nmf_process(X, K, 1, False, True, perturb=lambda q, which, it: q * 2.0)[1]
    assert np.array_equal(H2, 2.0 * R.nmf_process(X, K, 1, False, True)[1])


# ---- the inputs are what they claim ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.ONE_BUFFER_SHAPES, ids=R.shape_id)
def test_the_double_input_and_its_reference(shape):
    _, T, F, K = shape
    X = R.nmf_input(T, F, K)
    level = X[:, :F - 1].max(axis=1)
    live = level[level > 0]
    if T > 2:
        assert not X[T // 2].any() and len(live) == T - 1
        assert len(np.unique(np.round(np.log10(live), 1))) > min(T, 80) // 2      # a level of its own per frame
    if T >= 31:
        assert live.max() / live.min() > 1e8                                     # over at least eight decades
    if F > 2:
        assert not X[:, F // 3].any()
        body = np.delete(X, [F // 3, F - 1], axis=1)
        assert (np.delete(body, T // 2, axis=0) > 0).all() if T > 2 else (body > 0).all()
    # the last bin sits nine decades under the others, as a Nyquist bin does: every live frame's last bin is at least five
    # decades under that frame's largest (the bins of a frame are within four decades of each other), and not zero
    rows = [t for t in range(T) if X[t].any()]
    assert all(0 < X[t, F - 1] < 1e-5 * X[t, :F - 1].max() for t in rows)
    assert np.median(X[rows, F - 1] / X[rows][:, :F - 1].max(axis=1)) < 1e-8
    W, H, V = R.reference(T, F, K, 10)
    assert np.isfinite(W).all() and np.isfinite(H).all()
    if T > 2:
        assert not H[T // 2].any() and H[[t for t in range(T) if t != T // 2]].all()       # the silent frame: an exact zero row
    if F > 2:
        assert not W[:, F // 3].any() and np.delete(W, F // 3, axis=1).all()                # the empty bin: an exact zero row
    for a in (W, H):
        assert not ((a > 0) & (a < 1e-280)).any()                                           # elrel never meets a subnormal


@pytest.mark.parametrize("shape", R.CORPUS_SHAPES, ids=R.shape_id)
def test_the_corpus_audio_and_its_reference(shape):
    B, T, F, K = shape
    n, win, fft, hop = R.corpus_geometry(T, F)
    assert (n + hop) // hop == T and fft // 2 + 1 == F
    audio = R.corpus_audio(B, T, F)
    assert audio.dtype == np.float32 and audio.shape == (B, n)
    assert len({a.tobytes() for a in audio}) == B                                           # every buffer other audio
    segs = R.level_segments(n, win)
    assert [g for _, _, g in segs] == [1.0, 1e-2, 0.0, 1e-4, 1e-6]
    assert segs[2][1] - segs[2][0] > win + hop and segs[0][0] == 0 and segs[-1][1] == n
    for b in R.bar_buffers(shape):
        plain = oracle_np.synth_audio(n, 6000 + b).astype(np.float64)
        for a, e, g in segs:
            assert np.array_equal(audio[b, a:e], (plain[a:e] * g).astype(np.float32)) and (g == 0 or audio[b, a:e].any())
        mag = R.corpus_magnitudes_cpu(B, T, F, b)
        silent = [t for t in range(T) if not mag[t].any()]
        assert silent and len(silent) < T // 2
        W, H, V = R.nmf_process(mag, K, 10, seed=R.corpus_seeds(B)[b])
        assert not H[silent].any() and np.delete(H, silent, axis=0).all() and W.all()
        for a in (W, H):
            assert not ((a > 0) & (a < 1e-280)).any()
    assert len(set(R.corpus_seeds(B))) > 1


def test_the_ragged_lengths_straddle_32_frames():
    Ts = [(n + 256) // 256 for n in R.RAGGED_LENS]
    assert Ts == [31, 32, 32, 33, 34]
    assert all(np.abs(a).max() > 0 for a in R.ragged_audio())


def test_elrel_exempts_nothing():
    want = np.array([[1.0, 1e-30, 0.0], [2.0, 3.0, 4.0]])
    assert R.elrel(want, want) == 0.0
    got = want.copy()
    got[0, 1] = 1.5e-30                        # far under the peak: a measure relative to the peak sees 5e-31 / 4
    assert R.elrel(got, want) == pytest.approx(0.5)
    assert np.abs(got - want).max() / want.max() < 1e-30
    got = want.copy()
    got[0, 2] = 1e-300
    with pytest.raises(AssertionError):
        R.elrel(got, want)                     # not zero where the reference is exactly zero
    assert R.rowrels(want, want, want, want) == (0.0, 0.0, 0.0, 0.0)


# ---- the shape table reaches every regime of the planner --------------------------------------------------------------------
def test_the_shapes_reach_every_regime(lib):
    assert set(R.SHAPES) == set(R.REGIMES)
    plan = {}
    for name, shapes in R.SHAPES.items():
        for s in shapes:
            plan[s] = R.plan_shape(lib, *s)
            print(name, R.shape_id(s), plan[s][:15])
            assert R.REGIMES[name](plan[s]), (name, s, plan[s][:15])
    last, first = R.SHAPES["strip_edge"]
    assert last[1] + 1 == first[1] and plan[last][8] == 1 and plan[first][8] == 0
    assert plan[R.SHAPES["uniform_off_size"][0]][6:8] == [128, 104] and plan[R.SHAPES["lists_compute_rank"][0]][6:8] == [32, 24]
    # either side of every padded rank: the compute-rank classes of the MFMA kernels, and the any-rank kernels past 128
    edge = {s[3]: R.plan_shape(lib, *s) for s in R.RANK_EDGE_SHAPES}
    assert {K: (p[6], p[7]) for K, p in edge.items()} == {17: (32, 24), 24: (32, 24), 25: (32, 32), 32: (32, 32), 33: (64, 40),
                                                        40: (64, 40), 41: (64, 48), 64: (64, 64), 65: (128, 72),
                                                        128: (128, 128)}
    assert all(p[0] == 5 and p[8] == 0 for p in edge.values())
    assert plan[(1, 33, 100, 16)][8] == 1 and plan[(1, 87, 129, 130)][0] == 0
    # T in 1, 31, 32, 33; bin counts that are no 2^k + 1
    assert {s[1] for s in R.SHAPES["split_h"]} == {1, 31, 32, 33}
    assert {3, 33, 100} <= {s[2] for s in R.ONE_BUFFER_SHAPES}
    # the sweeps run on shapes of the table: one strip, one uniform and one work-list shape for the iteration counts
    every = R.ONE_BUFFER_SHAPES + R.CORPUS_SHAPES
    assert all(s in every for s in R.ITER_SHAPES + R.MODE_SHAPES + R.STRIDED_SHAPES + [R.MODE_CORPUS_SHAPE, R.CANCEL_SHAPE])
    a, b, c = (plan[s] for s in R.ITER_SHAPES)
    assert a[8] == 1 and R.REGIMES["uniform_side_column"](b) and c[9] == 1
    # the ragged corpus plans from its own frame counts (plan_updates): its ranks are one strip-kernel rank and one MFMA rank
    assert R.RAGGED_RANKS == (5, 32)
