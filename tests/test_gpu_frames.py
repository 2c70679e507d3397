"""GPU tests of NMF::processFrame over every frame of a matrix (fluhip_nmf_process_frames_f64) and of its two users behind
the STFT, fluhip_nmfmatch_f32 and fluhip_nmffilter_f32, frame by frame against tests/frames_ref.py.

Frames are independent solves and a real buffer spans many decades of level, so the only error measure is
frames_ref.rowrel -- per frame, relative to that frame's own largest value, no frame exempted -- and every frame of every
shape is compared.  The bars are derived on the CPU (tests/test_frames_ref.py): FRAMES_BAR is 8 x what the device's
documented quotient (relative error <= 2^-46) may cost on the reference; MATCH_BAR / FILTER_BAR are 64 x the floor between
two independent double STFTs, the factor the onset, novelty, HPSS and pitch files put over such a floor.  The shapes reach
every regime of the planner's answer for one buffer of T frames (test_frames_ref.py asserts which).

Measured on an MI355X when the file was written (rowrel of H / of V; every test prints its own):
  10 iterations, bar 1.1e-12: 300x513x5 3.7e-15 / 2.3e-15, 2000x513x16 3.1e-15 / 1.2e-15, 1040x3x2 1.2e-15 / 8.9e-16,
    12288x33x3 8.9e-16 / 9.1e-16, 12289x33x3 8.0e-16 / 8.4e-16, 1x513x32 1.3e-15 / 7.4e-16, 31x513x32 5.7e-15 / 1.8e-15,
    33x513x32 8.0e-15 / 2.8e-15, 4200x33x32 2.7e-15 / 9.9e-16, 2100x33x128 5.0e-15 / 1.3e-15, 2100x33x100 3.4e-15 / 1.1e-15,
    300x1025x32 5.6e-15 / 1.6e-15, 1100x2049x72 4.0e-15 / 1.4e-15, 6000x513x40 4.2e-15 / 1.4e-15, 9000x513x128 7.2e-15 / 1.5e-15,
    4200x1025x20 4.3e-15 / 1.5e-15, 8200x513x32 5.1e-15 / 1.8e-15, 9000x513x64 4.5e-15 / 1.3e-15, 2100x2049x33 3.9e-15 / 1.5e-15,
    300x129x130 7.2e-15 / 1.6e-15, 2100x33x200 4.5e-15 / 1.3e-15, 65535x3x130 3.1e-15 / 1.1e-15
  0 iterations (bar 1.3e-13): H bit for bit, V 1.7e-16 .. 2.7e-16;  1 (1.3e-13): 9.1e-16 .. 2.1e-15 / 7.0e-16 .. 1.2e-15;
  25 (2.5e-12): 4.2e-15 .. 1.0e-14 / 1.2e-15 .. 5.8e-15;  50 (5.2e-12): 8.8e-15 .. 2.0e-14 / 3.0e-15 .. 1.1e-14
  -- the device sits where the float64 reference sits against its own long double form (1e-15 .. 2e-14).
  NMFMatch: every float of every case is the rounding of the double reference (worst error 0.998 of the allowance).
  NMFFilter: 7.4e-09 .. 4.2e-08 of peak per component (bar 5.96e-08: the float32 output), the chunked case 1.5e-08."""
import numpy as np
import pytest

import frames_ref as R
from test_frames_ref import (CHUNKED_FILTER_CASE, FILTER_BAR, FILTER_CASES, FILTER_FLOOR, FRAMES_BAR, LIST_MATCH_CASE, MATCH_BAR,
                             MATCH_CASES, filter_inputs, match_inputs, peak_of)

pytestmark = pytest.mark.gpu


def check_frames(ctx, shape, iters, X=None, want_v=True, label=""):
    """H (and V) of the device over ALL rows against the shared reference"""
    Xc, W0 = R.frames_input(*shape)
    H, V = ctx.nmf_process_frames(Xc if X is None else X, W0, iters, R.SEED, want_v=want_v)
    rH, rV = R.reference(*shape, iters)
    assert H.shape == rH.shape and np.isfinite(H).all() and (H >= 0).all()
    eh = R.rowrel(H, rH)
    ev = R.rowrel(V, rV) if want_v else 0.0
    print(f"frames {R.shape_id(shape)} x {iters}{label}: rowrel H {eh:.3e} V {ev:.3e} (bar {FRAMES_BAR[iters]:.1e})")
    if iters == 0:
        assert np.array_equal(H, rH)               # max(h0, eps): nothing is computed
    assert eh <= FRAMES_BAR[iters]
    if want_v:
        assert V.shape == rV.shape and np.isfinite(V).all() and ev <= FRAMES_BAR[iters]
    else:
        assert V is None
    return H, V


# ---- fluhip_nmf_process_frames_f64: all frames, every regime ------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.ALL_SHAPES, ids=R.shape_id)
def test_every_frame_against_the_reference(ctx, shape):
    check_frames(ctx, shape, 10)


@pytest.mark.parametrize("iters", R.ITER_COUNTS)
@pytest.mark.parametrize("shape", R.ITER_SHAPES, ids=R.shape_id)
def test_iteration_counts(ctx, shape, iters):
    check_frames(ctx, shape, iters)


@pytest.mark.parametrize("shape", R.STRIDED_SHAPES, ids=R.shape_id)
def test_strided_input(ctx, shape):
    """ldx > F: the padding behind every row holds 7.0 and must not reach a frame (nor count as one)"""
    T, F, K = shape
    Xc, _ = R.frames_input(*shape)
    buf = np.full((T, F + 5), 7.0)
    buf[:, :F] = Xc
    X = buf[:, :F]
    assert X.strides == (8 * (F + 5), 8)
    check_frames(ctx, shape, 10, X=X, label=" strided")
    assert (buf[:, F:] == 7.0).all() and np.array_equal(buf[:, :F], Xc)


@pytest.mark.parametrize("shape", R.STRIDED_SHAPES, ids=R.shape_id)
def test_without_the_estimate(ctx, shape):
    check_frames(ctx, shape, 10, want_v=False, label=" V=None")


def test_unseeded_activations_differ_from_frame_to_frame(ctx):
    """seed -1, no iteration: the rows are draws of their own (a seeded call repeats ONE row), clamped into [eps, 1)"""
    X, W0 = R.frames_input(300, 513, 5)
    H, V = ctx.nmf_process_frames(X, W0, 0, -1)
    assert H.shape == (300, 5) and (H >= R.EPS).all() and (H < 1.0).all()
    assert len({row.tobytes() for row in H}) == 300 and len(np.unique(H)) > 1400
    Wn = R.normalised_dictionary(W0)
    assert R.rowrel(V, H @ Wn) <= FRAMES_BAR[0]


def test_refusal_one_frame_past_the_any_rank_limit(ctx):
    """ranks above 128 index frames and bins with 16 bits (check_rank): 65535 frames are the last accepted size
    (test_every_frame_against_the_reference runs it), 65536 are refused by name, the outputs stay as they were, and the
    context goes on working"""
    import fluhip
    T, F, K = R.REFUSED_SHAPE
    assert (T - 1, F, K) in R.ALL_SHAPES
    rng = np.random.default_rng(1)
    X, W0 = rng.random((T, F)), rng.random((K, F))
    H, V = np.full((T, K), -7.0), np.full((T, F), -7.0)
    dp = fluhip._dp
    rc = ctx.lib.fluhip_nmf_process_frames_f64(ctx.h, X.ctypes.data_as(dp), T, F, F, W0.ctypes.data_as(dp), K, 10, R.SEED,
                                               H.ctypes.data_as(dp), V.ctypes.data_as(dp))
    msg = ctx.lib.fluhip_last_error(ctx.h).decode()
    assert rc == fluhip.ERROR and "65535" in msg and "128" in msg, (rc, msg)
    assert (H == -7.0).all() and (V == -7.0).all()
    with pytest.raises(fluhip.FluhipError, match="65535"):
        ctx.nmf_process_frames(X, W0, 10, R.SEED)
    check_frames(ctx, (1040, 3, 2), 10, label=" after the refusal")


# ---- NMFMatch ----------------------------------------------------------------------------------------------------------------
def check_match(got, want, k0, label):
    """per column: |got - want| <= MATCH_BAR max|want column|, plus the rounding of that double to the float the client
    writes (half a float ulp; 2^-149 where floats are subnormal), element by element"""
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all()
    assert not got[:, :k0].any()
    bar = MATCH_BAR * np.abs(want).max(axis=0, keepdims=True)
    allow = bar + np.maximum((np.abs(want) + bar) * 2.0 ** -24, 2.0 ** -149)
    err = np.abs(got.astype(np.float64) - want)
    same = int((got == want.astype(np.float32)).sum())
    print(f"nmfmatch {label}: worst err / allowance {(err / allow)[:, k0:].max():.3f}, {same} of {got.size} floats identical "
          f"to the rounded reference (MATCH_BAR {MATCH_BAR:.2e})")
    assert (err[:, k0:] <= allow[:, k0:]).all(), (label, np.unravel_index(np.argmax(err / allow), err.shape))


@pytest.mark.parametrize("case", MATCH_CASES, ids=[R.shape_id(c) for c in MATCH_CASES])
def test_nmfmatch_per_column(ctx, case):
    """every frame of every channel as ONE batch of the H update: the plan follows the TOTAL frame count, so a channel of a
    multi-channel call and the same channel alone may run different schedules -- both are held to the same reference"""
    n, win, fft, hop, K, mode, channels, kind = case
    audio, bases = match_inputs(case)
    T, _, k0 = R.match_geometry(n, win, hop, mode)
    if case == LIST_MATCH_CASE:
        assert R.plan_shape(ctx.lib, channels * T, fft // 2 + 1, K)["lists"] == 1
    got = ctx.nmfmatch(audio, bases, win, fft, hop, seed=R.SEED, padding_mode=mode)
    assert got.shape == (channels, K, T)
    for c in range(channels):
        want = R.nmfmatch_double(audio[c], bases, win, fft, hop, R.SEED, mode)
        assert np.abs(want).max() > 0
        check_match(got[c], want, k0, f"{case} channel {c} of {channels}")
        if channels > 1:
            alone = ctx.nmfmatch(audio[c], bases, win, fft, hop, seed=R.SEED, padding_mode=mode)
            check_match(alone[0], want, k0, f"{case} channel {c} alone")


# ---- NMFFilter ---------------------------------------------------------------------------------------------------------------
def check_filter(ctx, case):
    n, win, fft, hop, K, iters, channels, kind = case
    audio, bases = filter_inputs(case)
    got = ctx.nmffilter(audio, bases, win, fft, hop, iters=iters, seed=R.SEED)
    assert got.shape == (channels, K, n) and got.dtype == np.float32 and np.isfinite(got).all()
    for c in range(channels):
        want = R.nmffilter_double(audio[c], bases, win, fft, hop, iters, R.SEED)
        peak = peak_of(audio[c], want)
        errs = np.abs(got[c].astype(np.float64) - want).max(axis=1) / peak
        print(f"nmffilter {case} channel {c}: |got - want| / peak per component max {errs.max():.3e} (bar {FILTER_BAR:.3e})")
        assert np.abs(want).max(axis=1).min() > 0          # every component carries signal
        assert (errs <= FILTER_BAR).all(), (c, errs)
        if kind == "step":
            # the quiet half on its own peak: the samples only frames wholly behind the step reach
            q = slice(n // 2 + win, n)
            pq = peak_of(audio[c][q], want[:, q])
            eq = np.abs(got[c][:, q].astype(np.float64) - want[:, q]).max(axis=1) / pq
            print(f"  behind the step: per component max {eq.max():.3e} of the quiet half's peak {pq:.2e}")
            assert pq < 2e-3 * peak and (eq <= FILTER_BAR).all(), eq
        if hop < win and win % hop == 0:
            # the masks of a frame add up to one: the components add up to the input, each within the bar of its own reference
            es = np.abs(got[c].astype(np.float64).sum(axis=0) - audio[c]).max() / peak
            # (the reference's own sum is within FILTER_FLOOR of the input: test_frames_ref.py)
            print(f"  the components add up to the input within {es:.3e} of peak (bar {K * FILTER_BAR + FILTER_FLOOR:.3e})")
            assert es <= K * FILTER_BAR + FILTER_FLOOR and es * peak < 1e-4


@pytest.mark.parametrize("case", FILTER_CASES, ids=[R.shape_id(c) for c in FILTER_CASES])
def test_nmffilter_per_component(ctx, case):
    check_filter(ctx, case)


def test_nmffilter_resynthesis_in_two_launches(ctx):
    """the components of a long buffer leave in chunks (api_frames.hip compsPerLaunch): 3188 frames of 4096 samples are
    104.5 MB per component, ten components fit 2^30 bytes, rank 12 goes as ten and two -- the second launch starts at
    component 10 and writes behind the first ten outputs (test_frames_ref.py asserts this arithmetic)"""
    check_filter(ctx, CHUNKED_FILTER_CASE)


def test_nmffilter_refuses_a_hop_above_the_window(ctx):
    audio, bases = filter_inputs(FILTER_CASES[3])
    with pytest.raises(Exception, match="hop"):
        ctx.nmffilter(audio, bases, 256, 256, 300)
