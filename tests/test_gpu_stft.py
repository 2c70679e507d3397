"""GPU tests of the forward STFT, K1, at double precision and FRAME BY FRAME: fluhip_stft_f32 / _f64, fluhip_bufstft_forward_f32
and the corpus transform (fluhip_corpus_stft, fluhip_corpus_stft_mag_only, equal-length and ragged) against the long double
restatement tests/stft_ref.py -- every frame of every buffer relative to that frame's own peak (stft_ref.frame_err), spectrum
and magnitudes alike, in every kernel form: the block kernel (one round and several, one and two sets of staging buffers,
prefetched samples), the generic on-chip kernel (each LDS variant, the stride loop) and the global-memory passes (across a
chunk).  The corpus's bin-major copy is held BIT-IDENTICAL to the transpose of the frame-major one, exactly zero in its
padding (fluhip_debug_corpus_read_layouts_f64), and the magnitudes to hypot of the device's own spectrum within 2 ulp.

The bars are tests/test_stft_ref.py's STFT_BAR[fft]: 8 x the floor two float64 transforms (numpy's rfft, the C oracle) keep
from the restatement on the same inputs, 1.5e-15 at fft 4 to 8.5e-15 at fft 32768.  Where a case is too large for long double
on every frame, the frames of stft_ref's named blocks are held to long double and ALL frames to numpy's float64 rfft with the
bar widened by that rfft's own measured distance from long double on the named frames.

Measured on an MI355X (the worst frame of each class; its bar in brackets):
  one buffer    fft 4 .. 64      1.4e-16 .. 5.1e-16 (1.5e-15 .. 4.5e-15)     fft 128 .. 512   3.2e-16 .. 4.0e-16 (4.1e-15 .. 5.6e-15)
                fft 1024 block   5.1e-16 (6.3e-15)    fft 2048 block   4.7e-16 (5.7e-15)    fft 4096 block   5.4e-16 (7.2e-15)
                fft 8192 generic 5.8e-16 (7.6e-15)    big passes 16384 / 32768 / 65536   5.3e-16 / 5.3e-16 / 5.8e-16 (8.0e-15 / 8.5e-15 / 8.2e-15)
                across the chunk: named frames 5.6e-16 (8.2e-15); all 1032 frames against float64 rfft 8.0e-16 (8.2e-15 + 4.7e-16)
  corpora       one round 1024 / 2048 / 4096   4.7e-16 / 4.2e-16 / 4.9e-16      second-round blocks   4.5e-16 / 4.2e-16 / 4.7e-16
                every frame of the two-round corpora against float64 rfft   8.3e-16 / 7.8e-16 / 7.2e-16 (bar + rfft's own 4 - 5e-16)
                ragged   4.1e-16 / 4.5e-16 / 4.4e-16      no block form: fft 512 4.1e-16, 1023 / 1024 4.4e-16, 8192 4.5e-16, 16384 6.1e-16
  magnitudes from hypot of the own spectrum   2.1e-16 at worst (4.4e-16)      BufSTFT, float32   4.3e-8 .. 5.7e-8 (6.0e-8)
  every bin-major copy bit-identical to the transpose and zero in its padding.  No form of K1 missed its bar.
  frames outside their buffer (fluhip_debug_stft_frames_*, every form, float and double input, guards of 1e30 around each buffer):
                fft 64  5.7e-16 (4.5e-15)    block 1024 / 2048 / 4096   8.0e-16 / 7.1e-16 / 9.3e-16 (6.3e-15 / 5.7e-15 / 7.2e-15)
                fft 8192   1.1e-15 (7.6e-15)    big passes 16384   1.3e-15 (8.0e-15)    every frame with no sample of its buffer
                exactly zero, the kernels' own magnitudes of such a frame 0 or 2^-511; no guard value in any result.

Which deliberate breaks only this measure sees is shown on the CPU (test_stft_ref.py): one pass's twiddles at float32 in the
quiet frames reads 7e-14 on the old measure (max |a - b| / max |b| < 1e-12 over the spectrogram) and 2.5e-8 here; stale
padding columns of the bin-major copy were returned by no read-out.
"""
import numpy as np
import pytest

import stft_ref as R
from test_stft_ref import FLOAT32_ULP, STFT_BAR

pytestmark = pytest.mark.gpu
K = 5


def hold(what, got, ref, bar):
    """frame_err of spectrum and / or magnitudes against the reference, printed, then asserted"""
    worst = 0.0
    for name, g, r in (("spec", got[0], ref[0]), ("mag", got[1], ref[1])):
        if g is None:
            continue
        e, t = R.frame_err(g, r)
        print(f"{what} {name}: worst frame {t} of {len(r)} at {e:.2e} (bar {bar:.1e}); old measure {R.rel_err(g, r):.2e}")
        worst = max(worst, e)
        assert e <= bar, (what, name, t, e)
    return worst


def one_buffer(ctx, family, n, seed, dtype, win, fft, hop, kind=0, want_spec=True, stride=1):
    x = R.INPUTS[family](n * stride if stride > 1 else n, seed, dtype)
    spec, mag = ctx.stft(x, win, fft, hop, window_type=kind, want_spec=want_spec, stride=stride)
    T = R.num_frames(n, hop)
    assert mag.shape == (T, fft // 2 + 1) and (spec is None) == (not want_spec)
    ref = R.reference(family, n, seed, dtype, win, fft, hop, kind, stride)
    what = f"{family} {dtype} n {n} win {win} fft {fft} hop {hop} window {kind} stride {stride} spec {want_spec}"
    e = hold(what, (spec, mag), ref, STFT_BAR[fft])
    if spec is not None:
        assert not spec[:, 0].imag.any() and not spec[:, -1].imag.any()          # DC and Nyquist purely real
        m = R.mag_of_spec_err(mag, spec)
        print(f"{what}: magnitudes from hypot of the own spectrum {m:.2e} (bar {R.MAG_OF_SPEC_BAR:.2e})")
        assert m <= R.MAG_OF_SPEC_BAR
    return e


# ---- one buffer, block form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft", R.BLOCK_FFTS)
@pytest.mark.parametrize("which", range(4), ids=["block_minus_one", "one_block", "block_plus_one", "two_and_a_half_blocks"])
def test_block_form_one_buffer(ctx, fft, which):
    T, hop = R.block_T(fft)[which], fft // 4
    n = R.n_for(T, hop)
    # (without the spectrum the entry point still keeps it on the device -- its magnitudes are hypot of it, api_algorithms.hip
    #  stft_common -- so the kernel's SPEC = false forms are the corpus tests' below)
    for dtype in ("float32", "float64"):
        for want_spec in (True, False):
            one_buffer(ctx, "dynamics", n, 20 + which, dtype, fft, fft, hop, want_spec=want_spec)
        one_buffer(ctx, "dynamics", n, 41, dtype, fft, fft, hop, stride=2)
        one_buffer(ctx, "dynamics", n, 42, dtype, R.SHORT_EVEN_WINDOWS[fft], fft, hop)
        one_buffer(ctx, "dynamics", R.n_for(T, hop - 1), 43, dtype, fft, fft, hop - 1)       # odd sample bases: the clamped gather inside
    one_buffer(ctx, "tones", n, 30 + which, "float32", fft, fft, hop)


@pytest.mark.parametrize("fft", R.BLOCK_FFTS)
def test_block_form_short_buffers_and_window_types(ctx, fft):
    hop = fft // 4
    for dtype in ("float32", "float64"):
        for short in (1, fft // 2 - 1, fft // 2, fft // 2 + 1):
            one_buffer(ctx, "dynamics", short, 44, dtype, fft, fft, hop)
    for kind in (0, 1, 2, 3):
        one_buffer(ctx, "tones", R.n_for(R.block_T(fft)[2], hop), 45, "float32", fft, fft, hop, kind=kind)


# ---- one buffer, the generic kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("win,fft,hop", R.GENERIC_POW2 + R.GENERIC_ODD, ids=lambda v: str(v))
def test_generic_kernel(ctx, win, fft, hop):
    n = R.n_for(9, hop)
    for dtype in ("float32", "float64"):
        one_buffer(ctx, "dynamics", n, 50, dtype, win, fft, hop)
    one_buffer(ctx, "tones", n, 51, "float32", win, fft, hop, want_spec=False)
    if win % 2:
        one_buffer(ctx, "tones", n, 52, "float32", win, fft, hop, kind=4)       # the Gaussian window exists at odd sizes only


def test_generic_kernel_strides_over_frames(ctx):
    win, fft, hop, T = R.GENERIC_STRIDE_CASE
    one_buffer(ctx, "dynamics", R.n_for(T, hop), 53, "float32", win, fft, hop)


# ---- one buffer, the global-memory passes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft", R.BIG_FFTS)
def test_big_passes(ctx, fft):
    n = R.n_for(R.BIG_T, fft // 4)
    one_buffer(ctx, "dynamics", n, 60, "float32", fft, fft, fft // 4)
    one_buffer(ctx, "tones", n, 61, "float64", fft - 1, fft, fft // 4, want_spec=False)


def test_big_passes_across_a_chunk_boundary(ctx):
    """1032 frames at fft 65536 against the 1024 one 512 MB chunk holds: long double on the frames around the boundary, the
    first and last four and every 64th; every frame against numpy's float64 rfft, 128 frames at a time"""
    win, fft, hop, n = R.CHUNK_CASE
    T = R.num_frames(n, hop)
    x = R.dynamics(n, 62, "float32", 12.0)
    _, mag = ctx.stft(x, win, fft, hop, want_spec=False)
    assert mag.shape == (T, fft // 2 + 1)
    named = R.chunk_frames_named()
    ref = R.stft_ld(x, win, fft, hop, frames=np.array(named))
    hold("chunk boundary, named frames", (None, mag[named]), ref, STFT_BAR[fft])
    floor = R.frame_err(R.stft_f64(x, win, fft, hop, frames=np.array(named))[1], ref[1])[0]
    worst = 0.0
    for t0 in range(0, T, 128):
        fr = np.arange(t0, min(t0 + 128, T))
        e, t = R.frame_err(mag[fr], R.stft_f64(x, win, fft, hop, frames=fr)[1])
        worst = max(worst, e)
        assert e <= STFT_BAR[fft] + floor, (t0 + t, e)
    print(f"chunk boundary, all {T} frames against float64 rfft: worst {worst:.2e} (bar {STFT_BAR[fft]:.1e} + rfft's own {floor:.2e})")


# ---- corpora -------------------------------------------------------------------------------------------------------------------
def corpus_audio(B, n, seed, decades=6.0):
    return np.stack([R.dynamics(n, seed + b, "float32", decades) for b in range(B)])


def transform(ctx, B, n, win, fft, hop, audio, mag_only=False, keep=True):
    import fluhip
    cor = fluhip.Corpus(ctx, B, n, win, fft, hop, K)
    try:
        cor.set_audio(audio)
        cor.keep_spectrum(keep)
        (cor.stft_mag_only if mag_only else cor.stft)()
        return cor.read_layouts_f64(mag=True, magT=not mag_only, spec=keep)
    finally:
        cor.close()


def hold_corpus(what, lay, audio, win, fft, hop, Ts=None):
    """every frame of every buffer of an equal-length or ragged corpus against long double; both layouts; the spectrum"""
    mag, magT, spec = lay
    B, F = mag.shape[0], fft // 2 + 1
    Ts = [R.num_frames(len(a), hop) for a in audio] if Ts is None else Ts
    if magT is not None:
        R.check_layouts(mag, magT, Ts, F)
    else:
        assert all(not mag[b, T:].any() and not mag[b, :, F:].any() for b, T in enumerate(Ts))
    worst = 0.0
    for b, T in enumerate(Ts):
        ref = R.stft_ld(audio[b], win, fft, hop)
        got_spec = None if spec is None else spec[b, :T]
        worst = max(worst, hold(f"{what} buffer {b}", (got_spec, mag[b, :T, :F]), ref, STFT_BAR[fft]))
        if got_spec is not None:
            m = R.mag_of_spec_err(mag[b, :T, :F], got_spec)
            print(f"{what} buffer {b}: magnitudes from hypot of the own spectrum {m:.2e} (bar {R.MAG_OF_SPEC_BAR:.2e})")
            assert m <= R.MAG_OF_SPEC_BAR
    return worst


@pytest.mark.parametrize("fft", R.BLOCK_FFTS)
@pytest.mark.parametrize("mag_only", [False, True], ids=["both_layouts", "mag_only"])
def test_corpus_block_form_one_round(ctx, fft, mag_only):
    B, n, win, _, hop = R.corpus_one_round(fft)
    audio = corpus_audio(B, n, 70)
    hold_corpus(f"corpus fft {fft}", transform(ctx, B, n, win, fft, hop, audio, mag_only), audio, win, fft, hop)
    # without the spectrum: SPEC = false, with and without the bin-major copy
    mag, magT, _ = transform(ctx, B, n, win, fft, hop, audio, mag_only, keep=False)
    hold_corpus(f"corpus fft {fft} no spectrum", (mag, magT, None), audio, win, fft, hop)


@pytest.mark.parametrize("fft", sorted(R.MULTI_ROUND))
@pytest.mark.parametrize("which", [0, 1], ids=["even_n_even_hop", "odd_hop"])
def test_corpus_block_form_second_round(ctx, fft, which):
    """more blocks than workgroups: a workgroup runs a second block, alternates its staging sets and (fft 2048) windows the
    samples it requested ahead.  Long double on the blocks dealt to the first and last workgroup of either round; every frame
    of every buffer against numpy's float64 rfft, the bar widened by that rfft's own distance from long double"""
    B, n, win, _, hop = R.MULTI_ROUND[fft][which]
    T, F = R.num_frames(n, hop), fft // 2 + 1
    audio = corpus_audio(B, n, 80 + which)
    d = R.dispatch(win, fft, B, T, True, True, n, hop)
    assert d["rounds"] == 2
    mag, magT, spec = transform(ctx, B, n, win, fft, hop, audio)
    R.check_layouts(mag, magT, [T] * B, F)
    floor = 0.0
    for b, t0 in R.round_blocks(d["dealing"]):
        fr = np.arange(t0, min(t0 + d["FPB"], T))
        ref = R.stft_ld(audio[b], win, fft, hop, frames=fr)
        hold(f"fft {fft} hop {hop} buffer {b} block at frame {t0}", (spec[b, fr], mag[b, fr, :F]), ref, STFT_BAR[fft])
        floor = max(floor, max(R.frame_err(g, r)[0] for g, r in zip(R.stft_f64(audio[b], win, fft, hop, frames=fr), ref)))
    for b in range(B):
        ref = R.stft_f64(audio[b], win, fft, hop)
        hold(f"fft {fft} hop {hop} buffer {b}, all {T} frames against float64 rfft (its own {floor:.2e})", (spec[b], mag[b, :T, :F]), ref,
             STFT_BAR[fft] + floor)
        assert R.mag_of_spec_err(mag[b, :T, :F], spec[b]) <= R.MAG_OF_SPEC_BAR


@pytest.mark.parametrize("fft", R.BLOCK_FFTS)
def test_ragged_corpus(ctx, fft):
    import fluhip
    lens, hop = R.ragged_lengths(fft), fft // 4
    audio = [R.dynamics(n, 90 + i) for i, n in enumerate(lens)]
    cor = fluhip.RaggedCorpus(ctx, lens, fft, fft, hop, K)
    try:
        assert cor.Ts == [R.num_frames(n, hop) for n in lens]
        cor.set_audio(audio)
        cor.keep_spectrum(True)
        cor.stft()
        lay = cor.read_layouts_f64(spec=True)
        m = cor.read_f64(factors=False)[0]
    finally:
        cor.close()
    # each buffer's own frames against the reference; the frames past them exactly zero in both layouts (check_layouts)
    hold_corpus(f"ragged fft {fft}", lay, audio, fft, fft, hop, cor.Ts)
    assert np.array_equal(m, lay[0][:, :cor.T, :cor.F])


@pytest.mark.parametrize("B,n,win,fft,hop", R.NO_BLOCK_CORPORA, ids=lambda v: str(v))
def test_corpus_without_a_block_form(ctx, B, n, win, fft, hop):
    """generic kernel or global-memory passes, then the transposing copy: both layouts"""
    audio = corpus_audio(B, n, 100)
    hold_corpus(f"corpus win {win} fft {fft}", transform(ctx, B, n, win, fft, hop, audio), audio, win, fft, hop)


# ---- BufSTFT ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,win,fft,hop", R.BUFSTFT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bufstft_forward_padding_modes(ctx, n, win, fft, hop, mode):
    """float32 magnitudes [F, T]: one rounding to float of a double within STFT_BAR"""
    x = R.dynamics(n, 110)
    T, off = R.bufstft_geometry(n, win, hop, mode)
    mag32, _ = ctx.bufstft_forward(x, win, fft, hop, mode)
    assert mag32.shape == (fft // 2 + 1, T)
    ref = R.stft_ld(x, win, fft, hop, offset=off, T=T)
    hold(f"BufSTFT mode {mode} win {win} fft {fft}", (None, mag32.T.astype(np.float64)), ref, FLOAT32_ULP + STFT_BAR[fft])


# ---- frames outside their buffer, every kernel form ---------------------------------------------------------------------------
@pytest.mark.parametrize("odd_hop", [False, True], ids=["hop_quarter", "odd_hop"])
@pytest.mark.parametrize("win,fft,dtypes", R.OUTSIDE_CASES, ids=lambda v: str(v) if isinstance(v, int) else "")
def test_frames_outside_the_buffer(ctx, win, fft, dtypes, odd_hop):
    """fluhip_debug_stft_frames_*: frames from more than two transforms before their buffer to at least one behind it, which
    STFT::process' framing never produces and the control clients' latency does; three buffers side by side, each between guards
    of 1e30 that reach past every frame.  Every frame of every buffer against the long double restatement at STFT_BAR[fft]; a frame
    with no sample of its buffer exactly zero (frame_err); no guard value, no neighbour's sample in any result.
    A second launch without the spectrum (the kernels' SPEC = false forms) returns the kernels' OWN magnitudes, as the corpus and
    the control clients consume them: the same bar on every frame with a sample of its buffer, and every bin of the others 0 or
    R.SILENT_BIN (the block form's sum of squares starts from DBL_MIN, fft_core.h mag_sumsq: sqrt(DBL_MIN) = 2^-511 exactly)."""
    form = {True: "big", False: "block" if win % 2 == 0 and fft in R.BLOCK_FFTS else "generic"}[fft > 8192]
    for dtype in dtypes:
        for shift in R.outside_shifts(fft, odd_hop):
            n, hop, frame0, T, guard = R.outside_geometry(fft, odd_hop, shift)
            assert R.dispatch(win, fft, R.OUTSIDE_B, T, False, dtype == "float32", n, hop)["branch"] == form
            padded, bufs = R.outside_input(n, guard, 120, dtype)
            spec, mag = ctx.debug_stft_frames(padded, n, guard, win, fft, hop, frame0, T)
            _, own = ctx.debug_stft_frames(padded, n, guard, win, fft, hop, frame0, T, want_spec=False)
            assert spec.shape == mag.shape == own.shape == (R.OUTSIDE_B, T, fft // 2 + 1)
            # (|x| < 2: a guard sample would read 1e30 x the window)
            assert np.abs(spec).max() < fft and mag.max() < fft and own.max() < fft
            silent = 0
            for b, x in enumerate(bufs):
                what = f"outside {dtype} win {win} fft {fft} hop {hop} frame0 {frame0} buffer {b}"
                ref = R.stft_ld(x, win, fft, hop, offset=frame0, T=T)
                hold(what, (spec[b], mag[b]), ref, STFT_BAR[fft])
                live = np.abs(ref[1]).max(axis=1) != 0
                hold(what + " own magnitudes", (None, own[b][live]), (None, ref[1][live]), STFT_BAR[fft])
                assert np.isin(own[b][~live], (0.0, R.SILENT_BIN)).all(), what
                silent += int((~live).sum())
            assert silent >= 2 * R.OUTSIDE_B                             # frames with no sample of their buffer, front and back


def test_frames_outside_an_empty_buffer(ctx):
    """n = 0: every frame of every form exactly zero, whatever lies around the (empty) buffer"""
    for win, fft, dtypes in R.OUTSIDE_CASES:
        for dtype in dtypes:
            guard, hop, T = 4 * fft, fft // 4, 9
            padded = np.full((2, 2 * guard), R.OUTSIDE_GUARD_VALUE, dtype=dtype)
            spec, mag = ctx.debug_stft_frames(padded, 0, guard, win, fft, hop, -fft - hop, T)
            _, own = ctx.debug_stft_frames(padded, 0, guard, win, fft, hop, -fft - hop, T, want_spec=False)
            assert not spec.any() and not mag.any() and np.isin(own, (0.0, R.SILENT_BIN)).all(), (win, fft, dtype)


def test_frames_outside_the_buffer_refuses_short_guards(ctx):
    import fluhip
    n, hop, frame0, T, guard = R.outside_geometry(1024, False, 0)
    padded, _ = R.outside_input(n, guard - 1, 120, "float32")
    with pytest.raises(fluhip.FluhipError, match="guards must reach"):
        ctx.debug_stft_frames(padded, n, guard - 1, 1024, 1024, hop, frame0, T)
