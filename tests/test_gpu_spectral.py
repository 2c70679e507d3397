"""GPU tests of BufSpectralShape and BufChroma through the C ABI, against tests/spectral_ref.py.  The algorithms are pinned apart
from the STFT on the restatement's own magnitudes (fluhip_spectralshape_frames_f64, fluhip_chroma_frames_f64);
fluhip_bufspectralshape_f32 and fluhip_bufchroma_f32 are held to the same bars plus float32 rounding.  No frame and no
descriptor is exempted."""
import os

import numpy as np
import pytest

import pitch_ref as R
import spectral_ref as S
from test_pitch_ref import shape_mags
from test_spectral_ref import CHROMA_FLOOR, FILTER_CASES, FILTER_FLOOR, SHAPE_FLOOR, UNIT_POWER

pytestmark = pytest.mark.gpu

# 64 x the floor between two double STFTs on the CPU (tests/test_spectral_ref.py::test_floors_between_two_double_stfts), the
# factor the onset, novelty and pitch tests use: the device's log and exp differ from glibc's in the last places
SHAPE_BAR = np.array([64 * SHAPE_FLOOR[d] for d in S.DESCRIPTORS])
CHROMA_BAR = {n: 64 * v for n, v in CHROMA_FLOOR.items()}
FILTER_BAR = 64 * FILTER_FLOOR
F32 = 2.0 ** -23   # one rounding to float32, relative
SHAPES = R.SHAPES[:6]   # (256,256,64) (400,512,128) two-pass; (1024,1024,512) (1500,2048,300) (4096,4096,1024) on chip; (1001,1024,256) odd
IDS = [str(s) for s in SHAPES]
ON_CHIP = {(1024, 1024, 512), (1500, 2048, 300), (4096, 4096, 1024)}

_want = {}


def want_shape(shape, **kw):
    key = ("shape", shape, tuple(sorted(kw.items())))
    if key not in _want:
        mags, sr = shape_mags(shape)
        kw.setdefault("sr", sr)
        _want[key] = S.shape_frames(mags, **kw)
    return _want[key]


def want_chroma(shape, **kw):
    key = ("chroma", shape, tuple(sorted(kw.items())))
    if key not in _want:
        mags, sr = shape_mags(shape)
        kw.setdefault("sr", sr)
        _want[key] = S.chroma_frames(mags, **kw)
    return _want[key]


def check_shape(got, want, extra=0.0, what="", cols=range(7)):
    """got, want [T, 7] (or the selected columns `cols` of it)"""
    cols = list(cols)
    assert got.shape == want.shape == (len(want), len(cols))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    with np.errstate(invalid="ignore"):
        err = np.nan_to_num(np.abs(got - want) / np.maximum(1.0, np.abs(want)), nan=0.0).max(axis=0)
    bar = SHAPE_BAR[cols] + extra
    print(what, " ".join(f"{S.DESCRIPTORS[c]} {e:.2e}/{b:.1e}" for c, e, b in zip(cols, err, bar)))
    assert np.all(err <= bar), [S.DESCRIPTORS[c] for c, e, b in zip(cols, err, bar) if e > b]


def check_chroma(got, want, normalize, extra=0.0, what=""):
    """got, want [T, nChroma]: |a - b| relative to the frame's peak"""
    assert got.shape == want.shape
    peak = np.abs(want).max(axis=1, keepdims=True)
    err = float((np.abs(got - want) / np.where(peak == 0, 1.0, peak)).max())
    print(f"{what} chroma normalize {normalize}: {err:.3e} (bar {CHROMA_BAR[normalize] + extra:.1e})")
    assert np.array_equal(got[peak[:, 0] == 0], want[peak[:, 0] == 0])
    assert err <= CHROMA_BAR[normalize] + extra


# ---- SpectralShape -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit,power", UNIT_POWER)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shape_frames_against_the_restatement(ctx, shape, unit, power):
    mags, sr = shape_mags(shape)
    got = ctx.spectralshape_frames(mags, unit=unit, power=power, sample_rate=sr)[0]
    check_shape(got, want_shape(shape, unit=unit, power=power), what=f"{shape} unit {unit} power {power}")


@pytest.mark.parametrize("unit,power", UNIT_POWER)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bufspectralshape_against_the_restatement(ctx, shape, unit, power):
    x, sr = R.material(shape)
    win, fft, hop = shape
    got = ctx.bufspectralshape(x, unit=unit, power=power, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    check_shape(got.T.astype(np.float64), want_shape(shape, unit=unit, power=power), extra=F32, what=f"{shape} f32 unit {unit} power {power}")


# (minFreq, maxFreq, unit, sample rate) on the (1024, 1024, 512) input
BOUNDS = {"one-bin": (5000.0, 5100.0, 0, 44100.0), "min0-midi": (0.0, -1.0, 1, 44100.0), "min0-midi-max": (0.0, 3000.0, 1, 44100.0),
          "beyond-nyquist": (100.0, 30000.0, 0, 44100.0), "8k": (20.0, 20000.0, 1, 8000.0), "band": (300.0, 4000.0, 0, 44100.0)}
EMPTY = {"min==max": (5000.0, 5000.0), "min>max": (6000.0, 5000.0), "min-beyond-nyquist": (30000.0, -1.0), "max0": (0.0, 0.0)}


@pytest.mark.parametrize("case", BOUNDS, ids=list(BOUNDS))
def test_shape_frequency_bounds(ctx, case):
    lo, hi, unit, sr = BOUNDS[case]
    shape = (1024, 1024, 512)
    mags, _ = shape_mags(shape)
    got = ctx.spectralshape_frames(mags, lo, hi, unit=unit, sample_rate=sr)[0]
    check_shape(got, want_shape(shape, min_freq=lo, max_freq=hi, unit=unit, sr=sr), what=case)
    if case == "one-bin":
        # a segment of one bin has the spread d^2 with d = f - (a f) / a: exactly 0 or one rounding of f, as the bits of a fall,
        # and skewness and kurtosis are 0 / 0 or huge accordingly.  On the same magnitudes the device repeats the
        # restatement's operations (above); on the device's own transform that is no property to hold
        return
    x, _ = R.material(shape)
    buf = ctx.bufspectralshape(x, min_freq=lo, max_freq=hi, unit=unit, win=1024, fft=1024, hop=512, sample_rate=sr)[0]
    check_shape(buf.T.astype(np.float64), want_shape(shape, min_freq=lo, max_freq=hi, unit=unit, sr=sr), extra=F32, what=case + " f32")


@pytest.mark.parametrize("case", EMPTY, ids=list(EMPTY))
def test_an_empty_range_gives_exact_zeros(ctx, case):
    lo, hi = EMPTY[case]
    mags, sr = shape_mags((400, 512, 128))
    x, _ = R.material((400, 512, 128))
    got = ctx.spectralshape_frames(mags, lo, hi)
    assert got.shape == (1, len(mags), 7) and np.all(got == 0) and not np.any(np.signbit(got))
    buf = ctx.bufspectralshape(x, min_freq=lo, max_freq=hi, win=400, fft=512, hop=128)
    assert buf.shape == (1, 7, len(mags)) and np.all(buf == 0)
    assert np.all(S.shape_frames(mags, min_freq=lo, max_freq=hi) == 0)


@pytest.mark.parametrize("percent", (0.0, 50.0, 95.0))
@pytest.mark.parametrize("shape", [(400, 512, 128), (1500, 2048, 300)], ids=str)
def test_rolloff_percent(ctx, shape, percent):
    mags, sr = shape_mags(shape)
    got = ctx.spectralshape_frames(mags, rolloff_percent=percent, sample_rate=sr)[0]
    check_shape(got, want_shape(shape, rolloff_percent=percent), what=f"{shape} rolloff {percent}")
    x, _ = R.material(shape)
    win, fft, hop = shape
    buf = ctx.bufspectralshape(x, rolloff_percent=percent, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    check_shape(buf.T.astype(np.float64), want_shape(shape, rolloff_percent=percent), extra=F32, what=f"{shape} f32 rolloff {percent}")


def test_rolloff_percent_100_is_unpinned(ctx):
    """the reference compares a sequential running sum against a separately ordered total: either the last frequency step or
    maxBin - 1"""
    mags, sr = shape_mags((1024, 1024, 512))
    got = ctx.spectralshape_frames(mags, rolloff_percent=100.0, sample_rate=sr)[0]
    ax = S.shape_axis(0, 512, sr / 1024)
    r = got[:, 4]
    assert np.all((r == 511.0) | ((r >= ax[-2]) & (r <= ax[-1])))
    check_shape(got[:, [0, 1, 2, 3, 5, 6]], want_shape((1024, 1024, 512))[:, [0, 1, 2, 3, 5, 6]], cols=(0, 1, 2, 3, 5, 6), what="100 %")


@pytest.mark.parametrize("select", (1, 16, 0b1010010, 0b0101101, 127))
def test_select_orders_and_counts_the_channels(ctx, select):
    shape = (400, 512, 128)
    x, sr = R.material(shape)
    got = ctx.bufspectralshape(x, select=select, win=400, fft=512, hop=128, sample_rate=sr)[0]
    cols = [i for i in range(7) if select >> i & 1]
    assert got.shape == (len(cols), len(want_shape(shape)))
    check_shape(got.T.astype(np.float64), want_shape(shape)[:, cols], extra=F32, cols=cols, what=f"select {select:#b}")
    assert np.array_equal(got, ctx.bufspectralshape(x, win=400, fft=512, hop=128, sample_rate=sr)[0][cols])


@pytest.mark.parametrize("padding_mode", (0, 1, 2))
@pytest.mark.parametrize("shape", [(400, 512, 128), (1024, 1024, 512), (1500, 2048, 300)], ids=str)
def test_padding_modes(ctx, shape, padding_mode):
    win, fft, hop = shape
    x = R.glide(9000, seed=21)
    mags = R.client_magnitudes(x, win, fft, hop, padding_mode)
    got = ctx.bufspectralshape(x, win=win, fft=fft, hop=hop, padding_mode=padding_mode)[0]
    assert got.shape[1] == R.client_frames(len(x), win, hop, padding_mode)[1]
    check_shape(got.T.astype(np.float64), S.shape_frames(mags), extra=F32, what=f"{shape} padding {padding_mode}")
    for normalize in (0, 2):
        c = ctx.bufchroma(x, normalize=normalize, win=win, fft=fft, hop=hop, padding_mode=padding_mode)[0]
        check_chroma(c.T.astype(np.float64), S.chroma_frames(mags, normalize=normalize), normalize, extra=F32,
                     what=f"{shape} padding {padding_mode}")


# ---- Chroma ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,n_bins,ref,sr", FILTER_CASES, ids=[f"{c[0]}x{c[1]}-{c[2]:g}-{c[3]:g}" for c in FILTER_CASES])
def test_the_filter_table(ctx, nc, n_bins, ref, sr):
    got = ctx.chroma_filters(nc, n_bins, ref, sr)
    want, _ = S.chroma_filters(nc, n_bins, ref, sr)
    err = float(np.abs(got - want).max())
    print(f"filter table {nc} x {n_bins}, ref {ref}: {err:.3e} (bar {FILTER_BAR:.1e})")
    assert err <= FILTER_BAR


@pytest.mark.parametrize("normalize", (0, 1, 2))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_chroma_frames_against_the_restatement(ctx, shape, normalize):
    mags, sr = shape_mags(shape)
    got = ctx.chroma_frames(mags, normalize=normalize, sample_rate=sr)[0]
    check_chroma(got, want_chroma(shape, normalize=normalize), normalize, what=str(shape))


@pytest.mark.parametrize("normalize", (0, 1, 2))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bufchroma_against_the_restatement(ctx, shape, normalize):
    x, sr = R.material(shape)
    win, fft, hop = shape
    got = ctx.bufchroma(x, normalize=normalize, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    assert got.shape == (12, len(want_chroma(shape, normalize=normalize)))
    check_chroma(got.T.astype(np.float64), want_chroma(shape, normalize=normalize), normalize, extra=F32, what=f"{shape} f32")


# (numChroma, ref, sample rate, minFreq, maxFreq): 7 has an odd half; ref 22000 at fft 4096 (at 8 kHz the argument of fmod goes
# negative; at 44.1 kHz it stays positive at this size); min_freq 0 with max_freq set zeroes bin 0; both set
CHROMA_CASES = {"7": (7, 440.0, 44100.0, 0.0, -1.0), "24": (24, 440.0, 44100.0, 0.0, -1.0), "2": (2, 440.0, 44100.0, 0.0, -1.0),
                "128": (128, 440.0, 44100.0, 0.0, -1.0), "ref22000": (12, 22000.0, 44100.0, 0.0, -1.0),
                "ref22000-8k": (12, 22000.0, 8000.0, 0.0, -1.0), "min0-max": (12, 440.0, 44100.0, 0.0, 5000.0),
                "min-max": (12, 440.0, 44100.0, 100.0, 5000.0), "beyond": (12, 440.0, 44100.0, 30000.0, 40000.0)}


@pytest.mark.parametrize("normalize", (0, 1, 2))
@pytest.mark.parametrize("case", CHROMA_CASES, ids=list(CHROMA_CASES))
def test_chroma_parameters(ctx, case, normalize):
    nc, ref, sr, lo, hi = CHROMA_CASES[case]
    shape = (4096, 4096, 1024)
    mags, _ = shape_mags(shape)
    mags = mags.copy()
    mags[:, 0] += 0.5 * mags.max()                        # a bin 0 that matters when it is zeroed
    want = S.chroma_frames(mags, nc, ref, normalize, lo, hi, sr)
    got = ctx.chroma_frames(mags, nc, ref, normalize, lo, hi, sr)[0]
    check_chroma(got, want, normalize, what=case)
    if sr == 44100.0:
        x, _ = R.material(shape)
        buf = ctx.bufchroma(x, nc, ref, normalize, lo, hi, win=4096, fft=4096, hop=1024, sample_rate=sr)[0]
        check_chroma(buf.T.astype(np.float64), S.chroma_frames(shape_mags(shape)[0], nc, ref, normalize, lo, hi, sr), normalize,
                     extra=F32, what=case + " f32")


def test_chroma_leaves_its_input_alone(ctx):
    mags = np.ascontiguousarray(shape_mags((1024, 1024, 512))[0])
    keep = mags.copy()
    ctx.chroma_frames(mags, min_freq=100.0, max_freq=5000.0)
    assert mags.tobytes() == keep.tobytes()


# ---- the smallest transforms, silence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bins", (3, 5))
def test_the_frames_calls_at_3_and_5_bins(ctx, n_bins):
    rng = np.random.default_rng(n_bins)
    mags = np.abs(rng.standard_normal((9, n_bins))) + 0.01
    for unit, power in UNIT_POWER:
        got = ctx.spectralshape_frames(mags, unit=unit, power=power)[0]
        check_shape(got, S.shape_frames(mags, unit=unit, power=power), what=f"F {n_bins} unit {unit} power {power}")
    assert np.all(ctx.spectralshape_frames(mags, max_freq=1.5 * 44100.0 / (2 * (n_bins - 1)), unit=1) == 0)
    for normalize in (0, 1, 2):
        check_chroma(ctx.chroma_frames(mags, normalize=normalize)[0], S.chroma_frames(mags, normalize=normalize), normalize,
                     what=f"F {n_bins}")


def test_silence(ctx):
    z = np.zeros(6000, dtype=np.float32)
    for shape in ((256, 256, 64), (1024, 1024, 512)):
        win, fft, hop = shape
        F = fft // 2 + 1
        eps_frame = S.shape_frames(np.full((1, F), S.EPSILON))
        got = ctx.bufspectralshape(z, win=win, fft=fft, hop=hop)[0]
        check_shape(got.T.astype(np.float64), np.repeat(eps_frame, got.shape[1], axis=0), extra=F32, what=f"silence {shape}")
        for normalize in (0, 1, 2):
            c = ctx.bufchroma(z, normalize=normalize, win=win, fft=fft, hop=hop)
            assert c.shape[1] == 12 and np.all(c == 0) and not np.any(np.signbit(c))
    zeros = np.zeros((3, 513))
    check_shape(ctx.spectralshape_frames(zeros)[0], np.repeat(S.shape_frames(np.full((1, 513), S.EPSILON)), 3, axis=0), what="zeros")
    for normalize in (0, 1, 2):
        c = ctx.chroma_frames(zeros, normalize=normalize)
        assert np.all(c == 0) and not np.any(np.signbit(c))


# ---- batches, rounds, runs, forms --------------------------------------------------------------------------------------
def test_a_batch_gives_the_bits_of_single_calls(ctx):
    shape = (1500, 2048, 300)
    win, fft, hop = shape
    xs = np.stack([R.glide(14000, seed=s) for s in (9, 12, 14)])
    batch = ctx.bufspectralshape(xs, win=win, fft=fft, hop=hop)
    cbatch = ctx.bufchroma(xs, normalize=1, win=win, fft=fft, hop=hop)
    for b in range(3):
        assert np.array_equal(batch[b], ctx.bufspectralshape(xs[b], win=win, fft=fft, hop=hop)[0])
        assert np.array_equal(cbatch[b], ctx.bufchroma(xs[b], normalize=1, win=win, fft=fft, hop=hop)[0])
    xs2 = xs[:, :9000]
    batch = ctx.bufspectralshape(xs2, win=400, fft=512, hop=128)          # ... and in the two-pass form
    cbatch = ctx.bufchroma(xs2, win=400, fft=512, hop=128)
    for b in range(3):
        assert np.array_equal(batch[b], ctx.bufspectralshape(xs2[b], win=400, fft=512, hop=128)[0])
        assert np.array_equal(cbatch[b], ctx.bufchroma(xs2[b], win=400, fft=512, hop=128)[0])
    mags = np.stack([R.client_magnitudes(x, win, fft, hop) for x in xs])
    fb, cb = ctx.spectralshape_frames(mags), ctx.chroma_frames(mags)
    for b in range(3):
        assert np.array_equal(fb[b], ctx.spectralshape_frames(mags[b])[0])
        assert np.array_equal(cb[b], ctx.chroma_frames(mags[b])[0])


@pytest.mark.parametrize("shape", [(1001, 1024, 256), (1024, 1024, 512)], ids=str)
def test_a_round_boundary_changes_no_bit(ab_ctx, shape):
    """the build with live switches cuts the frames into rounds of 7 (FLUHIP_SPECTRAL_ROUND_FRAMES): frames on either side of a
    boundary equal those of a call without one, in the two-pass form and on chip"""
    win, fft, hop = shape
    x, _ = R.material(shape)
    whole = ab_ctx.bufspectralshape(x, win=win, fft=fft, hop=hop)
    cwhole = ab_ctx.bufchroma(x, normalize=2, win=win, fft=fft, hop=hop)
    os.environ["FLUHIP_SPECTRAL_ROUND_FRAMES"] = "7"
    try:
        cut = ab_ctx.bufspectralshape(x, win=win, fft=fft, hop=hop)
        cut3 = ab_ctx.bufspectralshape(np.stack([x, x, x]), win=win, fft=fft, hop=hop)
        ccut = ab_ctx.bufchroma(x, normalize=2, win=win, fft=fft, hop=hop)
        ccut3 = ab_ctx.bufchroma(np.stack([x, x, x]), normalize=2, win=win, fft=fft, hop=hop)
    finally:
        del os.environ["FLUHIP_SPECTRAL_ROUND_FRAMES"]
    assert whole.shape[2] > 14
    assert np.array_equal(whole, cut) and np.array_equal(cwhole, ccut)
    assert all(np.array_equal(whole[0], cut3[b]) and np.array_equal(cwhole[0], ccut3[b]) for b in range(3))


def test_a_run_boundary_changes_no_bit(ctx):
    """the on-chip form hands runs of 32 frames to workgroups.  Frame t of the whole signal holds the samples
    [300 t - 750, 300 t + 750) (padding 1: win / 2 in front), so frame t of x[4800:12300] is frame t + 16 of x wherever the
    window touches no padding: frames 19 .. 38 of the long call, across the boundary at 32, against frames 3 .. 22 of a call
    of 26 frames, which has no boundary"""
    win, fft, hop = 1500, 2048, 300
    x, sr = R.material((win, fft, hop))
    assert ctx.spectral_plan(fft, win, 0)[:2] == (0, 32)
    for call in (lambda a: ctx.bufspectralshape(a, win=win, fft=fft, hop=hop, sample_rate=sr),
                 lambda a: ctx.bufchroma(a, win=win, fft=fft, hop=hop, sample_rate=sr)):
        long, short = call(x)[0], call(x[4800:12300])[0]
        assert long.shape[1] > 39 and short.shape[1] == 26
        assert np.array_equal(long[:, 19:39], short[:, 3:23])
        assert np.array_equal(call(np.stack([x[::-1], x]))[1], long)      # the boundary in a buffer that is not the first


@pytest.mark.parametrize("shape", sorted(ON_CHIP), ids=str)
def test_the_two_pass_form_at_the_on_chip_sizes(ab_ctx, shape):
    """FLUHIP_SPECTRAL_FORM=1 (the build with live switches) sends an on-chip shape through the two-pass form: the same bars"""
    x, sr = R.material(shape)
    win, fft, hop = shape
    chip = ab_ctx.bufspectralshape(x, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    cchip = ab_ctx.bufchroma(x, normalize=1, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    os.environ["FLUHIP_SPECTRAL_FORM"] = "1"
    try:
        two = ab_ctx.bufspectralshape(x, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
        ctwo = ab_ctx.bufchroma(x, normalize=1, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    finally:
        del os.environ["FLUHIP_SPECTRAL_FORM"]
    check_shape(two.T.astype(np.float64), want_shape(shape), extra=F32, what=f"{shape} two-pass")
    check_shape(chip.T.astype(np.float64), want_shape(shape), extra=F32, what=f"{shape} on-chip")
    check_chroma(ctwo.T.astype(np.float64), want_chroma(shape, normalize=1), 1, extra=F32, what=f"{shape} two-pass")
    check_chroma(cchip.T.astype(np.float64), want_chroma(shape, normalize=1), 1, extra=F32, what=f"{shape} on-chip")


@pytest.mark.parametrize("shape", R.SHAPES, ids=[str(s) for s in R.SHAPES])
def test_plan(ctx, shape):
    win, fft, hop = shape
    # fft 1024 / 2048 / 4096 with an even window run the on-chip form in runs of 32 frames, every other shape the two-pass form
    form, run = (0, 32) if shape in ON_CHIP else (1, 0)
    assert ctx.spectral_plan(fft, win, 0) == (form, run, 1, 0)
    assert ctx.spectral_plan(fft, win, 1) == (form, run, 1, 1)
    # an odd window has no on-chip form at any size
    assert ctx.spectral_plan(fft, win - 1 if win % 2 == 0 else win, 0)[:2] == (1, 0)
    for f in (512, 8192):
        assert ctx.spectral_plan(f, f, 0)[0] == 1


# ---- announced errors --------------------------------------------------------------------------------------------------
SHAPE_ERRORS = [(dict(min_freq=-1.0), "minFreq"), (dict(max_freq=-2.0), "maxFreq"), (dict(rolloff_percent=-0.5), "rolloffPercent"),
                (dict(rolloff_percent=100.5), "rolloffPercent"), (dict(rolloff_percent=float("nan")), "rolloffPercent"),
                (dict(unit=2), "unit"), (dict(unit=-1), "unit"), (dict(power=2), "power"), (dict(power=-1), "power"),
                (dict(sample_rate=0.0), "sample rate"), (dict(sample_rate=float("inf")), "sample rate")]
CHROMA_ERRORS = [(dict(num_chroma=1), "numChroma"), (dict(num_chroma=129), "numChroma"), (dict(ref=0.0), "ref"),
                 (dict(ref=22000.5), "ref"), (dict(normalize=3), "normalize"), (dict(normalize=-1), "normalize"),
                 (dict(min_freq=-1.0), "minFreq"), (dict(max_freq=-0.5), "maxFreq"), (dict(max_freq=-2.0), "maxFreq"),
                 (dict(sample_rate=-1.0), "sample rate"), (dict(sample_rate=float("nan")), "sample rate")]


def test_announced_errors_leave_the_context_usable(ctx):
    import fluhip
    shape = (256, 256, 64)
    x, sr = R.material(shape)
    mags, _ = shape_mags(shape)
    for kw, word in SHAPE_ERRORS:
        with pytest.raises(fluhip.FluhipError, match=word):
            ctx.bufspectralshape(x, win=256, fft=256, hop=64, **kw)
        with pytest.raises(fluhip.FluhipError, match=word):
            ctx.spectralshape_frames(mags, **kw)
    for select in (0, 128, -1):
        with pytest.raises(fluhip.FluhipError, match="select"):
            ctx.bufspectralshape(x, select=select, win=256, fft=256, hop=64)
    for kw, word in CHROMA_ERRORS:
        with pytest.raises(fluhip.FluhipError, match=word):
            ctx.bufchroma(x, win=256, fft=256, hop=64, **kw)
        with pytest.raises(fluhip.FluhipError, match=word):
            ctx.chroma_frames(mags, **kw)
        if "num_chroma" in kw or "ref" in kw or "sample_rate" in kw:
            with pytest.raises(fluhip.FluhipError, match=word):
                ctx.chroma_filters(kw.get("num_chroma", 12), 129, kw.get("ref", 440.0), kw.get("sample_rate", 44100.0))
    with pytest.raises(fluhip.FluhipError, match="fft"):
        ctx.spectralshape_frames(np.ones((2, 100)))                      # 2 (F - 1) = 198 is no power of two
    with pytest.raises(fluhip.FluhipError, match="fft"):
        ctx.chroma_frames(np.ones((2, 65538)))                           # beyond 65536
    with pytest.raises(fluhip.FluhipError, match="kind"):
        ctx.spectral_plan(1024, 1024, 2)
    # nothing was written by a refused call
    out = np.full((1, 7, 200), 7.0, dtype=np.float32)
    import ctypes
    rc = ctx.lib.fluhip_bufspectralshape_f32(ctx.h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1, len(x), 256, 256, 64, 1, 127,
                                             0.0, -1.0, 101.0, 0, 0, 44100.0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), None)
    assert rc == 2 and np.all(out == 7.0)
    got = ctx.bufspectralshape(x, win=256, fft=256, hop=64, sample_rate=sr)[0]
    check_shape(got.T.astype(np.float64), want_shape(shape), extra=F32, what="after the errors")
    got = ctx.bufchroma(x, win=256, fft=256, hop=64, sample_rate=sr)[0]
    check_chroma(got.T.astype(np.float64), want_chroma(shape), 0, extra=F32, what="after the errors")


# ---- the C++ host clients (include/flucoma_hip/SpectralShapeClient.hpp, ChromaClient.hpp) through tests/cpp/spectral_driver.cpp ----
@pytest.fixture(scope="module")
def spectral_driver(fluhip_lib_path):
    return S.build_driver()


def _run(driver, kind, path, outp, n, chans, rate, params, win=1024, hop=512, fft=1024, padding=1, asynchronous=0):
    out = R.drive(driver, "run", kind, path, n, chans, rate, *params, win, hop, fft, padding, asynchronous, outp)
    return [l.split("|") for l in out.splitlines()]


def shape_args(select=127, lo=0.0, hi=-1.0, percent=95.0, unit=0, power=0):
    return (select, lo, hi, percent, unit, power)


def chroma_args(nc=12, ref=440.0, normalize=0, lo=0.0, hi=-1.0):
    return (nc, ref, normalize, lo, hi)


def test_cpp_clients_against_the_c_abi(ctx, spectral_driver, tmp_path):
    shape = (1024, 1024, 512)
    x, sr = R.material(shape)
    xs = np.stack([x, x[::-1]])                                  # two channels
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    np.ascontiguousarray(xs.T).tofile(path)                      # the memory buffer is frames x channels
    T = len(want_shape(shape))
    for asynchronous in (0, 1):
        lines = _run(spectral_driver, "shape", path, outp, len(x), 2, sr, shape_args(), asynchronous=asynchronous)
        assert lines[-2] == ["run", "0", ""]
        assert lines[-1][:4] == ["shape", "features", str(T), "14"] and float(lines[-1][4]) == sr / 512
        got = np.fromfile(outp, dtype=np.float32).reshape(14, T)  # feature i of channel j in buffer channel i + 7 j
        check_shape(got[:7].T.astype(np.float64), want_shape(shape), extra=F32, what="client ch 0")
        assert np.array_equal(got, ctx.bufspectralshape(xs, win=1024, fft=1024, hop=512, sample_rate=sr).reshape(14, T))
        lines = _run(spectral_driver, "chroma", path, outp, len(x), 2, sr, chroma_args(normalize=1), asynchronous=asynchronous)
        assert lines[-2] == ["run", "0", ""]
        assert lines[-1][:4] == ["shape", "features", str(T), "24"] and float(lines[-1][4]) == sr / 512
        got = np.fromfile(outp, dtype=np.float32).reshape(24, T)
        check_chroma(got[:12].T.astype(np.float64), want_chroma(shape, normalize=1), 1, extra=F32, what="client ch 0")
        assert np.array_equal(got, ctx.bufchroma(xs, normalize=1, win=1024, fft=1024, hop=512, sample_rate=sr).reshape(24, T))


def test_cpp_clients_select_and_announced_errors(ctx, spectral_driver, tmp_path):
    shape = (400, 512, 128)
    x, sr = R.material(shape)
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    x.tofile(path)
    fftkw = dict(win=400, hop=128, fft=512)
    lines = _run(spectral_driver, "shape", path, outp, len(x), 1, sr, shape_args(select=0b10010, unit=1, power=1), **fftkw)
    assert lines[-2] == ["run", "0", ""] and lines[-1][3] == "2"
    got = np.fromfile(outp, dtype=np.float32).reshape(2, -1)
    assert np.array_equal(got, ctx.bufspectralshape(x, select=0b10010, unit=1, power=1, win=400, fft=512, hop=128, sample_rate=sr)[0])
    lines = _run(spectral_driver, "chroma", path, outp, len(x), 1, sr, chroma_args(nc=7, ref=300.0, normalize=2, lo=100.0, hi=5000.0), **fftkw)
    assert lines[-2] == ["run", "0", ""] and lines[-1][3] == "7"
    got = np.fromfile(outp, dtype=np.float32).reshape(7, -1)
    assert np.array_equal(got, ctx.bufchroma(x, 7, 300.0, 2, 100.0, 5000.0, win=400, fft=512, hop=128, sample_rate=sr)[0])
    for params, word in ((shape_args(select=0), "select"), (shape_args(lo=-1.0), "minFreq"), (shape_args(percent=101.0), "rolloffPercent"),
                         (shape_args(unit=2), "unit"), (shape_args(power=3), "power")):
        lines = _run(spectral_driver, "shape", path, outp, len(x), 1, sr, params, **fftkw)
        assert lines[-2][0] == "run" and lines[-2][1] == "2" and word in lines[-2][2], lines
    for params, word in ((chroma_args(nc=1), "numChroma"), (chroma_args(nc=129), "numChroma"), (chroma_args(ref=0.0), "ref"),
                         (chroma_args(normalize=3), "normalize"), (chroma_args(hi=-0.5), "maxFreq")):
        lines = _run(spectral_driver, "chroma", path, outp, len(x), 1, sr, params, **fftkw)
        assert lines[-2][0] == "run" and lines[-2][1] == "2" and word in lines[-2][2], lines
