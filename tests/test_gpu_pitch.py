"""GPU tests of BufPitch through the C ABI, against tests/pitch_ref.py.  The algorithms are pinned apart from the STFT on the
restatement's own magnitudes (fluhip_pitch_frames_f64, fluhip_debug_pitch_curve_f64); fluhip_bufpitch_f32 is held to the
same bars plus float32 rounding.  No frame is exempted: tests/test_pitch_ref.py proves every frame of these inputs
(pitch_ref.material and pitch_ref.extra_inputs) clear of a tie."""
import os

import numpy as np
import pytest

import pitch_ref as R
from test_pitch_ref import ALGORITHMS, CONF_FLOOR, CURVE_FLOOR, EDGE_BOUNDS, PITCH_FLOOR, shape_mags

pytestmark = pytest.mark.gpu

# 64 x the floor between two double STFTs on the CPU (tests/test_pitch_ref.py::test_floors_between_two_double_stfts), the factor
# the onset and novelty tests use: the device's log and cos differ from glibc's in the last places
CURVE_BAR = {a: 64 * v for a, v in CURVE_FLOOR.items()}
PITCH_BAR = {a: 64 * v for a, v in PITCH_FLOOR.items()}
CONF_BAR = {a: 64 * v for a, v in CONF_FLOOR.items()}
F32 = 2.0 ** -23   # one rounding to float32, relative
IDS = [str(s) for s in R.SHAPES]

_want = {}


def want_frames(shape, algorithm, **kw):
    key = (shape, algorithm, tuple(sorted(kw.items())))
    if key not in _want:
        mags, sr = shape_mags(shape)
        kw.setdefault("sr", sr)
        _want[key] = R.frames(mags, algorithm, **kw)
    return _want[key]


def check_frames(got, want, algorithm, extra=0.0, what=""):
    zero = want[:, 0] == 0
    pe = float((np.abs(got[:, 0] - want[:, 0]) / np.where(zero, 1.0, np.abs(want[:, 0]))).max())
    ce = float(np.abs(got[:, 1] - want[:, 1]).max())
    print(f"{what} algorithm {algorithm}: pitch {pe:.3e} (bar {PITCH_BAR[algorithm] + extra:.1e}), confidence {ce:.3e} "
          f"(bar {CONF_BAR[algorithm] + extra:.1e})")
    assert np.array_equal(got[:, 0] == 0, zero)
    assert pe <= PITCH_BAR[algorithm] + extra
    assert ce <= CONF_BAR[algorithm] + extra


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_curve_against_the_restatement(ctx, shape, algorithm):
    mags, sr = shape_mags(shape)
    got = ctx.pitch_curve(mags, algorithm, sample_rate=sr)[0]
    want = R.curves(mags, algorithm)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err = float(np.nanmax(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    print(f"{shape} algorithm {algorithm}: curve {err:.3e} (bar {CURVE_BAR[algorithm]:.1e})")
    assert err <= CURVE_BAR[algorithm]


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_frames_against_the_restatement(ctx, shape, algorithm):
    mags, sr = shape_mags(shape)
    got = ctx.pitch_frames(mags, algorithm, sample_rate=sr)[0]
    check_frames(got, want_frames(shape, algorithm), algorithm, what=str(shape))


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_bufpitch_against_the_restatement(ctx, shape, algorithm):
    x, sr = R.material(shape)
    win, fft, hop = shape
    got = ctx.bufpitch(x, algorithm, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    want = want_frames(shape, algorithm)
    assert got.shape == (2, len(want))
    check_frames(got.T.astype(np.float64), want, algorithm, extra=F32, what=f"{shape} f32")


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_a_batch_gives_the_bits_of_single_calls(ctx, algorithm):
    shape = (1500, 2048, 300)
    win, fft, hop = shape
    xs = np.stack([R.glide(14000, seed=s) for s in (9, 12, 14)])   # (seed 9 is the shape's material)
    batch = ctx.bufpitch(xs, algorithm, win=win, fft=fft, hop=hop)
    for b in range(3):
        assert np.array_equal(batch[b], ctx.bufpitch(xs[b], algorithm, win=win, fft=fft, hop=hop)[0])
    mags = np.stack([R.client_magnitudes(x, win, fft, hop) for x in xs])
    fb = ctx.pitch_frames(mags, algorithm)
    for b in range(3):
        assert np.array_equal(fb[b], ctx.pitch_frames(mags[b], algorithm)[0])


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_a_round_boundary_changes_no_bit(ab_ctx, algorithm):
    """the build with live switches cuts the frames into rounds of 7 (FLUHIP_PITCH_ROUND_FRAMES): frames on either side of a
    boundary equal those of a call without one"""
    x, _ = R.material((1001, 1024, 256))
    whole = ab_ctx.bufpitch(x, algorithm, win=1001, fft=1024, hop=256)
    os.environ["FLUHIP_PITCH_ROUND_FRAMES"] = "7"
    try:
        cut = ab_ctx.bufpitch(x, algorithm, win=1001, fft=1024, hop=256)
        cut3 = ab_ctx.bufpitch(np.stack([x, x, x]), algorithm, win=1001, fft=1024, hop=256)
    finally:
        del os.environ["FLUHIP_PITCH_ROUND_FRAMES"]
    assert whole.shape[2] > 14
    assert np.array_equal(whole, cut)
    assert all(np.array_equal(whole[0], cut3[b]) for b in range(3))


# ---- edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", (R.HPS, R.YINFFT))
def test_silence_is_exactly_zero(ctx, algorithm):
    # (the cepstrum of a constant log spectrum is rounding noise in every row but the first, in the reference too: its peaks
    # there are not a property to hold)
    z = np.zeros(6000, dtype=np.float32)
    for shape in ((256, 256, 64), (1024, 1024, 512)):
        win, fft, hop = shape
        hz = ctx.bufpitch(z, algorithm, win=win, fft=fft, hop=hop)[0]
        assert np.all(hz == 0) and hz.shape[0] == 2
        midi = ctx.bufpitch(z, algorithm, unit=1, win=win, fft=fft, hop=hop)[0]
        assert np.all(midi[0] == -999) and np.all(midi[1] == 0)
    assert np.all(ctx.pitch_frames(np.zeros((3, 513)), algorithm) == 0)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("bounds", EDGE_BOUNDS, ids=["min==max", "min0", "8k-clamps", "8k-empty"])
def test_frequency_bounds(ctx, algorithm, bounds):
    lo, hi, sr = bounds
    shape = (1024, 1024, 512)
    mags, _ = shape_mags(shape)
    got = ctx.pitch_frames(mags, algorithm, lo, hi, sr)[0]
    want = want_frames(shape, algorithm, min_freq=lo, max_freq=hi, sr=sr)
    check_frames(got, want, algorithm, what=f"bounds {bounds}")


def test_announced_errors_leave_the_context_usable(ctx):
    import fluhip
    x, _ = R.material((256, 256, 64))
    with pytest.raises(fluhip.FluhipError, match="8192"):
        ctx.bufpitch(R.tone(40000), R.CEPSTRUM, win=16384, fft=16384, hop=8192)
    with pytest.raises(fluhip.FluhipError, match="select"):
        ctx.bufpitch(x, R.YINFFT, select=0, win=256, fft=256, hop=64)
    with pytest.raises(fluhip.FluhipError, match="algorithm"):
        ctx.bufpitch(x, 3, win=256, fft=256, hop=64)
    with pytest.raises(fluhip.FluhipError, match="minFreq"):
        ctx.bufpitch(x, R.YINFFT, min_freq=500.0, max_freq=100.0, win=256, fft=256, hop=64)
    got = ctx.bufpitch(x, R.HPS, win=256, fft=256, hop=64)[0]
    check_frames(got.T.astype(np.float64), want_frames((256, 256, 64), R.HPS), R.HPS, extra=F32, what="after the errors")
    # YinFFT and HPS have no such limit
    assert ctx.bufpitch(R.tone(40000), R.YINFFT, win=16384, fft=16384, hop=8192).shape[1] == 2


@pytest.mark.parametrize("unit", (0, 1))
@pytest.mark.parametrize("select", (1, 2, 3))
def test_select_and_unit(ctx, select, unit):
    shape = (400, 512, 128)
    x, sr = R.material(shape)
    got = ctx.bufpitch(x, R.YINFFT, unit=unit, select=select, win=400, fft=512, hop=128, sample_rate=sr)[0]
    want = R.bufpitch(None, R.YINFFT, unit=unit, select=select, mags=shape_mags(shape)[0], sr=sr, as_double=True)
    assert got.shape == want.shape == (bin(select).count("1"), want.shape[1])
    # MIDI: 12 / ln 2 times the relative pitch error, far below the float32 rounding of values up to 140
    assert np.all(np.abs(got - want) <= 2 * F32 * np.maximum(1.0, np.abs(want)))


@pytest.mark.parametrize("padding_mode", (0, 1, 2))
@pytest.mark.parametrize("shape", [(400, 512, 128), (1024, 1024, 512), (1500, 2048, 300)], ids=str)
def test_padding_modes(ctx, shape, padding_mode):
    win, fft, hop = shape
    x = R.glide(9000, seed=21)
    got = ctx.bufpitch(x, R.HPS, win=win, fft=fft, hop=hop, padding_mode=padding_mode)[0]
    assert got.shape[1] == R.client_frames(len(x), win, hop, padding_mode)[1]
    want = R.frames(R.client_magnitudes(x, win, fft, hop, padding_mode), R.HPS)
    check_frames(got.T.astype(np.float64), want, R.HPS, extra=F32, what=f"{shape} padding {padding_mode}")


ON_CHIP = {(1024, 1024, 512), (1500, 2048, 300), (4096, 4096, 1024)}


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_plan(ctx, shape):
    win, fft, hop = shape
    # fft 1024 / 2048 / 4096 with an even window run the on-chip form in runs of 32 frames, every other shape the two-pass
    # form; YinFFT transforms twice; the cepstrum multiplies row 0 and the rows
    # [lrint(44100 / 10000), min(lrint(44100 / 20), nBins)) of its table
    form, run = (0, 32) if shape in ON_CHIP else (1, 0)
    rows = 1 + min(2205, fft // 2 + 1) - 4
    assert ctx.pitch_plan(fft, win, R.YINFFT) == (form, run, 2, 0)
    assert ctx.pitch_plan(fft, win, R.HPS) == (form, run, 1, 0)
    assert ctx.pitch_plan(fft, win, R.CEPSTRUM) == (form, run, 1, rows)
    # an odd window has no on-chip form at any size
    assert ctx.pitch_plan(fft, win - 1 if win % 2 == 0 else win, R.YINFFT)[:2] == ((form, run) if win % 2 else (1, 0))


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_a_run_boundary_changes_no_bit(ctx, algorithm):
    """the on-chip form hands runs of 32 frames to workgroups.  Frame t of the whole signal holds the samples
    [300 t - 750, 300 t + 750) (padding 1: win / 2 in front), so frame t of x[4800:12300] is frame t + 16 of x wherever the
    window touches no padding: frames 19 .. 38 of the long call, across the boundary at 32, against frames 3 .. 22 of a call
    of 26 frames, which has no boundary"""
    win, fft, hop = 1500, 2048, 300
    x, sr = R.material((win, fft, hop))
    long = ctx.bufpitch(x, algorithm, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    short = ctx.bufpitch(x[4800:12300], algorithm, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    assert ctx.pitch_plan(fft, win, algorithm)[:2] == (0, 32)
    assert long.shape[1] > 39 and short.shape[1] == 26
    assert np.array_equal(long[:, 19:39], short[:, 3:23])
    # and the boundary inside a batch, in a buffer that is not the first
    batch = ctx.bufpitch(np.stack([x[::-1], x]), algorithm, win=win, fft=fft, hop=hop, sample_rate=sr)
    assert np.array_equal(batch[1], long)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("shape", sorted(ON_CHIP), ids=str)
def test_the_two_pass_form_at_the_on_chip_sizes(ab_ctx, shape, algorithm):
    """FLUHIP_PITCH_FORM=1 (the build with live switches) sends an on-chip shape through the two-pass form: the same bars;
    and rounds of 7 frames cut the on-chip form's launches without changing a bit"""
    x, sr = R.material(shape)
    win, fft, hop = shape
    want = want_frames(shape, algorithm)
    chip = ab_ctx.bufpitch(x, algorithm, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    os.environ["FLUHIP_PITCH_ROUND_FRAMES"] = "7"
    try:
        cut = ab_ctx.bufpitch(x, algorithm, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    finally:
        del os.environ["FLUHIP_PITCH_ROUND_FRAMES"]
    assert np.array_equal(chip, cut)
    os.environ["FLUHIP_PITCH_FORM"] = "1"
    try:
        two = ab_ctx.bufpitch(x, algorithm, win=win, fft=fft, hop=hop, sample_rate=sr)[0]
    finally:
        del os.environ["FLUHIP_PITCH_FORM"]
    check_frames(two.T.astype(np.float64), want, algorithm, extra=F32, what=f"{shape} two-pass")
    check_frames(chip.T.astype(np.float64), want, algorithm, extra=F32, what=f"{shape} on-chip")


EXTRA_8K = [e for e in R.extra_inputs() if e[0].startswith("8k-")]


@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("case", EXTRA_8K, ids=[e[0] for e in EXTRA_8K])
def test_bufpitch_at_8_khz(ctx, case, algorithm):
    """the glide at 8 kHz through the client entry point: maxFreq beyond the sample rate (every clamp bites), minFreq 0, and
    minFreq == maxFreq"""
    _, x, shape, mode, lo, hi, sr = case
    win, fft, hop = shape
    got = ctx.bufpitch(x, algorithm, lo, hi, win=win, fft=fft, hop=hop, padding_mode=mode, sample_rate=sr)[0]
    want = R.frames(R.client_magnitudes(x, win, fft, hop, mode), algorithm, lo, hi, sr)
    check_frames(got.T.astype(np.float64), want, algorithm, extra=F32, what=case[0])


# ---- the C++ host client (include/flucoma_hip/PitchClient.hpp) through tests/cpp/pitch_driver.cpp ------------------------
@pytest.fixture(scope="module")
def pitch_driver(fluhip_lib_path):
    return R.build_driver()


def _run(driver, path, outp, n, chans, rate=44100.0, select=3, algorithm=2, lo=20.0, hi=10000.0, unit=0, win=1024, hop=512,
         fft=1024, padding=1, asynchronous=0):
    out = R.drive(driver, "run", path, n, chans, rate, select, algorithm, lo, hi, unit, win, hop, fft, padding, asynchronous, outp)
    return [l.split("|") for l in out.splitlines()]


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_cpp_client_against_the_restatement(ctx, pitch_driver, tmp_path, algorithm):
    shape = (1024, 1024, 512)
    x, sr = R.material(shape)
    xs = np.stack([x, x[::-1]])                                  # two channels
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    np.ascontiguousarray(xs.T).tofile(path)                      # the memory buffer is frames x channels
    for asynchronous in (0, 1):
        lines = _run(pitch_driver, path, outp, len(x), 2, sr, algorithm=algorithm, asynchronous=asynchronous)
        assert lines[-2] == ["run", "0", ""]
        T = len(want_frames(shape, algorithm))
        assert lines[-1][:4] == ["shape", "features", str(T), "4"] and float(lines[-1][4]) == sr / 512
        got = np.fromfile(outp, dtype=np.float32).reshape(4, T)   # feature i of channel j in buffer channel i + 2 j
        check_frames(got[:2].T.astype(np.float64), want_frames(shape, algorithm), algorithm, extra=F32, what="client ch 0")
        assert np.array_equal(got, ctx.bufpitch(xs, algorithm, win=1024, fft=1024, hop=512, sample_rate=sr).reshape(4, T))


def test_cpp_client_select_unit_and_announced_errors(ctx, pitch_driver, tmp_path):
    shape = (400, 512, 128)
    x, sr = R.material(shape)
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    x.tofile(path)
    lines = _run(pitch_driver, path, outp, len(x), 1, sr, select=2, unit=1, win=400, hop=128, fft=512)
    assert lines[-2] == ["run", "0", ""] and lines[-1][3] == "1"
    got = np.fromfile(outp, dtype=np.float32)
    assert np.array_equal(got, ctx.bufpitch(x, R.YINFFT, unit=1, select=2, win=400, fft=512, hop=128, sample_rate=sr)[0, 0])
    for kw, word in ((dict(select=0), "select"), (dict(algorithm=3), "algorithm"), (dict(lo=500.0, hi=100.0), "minFreq"),
                     (dict(algorithm=0, win=16384, hop=8192, fft=16384), "8192")):
        lines = _run(pitch_driver, path, outp, len(x), 1, sr, **kw)
        assert lines[-2][0] == "run" and lines[-2][1] == "2" and word in lines[-2][2], lines

