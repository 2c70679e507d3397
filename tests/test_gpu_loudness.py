"""GPU tests of BufLoudness through the C ABI, against tests/loudness_ref.py, the literal model of the reference's Loudness,
KWeightingFilter, TruePeak and LoudnessClient.  fluhip_loudness_frames_f64 pins the kernels apart from the wrapper on the cases
of loudness_ref.CASES; fluhip_bufloudness_f32 is held to the same bars plus one float32 rounding, and bit for bit to the frames
entry on its own padded rows.  The bar on every frame of every buffer, none exempted, is 64 x the stored floor of its case
(tests/test_loudness_ref.py FLOORS: the literal model in double against itself in long double)."""
import ctypes

import numpy as np
import pytest

import loudness_ref as L
from test_loudness_ref import floor_of

pytestmark = pytest.mark.gpu

FACTOR = 64          # the project's factor: the device's log10 and order of summation differ from glibc's and numpy's
F32 = 2.0 ** -23     # one rounding to float32, relative to the value
SWITCHES = [(1, 1), (1, 0), (0, 1), (0, 0)]
# loudness and peak of digital silence: 10 resp. 20 log10(epsilon); a few (4) ulp of log10(epsilon) = -15.65
SILENCE_BAR = 4 * np.spacing(15.65)


def check(got, want, name, kw, tp, what="", f32=False):
    """got, want [..., T, 2] in dB: every frame of every buffer under 64 x the floor of its case and column"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.shape[-1] == 2
    assert np.all(np.isfinite(got))
    for col, sw, label in ((0, kw, "loudness"), (1, tp, "peak")):
        bar = FACTOR * floor_of(name, col, sw)
        err = np.abs(got[..., col] - want[..., col])
        room = bar + (np.abs(want[..., col]) * F32 if f32 else 0.0)
        print(f"{what or name} kw {kw} tp {tp} {label}: {err.max():.3e} dB (bar {bar:.1e}{' + f32' if f32 else ''}), "
              f"{err.max() / floor_of(name, col, sw):.1f} floors")
        assert np.all(err <= room), (label, float(err.max()), bar)


# ---- the kernels, apart from the wrapper -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(L.CASES))
def test_frames_against_the_model(ctx, name):
    _, win, hop, T, sr = L.CASES[name]
    x = L.case_signals(name)
    got = ctx.loudness_frames(x, win, hop, 1, 1, sr)
    assert got.shape == (L.COUNT, T, 2)
    check(got, L.case_model(name, True, True), name, 1, 1)


@pytest.mark.parametrize("kw,tp", SWITCHES)
@pytest.mark.parametrize("name", ["noise_256_64", "sine_dc_5_2", "sine_dc_3_7", "noise_192k"])
def test_the_four_switch_combinations(ctx, name, kw, tp):
    _, win, hop, _, sr = L.CASES[name]
    got = ctx.loudness_frames(L.case_signals(name), win, hop, kw, tp, sr)
    want = np.stack([L.case_model(name, kw, kw)[..., 0], L.case_model(name, tp, tp)[..., 1]], axis=-1)
    check(got, want, name, kw, tp)
    if not kw:
        # the offset stays without the weighting (Loudness.hpp:55)
        ms = np.stack([[np.mean(np.square(x[j * hop:j * hop + win])) for j in range(got.shape[1])] for x in L.case_signals(name)])
        assert np.abs(got[..., 0] - (L.OFFSET + 10 * np.log10(ms + L.EPSILON))).max() < 1e-12


def test_the_first_frame_is_the_literal_recursion_s_own(ctx):
    # frame 0 enters with zero state and the kernel keeps processSample's order of operations: its filtered samples are the
    # model's to the bit, so its loudness differs by the order of summation and log10 alone
    name = "noise_1024_512"
    _, win, hop, _, sr = L.CASES[name]
    got = ctx.loudness_frames(L.case_signals(name)[0], win, hop, 1, 1, sr)[0, 0, 0]
    want = L.case_model(name, True, True)[0, 0, 0]
    assert abs(got - want) <= 8 * np.spacing(abs(want))


@pytest.mark.parametrize("sr,factor,history", [(44100.0, 4, 12), (96000.0, 2, 24), (192000.0, 1, 0), (8000.0, 4, 12),
                                               (88199.0, 4, 12), (88200.0, 2, 24), (176400.0, 1, 0)])
def test_plan_factor_by_sample_rate(ctx, sr, factor, history):
    form, run, f, h = ctx.loudness_plan(1024, 512, sr)
    assert (form, f, h) == (0, factor, history) and run >= 1
    assert L.interpolation_factor(sr) == factor and (L.ring_size(factor) - 1 if factor > 1 else 0) == history


@pytest.mark.parametrize("win,hop", [(1, 1), (5, 2), (3, 7), (256, 64), (1024, 512), (2048, 300), (32768, 8192)])
def test_plan_fits_a_workgroup_s_lds_at_every_window(ctx, win, hop):
    form, run, _, _ = ctx.loudness_plan(win, hop, 44100.0)
    assert form == 0 and 1 <= run <= 256
    # a workgroup stages run rows of min(win, 32) + 1 doubles, whatever the window: under the 64 KiB a workgroup may take
    assert run * (min(win, 32) + 1) * 8 <= 64 * 1024
    # ... and ctx may be NULL for the plan
    out = (ctypes.c_int64 * 4)()
    assert ctx.lib.fluhip_debug_loudness_plan(None, win, hop, 44100.0, out) == 0 and int(out[1]) == run
    assert ctx.lib.fluhip_debug_loudness_plan(None, 0, hop, 44100.0, out) == 2


# ---- the client's framing --------------------------------------------------------------------------------------------------
BUF_CASES = [("noise32_1024_512", 0), ("noise32_1024_512", 1), ("noise32_1024_512", 2), ("noise32_256_64", 1), ("sine_dc_256_64", 2),
             ("noise_2048_300", 1), ("sine_dc_2048_300", 2), ("noise_5_2", 0), ("sine_dc_5_2", 1), ("noise_5_2", 2), ("noise_1_1", 1),
             ("sine_dc_1_1", 2), ("noise_3_7", 0), ("sine_dc_3_7", 1), ("noise_32768_8192", 1), ("sine_dc_96k", 1), ("noise_192k", 1),
             ("sine_dc_8k", 0)]


def buf_audio(name):
    return L.case_signals(name).astype(np.float32)


def padded_rows(audio, win, hop, padding):
    """the rows the client's frames are cut from: [win + userPad zeros][input][zeros], frame j = row[j hop : j hop + win]"""
    pad, T, drop = L.control_geometry(audio.shape[1], win, hop, padding)
    rows = np.zeros((len(audio), max(win + pad + audio.shape[1], (T - 1) * hop + win)))
    rows[:, win + pad:win + pad + audio.shape[1]] = audio
    return rows[:, :(T - 1) * hop + win], drop


@pytest.mark.parametrize("name,padding", BUF_CASES, ids=[f"{n}-pad{p}" for n, p in BUF_CASES])
def test_bufloudness_against_the_model(ctx, name, padding):
    _, win, hop, _, sr = L.CASES[name]
    audio = buf_audio(name)
    got = ctx.bufloudness(audio, win=win, hop=hop, padding_mode=padding, sample_rate=sr)
    want = np.stack([L.bufloudness(a, win, hop, padding, 3, True, True, sr, as_double=True) for a in audio])
    assert got.shape == want.shape and got.dtype == np.float32
    # the material and (win, hop, sample rate) of the case, its frames moved by the padding: the case's floor, and the
    # rounding of the result to float32 on top (which is 1e-6 dB at 10 dB: the larger term everywhere but at win 1)
    check(got.transpose(0, 2, 1), want.transpose(0, 2, 1), name, 1, 1, what=f"{name} padding {padding} f32", f32=True)
    # ... and bit for bit what the frames entry gives on the padded rows, the latency frames run and then dropped
    rows, drop = padded_rows(audio, win, hop, padding)
    frames = ctx.loudness_frames(rows, win, hop, 1, 1, sr)
    assert np.array_equal(got, frames[:, drop:].transpose(0, 2, 1).astype(np.float32))


@pytest.mark.parametrize("kw,tp", SWITCHES)
def test_bufloudness_switches(ctx, kw, tp):
    name = "noise32_256_64"
    _, win, hop, _, sr = L.CASES[name]
    audio = buf_audio(name)
    got = ctx.bufloudness(audio, k_weighting=kw, true_peak=tp, win=win, hop=hop, sample_rate=sr)
    want = np.stack([L.bufloudness(a, win, hop, 1, 3, bool(kw), bool(tp), sr, as_double=True) for a in audio])
    check(got.transpose(0, 2, 1), want.transpose(0, 2, 1), name, kw, tp, what=f"{name} f32", f32=True)


@pytest.mark.parametrize("select", (1, 2, 3))
def test_select_and_the_size_query(ctx, select):
    name = "noise32_256_64"
    _, win, hop, _, sr = L.CASES[name]
    audio = buf_audio(name)
    both = ctx.bufloudness(audio, win=win, hop=hop, sample_rate=sr)
    got = ctx.bufloudness(audio, select=select, win=win, hop=hop, sample_rate=sr)
    cols = [c for c in (0, 1) if select >> c & 1]
    assert got.shape == (L.COUNT, len(cols), both.shape[2]) and np.array_equal(got, both[:, cols])
    for padding in (0, 1, 2):
        frames = ctypes.c_int64(-1)
        rc = ctx.lib.fluhip_bufloudness_f32(ctx.h, audio.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), L.COUNT, audio.shape[1], win, hop,
                                            padding, select, 1, 1, sr, None, ctypes.byref(frames))
        _, T, drop = L.control_geometry(audio.shape[1], win, hop, padding)
        assert rc == 0 and frames.value == T - drop


def test_digital_silence(ctx):
    got = ctx.loudness_frames(np.zeros((2, 4096)), 1024, 512)
    assert np.abs(got[..., 0] - (L.OFFSET + 10 * np.log10(L.EPSILON))).max() <= 10 * SILENCE_BAR
    assert np.abs(got[..., 1] - 20 * np.log10(L.EPSILON)).max() <= 20 * SILENCE_BAR
    buf = ctx.bufloudness(np.zeros(3000, dtype=np.float32))[0]
    assert np.all(buf[0] == np.float32(L.OFFSET + 10 * np.log10(L.EPSILON))) and np.all(buf[1] == np.float32(20 * np.log10(L.EPSILON)))


# ---- isolation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sine_dc_1024_512", "noise_5_2", "noise_3_7"])
def test_a_batch_gives_the_bits_of_single_calls(ctx, name):
    _, win, hop, _, sr = L.CASES[name]
    x = L.case_signals(name)
    x[1] *= 0.25                                         # (different content per buffer, and a different level)
    batch = ctx.loudness_frames(x, win, hop, 1, 1, sr)
    for b in range(L.COUNT):
        assert np.array_equal(batch[b], ctx.loudness_frames(x[b], win, hop, 1, 1, sr)[0])
    a32 = x.astype(np.float32)
    for padding in (0, 1):
        batch = ctx.bufloudness(a32, win=win, hop=hop, padding_mode=padding, sample_rate=sr)
        for b in range(L.COUNT):
            assert np.array_equal(batch[b], ctx.bufloudness(a32[b], win=win, hop=hop, padding_mode=padding, sample_rate=sr)[0])


# ---- announced errors ------------------------------------------------------------------------------------------------------
ERRORS = [(dict(win=0), "windowSize"), (dict(win=32769), "windowSize"), (dict(hop=0), "hopSize"), (dict(hop=-3), "hopSize"),
          (dict(k_weighting=2), "kWeighting"), (dict(k_weighting=-1), "kWeighting"), (dict(true_peak=2), "truePeak"),
          (dict(true_peak=-1), "truePeak"), (dict(sample_rate=0.0), "sample rate"), (dict(sample_rate=-44100.0), "sample rate"),
          (dict(sample_rate=float("inf")), "sample rate"), (dict(sample_rate=float("nan")), "sample rate")]


def test_announced_errors_leave_the_context_usable(ctx):
    import fluhip
    name = "noise32_256_64"
    audio = buf_audio(name)[0]
    for kw, word in ERRORS:
        with pytest.raises(fluhip.FluhipError, match=word):
            ctx.bufloudness(audio, **{"win": 256, "hop": 64, **kw})
        with pytest.raises(fluhip.FluhipError, match=word):
            ctx.loudness_frames(audio.astype(np.float64), **{"win": 256, "hop": 64, **kw})
        if "k_weighting" not in kw and "true_peak" not in kw:
            with pytest.raises(fluhip.FluhipError, match=word):
                ctx.loudness_plan(kw.get("win", 256), kw.get("hop", 64), kw.get("sample_rate", 44100.0))
    for select in (0, 4, -1):
        with pytest.raises(fluhip.FluhipError, match="select"):
            ctx.bufloudness(audio, select=select)
    for padding in (-1, 3):
        with pytest.raises(fluhip.FluhipError, match="padding"):
            ctx.bufloudness(audio, padding_mode=padding)
    with pytest.raises(fluhip.FluhipError, match="padding"):
        ctx.bufloudness(audio, win=3, hop=7, padding_mode=2)               # Full padding is win - hop samples
    with pytest.raises(fluhip.FluhipError, match="not enough frames"):
        ctx.loudness_frames(np.ones(100), win=256, hop=64)
    with pytest.raises(fluhip.FluhipError, match="not enough frames"):
        ctx.bufloudness(np.ones(10, dtype=np.float32), win=1000, hop=1000, padding_mode=0)   # one frame, and it is dropped
    # nothing was written by a refused call
    out = np.full((1, 2, 400), 7.0, dtype=np.float32)
    frames = ctypes.c_int64(-5)
    rc = ctx.lib.fluhip_bufloudness_f32(ctx.h, audio.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1, len(audio), 256, 64, 1, 3, 1, 2,
                                        44100.0, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(frames))
    assert rc == 2 and np.all(out == 7.0) and frames.value == -5
    got = ctx.bufloudness(buf_audio(name), win=256, hop=64)
    want = np.stack([L.bufloudness(a, 256, 64, 1, as_double=True) for a in buf_audio(name)])
    check(got.transpose(0, 2, 1), want.transpose(0, 2, 1), name, 1, 1, what="after the errors", f32=True)


# ---- the C++ host client (include/flucoma_hip/LoudnessClient.hpp) through tests/cpp/loudness_driver.cpp ---------------------
@pytest.fixture(scope="module")
def loudness_driver(fluhip_lib_path):
    return L.build_driver()


def _run(driver, path, outp, n, chans, rate, select=3, kw=1, tp=1, win=1024, hop=512, max_win=16384, padding=1, asynchronous=0):
    out = L.drive(driver, "run", path, n, chans, rate, select, kw, tp, win, hop, max_win, padding, asynchronous, outp)
    return [l.split("|") for l in out.splitlines()]


def test_cpp_client_against_the_c_abi(ctx, loudness_driver, tmp_path):
    name = "noise32_1024_512"
    _, win, hop, _, sr = L.CASES[name]
    xs = buf_audio(name)[:2, :20000].copy()                     # two channels of different content
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    np.ascontiguousarray(xs.T).tofile(path)                      # the memory buffer is frames x channels
    want = ctx.bufloudness(xs, win=win, hop=hop, sample_rate=sr)
    T = want.shape[2]
    model = np.stack([L.bufloudness(a, win, hop, 1, as_double=True) for a in xs])
    check(want.transpose(0, 2, 1), model.transpose(0, 2, 1), name, 1, 1, what="client material f32", f32=True)
    for asynchronous in (0, 1):
        lines = _run(loudness_driver, path, outp, xs.shape[1], 2, sr, asynchronous=asynchronous)
        assert lines[-2] == ["run", "0", ""]
        assert lines[-1][:4] == ["shape", "features", str(T), "4"] and float(lines[-1][4]) == sr / hop
        got = np.fromfile(outp, dtype=np.float32).reshape(4, T)   # feature i of channel j in buffer channel i + 2 j
        assert np.array_equal(got, want.reshape(4, T))
        # each channel is its own single call, bit for bit: no state passes between channels
        for c in range(2):
            assert np.array_equal(got[2 * c:2 * c + 2], ctx.bufloudness(xs[c], win=win, hop=hop, sample_rate=sr)[0])


def test_cpp_client_select_and_announced_errors(ctx, loudness_driver, tmp_path):
    x = buf_audio("sine_dc_2048_300")[0]
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    x.tofile(path)
    kw = dict(win=2048, hop=300, padding=2)
    lines = _run(loudness_driver, path, outp, len(x), 1, 96000.0, select=2, kw=0, tp=1, **kw)
    assert lines[-2] == ["run", "0", ""] and lines[-1][3] == "1" and float(lines[-1][4]) == 96000.0 / 300
    got = np.fromfile(outp, dtype=np.float32).reshape(1, -1)
    assert np.array_equal(got, ctx.bufloudness(x, 2, 0, 1, win=2048, hop=300, padding_mode=2, sample_rate=96000.0)[0])
    for args, word in ((dict(select=0), "select"), (dict(select=4), "select"), (dict(kw=2), "kWeighting"), (dict(tp=-1), "truePeak"),
                       (dict(hop=0), "hopSize"), (dict(win=0), "windowSize"), (dict(win=32768), "windowSize"),
                       (dict(max_win=1000), "maxWindowSize"), (dict(padding=3), "padding"), (dict(win=30000, hop=30000, max_win=32768, padding=0), "not enough frames")):
        lines = _run(loudness_driver, path, outp, len(x), 1, 44100.0, **{**kw, **args})
        assert lines[-2][0] == "run" and lines[-2][1] == "2" and word in lines[-2][2], lines
