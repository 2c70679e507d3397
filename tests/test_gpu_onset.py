"""GPU tests of BufOnsetSlice / BufOnsetFeature through the C ABI, against tests/onset_ref.py and against the slice positions
the reference's own TestOnsetSegmentation.cpp asserts (tests/golden/onset_reference_cases.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import onset_ref as R
from test_onset_ref import (CURVE_FLOOR, DETECT_FILTERS, DETECT_MIN_SLICE, DETECT_THRESHOLDS, TIE_GUARD, detection_inputs,
                            filtered_allowance, floor_inputs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.gpu

# element-wise |got - want| / max(1, |want|) of the raw function value: 64 x the floor between two double STFTs on the CPU
# (tests/test_onset_ref.py::test_curve_floor_between_two_double_stfts), the factor the novelty tests use: the device's log,
# atan2 and sincos differ from glibc's in the last places
CURVE_BAR = {fn: 64 * v for fn, v in CURVE_FLOOR.items()}

CASES = json.load(open(os.path.join(GOLDEN, "onset_reference_cases.json")))["cases"]


def raw_err(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def filtered_ok(got, want_raw, want_filtered, bar):
    allow = filtered_allowance(want_raw, want_filtered, bar)
    return bool((np.abs(got - want_filtered) <= allow).all()), float((np.abs(got - want_filtered) / allow).max())


_signals = {}


def case_signal(name):
    if name not in _signals:
        _signals[name] = R.signal(name, GOLDEN)
    return _signals[name]


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_reference_held_positions_through_the_c_abi(ctx, case):
    """the acceptance: the reference's positions on the reference's audio out of the HIP path, under the harness framing"""
    z, T = R.harness_signal(case_signal(case["signal"]), case["window"], case["hop"])
    det, counts, _ = ctx.onset_slices(z, T, case["window"], case["fft"], case["hop"], case["metric"], case["filterSize"],
                                      case["frameDelta"], case["threshold"], case["minSliceLength"])
    got = R.harness_positions(det[0], case["hop"])
    print(case["label"], T, "frames", got[:6])
    assert counts[0] == det[0].sum()
    assert len(got) == len(case["expected"])
    if case["margin"] <= 1:
        assert got == case["expected"]
    else:
        assert np.abs(np.array(got) - np.array(case["expected"])).max() <= case["margin"]


@pytest.mark.parametrize("function", range(10))
def test_curves_against_the_restatement(ctx, function):
    """raw and filtered curves inside the bar, and detections IDENTICAL to the restatement's at the threshold whose distance
    from every frame tests/test_onset_ref.py::test_the_detection_thresholds_keep_clear_of_ties proves"""
    win, fft, hop = 512, 512, 128
    thr = DETECT_THRESHOLDS[function]
    for name, z, T, want_raw in detection_inputs(function):
        for fs in DETECT_FILTERS:
            raw, filt = ctx.onset_curve(z, T, win, fft, hop, function, fs)
            want_f = R.filter_curve(want_raw, fs)
            e = raw_err(raw[0], want_raw)
            ok, worst = filtered_ok(filt[0], want_raw, want_f, CURVE_BAR[function])
            print(f"onset curve {name} fn {function} fs {fs}: raw err {e:.3e} (bar {CURVE_BAR[function]:.3e}), "
                  f"filtered worst / allowance {worst:.3f}")
            assert e <= CURVE_BAR[function]
            assert ok
            det, counts, f2 = ctx.onset_slices(z, T, win, fft, hop, function, fs, 0, thr, DETECT_MIN_SLICE)
            wd = R.detect(want_f, thr, DETECT_MIN_SLICE)
            assert (f2[0] == filt[0]).all()
            assert (det[0] == wd).all() and counts[0] == wd.sum() and wd.sum() >= 1


@pytest.mark.parametrize("function", [2, 3, 4])
@pytest.mark.parametrize("delta", [1, 100, 700])
def test_frame_delta(ctx, function, delta):
    win, fft, hop = 1000, 1024, 220
    x = case_signal("monoDrums")[:40000]
    z, T = R.harness_signal(x, win, hop)
    want_raw, want_f = R.curve(z, T, win, fft, hop, function, 5, delta)
    raw, filt = ctx.onset_curve(z, T, win, fft, hop, function, 5, delta)
    e = raw_err(raw[0], want_raw)
    print(f"frame delta {delta} fn {function}: raw err {e:.3e} (bar {CURVE_BAR[function]:.3e})")
    assert ctx.onset_plan(fft, win, function, delta) == (0, 0, 2, 32)
    assert e <= CURVE_BAR[function]
    assert filtered_ok(filt[0], want_raw, want_f, CURVE_BAR[function])[0]
    assert not (raw[0] == ctx.onset_curve(z, T, win, fft, hop, function, 5, 0)[0][0]).all()   # the delta is used


def test_frame_delta_is_ignored_by_the_other_metrics(ctx):
    x = case_signal("monoDrums")[:20000]
    z, T = R.harness_signal(x, 512, 128)
    for function in (0, 1, 5, 6, 7, 8, 9):
        a = ctx.onset_curve(z, T, 512, 512, 128, function, 5, 0)
        b = ctx.onset_curve(z, T, 512, 512, 128, function, 5, 100)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


SMALL = [  # (win, fft, hop, T, n): sizes at which the code takes another path, and the smallest frame counts
    (4, 4, 1, 9, 12), (3, 4, 2, 5, 10), (64, 64, 1, 40, 103), (50, 64, 70, 7, 460), (512, 512, 128, 1, 600),
    (512, 512, 128, 2, 700), (512, 512, 128, 3, 800), (1000, 1024, 220, 17, 4000), (2048, 2048, 512, 9, 6000),
    (4096, 4096, 1024, 5, 8000), (8192, 8192, 2048, 4, 14000), (16384, 16384, 4096, 3, 30000), (300, 8192, 100, 5, 700),
    (512, 512, 128, 6, 100),   # a signal shorter than one window
]


@pytest.mark.parametrize("win,fft,hop,T,n", SMALL)
def test_smallest_shapes(ctx, win, fft, hop, T, n):
    rng = np.random.default_rng(win + fft + hop + T)
    z = 0.2 * rng.standard_normal(n)
    z[n // 2:] *= 3.0
    for function in range(10):
        want_raw, want_f = R.curve(z, T, win, fft, hop, function, 3)
        raw, filt = ctx.onset_curve(z, T, win, fft, hop, function, 3)
        e = raw_err(raw[0], want_raw)
        assert e <= CURVE_BAR[function], (function, e)
        assert filtered_ok(filt[0], want_raw, want_f, CURVE_BAR[function])[0], function


RUN = 32   # frames a workgroup of the on-chip form writes (fluhip_debug_onset_plan reports it)


@pytest.mark.parametrize("win,fft,hop", [(1000, 1024, 220), (2048, 2048, 300), (3000, 4096, 512)])
def test_runs_of_frames_behind_their_halo(ctx, win, fft, hop):
    """the on-chip form: T one below, at and one above a workgroup's run, and the same around two runs, for the metrics
    with no, one and two frames of history and for a frame delta; the frames in front of a run are recomputed"""
    rng = np.random.default_rng(fft)
    z = 0.3 * rng.standard_normal((2 * RUN + 1) * hop + win + 64)
    for function, delta in ((1, 0), (2, 0), (5, 0), (6, 0), (9, 0), (3, 37)):
        assert ctx.onset_plan(fft, win, function, delta)[0] == 0 and ctx.onset_plan(fft, win, function, delta)[3] == RUN
        want = R.raw_curve(z, 2 * RUN + 1, win, fft, hop, function, delta)
        for T in (RUN - 1, RUN, RUN + 1, 2 * RUN - 1, 2 * RUN, 2 * RUN + 1):
            raw = ctx.onset_curve(z, T, win, fft, hop, function, 1, delta)[0][0]
            assert raw_err(raw, want[:T]) <= CURVE_BAR[function], (function, T)


def test_rounds_of_frames_behind_their_halo(ctx):
    """the two-pass form: fft 65536 holds 2047 frames of spectra in a round; T at that number (one round) and one above it (a
    second round, which starts `history` frames below 2047 and recomputes them) for one and two frames of history.  The
    restatement is run on the first frames and on those around the end of the run only (a whole curve at this size is
    gigabytes on the host)."""
    win, fft, hop = 16, 65536, 3
    rows = (1 << 27) // (2 * (fft // 2 + 1))
    rng = np.random.default_rng(5)
    for function, history in ((2, 1), (8, 2)):
        assert ctx.onset_plan(fft, win, function)[:2] == (1, history)
        for T in (rows, rows + 1):
            z = 0.3 * rng.standard_normal(T * hop + win)
            raw = ctx.onset_curve(z, T, win, fft, hop, function, 1)[0][0]
            assert raw_err(raw[:4], R.raw_curve(z, 4, win, fft, hop, function)) <= CURVE_BAR[function]
            t0 = T - 6
            want = R.raw_curve(z[t0 * hop:], 6, win, fft, hop, function)[2:]   # (its first two frames lack their history)
            assert raw_err(raw[t0 + 2:], want) <= CURVE_BAR[function], (function, T)


def test_silence(ctx):
    z = np.zeros(5000)
    T = 30
    for function in range(10):
        want_raw, want_f = R.curve(z, T, 512, 512, 128, function, 5)
        raw, filt = ctx.onset_curve(z, T, 512, 512, 128, function, 5)
        assert np.isfinite(raw).all() and np.isfinite(filt).all()
        assert raw_err(raw[0], want_raw) <= CURVE_BAR[function]
        det, counts, _ = ctx.onset_slices(z, T, 512, 512, 128, function, 5, 0, 0.5, 2)
        assert det.sum() == 0 and counts[0] == 0
    silence = np.zeros((2, 1, 20000), dtype=np.float32)
    assert [list(g) for g in ctx.bufonsetslice(silence, 9, 0.1)] == [[-1], [-1]]


@pytest.mark.parametrize("count", [5, 64])
@pytest.mark.parametrize("function,delta", [(1, 0), (3, 0), (4, 50), (5, 0), (7, 0), (9, 0)])
def test_a_batch_gives_the_bits_of_single_calls(ctx, count, function, delta):
    x = case_signal("monoDrums")[:12000]
    z, T = R.harness_signal(x, 1000, 220)
    Z = np.stack([z] * count)
    raw, filt = ctx.onset_curve(Z, T, 1000, 1024, 220, function, 5, delta)
    r1, f1 = ctx.onset_curve(z, T, 1000, 1024, 220, function, 5, delta)
    assert (raw == r1[0][None]).all() and (filt == f1[0][None]).all()


def test_clients_against_the_wrapper_framings(ctx):
    drums = case_signal("monoDrums")[:60000].astype(np.float32)
    stereo = np.stack([drums, 0.5 * np.roll(drums, 3)]).astype(np.float32)
    imp = R.stereo_impulses().astype(np.float32)
    one = R.one_impulse().astype(np.float32)[None]
    # (audio, function, threshold, minSlice, filterSize, frameDelta, win, fft, hop)
    for audio, args in ((one, (0, 0.5, 2, 5, 0, 1024, 1024, 512)), (imp, (9, 0.1, 2, 5, 0, 512, 512, 64)),
                        (drums[None], (0, 0.5, 2, 5, 0, 1024, 1024, 512)), (stereo, (2, 0.2, 2, 5, 0, 1000, 1024, 220)),
                        (stereo, (3, 2.0, 2, 7, 300, 800, 1024, 330)), (stereo, (8, 0.1, 50, 5, 0, 512, 512, 50))):
        want, wf = R.bufonsetslice(audio, *args, start_frame=1234, want_filtered=True)
        assert np.abs(wf - args[1]).min() > TIE_GUARD
        got = ctx.bufonsetslice(audio, *args, start_frame=1234)[0]
        print("bufonsetslice", args, list(got)[:8])
        assert list(got) == list(want)
    assert abs(int(ctx.bufonsetslice(one, 0, 0.5, 2, 5, 0, 1024, 1024, 512)[0][0]) - 22050) <= 512
    for function, delta in ((0, 0), (2, 0), (4, 200), (6, 0), (9, 0)):
        for padding_mode in (0, 1, 2):
            want = R.bufonsetfeature(drums[:30000], function, 5, delta, 1000, 1024, 220, padding_mode, as_double=True)
            got = ctx.bufonsetfeature(drums[:30000], function, 5, delta, 1000, 1024, 220, padding_mode)[0]
            assert got.shape == want.shape
            raw = R.bufonsetfeature(drums[:30000], function, 1, delta, 1000, 1024, 220, padding_mode, as_double=True)
            # the float is the rounding of a double inside the filtered allowance: half a float ulp on top
            bar = CURVE_BAR[function]
            allow = bar * (np.maximum(1.0, np.abs(raw)) + np.maximum(1.0, np.abs(raw - want)))
            allow = allow + np.maximum((np.abs(want) + allow) * 2.0 ** -24, 2.0 ** -149)
            assert (np.abs(got.astype(np.float64) - want) <= allow).all(), (function, padding_mode)


def test_capacity_and_size_query(ctx):
    imp = R.stereo_impulses().astype(np.float32)
    args = (9, 0.1, 2, 5, 0, 512, 512, 64)
    full = ctx.bufonsetslice(imp, *args)[0]
    assert len(full) == 4
    got = ctx.bufonsetslice(imp, *args, capacity=2)[0]
    assert list(got) == list(full[:2]) and ctx.last_slice_counts[0] == 4
    lib, h = ctx.lib, ctx.h
    idx = np.full(8, -7, dtype=np.int64)
    cnt = np.zeros(1, dtype=np.int64)
    a = np.ascontiguousarray(imp)
    i64p, fp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float)
    rc = lib.fluhip_bufonsetslice_f32(h, a.ctypes.data_as(fp), 1, 2, a.shape[1], 0, 9, 0.1, 2, 5, 0, 512, 512, 64,
                                      idx.ctypes.data_as(i64p), 2, cnt.ctypes.data_as(i64p))
    assert rc == 0 and cnt[0] == 4 and list(idx[:2]) == list(full[:2]) and (idx[2:] == -7).all()
    x = a[0]
    T = ctypes.c_int64(-7)
    rc = lib.fluhip_bufonsetfeature_f32(h, x.ctypes.data_as(fp), 1, len(x), 0, 5, 0, 1024, 1024, 512, 1, None, ctypes.byref(T))
    assert rc == 0 and T.value == ctx.bufonsetfeature(x, 0, 5, 0, 1024, 1024, 512).shape[1]


def test_null_outputs(ctx):
    """either output of the curve call and the filtered output of the slices call may be NULL"""
    lib, h = ctx.lib, ctx.h
    dp, u8p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int64)
    z, T = R.harness_signal(case_signal("monoDrums")[:8000], 512, 128)
    raw, filt = ctx.onset_curve(z, T, 512, 512, 128, 8, 5)
    args = (h, z.ctypes.data_as(dp), 1, len(z), len(z), T, 512, 512, 128, 8, 5, 0)
    r1, f1 = np.full(T, -7.0), np.full(T, -7.0)
    assert lib.fluhip_onset_curve_f64(*args, r1.ctypes.data_as(dp), None) == 0 and (r1 == raw[0]).all()
    assert lib.fluhip_onset_curve_f64(*args, None, f1.ctypes.data_as(dp)) == 0 and (f1 == filt[0]).all()
    assert lib.fluhip_onset_curve_f64(*args, None, None) == 0
    det, cnt = np.full(T, 9, dtype=np.uint8), np.full(1, -7, dtype=np.int64)
    assert lib.fluhip_onset_slices_f64(*args, 0.1, 2, det.ctypes.data_as(u8p), cnt.ctypes.data_as(i64p), None) == 0
    want = ctx.onset_slices(z, T, 512, 512, 128, 8, 5, 0, 0.1, 2)
    assert (det == want[0][0]).all() and cnt[0] == want[1][0] and cnt[0] >= 1


def test_bad_parameters_are_errors_that_name_them(ctx):
    lib, h = ctx.lib, ctx.h
    z = np.zeros(4000)
    dp, u8p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_int64)
    fp = ctypes.POINTER(ctypes.c_float)
    x = np.zeros(4000, dtype=np.float32)

    def calls(fn=0, fs=5, d=0, win=512, fft=512, hop=128, thr=0.5, ms=2):
        raw, filt = np.full(10, -7.0), np.full(10, -7.0)
        det, cnt = np.full(10, 9, dtype=np.uint8), np.full(1, -7, dtype=np.int64)
        idx, out, T = np.full(16, -7, dtype=np.int64), np.full(64, -7, dtype=np.float32), ctypes.c_int64(-7)
        res = []
        rc = lib.fluhip_onset_curve_f64(h, z.ctypes.data_as(dp), 1, 4000, 4000, 10, win, fft, hop, fn, fs, d,
                                        raw.ctypes.data_as(dp), filt.ctypes.data_as(dp))
        res.append((rc, lib.fluhip_last_error(h).decode(), (raw == -7).all() and (filt == -7).all()))
        filt2 = np.full(10, -7.0)
        rc = lib.fluhip_onset_slices_f64(h, z.ctypes.data_as(dp), 1, 4000, 4000, 10, win, fft, hop, fn, fs, d, thr, ms,
                                         det.ctypes.data_as(u8p), cnt.ctypes.data_as(i64p), filt2.ctypes.data_as(dp))
        res.append((rc, lib.fluhip_last_error(h).decode(), (det == 9).all() and cnt[0] == -7 and (filt2 == -7).all()))
        cnt = np.full(1, -7, dtype=np.int64)
        rc = lib.fluhip_bufonsetslice_f32(h, x.ctypes.data_as(fp), 1, 1, 4000, 0, fn, thr, ms, fs, d, win, fft, hop,
                                          idx.ctypes.data_as(i64p), 16, cnt.ctypes.data_as(i64p))
        res.append((rc, lib.fluhip_last_error(h).decode(), (idx == -7).all() and cnt[0] == -7))
        rc = lib.fluhip_bufonsetfeature_f32(h, x.ctypes.data_as(fp), 1, 4000, fn, fs, d, win, fft, hop, 1, out.ctypes.data_as(fp),
                                            ctypes.byref(T))
        res.append((rc, lib.fluhip_last_error(h).decode(), (out == -7).all() and T.value == -7))
        return res

    for kw, word in ((dict(fn=-1), "function"), (dict(fn=10), "function"), (dict(fs=4), "filterSize"), (dict(fs=0), "filterSize"),
                     (dict(fs=103), "filterSize"), (dict(d=-1), "frameDelta"), (dict(d=8193), "frameDelta"),
                     (dict(fft=500), "fftSettings"), (dict(win=1024, fft=512), "fftSettings"), (dict(hop=0), "fftSettings"),
                     (dict(fft=1 << 17, win=512), "fftSettings")):
        for rc, msg, untouched in calls(**kw):
            assert rc == 2 and word in msg and untouched, (kw, msg)
    for kw, word in ((dict(thr=-0.5), "threshold"), (dict(ms=-1), "minSliceLength")):
        for rc, msg, untouched in calls(**kw)[1:3]:
            assert rc == 2 and word in msg and untouched, (kw, msg)
    out3 = (ctypes.c_int64 * 4)()
    assert lib.fluhip_debug_onset_plan(h, 512, 512, 11, 0, out3) == 2 and "function" in lib.fluhip_last_error(h).decode()
    assert all(rc == 0 for rc, _, _ in calls())


def test_the_plan_depends_on_the_four_arguments_only(ctx):
    # (form, history, transforms, run): the on-chip form where the on-chip FFT core is built, two passes elsewhere
    assert ctx.onset_plan(1024, 1024, 0) == (0, 0, 1, 32)
    assert ctx.onset_plan(1024, 1000, 2) == (0, 1, 1, 32) and ctx.onset_plan(1024, 1000, 2, 5) == (0, 0, 2, 32)
    assert ctx.onset_plan(2048, 2048, 5, 100) == (0, 1, 1, 32)
    assert ctx.onset_plan(4096, 4096, 9) == (0, 2, 1, 32) and ctx.onset_plan(8192, 8192, 9) == (1, 2, 1, 0)   # either side of the limit
    assert ctx.onset_plan(512, 512, 9) == (1, 2, 1, 0) and ctx.onset_plan(1024, 999, 9) == (1, 2, 1, 0)       # below it; an odd window
    assert ctx.onset_plan(16384, 16384, 9) == (1, 2, 1, 0)




# ---- the C++ host clients (include/flucoma_hip/OnsetSliceClient.hpp) through tests/cpp/onset_driver.cpp ----------------
@pytest.fixture(scope="module")
def onset_driver(fluhip_lib_path):
    return R.build_driver()


def _drive(driver, *args):
    return R.drive(driver, *args).splitlines()


def _client_audio(case):
    x = case_signal(case["signal"])
    if case["signal"] == "monoImpulses":
        return R.stereo_impulses().astype(np.float32)
    return x.astype(np.float32)[None]   # (the drum loop's 16-bit samples / 32768 are exact floats)


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_reference_held_positions_through_the_cpp_client(ctx, onset_driver, tmp_path, case):
    """every list of the reference out of the C++ client: under the wrapper's framing the frames and the latency correction are
    the harness's for frameDelta 0 or a metric that ignores it, which is every case of the fixture"""
    audio = _client_audio(case)                                  # [channels, n]
    path = tmp_path / "in.f32"
    np.ascontiguousarray(audio.T).tofile(path)                   # the memory buffer is frames x channels
    asynchronous = len(case["expected"]) % 2
    out = _drive(onset_driver, "slice", path, audio.shape[1], audio.shape[0], 44100, 0, case["metric"], case["threshold"],
                 case["minSliceLength"], case["filterSize"], case["frameDelta"], case["window"], case["hop"], case["fft"], asynchronous)
    lines = [l for l in out if not l.startswith("process|")]
    assert lines[0] == "run|0|"
    assert lines[1] == f"shape|{len(case['expected'])}|1|44100"
    got = [int(v) for v in lines[2:]]
    if case["margin"] <= 1:
        assert got == case["expected"]
    else:
        assert np.abs(np.array(got) - np.array(case["expected"])).max() <= case["margin"]


def test_cpp_feature_client_equals_the_c_abi(ctx, onset_driver, tmp_path):
    d = case_signal("monoDrums")
    x = np.stack([d[:20000], d[30000:50000]]).astype(np.float32)
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    np.ascontiguousarray(x.T).tofile(path)
    for metric, delta, pad in ((4, 200, 2), (9, 0, 1)):
        out = _drive(onset_driver, "feature", path, x.shape[1], 2, 44100, metric, 7, delta, 1000, 220, 1024, pad, outp)
        want = ctx.bufonsetfeature(x, metric, 7, delta, 1000, 1024, 220, padding_mode=pad)
        assert out[0] == "run|0|" and out[1] == f"shape|{want.shape[1]}|2|{44100 / 220!r}"
        assert (np.fromfile(outp, dtype=np.float32).reshape(2, -1) == want).all()
