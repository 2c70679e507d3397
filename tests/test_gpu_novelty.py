"""GPU tests of BufNoveltySlice / BufNoveltyFeature through the C ABI, against tests/novelty_ref.py."""
import ctypes
import json
import os

import numpy as np
import pytest

import novelty_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CURVE_BAR = 1e-10    # absolute, on a normalised quantity: the bar of NMFCross's double results
TIE_GUARD = 1e-7     # 1e3 x CURVE_BAR: every comparison of every input used for detections is further from equality
# bufnoveltyfeature: 64 x the largest difference between the restatement on numpy's FFT and on the project's C oracle STFT
# over FEATURE_INPUTS (two independent double implementations of the same chain), measured by
# tests/test_novelty_ref.py::test_feature_floor_between_two_double_stfts
# measured: 3.731e-13.  The constant is that figure rounded UP to two digits (2 % above 64 x the measured floor): the CPU
# test asserts measured <= FEATURE_FLOOR on every host it runs on, and another libm / FFT build may differ in the last digits
FEATURE_FLOOR = 3.8e-13
FEATURE_BAR = 64 * FEATURE_FLOOR

CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "novelty_reference_cases.json")))["cases"]


def sweep_features(seed, T, D, zeros=True, scale=1.0):
    rng = np.random.default_rng(seed)
    X = np.abs(rng.standard_normal((T, D))) + 0.05 * rng.standard_normal((T, D))
    X *= (1.0 + np.sin(np.arange(T) / 7.0))[:, None] ** 2 + 0.1
    jump = rng.integers(0, 2, size=T).cumsum() % 3
    X += (jump[:, None] == (np.arange(D)[None, :] % 3)) * 1.5
    if zeros and T > 12:
        X[T // 2:T // 2 + 3] = 0.0
    return X * scale


SWEEP = [  # (seed, T, D, k, f)
    (1, 1, 13, 3, 1), (2, 2, 2, 9, 4), (3, 5, 40, 17, 1), (4, 20, 513, 31, 4), (5, 64, 13, 3, 1), (6, 97, 2, 9, 12),
    (7, 150, 40, 17, 4), (8, 300, 513, 3, 1), (9, 300, 1025, 31, 12), (10, 200, 513, 65, 4), (11, 130, 13, 65, 1),
    (12, 90, 40, 101, 4), (13, 240, 513, 101, 1), (14, 50, 13, 101, 12), (15, 333, 1025, 9, 1), (16, 30, 2, 3, 4),
]


@pytest.mark.parametrize("seed,T,D,k,f", SWEEP)
def test_curve_and_slices_against_the_restatement(ctx, seed, T, D, k, f):
    X = sweep_features(seed, T, D)
    want = R.curve_batch(X, k, f)
    thr = 0.05
    assert R.comparison_margins(want, thr).min() > TIE_GUARD
    det, counts, curve = ctx.novelty_slices(X, k, f, thr, 2)
    err = np.abs(curve[0] - want).max()
    print(f"novelty curve T={T} D={D} k={k} f={f}: max abs err {err:.3e}")
    assert err <= CURVE_BAR
    assert np.abs(ctx.novelty_curve(X, k, f)[0] - want).max() <= CURVE_BAR
    wd = R.peaks_batch(want, thr, 2)
    assert (det[0] == wd).all() and counts[0] == wd.sum()


def test_both_plan_forms_are_exercised(ctx):
    forms = {ctx.novelty_plan(T, D, k)[0] for _, T, D, k, _ in SWEEP}
    assert forms == {0, 1, 2}
    assert ctx.novelty_plan(300, 513, 65)[0] == 0 and ctx.novelty_plan(300, 513, 67)[0] == 2
    assert ctx.novelty_plan(300, 13, 17) == (1, 32, 16)


def test_curve_of_a_sixty_second_buffer(ctx):
    T, D = 5168, 513   # 60 s at 44.1 kHz, hop 512
    X = sweep_features(21, T, D)
    for k, f in ((3, 1), (31, 4)):
        err = np.abs(ctx.novelty_curve(X, k, f)[0] - R.curve_batch(X, k, f)).max()
        print(f"60 s buffer k={k}: {err:.3e}")
        assert err <= CURVE_BAR


@pytest.mark.parametrize("scale", [1e-300, 1e150])
def test_curve_at_the_ends_of_the_double_range(ctx, scale):
    for D, k in ((13, 9), (513, 9), (1025, 101)):
        X = sweep_features(31, 80, D, scale=scale)
        X[10:14] *= 1.0 / scale if scale > 1 else 1.0   # a few rows of ordinary size among them
        want = R.curve_batch(X, k, 1)
        assert np.isfinite(want).all()
        assert np.abs(ctx.novelty_curve(X, k, 1)[0] - want).max() <= CURVE_BAR


def test_strided_rows(ctx):
    big = np.zeros((120, 600))
    big[:, :513] = sweep_features(41, 120, 513)
    big[:, 513:] = 7.0   # must not be read
    X = big[:, :513]
    assert np.abs(ctx.novelty_curve(X, 17, 4)[0] - R.curve_batch(np.ascontiguousarray(X), 17, 4)).max() <= CURVE_BAR


@pytest.mark.parametrize("count,T,D,k,f", [(7, 90, 513, 17, 4), (128, 60, 13, 9, 1), (128, 40, 513, 3, 1), (7, 70, 40, 101, 4)])
def test_a_batch_gives_the_bits_of_single_calls(ctx, count, T, D, k, f):
    X = np.stack([sweep_features(100 + b, T, D) for b in range(count)])
    det, counts, curve = ctx.novelty_slices(X, k, f, 0.05, 3)
    for b in range(count):
        d1, c1, cu1 = ctx.novelty_slices(X[b], k, f, 0.05, 3)
        assert (cu1[0] == curve[b]).all() and (d1[0] == det[b]).all() and c1[0] == counts[b]
    for b in (0, count - 1):
        want = R.curve_batch(X[b], k, f)
        assert np.abs(curve[b] - want).max() <= CURVE_BAR
        assert (det[b] == R.peaks_batch(want, 0.05, 3)).all()


def _case_audio(case):
    if case["signal"] == "monoImpulses":
        return R.mono_impulses().astype(np.float32)
    return R.SIGNALS[case["signal"]]().astype(np.float32)[None]


@pytest.mark.parametrize("case", CASES, ids=[c["signal"] for c in CASES])
def test_reference_held_positions_through_the_c_abi(ctx, case):
    audio = _case_audio(case)
    got = ctx.bufnoveltyslice(audio, 0, case["kernelSize"], case["threshold"], case["filterSize"], case["minSliceLength"],
                              case["window"], case["fft"], case["hop"])[0]
    print(case["signal"], got)
    assert len(got) == len(case["expected"])
    assert np.abs(got - np.array(case["expected"])).max() <= case["margin"]


@pytest.mark.parametrize("case", CASES, ids=[c["signal"] for c in CASES])
def test_mfcc_positions_equal_the_restatement(ctx, case):
    audio = _case_audio(case)
    args = (1, case["kernelSize"], case["threshold"], case["filterSize"], case["minSliceLength"], case["window"],
            case["fft"], case["hop"])
    want = R.bufnoveltyslice(audio, *args)
    got = ctx.bufnoveltyslice(audio, *args)[0]
    assert list(got) == list(want)


def drum_loop():
    ref = np.load(os.path.join(ROOT, "tests", "golden", "reference_c1.npz"))
    return (ref["pcm16"].astype(np.float32) / 32768.0).astype(np.float32)


@pytest.mark.parametrize("algorithm,thr", [(0, 0.1), (1, 0.1)])
def test_drum_loop_positions_equal_the_restatement(ctx, algorithm, thr):
    x = drum_loop()[:88200]
    stereo = np.stack([x, 0.5 * np.roll(x, 3)]).astype(np.float32)
    want = R.bufnoveltyslice(stereo, algorithm, 9, thr, 4, 8, 1024, 1024, 512, start_frame=1234)
    got = ctx.bufnoveltyslice(stereo, algorithm, 9, thr, 4, 8, 1024, 1024, 512, start_frame=1234)[0]
    print(algorithm, got)
    assert list(got) == list(want) and len(got) > 1


FEATURE_INPUTS = [("sharpSines", 512, 1024, 256), ("smoothSine", 1024, 1024, 512), ("drums", 1024, 2048, 256)]


@pytest.mark.parametrize("algorithm", [0, 1])
@pytest.mark.parametrize("padding_mode", [0, 1, 2])
def test_bufnoveltyfeature_against_the_restatement(ctx, algorithm, padding_mode):
    for name, win, fft, hop in FEATURE_INPUTS:
        x = (drum_loop()[:30000] if name == "drums" else R.SIGNALS[name]()[:30000]).astype(np.float32)
        for k, f in ((3, 1), (17, 4)):
            want = R.bufnoveltyfeature(x, algorithm, k, f, win, fft, hop, padding_mode=padding_mode, as_double=True)
            got = ctx.bufnoveltyfeature(x, algorithm, k, f, win, fft, hop, padding_mode=padding_mode)[0]
            assert got.shape == want.shape
            # the float the client writes is the rounding of a double x with |x - want| <= FEATURE_BAR, so element by
            # element |got - want| <= FEATURE_BAR + |x| 2^-24 (half a float ulp; 2^-149 where floats are subnormal)
            err = np.abs(got.astype(np.float64) - want)
            allow = FEATURE_BAR + np.maximum((np.abs(want) + FEATURE_BAR) * 2.0 ** -24, 2.0 ** -149)
            same = int((got == want.astype(np.float32)).sum())
            print(f"bufnoveltyfeature {name} alg {algorithm} pad {padding_mode} k {k}: worst err / allowance "
                  f"{(err / allow).max():.3f}, {same} of {got.size} floats identical to the rounded restatement")
            assert (err <= allow).all()


def test_refusals_leave_the_output_untouched(ctx):
    lib, h = ctx.lib, ctx.h
    x = R.sharp_sines().astype(np.float32)
    i64p = ctypes.POINTER(ctypes.c_int64)
    fp = ctypes.POINTER(ctypes.c_float)

    def slice_call(algorithm=0, k=3, thr=0.5, f=1, ms=2):
        idx = np.full(64, -7, dtype=np.int64)
        cnt = np.full(1, -7, dtype=np.int64)
        rc = lib.fluhip_bufnoveltyslice_f32(h, x.ctypes.data_as(fp), 1, 1, len(x), 0, algorithm, k, thr, f, ms, 1024, 1024, 512,
                                            44100.0, idx.ctypes.data_as(i64p), 64, cnt.ctypes.data_as(i64p))
        return rc, lib.fluhip_last_error(h).decode(), idx, cnt

    for alg, name in ((2, "Chroma"), (3, "Pitch"), (4, "Loudness")):
        rc, msg, idx, cnt = slice_call(algorithm=alg)
        assert rc == 2 and name in msg and (idx == -7).all() and cnt[0] == -7
        out = np.full(100, -7, dtype=np.float32)
        T = ctypes.c_int64(-7)
        rc = lib.fluhip_bufnoveltyfeature_f32(h, x.ctypes.data_as(fp), 1, len(x), alg, 3, 1, 1024, 1024, 512, 44100.0, 1,
                                              out.ctypes.data_as(fp), ctypes.byref(T))
        assert rc == 2 and name in lib.fluhip_last_error(h).decode() and (out == -7).all() and T.value == -7
    for kw, word in ((dict(k=4), "kernelSize"), (dict(k=1), "kernelSize"), (dict(f=0), "filterSize"),
                     (dict(thr=-0.1), "threshold"), (dict(ms=-1), "minSliceLength")):
        rc, msg, idx, cnt = slice_call(**kw)
        assert rc == 2 and word in msg and (idx == -7).all() and cnt[0] == -7
    for kw, word in ((dict(f=(1 << 20) + 1), "filterSize"), (dict(f=1 << 32), "filterSize")):
        rc, msg, idx, cnt = slice_call(**kw)
        assert rc == 2 and word in msg and (idx == -7).all() and cnt[0] == -7
    # the algorithm-level entry points, with sentinel-filled outputs of the caller
    X = sweep_features(1, 20, 13)
    dp, u8p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ubyte)

    def curve_call(k=3, f=1, ld=13):
        curve = np.full(20, -7.0)
        rc = lib.fluhip_novelty_curve_f64(h, X.ctypes.data_as(dp), 1, 20, 13, ld, k, f, curve.ctypes.data_as(dp))
        return rc, lib.fluhip_last_error(h).decode(), curve

    def slices_call(k=3, f=1, thr=0.5, ms=2):
        curve = np.full(20, -7.0)
        det = np.full(20, 9, dtype=np.uint8)
        cnt = np.full(1, -7, dtype=np.int64)
        rc = lib.fluhip_novelty_slices_f64(h, X.ctypes.data_as(dp), 1, 20, 13, 13, k, f, thr, ms, det.ctypes.data_as(u8p),
                                           cnt.ctypes.data_as(i64p), curve.ctypes.data_as(dp))
        return rc, lib.fluhip_last_error(h).decode(), curve, det, cnt

    for kw, word in ((dict(k=4), "kernelSize"), (dict(k=1), "kernelSize"), (dict(f=0), "filterSize"), (dict(f=1 << 32), "filterSize"),
                     (dict(ld=12), "row stride")):
        rc, msg, curve = curve_call(**kw)
        assert rc == 2 and word in msg and (curve == -7.0).all()
    for kw, word in ((dict(k=6), "kernelSize"), (dict(f=-1), "filterSize"), (dict(thr=-1.0), "threshold"),
                     (dict(thr=float("nan")), "threshold"), (dict(ms=-1), "minSliceLength")):
        rc, msg, curve, det, cnt = slices_call(**kw)
        assert rc == 2 and word in msg and (curve == -7.0).all() and (det == 9).all() and cnt[0] == -7
    rc, msg, curve, det, cnt = slices_call()
    assert rc == 0 and (curve != -7.0).all() and (det <= 1).all() and cnt[0] == det.sum()


def test_silence_and_capacity(ctx):
    silence = np.zeros((2, 1, 20000), dtype=np.float32)
    assert [list(g) for g in ctx.bufnoveltyslice(silence, 0)] == [[-1], [-1]]
    # MFCC of silence is not a row of zeros (20 log10(eps) in every band): against the zeros the reference's ring of frames
    # starts with, the curve peaks at frame 1 (0.857 at the default kernel) and the wrapper reports that as one slice at
    # 0 -- the restatement of the reference says so, and the device says what the restatement says
    want = R.bufnoveltyslice(silence[0], 1)
    assert list(want) == [0]
    assert [list(g) for g in ctx.bufnoveltyslice(silence, 1)] == [[0], [0]]
    case = CASES[1]
    audio = _case_audio(case)
    got = ctx.bufnoveltyslice(audio, 0, 3, case["threshold"], 1, case["minSliceLength"], case["window"], case["fft"], case["hop"],
                              capacity=2)
    assert list(got[0]) == case["expected"][:2] and ctx.last_slice_counts[0] == 4
    # nothing is written past the capacity
    lib, h = ctx.lib, ctx.h
    idx = np.full(8, -7, dtype=np.int64)
    cnt = np.zeros(1, dtype=np.int64)
    a = np.ascontiguousarray(audio)
    rc = lib.fluhip_bufnoveltyslice_f32(h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1, 1, a.shape[1], 0, 0, 3,
                                        case["threshold"], 1, case["minSliceLength"], case["window"], case["fft"], case["hop"],
                                        44100.0, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 2,
                                        cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    assert rc == 0 and cnt[0] == 4 and list(idx[:2]) == case["expected"][:2] and (idx[2:] == -7).all()


def test_no_device_memory_is_left_behind_by_the_novelty_calls(ctx):
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value

    x = R.sharp_sines().astype(np.float32)[None]
    X = sweep_features(5, 200, 513)

    def once(i):
        ctx.bufnoveltyslice(x, i % 2, 9, 0.3, 4, 4, 1024, 1024, 512)
        ctx.bufnoveltyfeature(x[0], i % 2, 9, 4, 1024, 1024, 512)
        ctx.novelty_slices(X, 101 if i % 3 == 0 else 17, 4, 0.05, 2)

    for i in range(6):
        once(i)
    free0 = free_bytes()
    for i in range(200):
        once(i)
    free1 = free_bytes()
    print("device bytes free before / after 200 rounds:", free0, free1)
    assert free0 - free1 <= (8 << 20)


# ---- the C++ host clients (include/flucoma_hip/NoveltySliceClient.hpp) through tests/cpp/novelty_driver.cpp -------------
@pytest.fixture(scope="module")
def novelty_driver(fluhip_lib_path):
    return R.build_driver()


def _drive(driver, *args):
    return R.drive(driver, *args).splitlines()


@pytest.mark.parametrize("asynchronous", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=[c["signal"] for c in CASES])
def test_reference_held_positions_through_the_cpp_client(ctx, novelty_driver, tmp_path, case, asynchronous):
    audio = _case_audio(case)                                    # [channels, n]
    path = tmp_path / "in.f32"
    np.ascontiguousarray(audio.T).tofile(path)                   # the memory buffer is frames x channels
    out = _drive(novelty_driver, "slice", path, audio.shape[1], audio.shape[0], 44100, 0, 0, case["kernelSize"], case["threshold"],
                 case["filterSize"], case["minSliceLength"], case["window"], case["hop"], case["fft"], asynchronous)
    lines = [l for l in out if not l.startswith("process|")]
    assert lines[0] == "run|0|"
    assert lines[1] == f"shape|{len(case['expected'])}|1|44100"
    got = np.array([int(v) for v in lines[2:]])
    assert np.abs(got - np.array(case["expected"])).max() <= case["margin"]


def test_cpp_feature_client_equals_the_c_abi_and_names_the_missing_algorithms(ctx, novelty_driver, tmp_path):
    x = np.stack([R.sharp_sines()[:20000], R.smooth_sine()[:20000]]).astype(np.float32)
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    np.ascontiguousarray(x.T).tofile(path)
    out = _drive(novelty_driver, "feature", path, x.shape[1], 2, 44100, 1, 9, 4, 1024, 512, 1024, 2, outp)
    want = ctx.bufnoveltyfeature(x, 1, 9, 4, 1024, 1024, 512, padding_mode=2)
    assert out[0] == "run|0|" and out[1] == f"shape|{want.shape[1]}|2|{44100 / 512!r}"
    assert (np.fromfile(outp, dtype=np.float32).reshape(2, -1) == want).all()
    out = _drive(novelty_driver, "feature", path, x.shape[1], 2, 44100, 4, 9, 4, 1024, 512, 1024, 1, outp)
    assert out[0].startswith("run|2|") and "Loudness" in out[0]
    out = _drive(novelty_driver, "slice", path, x.shape[1], 2, 44100, 0, 2, 3, 0.5, 1, 2, 1024, 512, 1024, 0)
    assert out[0].startswith("run|2|") and "Chroma" in out[0]
