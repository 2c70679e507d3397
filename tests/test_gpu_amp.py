"""GPU tests of BufAmpSlice / BufAmpFeature through the C ABI, against tests/amp_ref.py, the literal model of the reference's
Envelope, EnvelopeSegmentation and the two clients.  Detections are demanded identical: every input they are compared on
comes from amp_ref's table, which tests/test_amp_ref.py holds clear of ties.  The envelope is held, per signal, to 64 x the
model's own double-against-long-double difference, in the maximum and in the median (one ill-conditioned zero crossing of the
filtered signal must not make the bar lax); the client adds one float32 rounding of the value."""
import ctypes

import numpy as np
import pytest

import amp_ref as A

pytestmark = pytest.mark.gpu

FACTOR = 64
F32 = 2.0 ** -24     # one rounding to the nearest float32, relative to the value
C = A.CHUNK
RAMPS = ("fast_up", "fast_down", "slow_up", "slow_down")


def env_args(p, sr=A.FS):
    return dict(fast_up=p["fast_up"], fast_down=p["fast_down"], slow_up=p["slow_up"], slow_down=p["slow_down"], floor=p["floor"],
                hipass=A.hipass_fraction(p["high_pass_freq"], sr))


def slice_args(p, sr=A.FS):
    return dict(env_args(p, sr), on=p["on"], off=p["off"], min_slice=p["min_slice"])


def client_args(p):
    return {k: p[k] for k in A.PARAM_NAMES}


def feature_args(p):
    return {k: p[k] for k in RAMPS + ("floor", "high_pass_freq")}


def device_positions(ctx, x, p):
    det, counts, env = ctx.amp_slices(x, **slice_args(p))
    pos = [np.flatnonzero(d).tolist() for d in det]
    assert [len(q) for q in pos] == counts.tolist()
    return pos, env


LEVEL_ULP = float(np.spacing(144.0))   # one rounding of a level in dB


def check_envelope(got, key, x, p, what, f32=False, short=False):
    """one signal's envelope under 64 x the model's own precision floor, maximum and median; prints the ratios.  short: a
    signal of a few samples, whose floor is the chance of those few roundings and can be far below one rounding of a level
    (the device's log10 is not libm's): there the floor is at least one unit in the last place of 144 dB"""
    want, fmax, fmed = A.precision_floor(key, x, p)
    if short:
        fmax, fmed = max(fmax, LEVEL_ULP), max(fmed, LEVEL_ULP)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape and np.all(np.isfinite(got))
    err = np.abs(got - want)
    room = np.abs(want) * F32 if f32 else 0.0
    over = err - room
    if fmax == 0.0:
        print(f"{what}: the model's two precisions agree to the bit; device max |diff| {err.max():.3e}")
        assert np.all(over <= 0.0)
        return
    shown = np.maximum(over, 0.0)   # (through float32: what is left over one rounding of the value)
    print(f"{what}: max {err.max():.3e} dB{', over the float32 rounding' if f32 else ''} = {shown.max() / fmax:.2f} F (F {fmax:.2e}), "
          f"median {np.median(err):.3e} dB = {np.median(shown) / fmed if fmed else np.inf:.2f} median F ({fmed:.2e})")
    assert np.all(over <= FACTOR * fmax), (what, float(err.max()), fmax)
    assert np.median(np.maximum(over, 0.0)) <= FACTOR * fmed, (what, float(np.median(err)), fmed)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def test_plan(ctx):
    assert ctx.amp_plan(85.0 / 44100.0) == (0, C, 32, 1)
    assert ctx.amp_plan(0.5) == (0, C, 32, 1)
    assert ctx.amp_plan(0.0) == (0, C, 32, 0)      # the high-pass is bypassed: no scan launches
    out = (ctypes.c_int64 * 4)()
    assert ctx.lib.fluhip_debug_amp_plan(None, 0.25, out) == 0 and list(out) == [0, C, 32, 1]   # ctx may be NULL
    assert ctx.lib.fluhip_debug_amp_plan(None, 0.75, out) != 0


# ---- the reference's own cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.reference_cases(), ids=lambda c: c[0])
def test_reference_cases_exactly(ctx, case):
    name, signal, p, expected, _ = case
    x = A.reference_signal(signal)
    pos, _ = device_positions(ctx, x, p)
    assert pos[0] == expected
    # the client at float input: the drum loop is 16-bit, the same signal; the synthetic ones give the model's list there
    x32 = x.astype(np.float32)
    got = ctx.bufampslice(x32, **client_args(p))[0].tolist()
    want = A.bufampslice(x32, p).tolist()
    assert got == want
    if signal == "monoDrums":
        assert got == expected


def test_drums_through_the_cpp_client(ctx, tmp_path):
    driver = A.build_driver()
    _, signal, p, expected, _ = A.reference_cases()[-1]
    x = A.reference_signal(signal).astype(np.float32)
    path = tmp_path / "drums.f32"
    x.tofile(path)
    for start, use_async in ((0, 0), (1000, 1)):
        out = A.drive(driver, "slice", path, len(x), 1, 44100, start, *[p[k] for k in A.PARAM_NAMES], use_async).splitlines()
        lines = [l for l in out if not l.startswith("process|")]
        assert lines[0] == "run|0|", lines[0]
        want = A.bufampslice(x[start:], p, start_frame=start).tolist()
        assert lines[1] == f"shape|{len(want)}|1|44100"
        assert [int(v) for v in lines[2:]] == want
        if start == 0:
            assert want == expected


def test_feature_through_the_cpp_client(ctx, tmp_path):
    driver = A.build_driver()
    x, p = A.detection_inputs()["client"]
    n = len(x)
    audio = np.stack([x, x[::-1], 0.5 * x]).astype(np.float32)            # [3, n]
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    np.ascontiguousarray(audio.T).tofile(path)                            # frames x chans
    fa = feature_args(p)
    lines = A.drive(driver, "feature", path, n, 3, 48000, *[fa[k] for k in RAMPS + ("floor", "high_pass_freq")], outp).splitlines()
    assert lines[0] == "run|0|" and lines[1] == f"shape|{n}|3|48000"
    got = np.fromfile(outp, dtype=np.float32).reshape(3, n)
    assert np.array_equal(got, ctx.bufampfeature(audio, sample_rate=48000.0, **fa)[0])


# ---- the envelope against the model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.envelope_inputs()))
def test_envelope_against_the_model(ctx, name):
    x, p = A.envelope_inputs()[name]
    assert len(x) <= 20000
    got = ctx.amp_envelope(x, **env_args(p))
    check_envelope(got[0], ("env", name), x, p, name)
    _, _, env = ctx.amp_slices(x, on=10.0, off=5.0, min_slice=2, **env_args(p))
    assert np.array_equal(env, got)                                       # the slicer's envelope is the feature's
    x32 = x.astype(np.float32)
    got32 = ctx.bufampfeature(x32, **feature_args(p))
    assert got32.dtype == np.float32 and got32.shape == (1, 1, len(x))
    check_envelope(got32[0, 0], ("env32", name), x32.astype(np.float64), p, name + " (client)", f32=True)


# ---- the smallest shapes that can break the kernels ---------------------------------------------------------------------------
SHAPE_PARAMS = A.params(fast_up=3, fast_down=40, slow_up=150, slow_down=150, on=12.0, off=6.0, floor=-70.0)


def shape_signals(count, n):
    # (from sample 300 on: inside the first burst of every seed, so that even one sample is not silence)
    return np.stack([A.bursts(n + 300, 100 + s)[300:] for s in range(count)])


@pytest.mark.parametrize("count", [1, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 2, C - 1, C, C + 1, 2 * C + 3])
def test_shapes(ctx, count, n):
    x = shape_signals(count, n)
    det, counts, env = ctx.amp_slices(x, **slice_args(SHAPE_PARAMS))
    assert det.shape == (count, n) and env.shape == (count, n) and np.all(det <= 1)
    assert counts.tolist() == det.sum(axis=1).tolist()
    for s in sorted({0, count - 1}):                                      # against the model
        check_envelope(env[s], ("shape", n, s), x[s], SHAPE_PARAMS, f"n {n} count {count} signal {s}", short=n < 64)
    for s in sorted({0, count // 2, count - 1}):                          # the batch gives the bits of single calls
        d1, c1, e1 = ctx.amp_slices(x[s], **slice_args(SHAPE_PARAMS))
        assert np.array_equal(e1[0], env[s]) and np.array_equal(d1[0], det[s]) and c1[0] == counts[s]
    assert np.array_equal(ctx.amp_envelope(x, **env_args(SHAPE_PARAMS)), env)


def test_a_batch_of_65_equals_65_single_calls(ctx):
    x, p = A.detection_inputs()["client"]
    n = len(x)
    rng = np.random.default_rng(5)
    audio = np.stack([np.roll(x, 37 * b) * (0.5 + 0.5 * rng.uniform()) for b in range(65)]).astype(np.float32)
    audio[0] = x
    det, counts, env = ctx.amp_slices(audio.astype(np.float64), **slice_args(p))
    idx = ctx.bufampslice(audio[:, None, :], **client_args(p))
    feat = ctx.bufampfeature(audio[:, None, :], **feature_args(p))
    assert idx[0].tolist() == A.bufampslice(audio[0], p).tolist()
    for b in range(65):
        d1, c1, e1 = ctx.amp_slices(audio[b].astype(np.float64), **slice_args(p))
        assert np.array_equal(e1[0], env[b]) and np.array_equal(d1[0], det[b]) and c1[0] == counts[b]
        i1 = ctx.bufampslice(audio[b], **client_args(p))[0]
        assert np.array_equal(i1, idx[b])
        assert np.array_equal(ctx.bufampfeature(audio[b], **feature_args(p))[0, 0], feat[b, 0])
        want = np.flatnonzero(det[b]) if counts[b] else np.array([-1])
        assert np.array_equal(idx[b], want)                               # the client's indices are the detector's


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_channels(ctx, channels):
    x, p = A.detection_inputs()["client"]
    x32 = x.astype(np.float32)
    want = A.bufampslice(x32, p, start_frame=3).tolist()
    assert want != [-1]
    # the slice client sums in float, in channel order, from 0: ((0 + 1e8) + -1e8) + x is x; any other order is not
    big = np.full_like(x32, 1e8)
    audio = {1: [x32], 2: [0.5 * x32, 0.5 * x32], 3: [big, -big, x32]}[channels]
    audio = np.stack(audio)
    assert np.array_equal(A.mono_sum(audio), x32)
    assert ctx.bufampslice(audio, start_frame=3, **client_args(p))[0].tolist() == want
    # the feature client keeps them apart: every channel is its own single call, bit for bit
    chans = np.stack([x32, x32[::-1], 0.25 * x32][:channels])
    got = ctx.bufampfeature(chans, **feature_args(p))
    assert got.shape == (1, channels, len(x))
    for c in range(channels):
        assert np.array_equal(got[0, c], ctx.bufampfeature(chans[c], **feature_args(p))[0, 0])
    check_envelope(got[0, channels - 1], ("chan", channels), chans[channels - 1].astype(np.float64), p, f"channel {channels - 1}",
                   f32=True)


# ---- parameters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in A.detection_inputs() if not k.startswith("f32_")])
def test_parameters_and_non_finite_samples(ctx, name):
    """every ramp at 1, ramps of 44 100, the high-pass off / at 1 Hz / at and above half the sample rate, floors -144 and -20,
    on < off, an on-threshold below 0, minSliceLength 0 / 2 / above n, silence, NaN and +-inf samples at the start, in the
    middle and across a chunk boundary: the model's indices, and its envelope under the bar"""
    x, p = A.detection_inputs()[name]
    want = A.slices(x, p)
    pos, env = device_positions(ctx, x, p)
    assert pos[0] == want
    check_envelope(env[0], ("detect", name), x, p, name)
    if name == "silence":
        assert want == [] and np.all(env == 0.0)
        assert ctx.bufampslice(x, **client_args(p))[0].tolist() == [-1]
    if name in ("hp_off", "nonfinite_hp_off"):
        assert ctx.amp_plan(A.hipass_fraction(p["high_pass_freq"]))[3] == 0
    if name.startswith("nonfinite"):
        assert not np.all(np.isfinite(x)) and want
        x32 = x.astype(np.float32)
        got = ctx.bufampfeature(x32, **feature_args(p))[0, 0]
        check_envelope(got, ("detect32", name), x32.astype(np.float64), p, name + " (client)", f32=True)


def test_start_frame_and_capacity(ctx):
    _, signal, p, expected, _ = A.reference_cases()[-1]
    x = A.reference_signal(signal).astype(np.float32)
    assert ctx.bufampslice(x, start_frame=77, **client_args(p))[0].tolist() == [e + 77 for e in expected]
    # a capacity below the true count: the count stays true, nothing is written past the capacity
    idx = np.full(8, -2, dtype=np.int64)
    counts = np.zeros(1, dtype=np.int64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    rc = ctx.lib.fluhip_bufampslice_f32(ctx.h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1, 1, len(x), 0, p["fast_up"],
                                        p["fast_down"], p["slow_up"], p["slow_down"], p["on"], p["off"], p["floor"], p["min_slice"],
                                        p["high_pass_freq"], 44100.0, idx.ctypes.data_as(i64p), 3, counts.ctypes.data_as(i64p))
    assert rc == 0 and counts[0] == len(expected) == 23
    assert idx.tolist() == expected[:3] + [-2] * 5
    rc = ctx.lib.fluhip_bufampslice_f32(ctx.h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 1, 1, len(x), 0, p["fast_up"],
                                        p["fast_down"], p["slow_up"], p["slow_down"], p["on"], p["off"], p["floor"], p["min_slice"],
                                        p["high_pass_freq"], 44100.0, None, 0, counts.ctypes.data_as(i64p))
    assert rc == 0 and counts[0] == 23                                    # the count alone


def test_sample_rate_scales_the_cutoff(ctx):
    x, p = A.detection_inputs()["client"]
    x32 = x.astype(np.float32)
    a = ctx.bufampfeature(x32, sample_rate=22050.0, **dict(feature_args(p), high_pass_freq=42.5))
    b = ctx.bufampfeature(x32, sample_rate=44100.0, **dict(feature_args(p), high_pass_freq=85.0))
    assert np.array_equal(a, b)
    assert not np.array_equal(a, ctx.bufampfeature(x32, sample_rate=44100.0, **dict(feature_args(p), high_pass_freq=42.5)))


# ---- errors --------------------------------------------------------------------------------------------------------------------
BAD = [(dict(fast_up=0), "fastRampUp"), (dict(fast_down=0), "fastRampDown"), (dict(slow_up=-1), "slowRampUp"),
       (dict(slow_down=0), "slowRampDown"), (dict(floor=-144.5), "floor"), (dict(floor=200.0), "floor"),
       (dict(floor=float("nan")), "floor")]
BAD_SLICE = BAD + [(dict(on=144.5), "onThreshold"), (dict(on=float("nan")), "onThreshold"), (dict(off=-145.0), "offThreshold"),
                   (dict(min_slice=-1), "minSliceLength")]
BAD_RATE = [(dict(high_pass_freq=-1.0), "highPassFreq"), (dict(high_pass_freq=float("inf")), "highPassFreq"),
            (dict(high_pass_freq=float("nan")), "highPassFreq"), (dict(sample_rate=0.0), "sample rate"),
            (dict(sample_rate=-44100.0), "sample rate"), (dict(sample_rate=float("inf")), "sample rate")]


def last_error(ctx):
    return ctx.lib.fluhip_last_error(ctx.h).decode()


def test_errors_are_announced_by_name_and_write_nothing(ctx):
    x = A.bursts(300, 1)
    dp, fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    i64p, u8p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_ubyte)
    L = ctx.lib
    x32 = x.astype(np.float32)
    base = dict(fast_up=1, fast_down=1, slow_up=100, slow_down=100, on=10.0, off=5.0, floor=-60.0, min_slice=2, hipass=0.002,
                high_pass_freq=85.0, sample_rate=44100.0, count=1, channels=1, n=300)

    def env_call(a, out):
        return L.fluhip_amp_envelope_f64(ctx.h, x.ctypes.data_as(dp), a["count"], a["n"], 300, a["fast_up"], a["fast_down"], a["slow_up"],
                                         a["slow_down"], a["floor"], a["hipass"], out.ctypes.data_as(dp))

    def slices_call(a, det, counts, env):
        return L.fluhip_amp_slices_f64(ctx.h, x.ctypes.data_as(dp), a["count"], a["n"], 300, a["fast_up"], a["fast_down"], a["slow_up"],
                                       a["slow_down"], a["on"], a["off"], a["floor"], a["min_slice"], a["hipass"],
                                       det.ctypes.data_as(u8p), counts.ctypes.data_as(i64p), env.ctypes.data_as(dp))

    def slice_client_call(a, idx, counts):
        return L.fluhip_bufampslice_f32(ctx.h, x32.ctypes.data_as(fp), a["count"], a["channels"], a["n"], 0, a["fast_up"],
                                        a["fast_down"], a["slow_up"], a["slow_down"], a["on"], a["off"], a["floor"], a["min_slice"],
                                        a["high_pass_freq"], a["sample_rate"], idx.ctypes.data_as(i64p), 4, counts.ctypes.data_as(i64p))

    def feature_client_call(a, out):
        return L.fluhip_bufampfeature_f32(ctx.h, x32.ctypes.data_as(fp), a["count"], a["channels"], a["n"], a["fast_up"],
                                          a["fast_down"], a["slow_up"], a["slow_down"], a["floor"], a["high_pass_freq"],
                                          a["sample_rate"], out.ctypes.data_as(fp))

    shape = [(dict(count=0), "count:"), (dict(n=0), "n:")]
    hip = [(dict(hipass=-0.1), "hipass"), (dict(hipass=0.6), "hipass"), (dict(hipass=float("nan")), "hipass")]
    chan = [(dict(channels=0), "channels:")]
    checked = 0
    for bad, name in BAD + hip + shape:
        out = np.full(300, 7.0)
        assert env_call(dict(base, **bad), out) != 0
        assert name in last_error(ctx) and np.all(out == 7.0), (bad, last_error(ctx))
        checked += 1
    for bad, name in BAD_SLICE + hip + shape:
        det, counts, env = np.full(300, 9, dtype=np.uint8), np.full(1, -7, dtype=np.int64), np.full(300, 7.0)
        assert slices_call(dict(base, **bad), det, counts, env) != 0
        assert name in last_error(ctx) and np.all(det == 9) and counts[0] == -7 and np.all(env == 7.0), (bad, last_error(ctx))
        checked += 1
    for bad, name in BAD_SLICE + BAD_RATE + shape + chan:
        idx, counts = np.full(4, -2, dtype=np.int64), np.full(1, -7, dtype=np.int64)
        assert slice_client_call(dict(base, **bad), idx, counts) != 0
        assert name in last_error(ctx) and np.all(idx == -2) and counts[0] == -7, (bad, last_error(ctx))
        checked += 1
    for bad, name in BAD + BAD_RATE + shape + chan:
        out = np.full(300, 7.0, dtype=np.float32)
        assert feature_client_call(dict(base, **bad), out) != 0
        assert name in last_error(ctx) and np.all(out == 7.0), (bad, last_error(ctx))
        checked += 1
    assert checked == 2 * len(BAD) + 2 * len(BAD_SLICE) + 2 * len(hip) + 4 * len(shape) + 2 * len(BAD_RATE) + 2 * len(chan)
    # and the same calls with nothing wrong succeed
    out = np.full(300, 7.0)
    assert env_call(base, out) == 0 and not np.any(out == 7.0)
