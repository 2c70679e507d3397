"""A literal numpy / Python model of the reference's BufLoudness, for float64 and np.longdouble:
  algorithm::KWeightingFilter   include/flucoma/algorithms/util/KWeightingFilter.hpp:23-92
  algorithm::TruePeak           include/flucoma/algorithms/util/TruePeak.hpp:27-189 (impl::Interpolator, TruePeak)
  algorithm::Loudness           include/flucoma/algorithms/public/Loudness.hpp:43-61
  LoudnessClient                include/flucoma/clients/rt/LoudnessClient.hpp:77-126 behind StreamingControl::process,
                                clients/common/FluidNRTClientWrapper.hpp:551-660
What a tidy reader would write differently is kept and has a `variant` that tidies it (tests/test_loudness_ref.py shows that
each gives another answer):
  "filter_reset"     the K-weighting filter restarts from zero state in every frame (it never does: Loudness.hpp:53-54 calls
                     processSample on one filter object, and only Loudness::init resets it)
  "peak_filtered"    the peak is taken from the filtered frame (it is taken from the input: Loudness.hpp:56-57)
  "history_zeroed"   the interpolator's ring buffer is cleared before every frame (Interpolator::init alone clears it,
                     TruePeak.hpp:61-62; processFrame keeps mBuffer and mHead)
  "no_offset"        the -0.691 is dropped when kWeighting is off (Loudness.hpp:55 adds it either way)
  "latency_skipped"  (bufloudness only) the frames inside the client's latency are not run (StreamingControl runs every
                     frame, :607-634, and drops the first latency / hop results afterwards, :643-654)
The float64 model works on Python floats (IEEE doubles, one rounding per operation, the operations in the reference's order);
the long double model runs the same text on np.longdouble scalars, from the same double coefficients and samples.
"""
import math

import numpy as np

EPSILON = 2.220446049250313e-16      # util/AlgorithmUtils.hpp:19 (DBL_EPSILON)
OFFSET = -0.691                      # Loudness.hpp:55
TAPS = 49                            # TruePeak.hpp:147
VARIANTS = ("filter_reset", "peak_filtered", "history_zeroed", "no_offset", "latency_skipped")


# ---- KWeightingFilter ----------------------------------------------------------------------------------------------------
def kweighting_coefficients(sr):
    """KWeightingFilter::init :30-70: (mB[0..4], mA[0..4]) as Python floats; the shelving and the high-pass biquad multiplied
    out to one 5-tap direct-form-I recursion, every operation a double operation in the reference's order"""
    sr = float(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    sb = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    sa = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    hb = [1.0, -2.0, 1.0]
    ha = [1.0, 2.0 * (K * K - 1.0) / (1.0 + K / Q + K * K), (1.0 - K / Q + K * K) / (1.0 + K / Q + K * K)]
    b = [sb[0] * hb[0], sb[0] * hb[1] + sb[1] * hb[0], sb[0] * hb[2] + sb[1] * hb[1] + sb[2] * hb[0],
         sb[1] * hb[2] + sb[2] * hb[1], sb[2] * hb[2]]
    a = [sa[0] * ha[0], sa[0] * ha[1] + sa[1] * ha[0], sa[0] * ha[2] + sa[1] * ha[1] + sa[2] * ha[0],
         sa[1] * ha[2] + sa[2] * ha[1], sa[2] * ha[2]]
    return b, a


def _scalars(values, dtype):
    """a list of Python floats (float64) or of np.longdouble scalars"""
    if dtype == np.float64:
        return [float(v) for v in values]
    return [np.longdouble(v) for v in values]


def zero_state(dtype=np.float64):
    """mX[1..4], mY[0..3] (mX[0] is overwritten by every sample; mY[4] is never read): :71-75"""
    return _scalars([0.0] * 8, dtype)


def filter_run(x, state, b, a):
    """processSample :78-92 over the samples x (a list of scalars) from `state` = [mX[1..4], mY[0..3]]: returns the filtered
    samples and the state behind them.  y starts at 0, loses mA[i] mY[i - 1] for i = 1 .. 4, then gains mB[i] mX[i] for
    i = 0 .. 4, each a rounded operation"""
    x1, x2, x3, x4, y0, y1, y2, y3 = state
    b0, b1, b2, b3, b4 = b
    _, a1, a2, a3, a4 = a
    out = []
    zero = x1 * 0
    for x0 in x:
        y = zero
        y = y - a1 * y0
        y = y - a2 * y1
        y = y - a3 * y2
        y = y - a4 * y3
        y = y + b0 * x0
        y = y + b1 * x1
        y = y + b2 * x2
        y = y + b3 * x3
        y = y + b4 * x4
        x4, x3, x2, x1 = x3, x2, x1, x0
        y3, y2, y1, y0 = y2, y1, y0, y
        out.append(y)
    return out, [x1, x2, x3, x4, y0, y1, y2, y3]


# ---- TruePeak --------------------------------------------------------------------------------------------------------------
def interpolation_factor(sr):
    """TruePeak::init :160 and processFrame :171: 4 below 88200 Hz, 2 from there on; 1 = the interpolator is not run (176400
    Hz and above: the plain max |x|)"""
    if sr >= 4 * 44100:
        return 1
    return 4 if sr < 2 * 44100 else 2


def ring_size(factor):
    """Interpolator::init :58: mLatency = ceil(taps / factor): 13 at factor 4, 25 at factor 2"""
    return (TAPS + factor - 1) // factor


def interpolator_filters(factor):
    """Interpolator::init :68-86: per phase f the list of (delay, coefficient), in tap order; a 49-tap Hann-windowed sinc,
    taps with |c| <= 1e-6 dropped"""
    phases = [[] for _ in range(factor)]
    for i in range(TAPS):
        m = i - (TAPS - 1) / 2.0
        c = 1.0
        if abs(m) > 1e-6:
            c = math.sin(m * math.pi / factor) / (m * math.pi / factor)
        c *= 0.5 * (1 - math.cos(2 * math.pi * i / (TAPS - 1)))
        if abs(c) > 1e-6:
            phases[i % factor].append((i // factor, c))
    return phases


def _interpolated_peaks(stream, win, T, factor, dtype):
    """max |interpolated| per frame of a stream of T frames of win samples with ring - 1 samples of history in front.  The
    ring buffer holds the last `ring` samples fed, whatever frame they came from (Interpolator::processFrame :100-119): the
    output of phase f at stream sample p is sum_j stream[p - delay_j] c_j, accumulated in tap order"""
    hist = ring_size(factor) - 1
    peaks = np.zeros(T, dtype=dtype)
    pos = hist + np.arange(T * win)
    for taps in interpolator_filters(factor):
        acc = np.zeros(T * win, dtype=dtype)
        for d, c in taps:
            acc = acc + stream[pos - d] * dtype(c)
        peaks = np.maximum(peaks, np.abs(acc).reshape(T, win).max(axis=1))
    return peaks


def true_peaks(frames, sr, dtype=np.float64, variant=None):
    """TruePeak::processFrame over the frames [T, win] in order, the ring buffer carried: [T]"""
    frames = np.asarray(frames, dtype=dtype)
    T, win = frames.shape
    factor = interpolation_factor(sr)
    if factor == 1:
        return np.abs(frames).max(axis=1)
    hist = ring_size(factor) - 1
    if variant == "history_zeroed":
        return np.array([_interpolated_peaks(np.concatenate([np.zeros(hist, dtype=dtype), f]), win, 1, factor, dtype)[0]
                         for f in frames], dtype=dtype)
    stream = np.concatenate([np.zeros(hist, dtype=dtype), frames.reshape(-1)])
    return _interpolated_peaks(stream, win, T, factor, dtype)


# ---- Loudness ------------------------------------------------------------------------------------------------------------
def frame_count(n, win, hop):
    return 1 + (n - win) // hop if n >= win else 0


def loudness_frames(x, win, hop, k_weighting=True, true_peak=True, sr=44100.0, dtype=np.float64, variant=None):
    """Loudness::processFrame :43-61 on frame j = x[j hop : j hop + win], j = 0 .. (n - win) // hop, in order, on one Loudness
    object (init once): [T, 2] = (loudness, peak) in dB, in `dtype`"""
    x = np.asarray(x, dtype=np.float64)
    T = frame_count(len(x), win, hop)
    frames = np.stack([x[j * hop:j * hop + win] for j in range(T)]) if T else np.zeros((0, win))
    out = np.zeros((T, 2), dtype=dtype)
    b, a = kweighting_coefficients(sr)
    b, a = _scalars(b, dtype), _scalars(a, dtype)
    state = zero_state(dtype)
    eps = dtype(EPSILON)
    filtered = np.zeros((T, win), dtype=dtype)
    for j in range(T):
        if k_weighting:
            if variant == "filter_reset":
                state = zero_state(dtype)
            y, state = filter_run(_scalars(frames[j], dtype), state, b, a)
            filtered[j] = np.array(y, dtype=dtype)
        else:
            filtered[j] = frames[j]
    offset = dtype(0.0) if (variant == "no_offset" and not k_weighting) else dtype(OFFSET)
    out[:, 0] = offset + 10 * np.log10(np.mean(np.square(filtered), axis=1) + eps)
    src = filtered if variant == "peak_filtered" else frames
    if true_peak:
        peak = true_peaks(src, sr, dtype, variant)
    else:
        peak = np.abs(np.asarray(src, dtype=dtype)).max(axis=1) if T else np.zeros(0, dtype=dtype)
    out[:, 1] = 20 * np.log10(peak + eps)
    return out


# ---- LoudnessClient behind StreamingControl --------------------------------------------------------------------------------
def user_padding(win, hop, mode):
    """FluidNRTClientWrapper.hpp:393-418: 0 None, 1 Default win >> 1, 2 Full win - hop"""
    return 0 if mode == 0 else (win >> 1 if mode == 1 else win - hop)


def control_geometry(n, win, hop, mode):
    """StreamingControl::process :564-579, 643-644 with latency = windowSize (LoudnessClient.hpp:120): (userPad, analysis
    frames, dropped frames)"""
    pad = user_padding(win, hop, mode)
    padded = n + win + 2 * pad
    if mode == 2:
        padded = -(-padded // hop) * hop
    T = 1 + (padded - win) // hop
    return pad, T, win // hop


def bufloudness(audio, win=1024, hop=512, padding=1, select=3, k_weighting=True, true_peak=True, sr=44100.0,
                dtype=np.float64, variant=None, as_double=False):
    """NRTLoudnessClient on one mono buffer: [selected, frames] float32 (or `dtype` with as_double).  The host vector is one
    hop (:580); the buffered process fires one frame per vector, the window that ends where the vector begins
    (BufferedProcess.hpp:76-93 with mHostSize == hop), so analysis frame j holds samples j hop - win .. j hop of the padded
    signal, zeros in front; client.reset runs once per channel (:606), every frame is processed and moves both states, and
    the first win / hop results are dropped afterwards"""
    audio = np.asarray(audio, dtype=np.float64)
    pad, T, drop = control_geometry(len(audio), win, hop, padding)
    if pad < 0:
        raise ValueError("Full padding needs hop <= win")   # (the reference copies its input to a negative offset)
    if T - drop < 1:
        raise ValueError("not enough frames")
    row = np.zeros(max(win + pad + len(audio), (T - 1) * hop + win))
    row[win + pad:win + pad + len(audio)] = audio
    row = row[:(T - 1) * hop + win]
    if variant == "latency_skipped":
        res = loudness_frames(row[drop * hop:], win, hop, k_weighting, true_peak, sr, dtype)
    else:
        res = loudness_frames(row, win, hop, k_weighting, true_peak, sr, dtype, variant)[drop:]
    cols = [c for c in (0, 1) if select >> c & 1]
    out = res[:, cols].T
    return out if as_double else out.astype(np.float32)


# ---- the frame-parallel decomposition (what the device runs), restated -----------------------------------------------------
_transitions = {}


def frame_transition(win, sr):
    """M = A^win as an 8 x 8 list of Decimals of 32 digits (the precision of a double-double): the state [mX[1..4],
    mY[0..3]] behind a frame of zeros per unit of entering state, from the double coefficients; the one-sample map applied win
    times to every unit state"""
    from decimal import Decimal, localcontext
    key = (int(win), float(sr))
    if key not in _transitions:
        b, a = kweighting_coefficients(sr)
        with localcontext() as ctx:
            ctx.prec = 32
            b, a = [Decimal(v) for v in b], [Decimal(v) for v in a]
            zero = Decimal(0)
            cols = []
            for c in range(8):
                v = [zero] * 8
                v[c] = Decimal(1)
                for _ in range(win):
                    y = -a[1] * v[4] - a[2] * v[5] - a[3] * v[6] - a[4] * v[7] + b[1] * v[0] + b[2] * v[1] + b[3] * v[2] + b[4] * v[3]
                    v = [zero, v[0], v[1], v[2], y, v[4], v[5], v[6]]
                cols.append(v)
        _transitions[key] = [[cols[c][r] for c in range(8)] for r in range(8)]
    return _transitions[key]


def decomposed_loudness(x, win, hop, sr=44100.0, precision="dd"):
    """The K-weighted loudness of every frame as the device computes it: q_j, the state behind frame j run from zero state
    (plain double, frames independent); the entering states by the scan s_{j+1} = M s_j + q_j; every frame run again, in
    plain double, from its entering state rounded to double.  precision: "dd" M and the scan in 32 decimal digits (a
    double-double has 106 bits = 31.9 digits), "longdouble" both rounded to np.longdouble at every step, "double_m" the scan
    in long double on M rounded to double.  [T] float64"""
    from decimal import Decimal, localcontext
    x = np.asarray(x, dtype=np.float64)
    T = frame_count(len(x), win, hop)
    b, a = kweighting_coefficients(sr)
    M = frame_transition(win, sr)
    frames = [x[j * hop:j * hop + win].tolist() for j in range(T)]
    q = [filter_run(f, zero_state(), b, a)[1] for f in frames]
    out = np.zeros(T)

    def loudness(frame, state):
        y, _ = filter_run(frame, state, b, a)
        return OFFSET + 10 * np.log10(np.mean(np.square(np.array(y))) + EPSILON)

    if precision == "dd":
        with localcontext() as ctx:
            ctx.prec = 32
            s = [Decimal(0)] * 8
            for j in range(T):
                out[j] = loudness(frames[j], [float(v) for v in s])
                s = [sum((M[r][c] * s[c] for c in range(8)), Decimal(q[j][r])) for r in range(8)]
        return out
    Ml = np.array([[np.longdouble(str(m)) for m in row] for row in M], dtype=np.longdouble)
    if precision == "double_m":
        Ml = Ml.astype(np.float64).astype(np.longdouble)
    elif precision != "longdouble":
        raise ValueError(precision)
    s = np.zeros(8, dtype=np.longdouble)
    for j in range(T):
        out[j] = loudness(frames[j], [float(v) for v in s])
        s = Ml @ s + np.array(q[j], dtype=np.longdouble)
    return out


# ---- test material -----------------------------------------------------------------------------------------------------------
def material(kind, n, seed=0, sr=44100.0):
    """audible material only: "noise" (uniform, +-0.5), "sine_dc" (a 440 Hz sine of 0.25 on a DC offset of 0.7), "noise32"
    (float32-rounded noise)"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "noise":
        return rng.uniform(-0.5, 0.5, n)
    if kind == "noise32":
        return rng.uniform(-0.5, 0.5, n).astype(np.float32).astype(np.float64)
    if kind == "sine_dc":
        return 0.7 + 0.25 * np.sin(2 * np.pi * (440.0 + 37.0 * seed) * np.arange(n) / sr + 0.3 * seed)
    raise ValueError(kind)


# the cases the floors (tests/test_loudness_ref.py) and the device bars (tests/test_gpu_loudness.py) are taken on:
# name -> (material, win, hop, frames, sample rate); every case is three buffers (seeds 0, 1, 2) of (frames - 1) hop + win
# samples.  (1024, 512) has 300 frames so that the scan crosses several workgroup runs; (2048, 300) does not divide; (5, 2)
# and (1, 1) keep both histories across several frames; (3, 7) hops over samples; (32768, 8192) is the largest window
CASES = {}
for _kind in ("noise", "sine_dc", "noise32"):
    CASES[f"{_kind}_1024_512"] = (_kind, 1024, 512, 300, 44100.0)
    CASES[f"{_kind}_256_64"] = (_kind, 256, 64, 100, 44100.0)
for _kind in ("noise", "sine_dc"):
    CASES[f"{_kind}_2048_300"] = (_kind, 2048, 300, 40, 44100.0)
    CASES[f"{_kind}_5_2"] = (_kind, 5, 2, 200, 44100.0)
    CASES[f"{_kind}_1_1"] = (_kind, 1, 1, 300, 44100.0)
    CASES[f"{_kind}_3_7"] = (_kind, 3, 7, 100, 44100.0)
    CASES[f"{_kind}_32768_8192"] = (_kind, 32768, 8192, 3, 44100.0)
    CASES[f"{_kind}_96k"] = (_kind, 256, 64, 100, 96000.0)
    CASES[f"{_kind}_192k"] = (_kind, 256, 64, 100, 192000.0)
    CASES[f"{_kind}_8k"] = (_kind, 256, 64, 100, 8000.0)
COUNT = 3


def case_signals(name):
    """[COUNT, n] float64"""
    kind, win, hop, T, sr = CASES[name]
    return np.stack([material(kind, (T - 1) * hop + win, seed, sr) for seed in range(COUNT)])


_case_cache = {}


def case_model(name, k_weighting, true_peak, dtype=np.float64):
    """the literal model on every buffer of a case, [COUNT, T, 2]; computed once per process and never modified"""
    key = (name, bool(k_weighting), bool(true_peak), np.dtype(dtype).name)
    if key not in _case_cache:
        _, win, hop, _, sr = CASES[name]
        res = np.stack([loudness_frames(x, win, hop, k_weighting, true_peak, sr, dtype) for x in case_signals(name)])
        res.setflags(write=False)
        _case_cache[key] = res
    return _case_cache[key]


def build_driver():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fluhip_build_ld", os.path.join(root, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_loudness_driver()


def drive(driver, *args, timeout=300):
    import subprocess
    r = subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return r.stdout
