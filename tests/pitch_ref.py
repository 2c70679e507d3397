"""Restatement of the reference's pitch analysis in numpy, line by line:

    algorithm::YINFFT         include/flucoma/algorithms/public/YINFFT.hpp:33-91
    algorithm::HPS            include/flucoma/algorithms/public/HPS.hpp:25-67
    algorithm::CepstrumF0     include/flucoma/algorithms/public/CepstrumF0.hpp:44-75  (DCT.hpp:36-62)
    algorithm::PeakDetection  include/flucoma/algorithms/util/PeakDetection.hpp:30-71
    client::pitch::PitchClient  include/flucoma/clients/rt/PitchClient.hpp:93-150 behind StreamingControl

The reference's behaviour is kept, not tidied: HPS multiplies three factors (its loop stops before nHarmonics = 4), YinFFT
clamps maxBin to size - minBin - 1, the DCT's row 0 has its own scale.  Two places where the reference reads past an array
or rounds an unbounded quotient are defined here (and in the device code) instead: HPS searches [minBin, min(maxBin,
nBins)), and sr / freq at or beyond nBins counts as nBins before lrint.  std::sort leaves equal peak heights in
unspecified order; here the lowest index leads.  Comparisons are IEEE: a NaN fails them all.
"""
import numpy as np

EPSILON = np.finfo(np.float64).eps          # util/AlgorithmUtils.hpp:19
CEPSTRUM, HPS, YINFFT = 0, 1, 2
CEPSTRUM_MAX_FFT = 8192


def _bin(q, n_bins):
    return n_bins if not (q < n_bins) else int(np.rint(q))


def bins(algorithm, n_bins, min_freq, max_freq, sr, yin_clamp=True):
    if algorithm == YINFFT:
        max_freq = 1 if max_freq == 0 else max_freq
        min_freq = 1 if min_freq == 0 else min_freq
        lo, hi = _bin(sr / max_freq, n_bins), _bin(sr / min_freq, n_bins)
        lo = min(lo, n_bins - 1)
        hi = min(hi, n_bins - lo - 1) if yin_clamp else min(hi, n_bins)
        return lo, hi
    if algorithm == HPS:
        bin_hz = sr / ((n_bins - 1) * 2)
        return _bin(min_freq / bin_hz, n_bins), _bin(max_freq / bin_hz, n_bins)
    with np.errstate(divide="ignore"):
        return _bin(np.float64(sr) / max_freq, n_bins), _bin(np.float64(sr) / min_freq, n_bins)


def peaks(seg):
    """PeakDetection::process(seg, 1, seg.minCoeff(), interpolate, sort): every (position, height), highest first (equal
    heights: lowest index first)"""
    seg = np.asarray(seg, dtype=np.float64)
    if len(seg) < 3:
        return []
    with np.errstate(invalid="ignore", divide="ignore"):
        mn = np.fmin.reduce(seg)
        cur, prev, nxt = seg[1:-1], seg[:-2], seg[2:]
        idx = np.flatnonzero((cur > prev) & (cur > nxt) & (cur > mn))
        c, p, n = cur[idx], prev[idx], nxt[idx]
        q = 0.5 * (p - n) / (p - 2 * c + n)
        h = c - 0.25 * (p - n) * q
    order = np.argsort(-h, kind="stable")
    return [(float(idx[k] + 1 + q[k]), float(h[k])) for k in order]


def yin_curve(mag):
    """the normalised yin of one frame and the final running sum"""
    mag = np.asarray(mag, dtype=np.float64)
    n_bins = len(mag)
    sq = mag * mag
    sym = np.concatenate([sq[:1], sq[1:n_bins], sq[1:n_bins - 1][::-1]])
    yin = 2 * sq.sum() - np.fft.fft(sym).real[:n_bins]
    yin[0] = 1
    run = np.cumsum(np.concatenate([[0.0], yin[1:]]))
    with np.errstate(invalid="ignore", divide="ignore"):
        yin[1:] = yin[1:] * (np.arange(1, n_bins) / run[1:])
    return yin, run[-1]


def yinfft(mag, min_freq, max_freq, sr, clamp=True, want_peaks=False):
    yin, tmp_sum = yin_curve(mag)
    pitch = conf = 0.0
    pk = []
    if tmp_sum > 0:
        lo, hi = bins(YINFFT, len(yin), min_freq, max_freq, sr, clamp)
        if hi > lo:
            pk = peaks(-yin[lo:hi])
            if pk:
                pitch = sr / (lo + pk[0][0])
                conf = max(1.0 + pk[0][1], 0.0)
    return (pitch, conf, pk) if want_peaks else (pitch, conf)


def hps_curve(mag, n_harmonics=4):
    mag = np.asarray(mag, dtype=np.float64)
    n_bins = len(mag)
    hps = mag.copy()
    for i in range(2, n_harmonics):
        hb = n_bins // i
        hp = np.zeros(n_bins)
        hp[:hb] = mag[np.arange(hb) * i]
        hps = hps * hp
    return hps


def hps(mag, min_freq, max_freq, sr, n_harmonics=4):
    curve = hps_curve(mag, n_harmonics)
    n_bins = len(curve)
    lo, hi = bins(HPS, n_bins, min_freq, max_freq, sr)
    total = curve.sum()
    hi = min(hi, n_bins)
    if hi > lo and total > 0:
        i = int(np.argmax(curve[lo:hi]))
        return (lo + i) * (sr / ((n_bins - 1) * 2)), curve[lo + i] / total
    return 0.0, 0.0


_tables = {}


def dct_table(n, row0_like_others=False):
    key = (n, row0_like_others)
    if key not in _tables:
        t = np.empty((n, n))
        pts = np.linspace(0.5, n - 0.5, n)
        for i in range(n):
            scale = 1.0 / np.sqrt(n) if (i == 0 and not row0_like_others) else np.sqrt(2.0 / n)
            t[i] = np.cos(((np.pi / n) * i) * pts) * scale
        _tables[key] = t
    return _tables[key]


def cepstrum_curve(mag, row0_like_others=False):
    lg = np.log(np.maximum(np.asarray(mag, dtype=np.float64), EPSILON))
    return dct_table(len(lg), row0_like_others) @ lg


def cepstrum(mag, min_freq, max_freq, sr, row0_like_others=False, want_peaks=False):
    cep = cepstrum_curve(mag, row0_like_others)
    lo, hi = bins(CEPSTRUM, len(cep), min_freq, max_freq, sr)
    pitch = conf = 0.0
    pk = []
    if hi > lo:
        pk = peaks(cep[lo:hi])
        if pk:
            pitch = sr / (pk[0][0] + lo)
            conf = pk[0][1] / cep[0]
    out = (pitch, min(abs(conf), 1.0))
    return out + (pk,) if want_peaks else out


def frame(mag, algorithm, min_freq=20.0, max_freq=10000.0, sr=44100.0):
    if algorithm == CEPSTRUM:
        return cepstrum(mag, min_freq, max_freq, sr)
    if algorithm == HPS:
        return hps(mag, min_freq, max_freq, sr)
    if algorithm == YINFFT:
        return yinfft(mag, min_freq, max_freq, sr)
    raise ValueError("algorithm")


def frames(mags, algorithm, min_freq=20.0, max_freq=10000.0, sr=44100.0):
    """[T, F] magnitudes -> [T, 2] (pitch in Hz, confidence)"""
    return np.array([frame(m, algorithm, min_freq, max_freq, sr) for m in mags]).reshape(len(mags), 2)


def curves(mags, algorithm):
    if algorithm == CEPSTRUM:
        return np.array([cepstrum_curve(m) for m in mags])
    if algorithm == HPS:
        return np.array([hps_curve(m) for m in mags])
    return np.array([yin_curve(m)[0] for m in mags])


def lead(mag, algorithm, min_freq=20.0, max_freq=10000.0, sr=44100.0):
    """how far the best candidate of a frame leads its runner-up: the difference of interpolated peak heights (YinFFT,
    Cepstrum), the relative difference of bin values (HPS); inf with fewer than two candidates"""
    if algorithm == HPS:
        curve = hps_curve(mag)
        lo, hi = bins(HPS, len(curve), min_freq, max_freq, sr)
        seg = np.sort(curve[lo:min(hi, len(curve))])[::-1]
        if len(seg) < 2 or not curve.sum() > 0:
            return np.inf
        return (seg[0] - seg[1]) / seg[0]
    pk = (yinfft if algorithm == YINFFT else cepstrum)(mag, min_freq, max_freq, sr, want_peaks=True)[2]
    return np.inf if len(pk) < 2 else pk[0][1] - pk[1][1]


# ---- the client ------------------------------------------------------------------------------------------------------
def to_unit(x, unit):
    x = np.asarray(x, dtype=np.float64)
    if unit == 0:
        return x
    with np.errstate(divide="ignore"):
        return np.where(x == 0, -999.0, 69 + 12 * np.log2(np.where(x == 0, 1.0, x) / 440.0))


def hann(win):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)   # alg/WindowFuncs.hpp:41-45


def client_frames(n, win, hop, padding_mode):
    """(first sample of kept frame 0 in the input's coordinates, kept frames): StreamingControl::process with latency win"""
    pad = (0, win >> 1, win - hop)[padding_mode]
    padded = n + win + 2 * pad
    if padding_mode == 2:
        padded = -(-padded // hop) * hop
    drop = win // hop
    return drop * hop - win - pad, 1 + (padded - win) // hop - drop


def client_magnitudes(audio, win, fft, hop, padding_mode=1, stft=None):
    """[T, F] magnitudes of the frames the client keeps.  stft: None = numpy's FFT; else a callable (signal, win, fft, hop)
    -> (spec, mag) whose frame t starts at t hop - win // 2 (the project's C oracle), fed with the signal moved by whole
    hops"""
    x = np.asarray(audio, dtype=np.float32).astype(np.float64)
    start, T = client_frames(len(x), win, hop, padding_mode)
    # z: kept frame t = z[t hop, t hop + win)
    z = np.concatenate([np.zeros(max(0, -start)), x[max(0, start):]])
    z = np.concatenate([z, np.zeros(max(0, (T - 1) * hop + win - len(z)))])
    if stft is not None:
        s = -(-(win // 2) // hop)
        y = np.concatenate([np.zeros(s * hop - win // 2), z, np.zeros(hop + win)])
        return np.ascontiguousarray(stft(y, win, fft, hop)[1][s:s + T])
    fr = np.stack([z[t * hop: t * hop + win] for t in range(T)]) * hann(win)
    return np.abs(np.fft.rfft(fr, fft, axis=1))


def bufpitch(audio, algorithm=2, min_freq=20.0, max_freq=10000.0, unit=0, select=3, win=1024, fft=1024, hop=512,
             padding_mode=1, sr=44100.0, as_double=False, mags=None):
    """NRTPitchClient on one float32 channel -> [selected, frames]"""
    if select == 0:
        raise ValueError("select is empty")
    if mags is None:
        mags = client_magnitudes(audio, win, fft, hop, padding_mode)
    res = frames(mags, algorithm, min_freq, max_freq, sr)
    rows = []
    if select & 1:
        rows.append(to_unit(res[:, 0], unit))
    if select & 2:
        rows.append(res[:, 1])
    out = np.array(rows)
    return out if as_double else out.astype(np.float32)


# ---- test material ---------------------------------------------------------------------------------------------------
SHAPES = [(256, 256, 64), (400, 512, 128), (1024, 1024, 512), (1500, 2048, 300), (4096, 4096, 1024), (1001, 1024, 256),
          (8192, 8192, 4096)]


def glide(n=12000, sr=44100.0, f0=220.0, f1=320.0, seed=7, noise=1e-2):
    """five partials gliding f0 -> f1 plus noise; a quiet stretch (the whole signal 80 dB down) and a pure-noise tail"""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    f = f0 + (f1 - f0) * t / n
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = sum(np.sin(k * ph) / k for k in range(1, 6)) * 0.3
    x = x + noise * rng.standard_normal(n)
    a, b = int(0.45 * n), int(0.55 * n)
    x[a:b] *= 1e-4
    tail = int(0.85 * n)
    x[tail:] = noise * rng.standard_normal(n - tail)
    return x.astype(np.float32)


def tone(n, f0=440.0, sr=44100.0, seed=3, noise=1e-3):
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * f0 * np.arange(n) / sr
    x = 0.4 * sum(np.sin(k * ph) / k for k in range(1, 5)) + noise * rng.standard_normal(n)
    return x.astype(np.float32)


def material(shape):
    """(audio, sample rate) of a test shape: the smallest input that reaches the shape's frames"""
    win, fft, hop = shape
    if fft <= 512:
        return tone(6000 if fft == 256 else 9000, 880.0 if fft == 256 else 660.0), 44100.0
    if fft == 4096:
        return tone(70000, 220.0, seed=5), 44100.0
    if fft == 8192:
        return tone(40000, 110.0, seed=6), 44100.0
    if shape == (1500, 2048, 300):
        return glide(14000, seed=9), 44100.0
    return glide(12000), 44100.0


def extra_inputs():
    """the GPU tests' inputs beside material(): (id, audio, shape, padding mode, minFreq, maxFreq, sample rate); the CPU tests
    assert every frame of each clear of a tie"""
    out = []
    for seed in (12, 14):
        out.append((f"batch-seed{seed}", glide(14000, seed=seed), (1500, 2048, 300), 1, 20.0, 10000.0, 44100.0))
    pad_x = glide(9000, seed=21)
    for shape in ((400, 512, 128), (1024, 1024, 512), (1500, 2048, 300)):
        for mode in (0, 1, 2):
            out.append((f"padding{mode}-{shape}", pad_x, shape, mode, 20.0, 10000.0, 44100.0))
    x8 = glide(12000, sr=8000.0, seed=13)      # the same material at 8 kHz: every clamp bites
    for lo, hi in ((20.0, 20000.0), (0.0, 10000.0), (300.0, 300.0)):
        out.append((f"8k-{lo:g}-{hi:g}", x8, (1024, 1024, 512), 1, lo, hi, 8000.0))
    return out


# ---- the C++ client's test driver (tests/cpp/pitch_driver.cpp), for both test files -------------------------------------
def build_driver():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fluhip_build_pd", os.path.join(root, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_pitch_driver()


def drive(driver, *args, timeout=300):
    import subprocess
    r = subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return r.stdout
