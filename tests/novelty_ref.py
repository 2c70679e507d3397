"""numpy restatement of the reference's novelty slicing, for the tests of BufNoveltySlice / BufNoveltyFeature:

    algorithm::Novelty              algorithms/util/Novelty.hpp:48-117
    algorithm::NoveltyFeature       algorithms/public/NoveltyFeature.hpp:44-62
    algorithm::NoveltySegmentation  algorithms/public/NoveltySegmentation.hpp:44-63
    NoveltySliceClient / NoveltyFeatureClient (clients/rt), Slicing / StreamingControl (clients/common/
    FluidNRTClientWrapper.hpp:551-725), spikesToTimes (clients/common/SpikesToTimes.hpp)

Two forms of the curve: a literal streaming one (ring of frames, shifting similarity matrix, filter buffer, peak buffer,
debounce counter) and the closed batch form the kernels use.  tests/test_novelty_ref.py holds them against each other.
"""
import numpy as np

EPS = np.finfo(np.float64).eps


def gaussian(k):
    """WindowFuncs.hpp kGaussian: sigma = size / 3 on INTEGERS"""
    sigma = float(k // 3)
    h = (k - 1) // 2
    i = np.arange(-h, h + 1, dtype=np.float64)
    return np.exp(-(i * i) / (2 * sigma * sigma))


def checkerboard(k):
    """(K, sum(K .* K)) of Novelty::createKernel"""
    g = gaussian(k)
    h = (k - 1) // 2
    K = np.outer(g, g)
    K[h:, :h] *= -1
    K[:h, h:] *= -1
    return K, float((K * K).sum())


def _norm(x):
    return float(np.sqrt(np.dot(x, x)))  # Eigen's norm(): sqrt of the plain squared sum


class NoveltyStream:
    """Novelty::processFrame, state and all"""

    def __init__(self, k, dims):
        assert k % 2 == 1
        self.k = k
        self.K, self.norm = checkerboard(k)
        self.S = np.zeros((k, k))
        self.buf = np.zeros((k, dims))

    def process(self, x):
        k = self.k
        x = np.asarray(x, dtype=np.float64)
        self.buf[:k - 1] = self.buf[1:].copy()
        self.buf[k - 1] = x
        tmp = self.buf @ x
        nx = _norm(x)
        norm = np.array([max(_norm(r), EPS) for r in self.buf]) * nx
        norm = np.maximum(norm, EPS)
        tmp = tmp / norm
        self.S[:k - 1, :k - 1] = self.S[1:, 1:].copy()
        self.S[:, k - 1] = tmp
        self.S[k - 1, :] = tmp
        return float((self.S * self.K).sum() / self.norm)


class SegmentationStream:
    """NoveltySegmentation::processFrame on NoveltyFeature::processFrame"""

    def __init__(self, k, f, dims):
        self.nov = NoveltyStream(k, dims)
        self.filt = np.zeros(f)
        self.peak = np.zeros(3)
        self.debounce = 0

    def feature(self, x):
        v = self.nov.process(x)
        if len(self.filt) > 1:
            self.filt[:-1] = self.filt[1:].copy()
        self.filt[-1] = v
        return float(self.filt.mean())

    def process(self, x, threshold, min_slice):
        self.peak[:2] = self.peak[1:].copy()
        self.peak[2] = self.feature(x)
        p = self.peak
        if p[1] > p[0] and p[1] > p[2] and p[1] > threshold and self.debounce == 0:
            self.debounce = min_slice
            return 1, p[2]
        if self.debounce > 0:
            self.debounce -= 1
        return 0, p[2]


def streaming(X, k, f=1, threshold=0.5, min_slice=2):
    """(curve [T], detections [T] uint8) by the literal form"""
    X = np.asarray(X, dtype=np.float64)
    s = SegmentationStream(k, f, X.shape[1])
    out = [s.process(x, threshold, min_slice) for x in X]
    return np.array([o[1] for o in out]), np.array([o[0] for o in out], dtype=np.uint8)


def raw_batch(X, k):
    """nov[t] = sum K[a][b] C(t-k+1+a, t-k+1+b) / norm; C(p, q) = <x_p, x_q> / max(max(|x_lo|, eps) |x_hi|, eps)"""
    X = np.asarray(X, dtype=np.float64)
    T = X.shape[0]
    K, norm = checkerboard(k)
    Z = np.vstack([np.zeros((k - 1, X.shape[1])), X])
    n = np.sqrt((Z * Z).sum(axis=1))
    nov = np.empty(T)
    for t in range(T):
        W = Z[t:t + k]
        nw = n[t:t + k]
        G = W @ W.T
        lo = np.minimum.outer(np.arange(k), np.arange(k))
        hi = np.maximum.outer(np.arange(k), np.arange(k))
        den = np.maximum(np.maximum(nw[lo], EPS) * nw[hi], EPS)
        nov[t] = (K * (G / den)).sum() / norm
    return nov


def smooth_batch(nov, f):
    z = np.concatenate([np.zeros(f - 1), nov])
    return np.array([z[t:t + f].sum() / f for t in range(len(nov))])


def curve_batch(X, k, f=1):
    return smooth_batch(raw_batch(X, k), f)


def peaks_batch(curve, threshold, min_slice):
    """detections from a curve: three-point test, then the debounce as a scan over candidates"""
    T = len(curve)
    z = np.concatenate([[0.0, 0.0], curve])
    s0, s1, s2 = z[:T], z[1:T + 1], z[2:]
    cand = (s1 > s0) & (s1 > s2) & (s1 > threshold)
    det = np.zeros(T, dtype=np.uint8)
    last = None
    for t in np.flatnonzero(cand):
        if last is None or t - last > min_slice:
            det[t] = 1
            last = t
    return det


def comparison_margins(curve, threshold):
    """per frame the distances from equality of s[t-1] > s[t-2], s[t-1] > s[t], s[t-1] > threshold; [T, 3].  Frame 0
    compares the two zeros the peak buffer starts with: exact on every implementation, reported as inf."""
    T = len(curve)
    z = np.concatenate([[0.0, 0.0], curve])
    s0, s1, s2 = z[:T], z[1:T + 1], z[2:]
    m = np.stack([np.abs(s1 - s0), np.abs(s1 - s2), np.abs(s1 - threshold)], axis=1)
    m[0, 0] = np.inf
    return m


def outcome_margin(curve, threshold):
    """the smallest change of the curve that could alter any frame's three-point outcome: a frame that is a candidate
    needs all three comparisons to hold (its margin is their smallest distance); one that is not needs only ONE
    failing comparison to stay failed (its margin is the largest distance among the failing ones).  Exact ties between
    equal values (silence) fail on every implementation alike and do not count when another comparison fails clearly."""
    T = len(curve)
    z = np.concatenate([[0.0, 0.0], curve])
    s0, s1, s2 = z[:T], z[1:T + 1], z[2:]
    c = np.stack([s1 > s0, s1 > s2, s1 > threshold], axis=1)
    m = np.stack([np.abs(s1 - s0), np.abs(s1 - s2), np.abs(s1 - threshold)], axis=1)
    m[0, 0] = np.inf
    isc = c.all(axis=1)
    per = np.where(isc, m.min(axis=1), np.where(c, -np.inf, m).max(axis=1))
    return float(per.min())


# ---- features under the clients' framing -----------------------------------------------------------------------------
def hann(win):
    i = np.arange(win, dtype=np.float64)
    return 0.5 - 0.5 * np.cos((np.pi * 2 * i) / win)


def framed_magnitudes(x, win, fft, hop, T, shift=0, stft=None):
    """|STFT| of frames i = 0 .. T-1 holding x[i hop - win - shift, i hop - shift), zeros outside x (FluidSource::pull
    behind BufferedProcess::push: the window ends where the host vector that fired the frame begins).
    stft: None = numpy's FFT; else a callable (signal, win, fft, hop) -> (spec, mag) whose frame t starts at
    t hop - win // 2 (the project's C oracle), fed with the shifted signal."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if stft is not None:
        P = win - win // 2 + shift
        y = np.concatenate([np.zeros(P), x, np.zeros(max(0, T * hop + win - n))])
        mag = stft(y, win, fft, hop)[1]
        return np.ascontiguousarray(mag[:T])
    idx = np.arange(T)[:, None] * hop - win - shift + np.arange(win)[None, :]
    ok = (idx >= 0) & (idx < n)
    frames = np.where(ok, x[np.clip(idx, 0, n - 1)], 0.0) * hann(win)[None, :]
    return np.abs(np.fft.rfft(frames, n=fft, axis=1))


def mel_filters(lo, hi, n_bands, n_bins, sr):
    mel = lambda v: 1127.01048 * np.log(v / 700.0 + 1.0)
    centres = 700.0 * (np.exp(np.linspace(mel(lo), mel(hi), n_bands + 2) / 1127.01048) - 1.0)
    hz = np.linspace(0.0, sr / 2.0, n_bins)
    d = np.abs(centres[:-1] - centres[1:])
    lower = (hz[None, :] - centres[:n_bands, None]) / d[:n_bands, None]
    upper = (centres[2:, None] - hz[None, :]) / d[1:, None]
    return np.maximum(0.0, np.minimum(lower, upper))


def dct_table(n_in, n_out):
    i = np.arange(n_out)[:, None]
    j = np.linspace(0.5, n_in - 0.5, n_in)[None, :]
    scale = np.where(i == 0, 1.0 / np.sqrt(n_in), np.sqrt(2.0 / n_in))
    return np.cos((np.pi / n_in) * i * j) * scale


def features(mag, algorithm, sr=44100.0):
    """the feature rows of NoveltySliceClient::process for algorithm 0 (Spectrum) / 1 (MFCC: 40 bands 20 .. 20e3, log, 13
    coefficients from c0)"""
    if algorithm == 0:
        return mag
    assert algorithm == 1
    filt = mel_filters(20.0, 20e3, 40, mag.shape[1], sr)
    bands = 20.0 * np.log10(np.maximum(mag @ filt.T, EPS))
    return bands @ dct_table(40, 13).T


def latency(hop, k, f):
    fe = f + 1 if f % 2 else f
    return hop * (1 + ((k + 1) >> 1) + (fe >> 1))


def spikes_to_times(onsets, start_frame):
    """spikesToTimes on one row at hop 1"""
    idx = np.flatnonzero(onsets > 0)
    if len(idx) == 0:
        return np.array([-1], dtype=np.int64)
    return idx.astype(np.int64) + start_frame


def bufnoveltyslice(audio, algorithm=0, k=3, threshold=0.5, f=1, min_slice=2, win=1024, fft=1024, hop=512, sr=44100.0,
                    start_frame=0, stft=None, want_curve=False):
    """NRTNoveltySliceClient: audio [channels, n] float32 (the part of the buffer from start_frame on)"""
    audio = np.atleast_2d(np.asarray(audio, dtype=np.float32))
    n = audio.shape[1]
    mono = np.zeros(n, dtype=np.float32)
    for c in range(audio.shape[0]):
        mono = (mono + audio[c]).astype(np.float32)  # x += y on floats (Slicing::process :688-692)
    L = latency(hop, k, f)
    padded = -(-(n + L) // 64) * 64
    T = -(-padded // hop)
    X = features(framed_magnitudes(mono.astype(np.float64), win, fft, hop, T, 0, stft), algorithm, sr)
    curve = curve_batch(X, k, f)
    det = peaks_batch(curve, threshold, min_slice)
    onsets = np.zeros(padded + hop, dtype=np.float32)
    onsets[np.flatnonzero(det) * hop] = 1
    onsets = onsets[:padded]
    if (onsets[:L] > 0).any():
        onsets[L] = 1
    out = spikes_to_times(onsets[L:L + n], start_frame)
    return (out, curve) if want_curve else out


def bufnoveltyfeature(audio, algorithm=0, k=3, f=1, win=1024, fft=1024, hop=512, sr=44100.0, padding_mode=1, stft=None,
                      as_double=False):
    """NRTNoveltyFeatureClient on one float32 channel -> float32 [frames]"""
    x = np.asarray(audio, dtype=np.float32).astype(np.float64)
    n = len(x)
    L = latency(hop, k, f)
    pad = (0, win >> 1, win - hop)[padding_mode]
    padded = n + L + 2 * pad
    if padding_mode == 2:
        padded = -(-padded // hop) * hop
    T = 1 + (padded - win) // hop
    X = features(framed_magnitudes(x, win, fft, hop, T, pad, stft), algorithm, sr)
    curve = curve_batch(X, k, f)[L // hop:]
    return curve if as_double else curve.astype(np.float32)


def harness(signal, win, fft, hop, threshold, min_slice, k, f):
    """NoveltyTestHarness + NoveltySTFTTest of the reference's tests/algorithms/public/TestNoveltySegmentation.cpp:44-110, on
    the literal streaming form"""
    signal = np.asarray(signal, dtype=np.float64)
    filt = f + 1 if f % 2 else f
    padding = hop * (((k + 1) >> 1) + (filt >> 1))
    padded = np.zeros(win + win + padding + len(signal))
    padded[win:win + len(signal)] = signal
    n_hops = (len(padded) - win) // hop
    w = hann(win)
    seg = SegmentationStream(k, f, fft // 2 + 1)
    out = []
    for i in range(n_hops):
        mag = np.abs(np.fft.rfft(padded[i * hop:i * hop + win] * w, n=fft))
        if seg.process(mag, threshold, min_slice)[0]:
            out.append(i * hop - padding - hop)
    out = [max(0, v) for v in out]
    return [v for i, v in enumerate(out) if i == 0 or v != out[i - 1]]


# ---- the reference's synthetic test signals (tests/test_signals/Signals.cpp.in), fs = 44100 --------------------------
FS = 44100


def mono_impulses():
    x = np.zeros((2, FS))
    x[0, 1000] = 1
    x[0, 23051] = 1
    x[1, 12025] = 1
    x[1, 34076] = 1
    return x


def sharp_sines():
    i = np.arange(FS)
    sinx = np.sin(2 * np.pi * i * 640 / (FS - 1))
    phasor = ((FS - 1 - i) % (FS // 4)) / (FS / 4)
    x = sinx * phasor
    x[:1000] = 0
    return x


def smooth_sine():
    i = np.arange(FS)
    return np.sin(2 * np.pi * 320 * i / FS) * np.abs(np.sin(2 * np.pi * i / FS))


SIGNALS = {"monoImpulses": lambda: mono_impulses().sum(axis=0), "sharpSines": sharp_sines, "smoothSine": smooth_sine}


# ---- the C++ clients' test driver (tests/cpp/novelty_driver.cpp), for both test files --------------------------------
def build_driver():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fluhip_build_nd", os.path.join(root, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_novelty_driver()


def drive(driver, *args, timeout=300):
    import subprocess
    r = subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return r.stdout
