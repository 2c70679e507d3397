"""numpy restatement of the reference's harmonic / percussive separation, for the tests of BufHPSS:

    algorithm::HPSS            algorithms/public/HPSS.hpp:48-174
    algorithm::MedianFilter    algorithms/util/MedianFilter.hpp:34-56
    hpss::HPSSClient           clients/rt/HPSSClient.hpp:37-136
    STFTBufferedProcess        clients/common/BufferedProcess.hpp:187-241
    Streaming                  clients/common/FluidNRTClientWrapper.hpp:466-547

Two forms that tests/test_hpss_ref.py holds against each other: the LITERAL one (MedianFilterModel, HPSSModel,
HPSSClientModel, hpss_streaming: host vectors of 64 through the ring buffers, one processFrame per hop with its three ring
matrices) and the CLOSED form the GPU computes (hpss_planes, hpss_channel: whole-plane medians, masks, overlap-add).

HPSS::processFrame is a streaming routine with history, and its indexing is not the textbook centred one.  With frames
counted m = 1, 2, ... (frame m covers the audio samples [m hop - win, m hop)), h2 = (hSize - 1) / 2:
  * the frame a call masks is the input of hSize - 1 calls ago (buf.col(0));
  * the percussive median of bin f is the median of the bins f .. f + vSize - 1 of THAT frame, zeros past the last bin: the
    filter runs over a zero-padded copy and is read back at offset 3 v2, which makes it forward-looking;
  * the harmonic median is written to column h2 + 1 and read from column 0, i.e. the one produced h2 + 1 calls earlier: for
    the masked frame m the median of |X| over the frames m - h2 - 1 .. m + h2 - 1, centred ONE FRAME BEFORE m; frames
    before the first and behind the last are zeros.
"""
import bisect
import math

import numpy as np

from oracle_np import FluidSinkModel, FluidSourceModel, _stft_frame, hann

import onset_ref

EPS = np.finfo(np.float64).eps
DEFAULT_THRESH = (0.0, 1.0, 1.0, 1.0)   # FloatPairsArrayT::defaultValue, ParameterTypes.hpp:257: (x1, y1, x2, y2)
HOST = 64                                # NRTClientWrapper's host vector


# ---- MedianFilter, literally ------------------------------------------------------------------------------------------
class MedianFilterModel:
    """MedianFilter.hpp:34-56: the last `size` samples unsorted (rotated) and sorted (erase the oldest at its lower bound,
    insert the newest at its upper bound); the output is sorted[size / 2].  No arithmetic touches the values."""

    def __init__(self, size):
        self.init(size)

    def init(self, size):
        assert size >= 3 and size % 2
        self.size = size
        self.unsorted = [0.0] * size
        self.sorted = [0.0] * size

    def process_sample(self, val):
        old = self.unsorted[0]
        self.unsorted = self.unsorted[1:] + [val]
        del self.sorted[bisect.bisect_left(self.sorted, old)]
        self.sorted.insert(bisect.bisect_right(self.sorted, val), val)
        return self.sorted[len(self.sorted) // 2]


# ---- the threshold table ---------------------------------------------------------------------------------------------
def constrain_pairs(t):
    """FrequencyAmpPairConstraint (ParameterConstraints.hpp:235-268) at construction: frequencies clipped to [0, 1], a pair
    in the wrong order swapped"""
    x1, y1, x2, y2 = (float(v) for v in t)
    x1, x2 = min(max(x1, 0.0), 1.0), min(max(x2, 0.0), 1.0)
    if x1 > x2:
        x1, y1, x2, y2 = x2, y2, x1, y1
    return (x1, y1, x2, y2)


def lin_spaced(size, low, high):
    """Eigen's ArrayXd::LinSpaced(size, low, high): size 1 yields HIGH (numpy's linspace yields low); the last element is
    exactly high (or, when |high| < |low|, the first exactly low and the others counted back from high)"""
    if size <= 0:
        return np.zeros(0)
    if size == 1:
        return np.array([float(high)])
    step = (high - low) / (size - 1)
    i = np.arange(size, dtype=np.float64)
    if abs(high) < abs(low):
        out = high - (size - 1 - i) * step
        out[0] = low
    else:
        out = low + i * step
        out[-1] = high
    return out


def make_threshold(n_bins, x1, y1, x2, y2):
    """HPSS::makeThreshold (:157-174): 10^(y1 / 20) below the knee, 10^(y2 / 20) from its end on, 10^(LinSpaced / 20) inside"""
    start, end = int(math.floor(x1 * n_bins)), int(math.floor(x2 * n_bins))
    thr = np.ones(n_bins)
    thr[:start] = math.pow(10.0, y1 / 20.0)
    thr[start:end] = [math.pow(10.0, v / 20.0) for v in lin_spaced(end - start, y1, y2)]
    thr[end:] = math.pow(10.0, y2 / 20.0)
    return thr


def masks_of(h, v, mode, thr_h, thr_p):
    """the three masks of HPSS::processFrame (:106-151) from the two medians, min(1, .) applied; any shape whose last axis is
    the bins.  0 / 0 is NaN and compares false, x / 0 is +inf and compares true."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == 0:
            mult = 1.0 / np.maximum(h + v, EPS)
            hm, pm, rm = h * mult, v * mult, np.zeros_like(h)
        elif mode == 1:
            hm = ((h / v) > thr_h).astype(np.float64)
            pm, rm = 1.0 - hm, np.zeros_like(h)
        else:
            hm = ((h / v) > thr_h).astype(np.float64)
            pm = ((v / h) > thr_p).astype(np.float64)
            rm = np.ones_like(h) * (1.0 - hm)
            rm = rm * (1.0 - pm)
            norm = np.maximum(1.0 / (hm + pm + rm), EPS)
            hm, pm, rm = hm * norm, pm * norm, rm * norm
    return np.minimum(hm, 1.0), np.minimum(pm, 1.0), np.minimum(rm, 1.0)


# ---- HPSS::processFrame, literally -----------------------------------------------------------------------------------
class HPSSModel:
    """HPSS.hpp: the ring matrices v, h (medians) and buf (complex frames), nBins x hSize; one MedianFilter per bin along time,
    one along frequency that is re-initialised every frame"""

    def __init__(self):
        self.initialized = False

    def init(self, n_bins, h_size):                                 # :48-64
        assert h_size % 2
        self.v = np.zeros((n_bins, h_size))
        self.h = np.zeros((n_bins, h_size))
        self.buf = np.zeros((n_bins, h_size), dtype=np.complex128)
        self.h_filters = [MedianFilterModel(h_size) for _ in range(n_bins)]
        self.v_filter = None
        self.initialized = True

    def process_frame(self, x, v_size, h_size, mode, h_thresh=DEFAULT_THRESH, p_thresh=DEFAULT_THRESH):   # :66-152
        assert self.initialized and v_size <= len(x)
        h2, v2, n_bins = (h_size - 1) // 2, (v_size - 1) // 2, len(x)
        v, h, buf = self.v, self.h, self.buf
        v[:, :h_size - 1] = v[:, 1:].copy()                         # :86-88
        h[:, :h_size - 1] = h[:, 1:].copy()
        buf[:, :h_size - 1] = buf[:, 1:].copy()
        padded = np.zeros(2 * v_size + n_bins)                      # :90-98
        padded[v2:v2 + n_bins] = np.abs(x)
        self.v_filter = MedianFilterModel(v_size)
        for i in range(len(padded)):
            padded[i] = self.v_filter.process_sample(padded[i])
        v[:, h_size - 1] = padded[v2 * 3:v2 * 3 + n_bins]           # :100
        buf[:, h_size - 1] = x                                      # :101
        mag = np.abs(x)
        h[:, h2 + 1] = [self.h_filters[i].process_sample(mag[i]) for i in range(n_bins)]   # :102-104
        hm, pm, rm = masks_of(h[:, 0], v[:, 0], mode, make_threshold(n_bins, *h_thresh), make_threshold(n_bins, *p_thresh))
        return buf[:, 0] * hm, buf[:, 0] * pm, buf[:, 0] * rm       # :149-151


class HPSSClientModel:
    """rt/HPSSClient.hpp behind STFTBufferedProcess<true>: per completed frame the forward transform, HPSS::processFrame, three
    inverse frames (inverse FFT, 1 / fft, window) overlap-added, and window^2 overlap-added on a fourth channel EVERY call;
    a pulled block is normalised by x /= g where x != 0 and g > 0 (BufferedProcess.hpp:219-239)."""

    def __init__(self, win, fft, hop, h_size, v_size, mode, h_thresh, p_thresh, host_size):
        self.win, self.fft, self.hop, self.host = win, fft, hop, host_size
        self.h_size, self.v_size, self.mode = h_size, v_size, mode
        self.h_thresh, self.p_thresh = constrain_pairs(h_thresh), constrain_pairs(p_thresh)
        self.w = hann(win)
        self.hpss = HPSSModel()
        self.reset()

    def latency(self):                                              # :80-84
        return (self.h_size - 1) * self.hop + self.win

    def reset(self):                                                # :86-90
        self.src = FluidSourceModel(self.win, self.host)
        self.sinks = [FluidSinkModel(self.win, self.host) for _ in range(4)]
        self.frame_time = 0
        self.hpss.init(self.fft // 2 + 1, self.h_size)

    def process(self, block):
        nb = len(block)
        self.src.push(np.asarray(block, dtype=np.float64))
        while self.frame_time < self.host:                          # BufferedProcess::process
            X = _stft_frame(self.src.pull(self.win, self.frame_time), self.w, self.fft)
            outs = self.hpss.process_frame(X, self.v_size, self.h_size, self.mode, self.h_thresh, self.p_thresh)
            for i in range(3):
                self.sinks[i].push(np.fft.irfft(outs[i], n=self.fft)[:self.win] * self.w, self.frame_time)
            self.sinks[3].push(self.w * self.w, self.frame_time)
            self.frame_time += self.hop
        self.frame_time -= self.host
        g = self.sinks[3].pull(nb)
        out = np.empty((3, nb))
        for i in range(3):
            x = self.sinks[i].pull(nb)
            out[i] = np.where(x != 0, x / np.where(g > 0, g, 1.0), x)
        return out


def hpss_streaming(audio, win, fft, hop, h_size=17, v_size=31, mode=0, h_thresh=DEFAULT_THRESH, p_thresh=DEFAULT_THRESH,
                   host=HOST):
    """HPSSClient behind Streaming (FluidNRTClientWrapper.hpp:466-547), literally: host vectors of 64, the input followed by
    zeros up to a whole number of vectors covering nFrames + latency, the first `latency` output samples dropped.
    -> float64 [3, n]: harmonic, percussive, residual"""
    audio = np.asarray(audio, dtype=np.float64)
    n = audio.shape[0]
    client = HPSSClientModel(win, fft, hop, h_size, v_size, mode, h_thresh, p_thresh, host)
    lat = client.latency()
    n_hops = -(-(n + lat) // host)
    inp = np.zeros(host * n_hops)
    inp[:n] = audio
    out = np.concatenate([client.process(inp[j * host:(j + 1) * host]) for j in range(n_hops)], axis=1)
    return out[:, lat:lat + n]


# ---- the closed form -------------------------------------------------------------------------------------------------
def num_frames(n, win, hop):
    """frames m = 1 .. T that touch the buffer: m hop - win < n (the T of fluhip_nmffilter_f32)"""
    return (n + win + hop - 1) // hop - 1


def hpss_planes(mag, h_size=17, v_size=31, mode=0, h_thresh=DEFAULT_THRESH, p_thresh=DEFAULT_THRESH, _h_back=1,
                _v_centred=False):
    """(hmed, vmed, (harmonic, percussive, residual masks)), each [T, F], from a magnitude plane [T, F] whose row t is frame
    m = t + 1.  _h_back / _v_centred exist for ONE test, which shows that the textbook centred variants are not what the
    reference computes."""
    mag = np.asarray(mag, dtype=np.float64)
    T, F = mag.shape
    assert h_size % 2 and v_size % 2 and h_size >= 3 and 3 <= v_size <= F
    h2, v2 = (h_size - 1) // 2, (v_size - 1) // 2
    zt = np.concatenate([np.zeros((h2 + _h_back, F)), mag, np.zeros((h2, F))])        # rows t - h2 - 1 .. t + h2 - 1
    hmed = np.sort(np.lib.stride_tricks.sliding_window_view(zt, h_size, axis=0), axis=2)[:T, :, h_size // 2]
    lead = v2 if _v_centred else 0
    zf = np.concatenate([np.zeros((T, lead)), mag, np.zeros((T, v_size - 1 - lead))], axis=1)   # bins f .. f + vSize - 1
    vmed = np.sort(np.lib.stride_tricks.sliding_window_view(zf, v_size, axis=1), axis=2)[:, :, v_size // 2]
    thr_h = make_threshold(F, *constrain_pairs(h_thresh))
    thr_p = make_threshold(F, *constrain_pairs(p_thresh))
    return np.ascontiguousarray(hmed), np.ascontiguousarray(vmed), masks_of(hmed, vmed, mode, thr_h[None, :], thr_p[None, :])


def frame_spectra(audio, win, fft, hop, stft=None):
    """complex [T, F]: the frames m = 1 .. T at the audio samples [m hop - win, m hop), zeros outside the buffer"""
    audio = np.asarray(audio, dtype=np.float64)
    T = num_frames(len(audio), win, hop)
    if stft is None:
        X = onset_ref.spectra(audio, win, fft, hop, T, hop - win)
    else:
        # a callable (signal, win, fft, hop) -> (spec, mag) whose frame t starts at t hop - win // 2 (the project's C oracle):
        # behind win - win // 2 zeros its frame 1 + i starts at audio sample (i + 1) hop - win
        y = np.concatenate([np.zeros(win - win // 2), audio])
        y = np.concatenate([y, np.zeros(max(0, (T + 2) * hop + win - len(y)))])
        X = np.array(stft(y, win, fft, hop)[0][1:1 + T])
        assert X.shape[0] == T
    X[:, 0] = X[:, 0].real
    X[:, -1] = X[:, -1].real
    return X


def overlap_add(Y, win, fft, hop, n):
    """inverse frames (inverse FFT, 1 / fft, first win samples, window) of Y [T, F] added where frame m = t + 1 came from and
    divided by the window^2 of the frames 1 .. T covering a sample -> float64 [n]"""
    T = Y.shape[0]
    w = hann(win)
    y = np.fft.irfft(Y, n=fft, axis=1)[:, :win] * w[None, :]
    acc = np.zeros(T * hop + win)
    nrm = np.zeros(T * hop + win)
    for t in range(T):
        acc[(t + 1) * hop:(t + 1) * hop + win] += y[t]               # (position p of acc is audio sample p - win)
        nrm[(t + 1) * hop:(t + 1) * hop + win] += w * w
    out = np.where(acc != 0, acc / np.where(nrm > 0, nrm, 1.0), acc)
    out = np.concatenate([out, np.zeros(max(0, win + n - len(out)))])
    return out[win:win + n]


def hpss_channel(audio, win, fft, hop, h_size=17, v_size=31, mode=0, h_thresh=DEFAULT_THRESH, p_thresh=DEFAULT_THRESH,
                 stft=None, **variant):
    """what fluhip_bufhpss_f32 computes for one buffer: spectra of the frames 1 .. T, whole-plane medians and masks, three
    masked inverse transforms overlap-added where the frames came from -> float64 [3, n]"""
    audio = np.asarray(audio, dtype=np.float64)
    n = len(audio)
    X = frame_spectra(audio, win, fft, hop, stft)
    _, _, masks = hpss_planes(np.abs(X), h_size, v_size, mode, h_thresh, p_thresh, **variant)
    return np.stack([overlap_add(X * m, win, fft, hop, n) for m in masks])


def covered(n, win, hop):
    """bool [n]: the samples some frame's window^2 is non-zero on"""
    T = num_frames(n, win, hop)
    w2 = hann(win) ** 2
    nrm = np.zeros(T * hop + win + win + n)
    for t in range(T):
        nrm[(t + 1) * hop:(t + 1) * hop + win] += w2
    return nrm[win:win + n] > 0


def tie_margin(mag, h_size, v_size, mode, h_thresh=DEFAULT_THRESH, p_thresh=DEFAULT_THRESH):
    """the smallest relative distance |ratio - threshold| / threshold over the FINITE ratios the mode compares"""
    hmed, vmed, _ = hpss_planes(mag, h_size, v_size, mode, h_thresh, p_thresh)
    F = mag.shape[1]
    worst = np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        pairs = [(hmed / vmed, make_threshold(F, *constrain_pairs(h_thresh)))]
        if mode == 2:
            pairs.append((vmed / hmed, make_threshold(F, *constrain_pairs(p_thresh))))
        for ratio, thr in pairs:
            rel = np.abs(ratio - thr[None, :]) / thr[None, :]
            rel = rel[np.isfinite(ratio)]
            if rel.size:
                worst = min(worst, float(rel.min()))
    return worst


# ---- the C++ driver ---------------------------------------------------------------------------------------------------
def build_driver():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fluhip_build_hd", os.path.join(root, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_hpss_driver()


def drive(driver, *args, timeout=300):
    import subprocess
    r = subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr
    return r.stdout
