"""Restatement of the reference's spectral shape and chroma analysis in numpy, line by line:

    algorithm::SpectralShape      include/flucoma/algorithms/public/SpectralShape.hpp:32-102
    algorithm::ChromaFilterBank   include/flucoma/algorithms/public/ChromaFilterBank.hpp:35-115
    client::spectralshape::SpectralShapeClient  include/flucoma/clients/rt/SpectralShapeClient.hpp:88-129 behind StreamingControl
    client::chroma::ChromaClient                include/flucoma/clients/rt/ChromaClient.hpp:75-111 behind StreamingControl

The reference's behaviour is kept, not tidied; every kept behaviour has a tidied variant behind a keyword argument (default:
as the reference), and tests/test_spectral_ref.py shows each variant to give another answer.  Framing and magnitudes are
pitch_ref.client_magnitudes (both clients' latency is the window).

Three places are defined here (and in the device code) where the reference leaves its arrays: a quotient freq / binHz at or
beyond the bin count counts as the bin count before it is rounded; SpectralShape's segment left empty by the MIDI axis
(minBin 0 -> 1 with maxBin 1) gives seven zeros like an empty range; the chroma range's zeroed runs are clamped to the frame.
rolloffPercent == 100 compares a sequential running sum against Eigen's separately ordered total and so depends on summation
order in the reference itself: it is not pinned (either the last frequency step or maxBin - 1).
"""
import math

import numpy as np

from hpss_ref import lin_spaced
from pitch_ref import client_magnitudes

EPSILON = np.finfo(np.float64).eps          # util/AlgorithmUtils.hpp:19
LOG2E = 1.44269504088896340736              # util/AlgorithmUtils.hpp, ChromaFilterBank.hpp:38
DESCRIPTORS = ("centroid", "spread", "skew", "kurtosis", "rolloff", "flatness", "crest")


def _bin(q, n_bins, rnd):
    """an index from a quotient: at or beyond the bin count it counts as the bin count (the cast of a huge value is undefined)"""
    return n_bins if not (q < n_bins) else int(rnd(q))


# ---- SpectralShape ---------------------------------------------------------------------------------------------------
def shape_bins(n_bins, min_freq, max_freq, sr):
    """(minBin, maxBin, binHz) of SpectralShape.hpp:37-44"""
    max_freq = sr / 2 if max_freq == -1 else min(max_freq, sr / 2)
    bin_hz = sr / ((n_bins - 1) * 2.0)
    lo = _bin(min_freq / bin_hz, n_bins, math.ceil)
    hi = min(_bin(max_freq / bin_hz, n_bins, math.floor), n_bins - 1)
    return lo, hi, bin_hz


def shape_axis(lo, hi, bin_hz, unit=0, axis_step_is_bin=False):
    """the frequency axis of the `hi - lo` bins lo .. hi - 1: LinSpaced(size, lo binHz, hi binHz), whose step is
    (hi - lo) binHz / (size - 1) and not binHz (tidied: axis_step_is_bin); then MIDI for unit 1"""
    size = hi - lo
    f = (lo + np.arange(size)) * bin_hz if axis_step_is_bin else lin_spaced(size, lo * bin_hz, hi * bin_hz)
    if unit == 1:
        f = 69 + (12 * np.log(f / 440) * LOG2E)
    return f


def spectral_shape(mag, min_freq=0.0, max_freq=-1.0, rolloff_percent=95.0, unit=0, power=0, sr=44100.0, *,
                   clamp_first=True, fold_dc=True, include_max_bin=False, axis_step_is_bin=False, raw_moments=False,
                   rooted_spread=False, rolloff_interpolates=True, rolloff_miss_is_frequency=False, db_floor=True):
    """SpectralShape::processFrame on one frame -> the seven descriptors.  Keyword arguments after `sr` switch a kept
    behaviour to its tidied form."""
    mag = np.asarray(mag, dtype=np.float64)
    n_bins = len(mag)
    lo, hi, bin_hz = shape_bins(n_bins, min_freq, max_freq, sr)
    if hi <= lo:
        return np.zeros(7)
    m = np.maximum(mag, EPSILON) if clamp_first else mag.copy()          # :39, before anything else
    if unit == 1 and lo == 0:                                               # :51-55
        lo = 1
        if fold_dc:
            m[1] += m[0]
    size = hi - lo + (1 if include_max_bin else 0)                          # :57: bin maxBin is never read
    if size < 1:
        return np.zeros(7)                                                  # (defined here: the reference reads an empty array)
    amp = m[lo:lo + size].copy()
    if not clamp_first:
        amp = np.maximum(amp, EPSILON)
    if power:
        amp = amp * amp
    amp_sum = amp.sum()
    freqs = shape_axis(lo, lo + size, bin_hz, unit, True) if include_max_bin else shape_axis(lo, hi, bin_hz, unit, axis_step_is_bin)
    with np.errstate(invalid="ignore", divide="ignore"):
        centroid = (amp * freqs).sum() / amp_sum
        if raw_moments:
            m1, m2, m3, m4 = [(amp * freqs ** k).sum() / amp_sum for k in (1, 2, 3, 4)]
            spread = m2 - m1 * m1
            mu3 = m3 - 3 * m1 * m2 + 2 * m1 ** 3
            mu4 = m4 - 4 * m1 * m3 + 6 * m1 * m1 * m2 - 3 * m1 ** 4
            skew, kurt = mu3 / (spread * np.sqrt(spread)), mu4 / (spread * spread)
        else:
            d = freqs - centroid
            spread = (amp * d ** 2).sum() / amp_sum
            den = np.sqrt(spread) if rooted_spread else spread
            skew = (amp * d ** 3).sum() / (den * np.sqrt(den) * amp_sum)
            kurt = (amp * d ** 4).sum() / (den * den * amp_sum)
        flatness = np.exp(np.log(amp).mean()) / amp.mean()
        rolloff = float(freqs[-1]) if rolloff_miss_is_frequency else float(hi - 1)   # :79: a bin index, not a frequency
        cum = 0.0
        target = amp_sum * rolloff_percent / 100.0
        for i in range(size):
            if not cum <= target:
                break
            cum += amp[i]
            if cum >= target:
                if i == 0 or not rolloff_interpolates:
                    rolloff = freqs[i]
                else:
                    rolloff = freqs[i] - (freqs[i] - freqs[i - 1]) * (cum - target) / amp[i]
                break
        crest = amp.max() / amp.mean()
        if db_floor:
            flat_db, crest_db = 20 * np.log10(max(flatness, EPSILON)), 20 * np.log10(max(crest, EPSILON))
        else:
            flat_db, crest_db = 20 * np.log10(flatness), 20 * np.log10(crest)
        return np.array([centroid, np.sqrt(spread), skew, kurt, rolloff, flat_db, crest_db])


def shape_frames(mags, **kw):
    """[T, F] magnitudes -> [T, 7]"""
    return np.array([spectral_shape(m, **kw) for m in mags]).reshape(len(mags), 7)


def bufspectralshape(audio, select=127, min_freq=0.0, max_freq=-1.0, rolloff_percent=95.0, unit=0, power=0, win=1024,
                     fft=1024, hop=512, padding_mode=1, sr=44100.0, as_double=False, mags=None):
    """NRTSpectralShapeClient on one float32 channel -> [selected, frames]; the selected descriptors in table order"""
    if mags is None:
        mags = client_magnitudes(audio, win, fft, hop, padding_mode)
    res = shape_frames(mags, min_freq=min_freq, max_freq=max_freq, rolloff_percent=rolloff_percent, unit=unit, power=power, sr=sr)
    out = np.array([res[:, i] for i in range(7) if select >> i & 1])
    return out if as_double else out.astype(np.float32)


# ---- ChromaFilterBank ------------------------------------------------------------------------------------------------
def chroma_filters(n_chroma, n_bins, ref=440.0, sr=44100.0, *, axis_over_fft=False, c_fmod=True, half_rounds_up=False,
                   unit_columns=True, dtype=np.float64):
    """ChromaFilterBank::init -> ([nChroma, nBins] filters, scale)"""
    fft = 2 * (n_bins - 1)
    T = dtype
    if axis_over_fft:
        freqs = np.arange(fft, dtype=T) * (T(sr) / T(fft))
    elif T is np.float64:
        freqs = lin_spaced(fft, 0.0, sr)        # LinSpaced(fftSize, 0, sr): step sr / (fftSize - 1), the last point exactly sr
    else:                                       # (the same in another precision, for the table's floor)
        freqs = np.arange(fft, dtype=T) * (T(sr) / T(fft - 1))
        freqs[-1] = T(sr)
    with np.errstate(divide="ignore"):
        freqs = T(n_chroma) * np.log(freqs / (T(ref) / T(16))) * T(LOG2E)
    freqs[0] = freqs[1] - T(1.5) * T(n_chroma)
    widths = np.ones(fft, dtype=T)
    widths[:fft - 1] = freqs[1:] - freqs[:-1]
    widths = np.maximum(widths, T(1.0))
    diffs = freqs[None, :] - np.arange(n_chroma, dtype=T)[:, None]
    half = (n_chroma + 1) // 2 if half_rounds_up else n_chroma // 2     # lrint(nChroma / 2) on an integer quotient
    x = (diffs + T(10 * n_chroma)) + T(half)
    rem = (np.fmod(x, T(n_chroma)) if c_fmod else np.mod(x, T(n_chroma))) - T(half)
    w = np.exp(T(-0.5) * (T(2) * rem / widths[None, :]) ** 2)[:, :n_bins]
    if unit_columns:
        w = w / np.sqrt((w * w).sum(axis=0))[None, :]
    return w, T(2.0) / T(fft * n_chroma)


def chroma_range(n_bins, min_freq, max_freq, sr, *, min_zero_keeps_all=True):
    """(lo, hi): the bins lo < j < hi survive ChromaFilterBank::processFrame's range branch (:91-103); (-1, nBins) when it
    does not run"""
    if min_freq == 0 and max_freq == -1:
        return -1, n_bins
    max_freq = sr / 2 if max_freq == -1 else min(max_freq, sr / 2)
    bin_hz = sr / ((n_bins - 1) * 2.0)
    lo = 0 if min_freq == 0 else _bin(min_freq / bin_hz, n_bins, math.ceil)
    hi = min(_bin(max_freq / bin_hz, n_bins, math.floor), n_bins - 1)
    if min_freq == 0 and not min_zero_keeps_all:
        lo = -1
    return min(lo, n_bins - 1), hi      # bins 0 .. lo INCLUSIVE and hi .. nBins - 1 are zeroed


def chroma_frames(mags, n_chroma=12, ref=440.0, normalize=0, min_freq=0.0, max_freq=-1.0, sr=44100.0, filters=None, **tidy):
    """ChromaFilterBank::processFrame on [T, F] magnitudes -> [T, nChroma]; the input is not modified"""
    mags = np.asarray(mags, dtype=np.float64)
    n_bins = mags.shape[1]
    range_kw = {k: tidy.pop(k) for k in list(tidy) if k == "min_zero_keeps_all"}
    w, scale = filters if filters is not None else chroma_filters(n_chroma, n_bins, ref, sr, **tidy)
    lo, hi = chroma_range(n_bins, min_freq, max_freq, sr, **range_kw)
    frame = mags.copy()
    frame[:, :lo + 1] = 0
    frame[:, hi:] = 0
    out = (frame * frame) @ w.T * scale
    if normalize > 0:
        norm = out.sum(axis=1) if normalize == 1 else out.max(axis=1)
        out = out / np.maximum(norm, EPSILON)[:, None]
    return out


def bufchroma(audio, n_chroma=12, ref=440.0, normalize=0, min_freq=0.0, max_freq=-1.0, win=1024, fft=1024, hop=512,
              padding_mode=1, sr=44100.0, as_double=False, mags=None):
    """NRTChromaClient on one float32 channel -> [nChroma, frames]"""
    if mags is None:
        mags = client_magnitudes(audio, win, fft, hop, padding_mode)
    out = chroma_frames(mags, n_chroma, ref, normalize, min_freq, max_freq, sr).T
    return np.ascontiguousarray(out if as_double else out.astype(np.float32))


# ---- the C++ clients' test driver (tests/cpp/spectral_driver.cpp), for both test files -----------------------------------
def build_driver():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fluhip_build_sd", os.path.join(root, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_spectral_driver()
