"""A plain numpy restatement of the inverse the resynthesising clients share -- RatioMask::process + ISTFT::process
(alg/RatioMask.hpp:33-57, alg/STFT.hpp:178-199) with the trim as a parameter -- the measure the double-precision tests of it
use, and the case lists tests/test_istft_ref.py (the floor, on the CPU) and tests/test_gpu_istft.py (the device) share.

Nothing here knows the device code: the inverse is numpy's irfft, the overlap-add runs in np.longdouble."""
import functools

import numpy as np

import oracle_np

EPS = oracle_np.EPS

# ---- the cases ------------------------------------------------------------------------------------------------------
# (n, win, fft, hop, trim) of the plain inverse, one per kernel form
PLAIN_CASES = [
    (40, 4, 4, 1, 2),                    # a single radix-2 pass
    (100, 8, 8, 2, 4),                   # a single radix-4 pass
    (300, 16, 16, 4, 8),                 # 64 threads over two-point loops
    (1500, 64, 64, 16, 32),
    (2500, 200, 256, 100, 100),          # win < fft, passes 4 4 4 2
    (6000, 301, 512, 75, 150),           # odd window, hop does not divide it
    (5000, 256, 256, 384, 128),          # hop > win: samples no frame covers
    (9000, 1024, 1024, 512, 512),
    (9000, 1024, 1024, 512, 0),          # BufSTFT padding 0: the first normalisers are nearly zero
    (9000, 1024, 1024, 256, 768),        # trim = win - hop, as NMFFilter and HPSS use
    (12345, 1000, 1024, 300, 500),
    (12000, 2048, 2048, 512, 1024),
    (20000, 4096, 4096, 1024, 2048),
    (30000, 8192, 8192, 2048, 4096),     # the largest LDS frame
    (70000, 16384, 16384, 4096, 8192),   # global-memory passes
    (40000, 3000, 16384, 1000, 1500),    # global-memory passes, win < fft
]
SHORT_CASES = [(n, 1024, 1024, 512, 512) for n in (1, 511, 513)]
# win 1024, fft 65536, hop 64: 1032 frames against a chunk of 1024 in the global-memory passes
CHUNK_CASE = (66000, 1024, 65536, 64, 512)
CHUNK_FRAMES = 1024
# (n, win, fft, hop, K) of the masked resynthesis, trim = win / 2
MASKED_CASES = [
    (9000, 1024, 1024, 256, 1),          # the mask is est / est: one ulp either side of 1, fmin decides
    (9000, 1024, 1024, 256, 3),
    (9000, 1024, 1024, 256, 9),
    (6000, 301, 512, 75, 3),
    (12000, 2048, 2048, 512, 4),
    (70000, 16384, 16384, 4096, 2),      # the global-memory form's loop over components
    (5000, 64, 64, 16, 17),
]


def case_id(c):
    return "_".join(str(v) for v in c)


def num_frames(n, hop):
    return (n + hop) // hop


# ---- inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain_spec(n, win, fft, hop):
    """the forward transform of the synthetic audio, times (1 + 0.5j): DC and Nyquist carry imaginary parts the inverse
    must ignore.  Shared between tests: do not write to it."""
    seed = 1034 if n == 1 else 1000 + n % 97      # (1034: a one-sample buffer whose sample is 0.029, not 0.003)
    spec = oracle_np.stft(oracle_np.synth_audio(n, seed), win, fft, hop)[0] * (1 + 0.5j)
    assert spec.shape == (num_frames(n, hop), fft // 2 + 1)
    spec.setflags(write=False)
    return spec


def chunk_spec():
    n, win, fft, hop, _ = CHUNK_CASE
    return np.random.RandomState(5).standard_normal((num_frames(n, hop), fft // 2 + 1, 2)).view(np.complex128)[..., 0]


@functools.lru_cache(maxsize=None)
def factors(T, F, K):
    """W [K][F] and H [T][K], |N(0,1)| + 1e-3, with three all-zero rows of H (V-hat is 0 there: the eps clamp acts, the mask
    is 0, the frame contributes nothing) and one all-zero column of W (a bin whose V-hat is 0 in every frame)"""
    rs = np.random.RandomState(1000 * K + T % 1000)
    W = np.abs(rs.standard_normal((K, F))) + 1e-3
    H = np.abs(rs.standard_normal((T, K))) + 1e-3
    if T >= 8:       # (a buffer of two or three frames keeps them all)
        H[[0, T // 2, T - 2]] = 0.0
    W[:, F // 3] = 0.0
    W.setflags(write=False)
    H.setflags(write=False)
    return W, H


# ---- the restatement -------------------------------------------------------------------------------------------------
def ratio_mask(W, H, k):
    """min(est * (1 / max(V, eps)), 1) with est = H[:, k] W[k, :] and V = H W"""
    est = np.outer(H[:, k], W[k, :])
    V = H @ W
    return np.minimum(est * (1.0 / np.maximum(V, EPS)), 1.0)


def normaliser(T, win, hop, n, trim):
    """the overlap-added window^2 at the n output positions (before the eps clamp), in long double"""
    w2 = oracle_np.hann(win).astype(np.longdouble) ** 2
    size = max((T - 1) * hop + win, trim + n)
    nrm = np.zeros(size, dtype=np.longdouble)
    for t in range(T):
        nrm[t * hop: t * hop + win] += w2
    return nrm[trim: trim + n]


def istft(spec, win, fft, hop, n, trim, mask=None, rows=256):
    """out[i] = position i + trim of (sum_t window * irfft(spec[t] * mask[t])[:win] at t hop) / max(sum_t window^2, eps)"""
    T, F = spec.shape
    assert F == fft // 2 + 1
    w = oracle_np.hann(win)
    size = max((T - 1) * hop + win, trim + n)
    acc = np.zeros(size, dtype=np.longdouble)
    for t0 in range(0, T, rows):       # (row blocks: the inverse of 1032 frames of fft 65536 at once is 0.5 GB)
        Y = spec[t0: t0 + rows] if mask is None else spec[t0: t0 + rows] * mask[t0: t0 + rows]
        frames = np.fft.irfft(Y, n=fft, axis=1)[:, :win] * w
        for j in range(frames.shape[0]):
            t = t0 + j
            acc[t * hop: t * hop + win] += frames[j]
    nrm = normaliser(T, win, hop, size - trim, trim)
    out = acc[trim:] / np.maximum(nrm, np.longdouble(EPS))
    return out[:n].astype(np.float64)


def weights(T, win, hop, n, trim):
    """w_i = min(max(nrm_i, eps), 1): an error at a position whose normaliser is small is the numerator's error divided by
    it, so the measure multiplies it back (as test_bufstft_forward_inverse does)"""
    return np.minimum(np.maximum(normaliser(T, win, hop, n, trim), np.longdouble(EPS)), 1).astype(np.float64)


def peak(ref, w):
    return float((np.abs(ref) * w).max())


def err(got, ref, w):
    """max_i |got_i - ref_i| w_i / max_i (|ref_i| w_i)"""
    return float((np.abs(np.asarray(got, dtype=np.float64) - ref) * w).max()) / peak(ref, w)
