"""BufNMFCross restated in numpy, operation for operation:

    algorithm::NMFCross     include/flucoma/algorithms/public/NMFCross.hpp:46-186
    algorithm::GriffinLim   include/flucoma/algorithms/public/GriffinLim.hpp:26-52
    client NMFCrossClient   include/flucoma/clients/nrt/NMFCrossClient.hpp:84-184

Matrices keep the reference's orientation inside the algorithm (V F x T, W F x K, H K x T) and leave as its outputs do
(H1 T x K).  The STFT and the random draws are oracle_np's.

The constraint factor of the reference is ``1 - ((iteration + 1) / mIterations)`` in INTEGER arithmetic (:132, :150): 1 on
every iteration but the last and 0 on the last.  Temporal sparsity and polyphony therefore leave H unchanged until iteration
``iters - 1`` and there zero every entry they do not keep (with ``iters == 1``: on iteration 0).  That is restated as such.
Polyphony's ``std::sort`` is not stable (:79-86); ties go to the lower source frame here (``kind="stable"``).

Two restatements of the constraints: the vectorised one the pipeline uses, and ``*_literal``, a loop transcription of the
C++ (padded blocks, decay factor and all) that the tests hold it against.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_np  # noqa: E402

EPS = oracle_np.EPS


def decay(iteration: int, iters: int) -> int:
    """1 - ((iteration + 1) / mIterations), index (integer) arithmetic"""
    return 1 - ((iteration + 1) // iters)


# ---- the constraints, vectorised ------------------------------------------------------------------------------------
def sparsity(H, r, iteration, iters):
    """enforceTemporalSparseness (:117-140): H[k][j] kept when the FIRST maximum of its zero-padded window is the centre"""
    d = decay(iteration, iters)
    K, T = H.shape
    h = (r - 1) // 2
    padded = np.zeros((K, T + r))
    padded[:, h:h + T] = H
    win = np.lib.stride_tricks.sliding_window_view(padded, r, axis=1)[:, :T, :]
    keep = np.argmax(win, axis=2) == h
    return np.where(keep, H, H * d)


def polyphony(H, energy, p, iteration, iters):
    """restrictPolyphony (:143-155): per column, the p largest H * energy kept (ties: lower row first)"""
    d = decay(iteration, iters)
    out = H * d
    score = H * energy[:, None]
    top = np.argsort(-score, axis=0, kind="stable")[:p]
    cols = np.broadcast_to(np.arange(H.shape[1])[None, :], top.shape)
    out[top, cols] = H[top, cols]
    return out


def continuity(H, c):
    """promoteContinuity (:99-115): Hc[i][j] = sum_d H[i + d - h][j + d - h], terms outside H are 0"""
    K, T = H.shape
    h = (c - 1) // 2
    padded = np.zeros((K + c, T + c))
    padded[h:h + K, h:h + T] = H
    out = np.zeros((K, T))
    for d in range(c):
        out += padded[d:d + K, d:d + T]
    return out


# ---- the constraints, loop by loop as the C++ writes them ---------------------------------------------------------
def sparsity_literal(H, size, iteration, iters):
    halfSize = (size - 1) // 2
    rows, cols = H.shape
    padded = np.zeros((rows, cols + size))
    output = np.zeros((rows, cols))
    padded[0:rows, halfSize:halfSize + cols] = H
    for i in range(rows):
        for j in range(cols):
            neighborhood = padded[i, j:j + size]
            maxIndex = 0
            for q in range(1, size):  # Eigen's maxCoeff(&index): the first maximum
                if neighborhood[q] > neighborhood[maxIndex]:
                    maxIndex = q
            if maxIndex != halfSize:
                output[i, j] = H[i, j] * (1 - ((iteration + 1) // iters))
            else:
                output[i, j] = H[i, j]
    return output


def polyphony_literal(H, energyInW, size, iteration, iters):
    rows, cols = H.shape
    output = np.zeros((rows, cols))
    for k in range(cols):
        wCol = H[:, k] * energyInW
        output[:, k] = H[:, k] * (1 - ((iteration + 1) // iters))
        idx = list(range(rows))
        idx.sort(key=lambda i: -wCol[i])  # (Python's sort is stable: ties keep the lower index first)
        for t in idx[:size]:
            output[t, k] = H[t, k]
    return output


def continuity_literal(H, size):
    halfSize = (size - 1) // 2
    rows, cols = H.shape
    kernel = np.eye(size)
    padded = np.zeros((rows + size, cols + size))
    output = np.zeros((rows, cols))
    padded[halfSize:halfSize + rows, halfSize:halfSize + cols] = H
    for i in range(rows):
        for j in range(cols):
            output[i, j] = (padded[i:i + size, j:j + size] * kernel).sum()
    return output


# ---- NMFCross ---------------------------------------------------------------------------------------------------------
def initial_h(K, T, seed):
    """EigenRandom<MatrixXd>(K, T, seed, [0, 1)): column-major K x T, one mt19937_64 draw per value"""
    return oracle_np.rng_uniform01(seed, K * T).reshape(T, K).T.copy()


def nmfcross(X, W0, r, p, c, iters, seed, literal=False, progress=None):
    """NMFCross(iters).process(X, H1, W0, r, p, c, seed): X T x F, W0 K x F -> H1 T x K"""
    X = np.asarray(X, dtype=np.float64)
    W0 = np.asarray(W0, dtype=np.float64)
    T, F = X.shape
    K = W0.shape[0]
    W = np.maximum(W0.T, EPS)                       # :164 (W = W0^T, F x K)
    energy = (W * W).sum(axis=0)                    # :167
    H = initial_h(K, T, seed)
    V = X.T
    ones = np.ones((F, T))
    for i in range(iters):
        if literal:
            H = sparsity_literal(H, r, i, iters)
            H = polyphony_literal(H, energy, p, i, iters)
            H = continuity_literal(H, c)
        else:
            H = sparsity(H, r, i, iters)
            H = polyphony(H, energy, p, i, iters)
            H = continuity(H, c)
        V2 = np.maximum(W @ H, EPS)
        hnum = W.T @ (V / V2)
        hden = W.T @ ones
        H = H * hnum / np.maximum(hden, EPS)
        if progress is not None and not progress(i + 1):
            break
    return H.T.copy()


# ---- STFT / ISTFT / GriffinLim --------------------------------------------------------------------------------------
def istft(spec, n, win, fft, hop):
    """ISTFT::process: inverse / fft, window, overlap-add, / max(sum w^2, eps), trim win / 2, n samples"""
    T = spec.shape[0]
    w = oracle_np.hann(win)
    frames = np.fft.irfft(spec, n=fft, axis=1)[:, :win] * w[None, :]
    size = (T - 1) * hop + win
    acc, nrm = np.zeros(size), np.zeros(size)
    for t in range(T):
        acc[t * hop:t * hop + win] += frames[t]
        nrm[t * hop:t * hop + win] += w * w
    y = acc / np.maximum(nrm, EPS)
    out = np.zeros(n)
    m = max(0, min(n, size - win // 2))
    out[:m] = y[win // 2:win // 2 + m]
    return out


def random_phase(T, F, seed):
    """EigenRandomPhase<ArrayXXcd>(T, F, seed): column-major T x F, theta = 2 pi u (uniform_real_distribution(0, 2 pi)),
    std::polar(1, theta)"""
    u = oracle_np.rng_uniform01(seed, T * F).reshape(F, T).T
    th = (2 * np.pi) * u + 0.0
    return np.cos(th) + 1j * np.sin(th)


def griffinlim(spec, n, iters, win, fft, hop, seed):
    momentum = 0.9
    mag = np.abs(spec)
    T, F = spec.shape
    phase = random_phase(T, F, seed)
    estimate = np.zeros((T, F), dtype=np.complex128)
    for _ in range(iters):
        prev = estimate
        x = istft(mag * phase, n, win, fft, hop)
        estimate, _m = oracle_np.stft(x, win, fft, hop)
        phase = estimate - (momentum / (1 + momentum)) * prev
        phase = phase / (np.abs(phase) + EPS)
    return mag * phase


# ---- the client -------------------------------------------------------------------------------------------------------
def check_client(n_src, n_tgt, hop, r, c):
    """NMFCrossClient.hpp:111-118: the reference's messages, in its order (None: OK)"""
    tgt_windows = (n_tgt + hop) // hop
    if n_src <= 0:
        return "Empty source buffer"
    if n_tgt <= 0:
        return "Empty target buffer"
    if r > tgt_windows:
        return "Time Sparsity is larger than target frames"
    if c > tgt_windows:
        return "Continuity is larger than target frames"
    return None


def bufnmfcross(source, target, win, fft, hop, r=7, p=11, c=7, iters=50, seed=42, gl_iters=50, return_h=False):
    """NMFCrossClient::process on channel 0: float output of n_target samples"""
    src = np.asarray(source, dtype=np.float32).astype(np.float64)
    tgt = np.asarray(target, dtype=np.float32).astype(np.float64)
    src_spec, W = oracle_np.stft(src, win, fft, hop)
    _tgt_spec, tgt_mag = oracle_np.stft(tgt, win, fft, hop)
    K = W.shape[0]
    H1 = nmfcross(tgt_mag, W, r, min(K, p), c, iters, seed)
    result = H1 @ src_spec                                # NMFCross::synthesize
    result = griffinlim(result, len(tgt), gl_iters, win, fft, hop, seed)
    out = istft(result, len(tgt), win, fft, hop).astype(np.float32)
    return (out, H1) if return_h else out
