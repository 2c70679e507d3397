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

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_np  # noqa: E402
import stft_ref  # noqa: E402
from nmf_ref import elrel  # noqa: E402,F401  (THE error measure of the H loop: every entry relative to itself)

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
    padded = np.zeros((K, T + r), dtype=H.dtype)
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
    padded = np.zeros((K + c, T + c), dtype=H.dtype)
    padded[h:h + K, h:h + T] = H
    out = np.zeros((K, T), dtype=H.dtype)
    for d in range(c):                              # (d = 0 .. c - 1: the order in which the kernel adds)
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


def nmfcross(X, W0, r, p, c, iters, seed, literal=False, progress=None, dtype=np.float64, perturb=None, last=None):
    """NMFCross(iters).process(X, H1, W0, r, p, c, seed): X T x F, W0 K x F -> H1 T x K.  Under ``dtype=np.longdouble``
    every array and every sum is long double, the two products included (numpy has no BLAS at that type: small shapes).
    ``perturb=d`` multiplies every quotient V / max(W H, eps) by (1 + d).  ``last(H, energy)`` is called with the K x T
    activations in front of the constraints of the last iteration (decision_margins)."""
    eps = dtype(EPS)
    X = np.asarray(X, dtype=dtype)
    W0 = np.asarray(W0, dtype=dtype)
    T, F = X.shape
    K = W0.shape[0]
    W = np.maximum(W0.T, eps)                       # :164 (W = W0^T, F x K)
    energy = (W * W).sum(axis=0)                    # :167
    H = initial_h(K, T, seed).astype(dtype)
    V = X.T
    ones = np.ones((F, T), dtype=dtype)
    for i in range(iters):
        if last is not None and i == iters - 1:
            last(H, energy)
        if literal:
            H = sparsity_literal(H, r, i, iters)
            H = polyphony_literal(H, energy, p, i, iters)
            H = continuity_literal(H, c)
        else:
            H = sparsity(H, r, i, iters)
            H = polyphony(H, energy, p, i, iters)
            H = continuity(H, c)
        V2 = np.maximum(W @ H, eps)
        q = V / V2
        if perturb is not None:
            q = q * dtype(1.0 + perturb)
        hnum = W.T @ q
        hden = W.T @ ones
        H = H * hnum / np.maximum(hden, eps)
        if progress is not None and not progress(i + 1):
            break
    return H.T.copy()


def _margins(H, energy, r, p, iters):
    K, T = H.shape
    h = (r - 1) // 2
    gap_r = np.inf
    if r > 1:
        padded = np.zeros((K, T + r), dtype=H.dtype)
        padded[:, h:h + T] = H
        win = np.lib.stride_tricks.sliding_window_view(padded, r, axis=1)[:, :T, :]
        others = np.delete(win, h, axis=2).max(axis=2)
        big = np.maximum(H, others)
        live = big > 0
        if live.any():
            gap_r = float((np.abs(H - others)[live] / big[live]).min())
    gap_p = np.inf
    if p < K:
        score = -np.sort(-(sparsity(H, r, iters - 1, iters) * energy[:, None]), axis=0)
        a, b = score[p - 1], score[p]
        live = a > 0
        if live.any():
            gap_p = float(((a - b)[live] / a[live]).min())
    return gap_r, gap_p


def nmfcross_ld(X, W0, r, p, c, iters, seed):
    """(H1 at long double, decision margins): how far that run's last iteration is from deciding otherwise -- (the smallest
    relative gap between a temporal-sparsity centre and the largest other value of its zero-padded window, where either is
    non-zero; the smallest relative gap between the p-th and the (p + 1)-th largest H * energy of a frame, where the p-th is
    non-zero).  inf where nothing is decided (iters == 0, r == 1, p == K)."""
    found = []
    H1 = nmfcross(X, W0, r, p, c, iters, seed, dtype=np.longdouble, last=lambda H, e: found.append(_margins(H, e, r, p, iters)))
    return H1, (found[0] if found else (np.inf, np.inf))


def decision_margins(X, W0, r, p, c, iters, seed):
    return nmfcross_ld(X, W0, r, p, c, iters, seed)[1]


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


# ---- the same at long double ------------------------------------------------------------------------------------------
def istft_ld(spec, n, win, fft, hop):
    """istft() at long double: the inverse transform is stft_ref.fft_ld by conjugation over the Hermitian extension (its real
    part: the imaginary parts of the DC and Nyquist bins drop out, as in irfft), window, overlap-add and quotient in long
    double as in istft_ref.istft"""
    LD, CLD = stft_ref.LD, stft_ref.CLD
    spec = np.asarray(spec, dtype=CLD)
    T = spec.shape[0]
    full = np.zeros((T, fft), dtype=CLD)
    full[:, :fft // 2 + 1] = spec
    full[:, fft // 2 + 1:] = np.conj(spec[:, 1:fft // 2][:, ::-1])
    w = oracle_np.hann(win).astype(LD)
    frames = (np.conj(stft_ref.fft_ld(np.conj(full))).real / LD(fft))[:, :win] * w[None, :]
    size = (T - 1) * hop + win
    acc, nrm = np.zeros(size, dtype=LD), np.zeros(size, dtype=LD)
    for t in range(T):
        acc[t * hop:t * hop + win] += frames[t]
        nrm[t * hop:t * hop + win] += w * w
    y = acc / np.maximum(nrm, LD(EPS))
    out = np.zeros(n, dtype=LD)
    m = max(0, min(n, size - win // 2))
    out[:m] = y[win // 2:win // 2 + m]
    return out


def griffinlim_ld(spec, n, iters, win, fft, hop, seed):
    """griffinlim() at long double: stft_ref.stft_ld forward, istft_ld back, the same phase draws (the doubles the host draws)"""
    LD, CLD = stft_ref.LD, stft_ref.CLD
    c = LD(0.9) / (LD(1) + LD(0.9))
    spec = np.asarray(spec, dtype=CLD)
    mag = np.abs(spec)
    T, F = spec.shape
    phase = random_phase(T, F, seed).astype(CLD)
    estimate = np.zeros((T, F), dtype=CLD)
    for _ in range(iters):
        prev = estimate
        x = istft_ld(mag * phase, n, win, fft, hop)
        estimate, _m = stft_ref.stft_ld(x, win, fft, hop)
        phase = estimate - c * prev
        phase = phase / (np.abs(phase) + LD(EPS))
    return mag * phase


def gl_frame_err(got, ref):
    """the largest, over frames, of max_f |got - ref| / max_f |ref| of that frame; a frame whose reference is all zero must be
    all zero.  No frame is exempted."""
    return stft_ref.frame_err(got, ref)[0]


# ---- the cases tests/test_gpu_nmfcross.py runs and tests/test_nmfcross_ref.py derives the bars on ---------------------------
# (K, T, F): source frames, target frames, bins.  EDGE: M or N of a GEMM one below, at and above the 64 / 128 tiles, a
# contraction of 1, 15, 16, 17, and depths at which a three-way split's last chunk is short
SMALL = [(1, 4, 33), (3, 5, 9), (37, 61, 129)]
EDGE = [(1, 1, 1), (16, 64, 17), (17, 65, 16), (15, 63, 33), (65, 129, 127), (129, 127, 65), (33, 128, 129)]
RPC = [(7, 11, 7), (1, 1, 1), (3, None, 5), (9, 1, 3), (4, 2, 6), (99, 1, 99)]     # (p None: the rank)
ITERS = (0, 1, 2, 3, 10, 50)
H_SEED = 42
SILENCE = (20, 30, 33)
SILENCE_RPC = (5, 3, 5)
SILENCE_ITERS = (2, 10)
LONG = (5, 65541, 3)                 # frames past the 65535 rows of a grid
LONG_RPC = (5, 3, 5)
LONG_ITERS = 2
STRIDED = ((20, 30, 65), 2, (3, 4, 3), 4, 9)      # shape, input seed, rpc, iterations, H seed
# the larger shapes of the GPU file that long double products still reach in seconds, the same five fields: 259 x 173 at
# every count and constraint set it runs, the forced GEMM forms' shape, the wide A/B path's.  1500 x 700 x 513 (5
# iterations) and 2600 x 1700 x 513 (2) are NOT here -- half a minute each without a BLAS -- and take the bar of their count
MEDIUM = [((259, 173, 513), 7, rpc, iters, 3) for iters in (1, 2, 50) for rpc in RPC[:4]] + [
    ((300, 200, 513), 17, (7, 11, 7), 3, 4), ((300, 200, 513), 17, (3, 300, 5), 1, 4), ((150, 90, 257), 19, (7, 11, 7), 5, 8)]
GL_CASES = [(3000, 256, 512, 64), (5000, 1024, 1024, 512), (2500, 200, 256, 100)]      # n, win, fft, hop
GL_ITERS = (0, 1, 2, 3, 50)
GL_SEED = 8
# (n_src, n_tgt, win, fft, hop): default FFT settings, win < fft, fft 2048, target shorter / longer than the source
CLIENT = [(22050, 22050, 1024, 1024, 512), (20000, 9000, 1000, 1024, 250), (30000, 26000, 2048, 2048, 512),
          (15000, 40000, 1024, 1024, 512), (26000, 3 * 512 + 100, 1024, 1024, 512)]


def forced_splits(Kd, split, depth=16):
    """(splits, split depth) the measurement build's FLUHIP_CROSS_SPLIT=split leaves of a contraction of Kd (cross_gemm_plan):
    chunks of whole stages of `depth`"""
    want = max(1, min(split, -(-Kd // depth)))
    chunk = -(-(-(-Kd // want)) // depth) * depth
    return -(-Kd // chunk), chunk


def rpc_of(rpc, K):
    """(r, p, c) with the client's polyphony min(source frames, polyphony)"""
    r, p, c = rpc
    return r, (K if p is None else min(p, K)), c


@functools.lru_cache(maxsize=None)
def audio_inputs_shared(K, T, F, seed):
    """audio_inputs, computed once and read-only"""
    X, W0 = audio_inputs(K, T, F, seed)
    X.setflags(write=False)
    W0.setflags(write=False)
    return X, W0


def audio_inputs(K, T, F, seed):
    """(X [T, F], W0 [K, F]): magnitudes of real audio -- the constraint comparisons then see the value spread the client sees"""
    rng = np.random.default_rng(seed)
    fft = 2 * (F - 1)
    hop = max(1, fft // 4)
    src = oracle_np.synth_audio(max(1, K * hop - hop // 2), 300 + seed)
    tgt = oracle_np.synth_audio(max(1, T * hop - hop // 2), 400 + seed)
    if fft >= 4:
        W0 = oracle_np.stft(src, fft, fft, hop)[1][:K]
        X = oracle_np.stft(tgt, fft, fft, hop)[1][:T]
    else:
        W0, X = rng.random((K, F)), rng.random((T, F))
    W0 = np.vstack([W0, rng.random((K - W0.shape[0], F))]) if W0.shape[0] < K else W0
    X = np.vstack([X, rng.random((T - X.shape[0], F))]) if X.shape[0] < T else X
    return np.ascontiguousarray(X), np.ascontiguousarray(W0)


def lognormal_inputs(K, T, F, seed):
    """log-normal magnitudes over about six decades (sigma 2.3 in the natural logarithm: +- 3 sigma = +- 3 decades)"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(0.0, 2.3, (T, F))), np.exp(rng.normal(0.0, 2.3, (K, F)))


@functools.lru_cache(maxsize=None)
def loop_inputs(K, T, F):
    """the input of an H-loop shape: audio magnitudes where 2 (F - 1) is a power of two, log-normal ones elsewhere"""
    fft = 2 * (F - 1)
    pow2 = fft >= 2 and fft & (fft - 1) == 0
    X, W0 = (audio_inputs if pow2 else lognormal_inputs)(K, T, F, K + T + F)
    X.setflags(write=False)
    W0.setflags(write=False)
    return X, W0


@functools.lru_cache(maxsize=None)
def silence_inputs():
    """digital silence: target frames 0, 7 .. 9 and T - 1 all zero, source frames 3 and K - 1 all zero"""
    K, T, F = SILENCE
    X, W0 = audio_inputs(K, T, F, K + T + F)
    X[[0, 7, 8, 9, T - 1]] = 0.0
    W0[[3, K - 1]] = 0.0
    X.setflags(write=False)
    W0.setflags(write=False)
    return X, W0


def bar_cases(iters):
    """[(name, X, W0, (r, p, c), H seed)]: every input and constraint set the GPU file runs at this iteration count on a shape
    small enough for long double products"""
    cases = []
    if iters in ITERS:
        for K, T, F in SMALL + EDGE:
            X, W0 = loop_inputs(K, T, F)
            for rpc in RPC:
                cases.append((f"{K}x{T}x{F} rpc {rpc_of(rpc, K)}", X, W0, rpc_of(rpc, K), H_SEED))
    if iters in SILENCE_ITERS:
        cases.append(("silence", *silence_inputs(), SILENCE_RPC, H_SEED))
    if iters == LONG_ITERS:
        cases.append(("65541 frames", *loop_inputs(*LONG), LONG_RPC, H_SEED))
    for (K, T, F), seed, rpc, n, hseed in [STRIDED] + MEDIUM:
        if n == iters:
            cases.append((f"{K}x{T}x{F} rpc {rpc_of(rpc, K)}", *audio_inputs_shared(K, T, F, seed), rpc_of(rpc, K), hseed))
    return cases


def gl_input(n, win, fft, hop):
    x = oracle_np.synth_audio(n, 21)
    return oracle_np.stft(x, win, fft, hop)[0] * (1.0 + 0.5j)


def client_audio(n_src, n_tgt):
    return oracle_np.synth_audio(n_src, 31).astype(np.float32), oracle_np.synth_audio(n_tgt, 32).astype(np.float32)


def client_rpc(n_tgt, hop):
    c = min(7, (n_tgt + hop) // hop)    # the last CLIENT case: target frames == continuity (the boundary of the check)
    return min(7, c), 11, c


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


def e2e_floor(source, target, win, fft, hop, r, p, c, iters, seed, gl_iters=50):
    """max |a - b| / max |b| of the client's double output before its float rounding: a with the float64 Griffin-Lim and
    inverse, b with the long double ones, both from the same (float64) H1"""
    src = np.asarray(source, dtype=np.float32).astype(np.float64)
    tgt = np.asarray(target, dtype=np.float32).astype(np.float64)
    src_spec, W = oracle_np.stft(src, win, fft, hop)
    H1 = nmfcross(oracle_np.stft(tgt, win, fft, hop)[1], W, r, min(W.shape[0], p), c, iters, seed)
    result = H1 @ src_spec
    a = istft(griffinlim(result, len(tgt), gl_iters, win, fft, hop, seed), len(tgt), win, fft, hop)
    b = istft_ld(griffinlim_ld(result, len(tgt), gl_iters, win, fft, hop, seed), len(tgt), win, fft, hop)
    return float(np.abs(a - b).max() / np.abs(b).max())
