"""NMF::processFrame (alg/NMF.hpp:45-89) for ALL frames of a magnitude matrix at once, in plain float64 numpy: the reference
fluhip_nmf_process_frames_f64 and, behind the STFT, fluhip_nmfmatch_f32 / fluhip_nmffilter_f32 are held to frame by frame
(tests/test_gpu_frames.py).  tests/test_frames_ref.py holds it against oracle_np.nmf_process_frame and the C oracle row by
row, against its own long double form, and measures on it what the device's documented quotient may cost -- the bars of
the GPU file are derived there, on the CPU.

Everything here is deterministic and cached: a reference is computed once and shared (read-only) by the tests that need it.
"""
import ctypes
import functools

import numpy as np

import oracle_np

EPS = oracle_np.EPS

# ---- the shapes (T, F, K) of fluhip_nmf_process_frames_f64's tests, by the planner's answer for one buffer of T frames --------
# (fluhip_debug_plan_shape with B = 1; test_frames_ref.py asserts every regime named here)
SHAPES = {
    "strip": [(300, 513, 5), (2000, 513, 16), (1040, 3, 2)],
    "strip_edge": [(12288, 33, 3), (12289, 33, 3)],                       # the last strip shape, the first that is not
    "tiny": [(1, 513, 32), (31, 513, 32), (33, 513, 32)],                 # around the padding of the rows to 32
    "split1_many_strips": [(4200, 33, 32), (2100, 33, 128), (2100, 33, 100)],
    "uniform_split": [(300, 1025, 32), (1100, 2049, 72), (6000, 513, 40), (9000, 513, 128)],
    "lists": [(4200, 1025, 20), (8200, 513, 32), (9000, 513, 64), (2100, 2049, 33)],
    "any_rank": [(300, 129, 130), (2100, 33, 200), (65535, 3, 130)],
}
ALL_SHAPES = [s for group in SHAPES.values() for s in group]
ITER_SHAPES = [(300, 513, 5), (4200, 33, 32), (4200, 1025, 20)]           # run at 0, 1, 25 and 50 iterations as well
ITER_COUNTS = (0, 1, 25, 50)
STRIDED_SHAPES = [(300, 513, 5), (4200, 1025, 20)]                        # one strip shape, one work-list shape
REFUSED_SHAPE = (65536, 3, 130)                                           # one frame past the any-rank kernels' limit
SEED = 42


def shape_id(s):
    return "x".join(str(v) for v in s)


def plan_shape(lib, T, F, K, B=1):
    """the planner's whole answer for B buffers of T frames (fluhip_debug_plan_shape, no device) as a dict of the slots the
    frame tests read"""
    out = (ctypes.c_int64 * 32)()
    assert lib.fluhip_debug_plan_shape(B, T, F, K, out) == 0, (B, T, F, K)
    p = [int(v) for v in out]
    return dict(variant=p[0], nsplitH=p[2], Kp=p[6], Kc=p[7], strip=p[8], lists=p[9], tailSplitH=p[10], stripsH=p[14])


# ---- the solve -----------------------------------------------------------------------------------------------------------
def normalised_dictionary(W0, dtype=np.float64):
    """:59, 64-65  W = max(W0, eps), every component divided by its L2 norm over the bins"""
    W = np.maximum(np.asarray(W0, dtype=dtype), dtype(EPS))
    return W / np.sqrt((W * W).sum(axis=1, keepdims=True))


def process_frames(X, W0, iters, seed, dtype=np.float64, perturb=None):
    """X [T, F], W0 [K, F] -> H [T, K], V = H W [T, F].  `perturb(q, it)` is applied to the quotient v0 / v1 of iteration `it`
    (the only place where the device departs from plain double arithmetic: test_frames_ref.py)."""
    W = normalised_dictionary(W0, dtype)
    den = np.maximum(W.sum(axis=1), dtype(EPS))                      # :66  the denominator: row sums of W
    v0 = np.maximum(np.asarray(X, dtype=dtype), dtype(EPS))          # :57-58, 61
    T, K = v0.shape[0], W.shape[0]
    h0 = np.maximum(oracle_np.rng_uniform01(seed, K), EPS).astype(dtype)   # :55-56, 60: the same K draws in every frame
    H = np.tile(h0, (T, 1))
    WT = np.ascontiguousarray(W.T)
    for it in range(iters):                                          # :71-79
        v1 = np.maximum(H @ W, dtype(EPS))
        q = v0 / v1
        if perturb is not None:
            q = perturb(q, it)
        H = H * (q @ WT) / den
    return H, H @ W


def rowrel(a, b):
    """max over rows of (max|a_row - b_row| / max|b_row|): THE error measure of H and V; no row is exempted"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.ndim == 2
    num = np.abs(a - b).max(axis=1)
    den = np.abs(b).max(axis=1)
    assert (den > 0).all()
    return float((num / den).max())


# ---- inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_input(T, F, K):
    """test_process_frames_vs_oracle's recipe (sparse activations of a cubed-uniform dictionary plus a noise floor), every row
    at a level of its own over twelve decades; one silent row, the leading bins of row 0 and of component 0 at zero (the
    max(x, eps) and max(W, eps) clamps)"""
    rng = np.random.default_rng(T + K)
    W0 = rng.random((K, F)) ** 3
    acts = rng.random((T, K)) * (rng.random((T, K)) < 0.4)
    X = acts @ W0 + 1e-3 * rng.random((T, F))
    X *= 10.0 ** rng.uniform(-9, 3, (T, 1))
    if T > 2:
        X[T // 2] = 0.0
    X[0, :7] = 0.0
    W0[0, :3] = 0.0
    X.setflags(write=False)
    W0.setflags(write=False)
    return X, W0


@functools.lru_cache(maxsize=None)
def reference(T, F, K, iters):
    """(H, V) of frames_input(T, F, K) at SEED: computed once, shared, read-only"""
    X, W0 = frames_input(T, F, K)
    H, V = process_frames(X, W0, iters, SEED)
    H.setflags(write=False)
    V.setflags(write=False)
    return H, V


def quotient_cost(T, F, K, iters):
    """what a relative error of 2^-46 in every quotient may cost at this shape: the larger rowrel (over H and V) against the
    unperturbed run of the one-sided perturbation (1 + 2^-46), the worst case, and of (1 + 2^-46 u), u uniform in [-1, 1]"""
    X, W0 = frames_input(T, F, K)
    H, V = reference(T, F, K, iters)
    d = 2.0 ** -46
    rs = np.random.RandomState(T + F + K + iters)
    one = process_frames(X, W0, iters, SEED, perturb=lambda q, it: q * (1.0 + d))
    rnd = process_frames(X, W0, iters, SEED, perturb=lambda q, it: q * (1.0 + d * rs.uniform(-1.0, 1.0, q.shape)))
    return (max(rowrel(one[0], H), rowrel(one[1], V)), max(rowrel(rnd[0], H), rowrel(rnd[1], V)))


# ---- NMFMatch / NMFFilter in double ----------------------------------------------------------------------------------------
def level_step_audio(n, seed):
    """oracle_np.synth_audio with a 60 dB step of level halfway through: the quiet half is what a normwise bar cannot see"""
    x = oracle_np.synth_audio(n, seed).astype(np.float64)
    x[n // 2:] *= 1e-3
    return x.astype(np.float32)


def match_geometry(n, win, hop, padding_mode):
    """(columns, start of the frame behind column 0, first column that has a frame) of oracle_np.nmfmatch_channel: kept
    column k is the frame at audio sample (k + latencyHops - 1) hop - win - padding; with no latency column 0 stays zero"""
    T, _ = oracle_np.feature_frames(n, win, hop, padding_mode)
    pad = oracle_np.feature_padding(win, hop, padding_mode)
    lat = win // hop
    return T, (lat - 1) * hop - win - pad, 1 if lat == 0 else 0


def filter_geometry(n, win, hop):
    """(frames, start of frame 0) of oracle_np.nmffilter_channel: frames m = 1, 2, ... at m hop - win while that is < n"""
    return (n + win + hop - 1) // hop - 1, hop - win


def spectra_numpy(audio, first, count, win, fft, hop):
    """complex [count, F]: the windowed transforms (numpy's FFT) of the frames at first + i hop, zeros outside the audio"""
    audio = np.asarray(audio, dtype=np.float64)
    n = audio.shape[0]
    idx = first + hop * np.arange(count)[:, None] + np.arange(win)[None, :]
    ok = (idx >= 0) & (idx < n)
    frames = np.where(ok, audio[np.clip(idx, 0, n - 1)], 0.0) * oracle_np.hann(win)[None, :]
    spec = np.fft.rfft(frames, n=fft, axis=1)
    spec[:, 0] = spec[:, 0].real
    spec[:, -1] = spec[:, -1].real
    return spec


def spectra_oracle(oracle, audio, first, count, win, fft, hop):
    """the same frames through the C oracle's STFT (its own FFT): the audio is placed in a zero buffer so that the oracle's
    frame j0 + i, which starts win / 2 before sample (j0 + i) hop, is the frame at first + i hop"""
    audio = np.asarray(audio, dtype=np.float64)
    n = audio.shape[0]
    j0 = max(0, -(-(first + win // 2) // hop))
    off = j0 * hop - first - win // 2
    assert off >= 0
    buf = np.zeros(max(off + n, (j0 + count) * hop))
    buf[off:off + n] = audio
    spec, _ = oracle.stft(buf, win, fft, hop)
    assert spec.shape[0] >= j0 + count
    return spec[j0:j0 + count]


def nmfmatch_double(audio, bases, win, fft, hop, seed, padding_mode=1, spectra=spectra_numpy):
    """oracle_np.nmfmatch_channel in closed form and in double throughout: [K, T] float64 (no float32 rounding)"""
    n = len(audio)
    bases = np.asarray(bases, dtype=np.float32).astype(np.float64)
    T, first, k0 = match_geometry(n, win, hop, padding_mode)
    out = np.zeros((bases.shape[0], max(T, 0)))
    if T > k0:
        mag = np.abs(spectra(audio, first + k0 * hop, T - k0, win, fft, hop))
        out[:, k0:] = process_frames(mag, bases, 10, seed)[0].T
    return out


def nmffilter_double(audio, bases, win, fft, hop, iters, seed, spectra=spectra_numpy):
    """oracle_np.nmffilter_channel in double throughout: [K, n] float64.  Per frame processFrame, the ratio mask of every
    component (alg/RatioMask.hpp:39-56, exponent 1), the inverse frame windowed and overlap-added where it came from, divided
    by the overlap-added window^2"""
    audio = np.asarray(audio, dtype=np.float64)
    n = audio.shape[0]
    bases = np.asarray(bases, dtype=np.float32).astype(np.float64)
    K = bases.shape[0]
    T, first = filter_geometry(n, win, hop)
    X = spectra(audio, first, T, win, fft, hop)
    H, V = process_frames(np.abs(X), bases, iters, seed)
    Wn = normalised_dictionary(bases)
    mult = 1.0 / np.maximum(V, EPS)
    w = oracle_np.hann(win)
    acc = np.zeros((K, n + 2 * win))
    nrm = np.zeros(n + 2 * win)
    for t in range(T):
        nrm[(t + 1) * hop:(t + 1) * hop + win] += w * w
    for i in range(K):
        mask = np.minimum(1.0, H[:, i:i + 1] * Wn[i][None, :] * mult)
        y = np.fft.irfft(X * mask, n=fft, axis=1)[:, :win] * w[None, :]
        for t in range(T):
            acc[i, (t + 1) * hop:(t + 1) * hop + win] += y[t]
    return (acc / np.maximum(nrm, EPS)[None, :])[:, win:win + n]
