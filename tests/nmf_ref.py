"""NMF::process (alg/NMF.hpp:91-176) -- the whole multiplicative-update loop, W and H -- in plain numpy at float64 or long
double: the reference fluhip_nmf_process_f64 and fluhip_corpus_nmf are held to ENTRY BY ENTRY (tests/test_gpu_nmf.py).
tests/test_nmf_ref.py holds it against oracle_np.nmf_process bit for bit, against the C oracle and against its own long
double form, and measures on it what the device's documented quotient may cost -- the bars of the GPU file are derived
there, on the CPU.

Every term of these updates is positive, nothing cancels: the error measure is `elrel`, every entry relative to itself, no
entry exempted, exact zeros where the reference has exact zeros.  A measure relative to the matrix's peak cannot see the
Nyquist bin, a quiet frame's row of H or a decayed component; this one can.

Everything here is deterministic and cached: a reference is computed once and shared (read-only) by the tests that need it.
"""
import ctypes
import functools

import numpy as np

import oracle_np

EPS = oracle_np.EPS
SEED = 42

# ---- the shapes (B, T, F, K), by the regime fluhip_debug_plan_shape puts them into ------------------------------------------
# B = 1 runs through fluhip_nmf_process_f64 on a double matrix, B > 1 through fluhip_corpus_nmf on float audio (F = fft / 2 + 1,
# hop = fft / 4).  (512, 87, 129, 100) is the shape tests/test_gpu_corpus_plan.py names as running in round-major windows; the
# windows are decided in the iteration loop from strip counts no planner slot reports, so that is taken from there and NOT
# asserted here.  Every entry is the smallest shape found of its regime (a CPU search over the planner's answer, from
# tests/test_gpu_corpus_plan.py::SHAPES and frames_ref.SHAPES); test_nmf_ref.py asserts each regime's predicate.
SHAPES = {
    "frame_strip": [(1, 87, 129, 3), (1, 33, 100, 16), (1, 1040, 3, 2)],
    "strip_edge": [(1, 12288, 33, 3), (1, 12289, 33, 3)],          # the last strip shape, the first that is not
    # deferred normalisation, whole contractions; the Nyquist bin as a side column ...
    "uniform_side_column": [(1, 33, 33, 32), (512, 87, 257, 32)],
    "uniform_no_side_column": [(1, 87, 33, 128)],                  # ... and with every bin in the strips
    "split_w": [(1, 173, 33, 20)],                                 # nsplitW > 1
    "split_h": [(1, 1, 513, 32), (1, 31, 513, 32), (1, 32, 513, 32), (1, 33, 513, 32)],   # nsplitH > 1, T around the row padding
    "two_launch_h": [(128, 257, 129, 100)],                        # tailSplitH > 0
    "many_h_strips": [(1, 4200, 33, 32)],                          # more than 64 strips of the H update
    "lists_plain_rank": [(8, 173, 513, 32)],
    "lists_compute_rank": [(8, 173, 513, 20)],                     # arrays of rank 32, the updates compute 24
    "uniform_off_size": [(512, 87, 129, 100)],                     # arrays of rank 128, the updates compute 104
    "any_rank": [(2, 87, 129, 200), (1, 87, 129, 130)],            # K > 128
}
# either side of every padded rank, one buffer of 33 frames x 100 bins (a bin count that is no 2^k + 1); 16 is in frame_strip,
# 130 (past the last padded rank, 128) in any_rank
RANK_EDGE_SHAPES = [(1, 33, 100, K) for K in (17, 24, 25, 32, 33, 40, 41, 64, 65, 128)]
ONE_BUFFER_SHAPES = [s for group in SHAPES.values() for s in group if s[0] == 1] + RANK_EDGE_SHAPES
CORPUS_SHAPES = [s for group in SHAPES.values() for s in group if s[0] > 1]
ITER_SHAPES = [(1, 87, 129, 3), (1, 33, 33, 32), (8, 173, 513, 20)]       # one strip, one uniform, one work-list shape
ITER_COUNTS = (0, 1, 2, 7, 8, 9, 10, 30)                                  # 7, 8, 9 straddle the progress-lag window
# ... of which the work-list shape, a corpus of audio, runs all but 30: by then plain float64 rounding on audio (7.2e-13 from
# long double, in entries that decayed fifteen decades under their frame's peak) is so close to what a quotient error of 2^-40
# costs (9.5e-13) that no bar 8 x above the one can refuse the other (test_nmf_ref.py)
AUDIO_ITER_COUNTS = ITER_COUNTS[:-1]
# one shape per regime family: strip, uniform, split contraction, any-rank -- and the work lists as a corpus
MODE_SHAPES = [(1, 87, 129, 3), (1, 33, 33, 32), (1, 33, 513, 32), (1, 87, 129, 130)]
MODE_CORPUS_SHAPE = (8, 173, 513, 20)
MODES = [(True, True), (False, True), (True, False), (False, False)]
STRIDED_SHAPES = [(1, 87, 129, 3), (1, 33, 33, 32)]
CANCEL_SHAPE = (1, 87, 129, 3)
CANCEL_AT = 5
# the ragged corpus: fft 1024, hop 256; frames (n + hop) // hop = 31, 32, 32, 33, 34 -- around 32 and one apart
RAGGED_LENS = [7700, 7936, 8000, 8200, 8448]
RAGGED_RANKS = (5, 32)


def bar_buffers(shape):
    """the buffers of a corpus shape whose reference test_nmf_ref.py measures the bar on: four spread over the corpus (the GPU
    file compares every buffer; numpy's long double products are slow, and a run of each of 512 buffers would take minutes)"""
    B = shape[0]
    return tuple(sorted({0, B // 3, 2 * B // 3, B - 1}))


def shape_id(s):
    return "x".join(str(v) for v in s)


def plan_shape(lib, B, T, F, K):
    """the planner's 32 slots for B buffers of T frames (fluhip_debug_plan_shape, no device)"""
    out = (ctypes.c_int64 * 32)()
    assert lib.fluhip_debug_plan_shape(B, T, F, K, out) == 0, (B, T, F, K)
    return [int(v) for v in out]


def _uniform(p):
    return p[0] == 5 and p[3] == 1 and not p[9] and not p[8] and p[1] == 1 and p[2] == 1 and p[10] <= 1


# what puts a plan into a regime (slots as corpus_plan.hip fluhip_debug_plan_shape documents them)
REGIMES = {
    "frame_strip": lambda p: p[8] == 1 and p[6] == 16,
    "strip_edge": lambda p: p[6] == 16,                                         # (which side: test_nmf_ref.py)
    "uniform_side_column": lambda p: _uniform(p) and p[4] == 1 and p[7] == p[6],
    "uniform_no_side_column": lambda p: _uniform(p) and p[4] == 0 and p[7] == p[6],
    "split_w": lambda p: p[0] == 5 and not p[9] and not p[8] and p[1] > 1,
    "split_h": lambda p: p[0] == 5 and not p[9] and not p[8] and p[2] > 1,
    "two_launch_h": lambda p: p[10] > 1,
    "many_h_strips": lambda p: p[0] == 5 and not p[9] and not p[8] and p[14] > 64,
    "lists_plain_rank": lambda p: p[9] == 1 and p[7] == p[6],
    "lists_compute_rank": lambda p: p[9] == 1 and p[7] != p[6],
    "uniform_off_size": lambda p: _uniform(p) and p[7] != p[6],
    "any_rank": lambda p: p[0] == 0 and p[6] > 128,
}


# ---- the solve -----------------------------------------------------------------------------------------------------------
def nmf_process(X, K, iters, updateW=True, updateH=True, seed=SEED, W0=None, H0=None, dtype=np.float64, perturb=None):
    """X [T, F] -> W1 [K, F], H1 [T, K], V1 = H1 W1 [T, F]: oracle_np.nmf_process operation by operation (so that at float64
    and without a hook the two are the same bits), in `dtype`.  `perturb(q, which, it)` is applied to the quotient
    V / max(W H, eps) of the W update (which = "W") and of the H update ("H") of iteration `it` -- the only place where the
    device departs from plain double arithmetic (a Newton-refined reciprocal, relative error <= 2^-46)."""
    eps = dtype(EPS)
    X = np.asarray(X, dtype=dtype)
    T, F = X.shape
    if W0 is None:
        W = oracle_np.rng_uniform01(seed, F * K).reshape(K, F).T.astype(dtype, order="C")     # column-major F x K fill
    else:
        W = np.asarray(W0, dtype=dtype).T.copy()
    if H0 is None:
        H = oracle_np.rng_uniform01(seed, K * T).reshape(T, K).T.astype(dtype, order="C")     # column-major K x T fill
    else:
        H = np.asarray(H0, dtype=dtype).T.copy()
    V = X.T.copy()
    H = np.maximum(H, eps)
    W = np.maximum(W, eps)
    W = W / np.sqrt((W * W).sum(axis=0, keepdims=True))
    H = H / np.sqrt((H * H).sum(axis=1, keepdims=True))
    for it in range(iters):
        if updateW:
            q = V / np.maximum(W @ H, eps)
            if perturb is not None:
                q = perturb(q, "W", it)
            wnum = q @ H.T
            wden = H.sum(axis=1)[None, :]
            W = W * wnum / np.maximum(wden, eps)
            if W.max() > eps:
                W = W / np.sqrt((W * W).sum(axis=0, keepdims=True))
        if updateH:
            q = V / np.maximum(W @ H, eps)
            if perturb is not None:
                q = perturb(q, "H", it)
            hnum = W.T @ q
            hden = W.sum(axis=0)[:, None]
            H = H * hnum / np.maximum(hden, eps)
    return W.T.copy(), H.T.copy(), (W @ H).T.copy()


# ---- the error measures -----------------------------------------------------------------------------------------------------
def elrel(got, want):
    """THE error measure: the largest |got - want| / want over every entry with want > 0, and got == 0 exactly wherever
    want == 0.  No entry is exempted."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all() and (want >= 0).all()
    zero = want == 0
    assert not got[zero].any(), f"{int(np.count_nonzero(got[zero]))} entries are not zero where the reference is exactly zero"
    if zero.all():
        return 0.0
    live = ~zero
    return float((np.abs(got[live] - want[live]) / want[live]).max())


def _rowrel(a, b, axis):
    num = np.abs(np.asarray(a) - np.asarray(b)).max(axis=axis)
    den = np.abs(np.asarray(b)).max(axis=axis)
    ok = den > 0
    assert not num[~ok].any()
    return float((num[ok] / den[ok]).max()) if ok.any() else 0.0


def rowrels(W, rW, H, rH):
    """(W per component, W per bin, H per frame, H per component): each row / column relative to its own peak -- context
    beside elrel (what frames_ref.rowrel measures for processFrame)"""
    return (_rowrel(W, rW, 1), _rowrel(W, rW, 0), _rowrel(H, rH, 1), _rowrel(H, rH, 0))


# ---- inputs: one buffer of doubles ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nmf_input(T, F, K):
    """frames_ref.frames_input's recipe (sparse activations of a cubed-uniform dictionary plus a noise floor) with every
    frame at a level of its own, spread evenly over nine decades (10^-6 .. 10^3) in a shuffled order; frame T // 2 silent
    (T > 2), bin F // 3 all zero (F > 2), and the last bin scaled by 1e-9 -- where the Nyquist bin of real audio sits"""
    rng = np.random.default_rng(1000 * T + F + K)
    W0 = rng.random((K, F)) ** 3
    acts = rng.random((T, K)) * (rng.random((T, K)) < 0.4)
    X = acts @ W0 + 1e-3 * rng.random((T, F))
    X *= 10.0 ** rng.permutation(np.linspace(-6.0, 3.0, T))[:, None]
    if T > 2:
        X[T // 2] = 0.0
    if F > 2:
        X[:, F // 3] = 0.0
    X[:, F - 1] *= 1e-9
    X.setflags(write=False)
    return X


def seed_factors(T, F, K, which=0):
    """float32 seeds W0 [K, F], H0 [T, K] (the corpus takes floats: the reference gets the same rounded values)"""
    rs = np.random.RandomState(7 * T + F + K + which)
    W0 = rs.uniform(0.05, 1.0, (K, F)).astype(np.float32)
    H0 = rs.uniform(0.05, 1.0, (T, K)).astype(np.float32)
    return W0, H0


# ---- inputs: corpora of float audio ------------------------------------------------------------------------------------------
def corpus_geometry(T, F):
    """(n, win, fft, hop) of a corpus buffer with T frames of F bins: T = (n + hop) // hop (alg/STFT.hpp:98-99)"""
    fft = 2 * (F - 1)
    hop = fft // 4
    return (T - 1) * hop + hop // 2, fft, fft, hop


def level_segments(n, win):
    """[(start, stop, gain)]: 0, -40, -80, -120 dB and exact zeros (longer than a window plus a hop, so that at least one
    frame is silent), the zeros third"""
    zero = 2 * win
    rest = (n - zero) // 4
    cuts = [0, rest, 2 * rest, 2 * rest + zero, 3 * rest + zero, n]
    return list(zip(cuts[:-1], cuts[1:], (1.0, 1e-2, 0.0, 1e-4, 1e-6)))


def corpus_buffer(n, win, seed):
    x = oracle_np.synth_audio(n, seed).astype(np.float64)
    for a, b, g in level_segments(n, win):
        x[a:b] *= g
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def corpus_audio(B, T, F):
    """[B, n] float32: every buffer other audio (synth_audio(n, 6000 + b)), cut into the level segments"""
    n, win, _, _ = corpus_geometry(T, F)
    a = np.stack([corpus_buffer(n, win, 6000 + b) for b in range(B)])
    a.setflags(write=False)
    return a


def ragged_audio():
    return [corpus_buffer(n, 1024, 6500 + i) for i, n in enumerate(RAGGED_LENS)]


def corpus_seeds(B):
    """per-buffer seeds: neighbours differ, and two buffers share one (equal seeds are drawn once)"""
    return [42 + (b % 7) for b in range(B)]


@functools.lru_cache(maxsize=None)
def corpus_magnitudes_cpu(B, T, F, b):
    """the magnitudes of buffer b from oracle_np.stft: what the CPU derivation of the bar runs on (the GPU tests feed the
    reference the device's own magnitudes, so the STFT is no part of their comparison)"""
    n, win, fft, hop = corpus_geometry(T, F)
    mag = oracle_np.stft(corpus_audio(B, T, F)[b], win, fft, hop)[1]
    assert mag.shape == (T, F)
    mag.setflags(write=False)
    return mag


# ---- shared references -----------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def reference(T, F, K, iters, updateW=True, updateH=True, seeded=False):
    """(W1, H1, V1) of nmf_input(T, F, K) at SEED (seeded: from seed_factors): computed once, shared, read-only"""
    W0, H0 = seed_factors(T, F, K) if seeded else (None, None)
    return _frozen(*nmf_process(nmf_input(T, F, K), K, iters, updateW, updateH, SEED, W0, H0))


def worst_elrel(got, want):
    """the larger elrel over W and H"""
    return max(elrel(got[0], want[0]), elrel(got[1], want[1]))


# ---- what the bars are measured on: every input the GPU file runs, by family ---------------------------------------------------
def bar_cases(iters):
    """[(name, family, X, K, seed, W0, H0)]: every input tests/test_gpu_nmf.py runs at this iteration count.  family "doubles":
    one buffer of nmf_input; "audio": a buffer of a corpus, its magnitudes from oracle_np.stft here (the GPU tests feed the
    reference the device's own magnitudes, so the STFT is no part of their comparison)"""
    cases = []

    def doubles(shape, seeded=False):
        _, T, F, K = shape
        W0, H0 = seed_factors(T, F, K) if seeded else (None, None)
        cases.append((shape_id(shape) + (" seeded" if seeded else ""), "doubles", nmf_input(T, F, K), K, SEED, W0, H0))

    def audio(shape, seeded=False):
        B, T, F, K = shape
        for b in bar_buffers(shape):
            W0, H0 = seed_factors(T, F, K, which=b) if seeded else (None, None)
            cases.append((f"{shape_id(shape)} buffer {b}" + (" seeded" if seeded else ""), "audio", corpus_magnitudes_cpu(B, T, F, b),
                          K, corpus_seeds(B)[b], W0, H0))

    for shape in ITER_SHAPES:
        if shape[0] == 1:
            doubles(shape)
        elif iters in AUDIO_ITER_COUNTS:
            audio(shape)
    if iters == 10:
        for shape in ONE_BUFFER_SHAPES:
            if shape not in ITER_SHAPES:
                doubles(shape)
        for shape in CORPUS_SHAPES:
            if shape not in ITER_SHAPES:
                audio(shape)
        for shape in MODE_SHAPES:
            doubles(shape, seeded=True)
        audio(MODE_CORPUS_SHAPE, seeded=True)
        seeds = corpus_seeds(len(RAGGED_LENS))
        for K in RAGGED_RANKS:
            for b, x in enumerate(ragged_audio()):
                cases.append((f"ragged rank {K} buffer {b}", "audio", oracle_np.stft(x, 1024, 1024, 256)[1], K, seeds[b], None, None))
    if iters == 1:                                  # a fixed factor is held to the bar of one iteration
        for shape in MODE_SHAPES:
            if shape not in ITER_SHAPES:
                doubles(shape)
    return cases


def measure(X, K, iters, seed, W0=None, H0=None):
    """(one-sided 2^-46, random 2^-46, float64 against long double, one-sided 2^-40): elrel, the larger of W and H, of the
    reference with every quotient times (1 + 2^-46), times (1 + 2^-46 u) with u uniform in [-1, 1], of its long double form,
    and with every quotient times (1 + 2^-40) -- each against the plain float64 reference"""
    kw = dict(seed=seed, W0=W0, H0=H0)
    ref = nmf_process(X, K, iters, **kw)
    rs = np.random.RandomState(X.shape[0] + X.shape[1] + K + iters)
    d = 2.0 ** -46
    one = nmf_process(X, K, iters, perturb=lambda q, which, it: q * (1.0 + d), **kw)
    rnd = nmf_process(X, K, iters, perturb=lambda q, which, it: q * (1.0 + d * rs.uniform(-1.0, 1.0, q.shape)), **kw)
    ld = nmf_process(X, K, iters, dtype=np.longdouble, **kw)
    far = nmf_process(X, K, iters, perturb=lambda q, which, it: q * (1.0 + 2.0 ** -40), **kw)
    return worst_elrel(one, ref), worst_elrel(rnd, ref), worst_elrel(ref, ld), worst_elrel(far, ref)
