"""algorithm::STFT::process + FFT::process + STFT::magnitude (alg/STFT.hpp:90-108, 61-66; util/FFT.hpp:92-108) in numpy at long
double: the reference the forward STFT -- K1 in every form: the block kernel, the generic on-chip kernel, the global-memory
passes -- is held to FRAME BY FRAME (tests/test_gpu_stft.py).  tests/test_stft_ref.py holds this restatement against both
oracles and the committed goldens, derives the bars of the GPU file on the CPU, shows what the measure buys on deliberate
breaks, and pins every GPU shape to the dispatch branch it is meant to reach.

The error measure is `frame_err`: per frame, max_k |got - ref| / max_k |ref| -- every frame relative to its OWN peak, no frame
exempted, an exactly silent frame exactly zero.  A measure relative to the spectrogram's peak cannot see a quiet frame: an
error of 1e-9 in the quietest frame of a signal with a 120 dB envelope reads 1e-15 there.

Everything here is deterministic and cached: a reference is computed once and shared (read-only) by the tests that need it.
"""
import functools
import math

import numpy as np

import oracle_np

LD = np.longdouble
CLD = np.clongdouble
HALF_ULP = 2.0 ** -53
MAG_OF_SPEC_BAR = 4 * HALF_ULP     # two products, a sum and a correctly rounded square root stay under 2 ulp (fft_core.h:86-88
#                                    documents "rounding error only" for the device's form: no wider bound to quote)


# ---- tables ---------------------------------------------------------------------------------------------------------------
def window(kind, size):
    """the float64 window table as the library's host side makes it (alg/WindowFuncs.hpp:38-72 through libm, what
    api_core.hip make_window calls): the device multiplies by this table, so the reference does too.  kind 0 is
    oracle_np.hann's formula (test_stft_ref.py holds the two tables together)."""
    pi = math.pi
    if kind == 0:
        return np.array([0.5 - 0.5 * math.cos((pi * 2 * i) / size) for i in range(size)])
    if kind == 1:
        return np.array([(pi / size) * math.sin((2 * pi * i) / size) for i in range(size)])
    if kind == 2:
        return np.array([0.54 - 0.46 * math.cos((pi * 2 * i) / size) for i in range(size)])
    if kind == 3:                                    # (the three cosines share one argument, as written there)
        c = [math.cos((pi * 2 * i) / size) for i in range(size)]
        return np.array([0.35875 - 0.48829 * v + 0.14128 * v + 0.01168 * v for v in c])
    if kind == 4:
        assert size % 2 == 1
        sigma, h = float(size // 3), (size - 1) // 2
        return np.array([math.exp(-i * i / (2 * sigma * sigma)) for i in range(-h, h + 1)])
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _twiddles_ld(N):
    """e^{-2 pi i m / N}, m < N / 2, long double"""
    pi = 4 * np.arctan(LD(1))
    ang = -2 * pi * np.arange(N // 2).astype(LD) / LD(N)
    return (np.cos(ang) + 1j * np.sin(ang)).astype(CLD)


@functools.lru_cache(maxsize=None)
def _bitrev(N):
    bits = N.bit_length() - 1
    r = np.zeros(N, dtype=np.int64)
    for b in range(bits):
        r |= ((np.arange(N) >> b) & 1) << (bits - 1 - b)
    return r


def fft_ld(x):
    """[M, N] -> [M, N]: radix-2 decimation in time along the last axis, long double data and twiddles"""
    x = np.asarray(x, dtype=CLD)
    M, N = x.shape
    assert N >= 2 and N & (N - 1) == 0
    tw = _twiddles_ld(N)
    X = x[:, _bitrev(N)]
    size = 2
    while size <= N:
        half = size // 2
        X = X.reshape(M, N // size, 2, half)
        o = X[:, :, 1, :] * tw[:: N // size][None, None, :]
        e = X[:, :, 0, :]
        X = np.concatenate([e + o, e - o], axis=-1)
        size *= 2
    return X.reshape(M, N)


# ---- geometry -------------------------------------------------------------------------------------------------------------
def num_frames(n, hop):
    return (n + hop) // hop                                                   # alg/STFT.hpp:98-99


def bufstft_geometry(n, win, hop, mode):
    """(T, first sample of frame 0) of BufSTFT's three padding modes (nrt/BufSTFTClient.hpp:121-162)"""
    pad = [0, win >> 1, win - hop][mode]
    padded = n + 2 * pad
    if mode == 2:
        padded = -(-padded // hop) * hop
    return 1 + (padded - win) // hop, -pad


def frames_of(x, win, fft, hop, frames, offset=None, kind=0, dtype=LD):
    """the windowed, zero-padded frames [len(frames), fft]: frame t is samples [t hop + offset, + win), zero outside [0, n)"""
    x = np.asarray(x)
    n = x.shape[0]
    offset = -(win // 2) if offset is None else offset
    idx = np.asarray(frames, dtype=np.int64)[:, None] * hop + offset + np.arange(win)[None, :]
    ok = (idx >= 0) & (idx < n)
    fr = np.zeros((len(frames), fft), dtype=dtype)
    fr[:, :win] = np.where(ok, x[np.clip(idx, 0, n - 1)].astype(dtype), dtype(0)) * window(kind, win).astype(dtype)[None, :]
    return fr


def stft_ld(x, win, fft, hop, frames=None, offset=None, kind=0, T=None):
    """(spec clongdouble [len(frames), F], mag long double): the literal model at long double; `frames` names the frames to
    transform (all T = (n + hop) // hop by default; `T`, `offset`: BufSTFT's framing)"""
    assert np.finfo(LD).eps < 2e-19
    if frames is None:
        frames = np.arange(num_frames(len(x), hop) if T is None else T)
    spec = fft_ld(frames_of(x, win, fft, hop, frames, offset, kind))[:, :fft // 2 + 1].copy()
    spec[:, 0] = spec[:, 0].real                                             # util/FFT.hpp:99-101
    spec[:, -1] = spec[:, -1].real
    return spec, np.abs(spec)


def stft_f64(x, win, fft, hop, frames=None, offset=None, kind=0, T=None):
    """the same with numpy's float64 rfft: an independent double implementation (bars, and the bulk of large cases)"""
    if frames is None:
        frames = np.arange(num_frames(len(x), hop) if T is None else T)
    spec = np.fft.rfft(frames_of(x, win, fft, hop, frames, offset, kind, dtype=np.float64), axis=1)
    spec[:, 0] = spec[:, 0].real
    spec[:, -1] = spec[:, -1].real
    return spec, np.abs(spec)


# ---- the error measures -----------------------------------------------------------------------------------------------------
def frame_errs(got, ref):
    """per frame max_k |got - ref| / max_k |ref|; a frame that is exactly zero in the reference must be exactly zero"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.ndim == 2, (got.shape, ref.shape)
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    wide = CLD if (np.iscomplexobj(got) or np.iscomplexobj(ref)) else LD
    num = np.abs(got.astype(wide) - ref.astype(wide)).max(axis=1)
    den = np.abs(ref).max(axis=1)
    silent = den == 0
    assert not num[silent].any(), f"frames {np.flatnonzero(silent & (num != 0))[:8]} are not zero where the reference is exactly zero"
    out = np.zeros(len(den))
    out[~silent] = (num[~silent] / den[~silent]).astype(np.float64)
    return out


def frame_err(got, ref):
    """THE error measure: (the worst frame's error relative to that frame's own peak, its index).  No frame is exempted."""
    e = frame_errs(got, ref)
    if not len(e):
        return 0.0, -1
    t = int(np.argmax(e))
    return float(e[t]), t


def rel_err(got, ref):
    """the old measure: max |got - ref| / max |ref| over the whole spectrogram"""
    return float(np.abs(np.asarray(got).astype(CLD) - ref).max() / np.abs(ref).max())


def mag_of_spec_err(mag, spec):
    """the device's magnitudes against hypot of the device's OWN spectrum (np.hypot at long double, so that the reference
    adds no rounding of its own), each entry relative to itself; exactly zero where the spectrum is"""
    h = np.hypot(spec.real.astype(LD), spec.imag.astype(LD))
    assert mag.shape == h.shape
    zero = h == 0
    assert not mag[zero].any()
    return float((np.abs(mag.astype(LD)[~zero] - h[~zero]) / h[~zero]).max()) if (~zero).any() else 0.0


def check_layouts(mag, magT, Ts, F):
    """the two layouts as they lie on the device, mag [B, Tp, Fp] and magT [B, Fp, Tp]: the bin-major copy BIT-IDENTICAL to the
    transpose of the frame-major one over [F][T_b], and both exactly zero everywhere else -- the padding columns T .. Tp, the
    padding bins F .. Fp, and the frames past a ragged buffer's own"""
    B, Tp, Fp = mag.shape
    assert magT.shape == (B, Fp, Tp) and len(Ts) == B and F <= Fp and max(Ts) <= Tp
    for b, T in enumerate(Ts):
        assert np.array_equal(magT[b, :F, :T], mag[b, :T, :F].T), f"buffer {b}: the bin-major copy is not the transpose"
        assert not magT[b, :, T:].any(), f"buffer {b}: bin-major columns {T} .. {Tp} are not zero"
        assert not magT[b, F:, :].any() and not mag[b, :, F:].any(), f"buffer {b}: padding bins are not zero"
        assert not mag[b, T:, :].any(), f"buffer {b}: frame-major rows {T} .. {Tp} are not zero"


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def dynamics(n, seed, dtype="float32", decades=6.0):
    """white noise under an exponential envelope from 10^-decades to 1 across the buffer: every frame distinct, every frame at
    a scale of its own"""
    rs = np.random.RandomState(seed)
    env = 10.0 ** (-decades * (1.0 - np.arange(n) / max(n - 1, 1)))
    return _frozen((rs.standard_normal(n) * env * 0.25).astype(dtype))


@functools.lru_cache(maxsize=None)
def tones(n, seed, dtype="float32"):
    """a few sinusoids plus noise 60 dB down: a frame's peak stands well above its floor"""
    rs = np.random.RandomState(seed)
    t = np.arange(n)
    x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((0.5, 0.3, 0.15), rs.uniform(0.003, 0.45, 3), rs.uniform(0, 6.28, 3)))
    return _frozen((x + 1e-3 * rs.standard_normal(n)).astype(dtype))


INPUTS = {"dynamics": dynamics, "tones": tones}


@functools.lru_cache(maxsize=None)
def reference(family, n, seed, dtype, win, fft, hop, kind=0, stride=1):
    """(spec, mag) at long double of every frame of INPUTS[family](n * stride, seed, dtype)[::stride]: computed once, shared,
    read-only"""
    x = INPUTS[family](n * stride if stride > 1 else n, seed, dtype)[::stride]
    s, m = stft_ld(x, win, fft, hop, kind=kind)
    return _frozen(s), _frozen(m)


# ---- the dispatch of K1, restated from launch_stft (kernels_stft.hip) and launch_block_t (kernels_stft_block.hip) --------------
LDS = 160 * 1024
BLOCK_FORMS = {1024: (8, 8, 8, 16), 2048: (16, 8, 8, 8), 4096: (16, 8, 16, 4)}      # R1, R2, R3, wavefronts = frames per block
CHUNK_BYTES = 512 << 20


def block_form(win, fft, magT):
    """None, or the block kernel's launch constants for this shape"""
    if win % 2 or win > fft or fft not in BLOCK_FORMS:                        # fft_core_supported
        return None
    R1, R2, R3, NW = BLOCK_FORMS[fft]
    N = R1 * R2 * R3
    assert 2 * N == fft
    xl = N // (64 * R3) == 1                                                  # FftCore::XL (FLUHIP_SPLIT_VIA_LDS)
    bufd = N + N // 16 + (34 if xl else 2)                                    # FftCore::BUFD
    tw = (R2 - 1) * R1 + (R3 - 1) * R1 * R2                                   # FftCore::TW
    db = fft == 2048 and magT                                                 # two sets of staging buffers, window through L1
    winlds = not db
    shmem = (tw + (N if winlds else 0)) * 16 + (2 if db else 1) * NW * bufd * 8
    assert shmem <= LDS
    per_cu = max(1, LDS // shmem)
    return dict(NW=NW, FPB=NW, DB=db, WINLDS=winlds, shmem=shmem, cap=256 * per_cu,
                PREFETCH=(N // 64 == 16 and NW <= 12))


def block_dealing(B, T, fpb, cap):
    """[(round, workgroup, buffer, first frame)] of every block, in launch_block_t's grid and decode's dealing"""
    bpb = -(-T // fpb)
    total = B * bpb
    chunk = -(-total // 8)
    grid = min(8 * chunk, cap)
    out = []
    for L in range(8 * chunk):
        slot, blk = L >> 3, (L & 7) * chunk + (L >> 3)
        if slot >= chunk or blk >= total:
            continue
        out.append((L // grid, L % grid, blk // bpb, (blk % bpb) * fpb))
    return out


def dispatch(win, fft, B, T, magT=False, f32=True, n=None, hop=None):
    """the branch a launch of B x T frames takes: a dict with `branch` in {"block", "generic", "big"} and that branch's figures"""
    nc = fft // 2
    if 2 * nc * 2 * 8 > LDS:                                                  # stft_needs_scratch
        cf = max(1, CHUNK_BYTES // (nc * 16))
        cf = min(cf, max(B * T, 1))
        passes, Ns = [], 1
        while Ns < nc:
            r = 4 if nc // Ns >= 4 else 2
            passes.append(r)
            Ns *= r
        return dict(branch="big", chunk_frames=cf, chunks=-(-B * T // cf), last_radix=passes[-1])
    form = block_form(win, fft, magT)
    if form is not None:
        deal = block_dealing(B, T, form["FPB"], form["cap"])
        rounds = 1 + max(r for r, _, _, _ in deal)
        # the prefetched-samples path: float audio, a later round, an interior frame on an 8-byte base
        pre = 0
        if form["PREFETCH"] and f32 and n is not None:
            for r, g, b, t0 in deal:
                if r == 0:
                    continue
                for t in range(t0, min(t0 + form["FPB"], T)):
                    s0 = t * hop - win // 2
                    pre += s0 >= 0 and s0 + fft <= n and (b * n + s0) % 2 == 0
        return dict(branch="block", rounds=rounds, prefetched=int(pre), dealing=deal, **form)
    tw_lds = 3 * nc * 2 * 8 <= LDS
    win_lds = tw_lds and 3 * nc * 2 * 8 + win * 8 <= 80 * 1024
    return dict(branch="generic", twInLds=tw_lds, winInLds=win_lds, grid=min(B * T, 2048), threads=min(256, max(64, nc // 4)),
                strided=B * T > 2048)


# ---- the shapes of tests/test_gpu_stft.py ---------------------------------------------------------------------------------------
def n_for(T, hop, odd=True):
    """a sample count with T frames: (T - 1) hop + about half a hop, odd (or even)"""
    n = max((T - 1) * hop + hop // 2, 1)
    if hop > 1 and n % 2 != int(odd):                                         # (a hop of 1 fixes n's parity with T)
        n += 1 if num_frames(n + 1, hop) == T else -1
    assert num_frames(n, hop) == T, (T, hop, n)
    return n


BLOCK_FFTS = (1024, 2048, 4096)


def block_T(fft):
    fpb = BLOCK_FORMS[fft][3]
    return (fpb - 1, fpb, fpb + 1, 5 * fpb // 2)


SHORT_EVEN_WINDOWS = {1024: 1000, 2048: 2, 4096: 4000}
# one buffer, generic kernel: (win, fft, hop) -- every power of two whose even window has no block form, and the odd windows
GENERIC_POW2 = [(f, f, max(1, f // 4)) for f in (4, 8, 16, 32, 64, 128, 256, 512, 8192)]
GENERIC_ODD = [(1023, 1024, 256), (2047, 2048, 512), (4095, 4096, 1024), (8191, 8192, 2048)]
GENERIC_LDS = {1024: (True, True), 2048: (True, True), 4096: (True, False), 8192: (False, False)}       # twiddles, window in the LDS
GENERIC_STRIDE_CASE = (64, 64, 16, 2100)                                      # win, fft, hop, T: past the grid cap of 2048 frames
BIG_FFTS = (16384, 32768, 65536)
BIG_T = 12
CHUNK_CASE = (65536, 65536, 64, 66000)                                        # win, fft, hop, n: 1032 frames, a chunk holds 1024


def chunk_frames_named():
    win, fft, hop, n = CHUNK_CASE
    T = num_frames(n, hop)
    named = set(range(4)) | set(range(T - 4, T)) | set(range(1020, 1029)) | set(range(0, T, 64))
    return sorted(named)


# corpora (B, n, win, fft, hop); K is 2 throughout (the factor workspaces are not used)
def corpus_one_round(fft):
    fpb = BLOCK_FORMS[fft][3]
    hop = fft // 4
    return (3, n_for(2 * fpb + fpb // 2 + 1, hop), fft, fft, hop)             # a ragged last block, odd n


# more than one round of a workgroup: (B, n, win, fft, hop) with an even n and hop, and with an odd hop
MULTI_ROUND = {
    2048: [(6, 45000, 2048, 2048, 128), (6, 45001, 2048, 2048, 127)],          # 264 blocks of 8 frames (issue); 270
    1024: [(4, n_for(65 * 16, 64, odd=False), 1024, 1024, 64), (4, n_for(65 * 16, 63), 1024, 1024, 63)],      # 260 blocks of 16
    4096: [(4, n_for(65 * 4, 128, odd=False), 4096, 4096, 128), (4, n_for(65 * 4, 127), 4096, 4096, 127)],    # 260 blocks of 4
}


def ragged_lengths(fft):
    """one sample, below one hop, one block exactly, and the longest (two and a half blocks, odd)"""
    fpb, hop = BLOCK_FORMS[fft][3], fft // 4
    return [1, hop - 3, n_for(fpb, hop), n_for(2 * fpb + fpb // 2, hop)]


NO_BLOCK_CORPORA = [(2, n_for(9, 128), 512, 512, 128), (2, n_for(9, 256), 1023, 1024, 256), (2, n_for(6, 2048), 8192, 8192, 2048),
                    (2, n_for(5, 4096), 16384, 16384, 4096)]
BUFSTFT_SHAPES = [(n_for(21, 256), 1024, 1024, 256), (n_for(21, 128), 400, 512, 128)]      # one block shape, one generic shape


# frames OUTSIDE their buffer (fluhip_debug_stft_frames_*): (win, fft, float types) of every kernel form -- the block form at
# its three sizes with a full and a short even window, a generic power of two, a generic odd window with no block form, the
# largest on-chip size, and the global-memory passes (float32 only)
OUTSIDE_CASES = ([(w, f, ("float32", "float64")) for f in BLOCK_FFTS for w in (f, SHORT_EVEN_WINDOWS[f])]
                 + [(64, 64, ("float32", "float64")), (1023, 1024, ("float32", "float64")), (8192, 8192, ("float32", "float64")),
                    (16384, 16384, ("float32",))])
OUTSIDE_B = 3
OUTSIDE_GUARD_VALUE = 1e30
SILENT_BIN = 2.0 ** -511           # sqrt(DBL_MIN): the block kernel's OWN magnitude of an exactly silent bin (fft_core.h mag_sumsq)


def outside_geometry(fft, odd_hop, shift):
    """(n, hop, frame0, T, guard) of a run of frames from more than two transforms before the buffer to at least one behind it:
    n = fft + fft / 2 + 5, hop = fft / 4 (or one less: odd bases), frame0 = -(2 fft + hop) + shift, the last frame at or behind
    n + fft; guard as far as the furthest frame (padded to the transform) lies outside, plus fft"""
    n, hop = fft + fft // 2 + 5, fft // 4 - int(odd_hop)
    frame0 = -(2 * fft + hop) + shift
    T = -(-(n + fft - frame0) // hop) + 1
    assert frame0 + (T - 1) * hop >= n + fft > frame0 + (T - 2) * hop
    guard = max(-frame0, frame0 + (T - 1) * hop + fft - n) + fft
    return n, hop, frame0, T, guard


def outside_shifts(fft, odd_hop):
    """-1, 0, +1, and the shifts that put a frame at s0 = -fft (no sample of the buffer) and -fft + 1 (one sample, with
    win = fft) at the front -- 0 and +1 themselves at hop = fft / 4 -- and at n - 1 (one sample) and n (none) at the back"""
    n, hop, frame0, _, _ = outside_geometry(fft, odd_hop, 0)
    front, back = (-fft - frame0) % hop, (n - frame0) % hop
    return sorted({-1, 0, 1, front, front + 1, back - 1, back})


def outside_starts(fft, odd_hop):
    """every frame start the shifts of a case produce"""
    out = set()
    for sh in outside_shifts(fft, odd_hop):
        _, hop, frame0, T, _ = outside_geometry(fft, odd_hop, sh)
        out |= {frame0 + t * hop for t in range(T)}
    return out


def outside_input(n, guard, seed, dtype):
    """[OUTSIDE_B, guard + n + guard]: each buffer's samples (seeds seed, seed + 1, ...: a neighbour's samples are the nearest
    wrong answer) between guards of 1e30; and the list of the buffers on their own"""
    bufs = [dynamics(n, seed + b, dtype) for b in range(OUTSIDE_B)]
    padded = np.full((OUTSIDE_B, n + 2 * guard), OUTSIDE_GUARD_VALUE, dtype=dtype)
    for b, x in enumerate(bufs):
        padded[b, guard:guard + n] = x
    return padded, bufs


def round_blocks(deal):
    """the blocks dealt to the first and the last workgroup of rounds one and two: [(buffer, first frame)]"""
    out = []
    for r in (0, 1):
        here = [d for d in deal if d[0] == r]
        if here:
            out += [here[0][2:], here[-1][2:]]
    return out


def all_fft_sizes():
    return sorted({f for _, f, _ in GENERIC_POW2 + GENERIC_ODD} | set(BLOCK_FFTS) | set(BIG_FFTS) | {GENERIC_STRIDE_CASE[1]}
                  | {c[3] for c in NO_BLOCK_CORPORA} | {s[2] for s in BUFSTFT_SHAPES})
