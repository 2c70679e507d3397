"""BufNMFCross on the MI355X, through the C ABI, against the numpy restatement (tests/nmfcross_ref.py): the three constraint
stencils bit for bit (fluhip_debug_cross_stencil_f64), the NMFCross H loop entry by entry (fluhip_nmfcross_process_f64),
Griffin-Lim frame by frame (fluhip_griffinlim_f64) and the client end to end (fluhip_bufnmfcross_f32).

The measures and their bars (derived on the CPU against the long double model, tests/test_nmfcross_ref.py; no bar was set from
what the device gives):
  stencils     np.array_equal with continuity (the kernel's order of addition), sparsity_literal and polyphony_literal on inputs
               the public entry's random draw cannot produce: exact ties and plateaus at both edges and in the middle (the tests
               assert that they are there and decide), tie groups cut by the polyphony count across k = 63|64, 255|256 and
               511|512, products that differ in the last radix byte alone, subnormal products, frames of zeros, sizes above T
               and above K, and 65541 frames (the stencils stride past a grid of 65535 rows).
  H loop       the zero pattern exactly, then nmf_ref.elrel -- every entry relative to ITSELF, no entry exempted -- under
               CROSS_BAR[iterations]: 8 x the float64 restatement's distance from its long double form.  The long double run's
               last iteration is at least 1e-8 from every sparsity and polyphony decision at every input (the smallest margin
               2.1e-7), so no entry and no frame is exempted here.  _compare_h prints the measure it replaces beside it
               (|H - ref| / |ref| over the whole matrix, formerly held to 1e-10).
  Griffin-Lim  gl_frame_err -- the worst frame, each relative to its own peak -- under GL_BAR[iterations] (64 x float64 against
               long double), at 0, 1, 2, 3 and 50 iterations; the former 1e-9 of the peak is still asserted.
  end to end   E2E_BAR = 64 x floor + 2^-24 of the peak = 5.97e-8 (formerly 1e-6).

Measured on an MI355X when the file was written (every test prints its own):
  stencils: 0 entries differ in all 108 shape x size cases and in every frame of the polyphony select test (K = 1 .. 700)
  H loop, production build, the worst of the 60 shape x constraint cases per count (SMALL + EDGE shapes, six (r, p, c)):
    0: bit for bit (bar 0)   1: 1.7e-15 (bar 3.7e-14)   2: 2.2e-15 (4.6e-14)   3: 2.8e-15 (4.6e-14)   10: 6.5e-15 (5.9e-14)
    50: 9.2e-15 (3.2e-13), each at 129x127x65; many small cases are bit-identical to the restatement
    259x173x513: 4.1e-15 / 5.8e-15 / 8.4e-14 at 1 / 2 / 50; 1500x700x513 x 5: 5.4e-15 (bar 5.9e-14); 2600x1700x513 x 2: 5.4e-15
    (4.6e-14); silence, 65541 frames, strided and the wide A/B path: bit-identical; of the norm everything reads <= 2.9e-15
  H loop, forced forms (tile 64 / 128 x split 1 / 3 at the seven EDGE shapes and 300x200x513): <= 4.6e-15 at 1 iteration,
    <= 5.6e-15 at 3; tile 64 and 128 give the same bits, a split costs up to 2.8e-15
  Griffin-Lim, the worst frame of the three cases: 0: 2.4e-16 (bar 2.0e-14)   1: 5.0e-15 (2.0e-13)   2: 1.5e-14 (4.7e-13)
    3: 1.1e-13 (3.0e-12)   50: 2.0e-12 (7.3e-11; of the peak 2.2e-13)
  end to end: 0 .. 2.2e-9 of the peak (the float output differs in a handful of last places); goldens and C++ client 0

What the file catches -- five deliberate breaks of kernels_nmfcross.hip, each built once in a scratch copy (none committed), each
wrong arithmetic on in-bounds data; "old" is what the assertions this file had before (1e-10 of the norm, 1e-9 and 1e-6 of the
peak) read on the same run:
  (a) cross_reduce_kernel leaves out the last split for column N - 1: every split-3 case of
      test_every_gemm_form_at_the_tile_and_depth_edges fails (12; e.g. 17x65x16: elrel 1.0e-1, of the norm 1.5e-4), as do
      test_nmfcross_process_259x173 (all 12: zero patterns differ, or elrel 0.36 at norm 1.8e-5), test_nmfcross_process_large,
      test_every_gemm_form[3-*], the 128-tile test and all five end-to-end cases (7e-2 .. 0.45 of the peak).  Gross: a third
      of a contraction is missing from a whole column, and the old assertions fail wherever a production shape splits
      (259x173 and up); below that -- no split without the forced forms -- only the new edge cases reach the reduce kernel.
  (b) cross_sparsity_kernel uses u > v on both sides: test_sparsity_bit_for_bit_with_exact_ties fails at every shape with
      T >= 2 and r >= 3 (20 cases; 6 .. 43504 entries differ).  Every old assertion passes: the H loop, Griffin-Lim and end to
      end read exactly what they read on the real code (real data has no exact ties but zeros).
  (c) the polyphony keep pass starts `taken` at 0 for every chunk: test_polyphony_bit_for_bit_on_tied_products fails at K = 300
      and 1000 for every p (12 cases) and test_polyphony_select_ties_last_byte_subnormals at K = 257 and 700 (a tie group cut
      across k = 255|256 or 511|512 keeps too many).  Every old assertion passes.
  (d) the continuity kernel's stride: a stride of gridDim.y - 1 still visits every frame (some twice, with the same result) and
      is 0 -- an endless loop -- at T = 1, so it was not run; the stride of gridDim.y + 1 was, which never visits frame 65535:
      test_continuity_bit_for_bit[*-65541-3] (all 6) and test_frames_past_65535_through_the_loop fail.  Every old assertion
      passes (the largest T elsewhere is 3801).
  (e) den[n] read as den[n - 1] for n == N - 1: 271 tests fail -- 224 of test_nmfcross_process_small, both silence cases, the
      65541 frames, the forced forms, 259x173, end to end (0.18 .. 0.85 of the peak) and golden a (5e-2).  Gross (the last
      source frame's activations are off by the ratio of two column sums, and continuity smears that): where the old tests
      ran they fail too (of the norm 1e-5 .. 0.34).
  -- (a) and (e) are coarse enough for the old measures wherever an old test reached them; (b), (c) and (d) are what only this
  file sees, through the stencil entry.  No test failed on the real code, and no kernel changed."""
import ctypes

import numpy as np
import pytest

import functools

import nmfcross_ref as R
import oracle_np
from test_nmfcross_ref import CROSS_BAR, E2E_BAR, GL_BAR, cross_bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(fluhip_lib_path):
    import fluhip
    c = fluhip.Context(0, fluhip.load_library(fluhip_lib_path))
    yield c
    c.close()


_inputs = R.audio_inputs


def _compare_h(H, ref, what, iters):
    """the zero pattern exactly, then every entry relative to itself (nmf_ref.elrel) under CROSS_BAR of the count; beside it
    what the norm-wide measure this replaces (<= 1e-10) reads"""
    assert np.isfinite(H).all(), what
    zg, zr = H > 0, ref > 0
    if not np.array_equal(zg, zr):
        bad = np.argwhere(zg != zr)[:5]
        gaps = [(tuple(int(i) for i in b), float(H[tuple(b)]), float(ref[tuple(b)])) for b in bad]
        pytest.fail(f"{what}: zero patterns differ at {int((zg != zr).sum())} entries, e.g. (index, device, restatement) {gaps}")
    err = R.elrel(H, ref)
    nrm = np.linalg.norm(H - ref) / max(np.linalg.norm(ref), 1e-300)
    print(f"nmfcross {what} x {iters}: elrel {err:.3e} (bar {cross_bar(iters):.1e}); of the norm {nrm:.3e}")
    assert err <= cross_bar(iters), (what, err, cross_bar(iters))
    return err


@functools.lru_cache(maxsize=None)
def _loop_ref(K, T, F, rpc, iters):
    """the float64 restatement of an H-loop shape: computed once, shared, read-only"""
    X, W0 = R.loop_inputs(K, T, F)
    ref = R.nmfcross(X, W0, *R.rpc_of(rpc, K), iters, R.H_SEED)
    ref.setflags(write=False)
    return ref


def _shape_id(s):
    return "x".join(str(v) for v in s)


SMALL = R.SMALL
RPC = R.RPC


# ---- the three stencils, bit for bit (fluhip_debug_cross_stencil_f64: the launches of the loop on the caller's doubles) ------
STENCIL_SHAPES = [(1, 1), (5, 3), (9, 4), (70, 300), (12, 1000), (65541, 3)]      # (T, K)
STENCIL_SIZES = [1, 2, 3, 4, 7, 15]                                                # below, at and above T and K


@pytest.mark.parametrize("T,K", STENCIL_SHAPES)
@pytest.mark.parametrize("c", STENCIL_SIZES)
def test_continuity_bit_for_bit(ctx, T, K, c):
    H = np.random.default_rng(T + K + c).random((T, K))
    got = ctx.cross_stencil(H, 0, c)
    want = R.continuity(H.T, c).T            # adds in the kernel's order, d = 0 .. c - 1
    print(f"continuity {T}x{K} c={c}: {int((got != want).sum())} entries differ")
    assert np.array_equal(got, want)


def _sparsity_with(H, r, before_ge, after_ge):
    """temporal sparsity on H [T, K] with the comparison of either side chosen: (True, False) is the first maximum"""
    T, K = H.shape
    h = (r - 1) // 2
    padded = np.zeros((T + 2 * r, K))
    padded[r:r + T] = H
    keep = np.ones((T, K), dtype=bool)
    for j in range(r):
        if j == h:
            continue
        u = padded[r - h + j:r - h + j + T]
        ge = before_ge if j < h else after_ge
        keep &= ~((u >= H) if ge else (u > H))
    return np.where(keep, H, 0.0)


def _levels(T, K, seed):
    """H [T, K] of four levels, 0 among them, with plateaus of the top level planted at the first two frames, the last two and
    two in the middle"""
    H = np.random.default_rng(seed).choice([0.0, 0.25, 0.5, 1.0], size=(T, K))
    if T >= 2:
        H[:2] = H[T - 2:] = 1.0
    if T >= 6:
        H[T // 2:T // 2 + 2] = 1.0
    return H


@pytest.mark.parametrize("T,K", STENCIL_SHAPES)
@pytest.mark.parametrize("r", STENCIL_SIZES)
def test_sparsity_bit_for_bit_with_exact_ties(ctx, T, K, r):
    H = _levels(T, K, 3 * T + K + r)
    got = ctx.cross_stencil(H, 1, r)
    want = R.sparsity_literal(H.T, r, 0, 1).T
    assert np.array_equal(want, _sparsity_with(H, r, True, False))
    # the ties are there and decide, at both edges and in the middle: with >= on both sides (the LAST maximum loses its
    # plateau's first frame) or > on both (a plateau's second frame survives) the result is another
    after = _sparsity_with(H, r, True, True) != want
    before = _sparsity_with(H, r, False, False) != want
    print(f"sparsity {T}x{K} r={r}: {int((got != want).sum())} entries differ; {int(before.sum())} entries rest on >= before the "
          f"centre, {int(after.sum())} on > after it")
    if T >= 2 and r >= 2:
        assert after[0].all() and (r > 2 or after[T - 2].all()) and (r > 2 or T < 6 or after[T // 2].all())
    if T >= 2 and r >= 3:
        assert before[1].all() and before[T - 1].all() and (T < 6 or before[T // 2 + 1].all())
    assert np.array_equal(got, want)


def _tied_scores(T, K, seed):
    """(H [T, K], energy [K]): H of a few levels and energies that are powers of two, so that the products tie exactly; the
    products of frame 0 are all equal"""
    rng = np.random.default_rng(seed)
    energy = rng.choice([0.5, 1.0, 2.0, 4.0], size=K)
    H = rng.choice([0.0, 0.5, 1.0, 2.0], size=(T, K))
    H[0] = 1.0 / energy
    return H, energy


def _cut_ties(H, energy, p):
    """the frames whose p-th and (p + 1)-th largest products are equal and positive: the cut falls inside a tie group"""
    s = -np.sort(-(H * energy[None, :]), axis=1)
    return np.flatnonzero((s[:, p - 1] == s[:, p]) & (s[:, p - 1] > 0)) if p < H.shape[1] else np.array([], dtype=int)


@pytest.mark.parametrize("T,K", STENCIL_SHAPES)
@pytest.mark.parametrize("p", STENCIL_SIZES)
def test_polyphony_bit_for_bit_on_tied_products(ctx, T, K, p):
    p = min(p, K)
    H, energy = _tied_scores(T, K, 5 * T + K + p)
    got = ctx.cross_stencil(H, 2, p, energy)
    want = R.polyphony_literal(H.T, energy, p, 0, 1).T
    ties = _cut_ties(H, energy, p)
    print(f"polyphony {T}x{K} p={p}: {int((got != want).sum())} entries differ; the cut falls inside a tie group in {len(ties)} frames")
    assert p == K or len(ties) > 0
    assert np.array_equal(got, want)


def _polyphony_frames(K, p, seed):
    """(H [frames, K], energy [K], names): the frames the radix select and the keep-in-k-order pass are never given by a random
    draw -- tied levels, all zeros, nextafter neighbours (products that differ in the last radix byte alone), subnormal
    products, and per boundary b of a wavefront or a 256-wide chunk (64, 256, 512 < K) a tie group laid across k = b - 1 | b
    with the p-th place inside it"""
    rng = np.random.default_rng(seed)
    energy = rng.choice([0.5, 1.0, 2.0, 4.0], size=K)
    names, rows = [], []

    def add(name, products):
        names.append(name)
        rows.append(products / energy)              # exact: the energies are powers of two

    add("levels", rng.choice([0.0, 0.5, 1.0, 2.0], size=K))
    add("zeros", np.zeros(K))
    chain = [1.0]
    for _ in range(min(K, 9) - 1):
        chain.append(np.nextafter(chain[-1], 2.0))
    add("nextafter", rng.permutation(np.resize(np.array(chain), K)))
    add("subnormal", rng.integers(1, 9, size=K) * 2.0 ** -1062)
    for b in (64, 256, 512):
        if b >= K:
            continue
        j = min(p, 3)                               # places of the group in front of the boundary, all kept
        above = p - j
        glen = min(6, K - above)
        prod = rng.choice([0.0, 0.25, 0.5], size=K)
        prod[b - j:b - j + glen] = 1.0
        rest = np.setdiff1d(np.arange(K), np.arange(b - j, b - j + glen))
        prod[rng.choice(rest, size=above, replace=False)] = rng.choice([2.0, 4.0], size=above)
        add(f"group across {b - 1}|{b}", prod)
    return np.array(rows), energy, names


@pytest.mark.parametrize("K", [1, 5, 64, 65, 256, 257, 700])
def test_polyphony_select_ties_last_byte_subnormals(ctx, K):
    for p in sorted({q for q in (1, 2, min(11, K), K - 1, K) if 1 <= q <= K}):
        H, energy, names = _polyphony_frames(K, p, 7 * K + p)
        prod = H * energy[None, :]
        sub = prod[names.index("subnormal")]
        assert (sub > 0).all() and (sub < np.finfo(np.float64).tiny).all()
        near = np.unique(prod[names.index("nextafter")]).view(np.uint64)
        assert len(near) == min(K, 9) and near[-1] - near[0] == len(near) - 1 < 256      # the last radix byte alone
        for i, name in enumerate(names):
            if name.startswith("group") and p < K:
                b = int(name.split("|")[1])
                assert i in _cut_ties(H, energy, p) and prod[i, b - 1] == prod[i, b] == 1.0      # the cut is inside, across b - 1 | b
        got = ctx.cross_stencil(H, 2, p, energy)
        want = R.polyphony_literal(H.T, energy, p, 0, 1).T
        kept = (want > 0).sum(axis=1)
        print(f"polyphony K={K} p={p}: frames {names}, kept {kept.tolist()}, {int((got != want).sum())} entries differ")
        assert not want[names.index("zeros")].any()
        for i, name in enumerate(names):
            assert np.array_equal(got[i], want[i]), (K, p, name, np.flatnonzero(got[i] != want[i])[:8])


def test_cross_stencil_refusals(ctx):
    dp = ctypes.POINTER(ctypes.c_double)
    H, e, out = np.ones((4, 3)), np.ones(3), np.empty((4, 3))
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    for args, word in [((None, 4, 3, 0, 1, None, out), "null"), ((H, 4, 3, 0, 1, None, None), "null"),
                       ((H, 4, 3, 2, 1, None, out), "energy"), ((H, 0, 3, 0, 1, None, out), "T and K"),
                       ((H, 4, 0, 1, 1, None, out), "T and K"), ((H, 4, 3, 0, 0, None, out), "size"),
                       ((H, 4, 3, 1, -2, None, out), "size"), ((H, 4, 3, 2, 4, e, out), "polyphony"),
                       ((H, 4, 3, 3, 1, e, out), "which")]:
        a, T, K, which, size, en, o = args
        rc = ctx.lib.fluhip_debug_cross_stencil_f64(ctx.h, ptr(a), T, K, which, size, ptr(en), ptr(o))
        msg = ctx.lib.fluhip_last_error(ctx.h).decode()
        assert rc == 2 and msg.startswith("fluhip_debug_cross_stencil_f64: ") and word in msg, (args[1:5], rc, msg)
    assert np.array_equal(ctx.cross_stencil(H, 2, 3, e), H)       # the context is usable afterwards; p == K keeps everything


# ---- the H loop, entry by entry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,T,F", SMALL + R.EDGE)
@pytest.mark.parametrize("iters", [1, 2, 50, 0, 3, 10])
@pytest.mark.parametrize("rpc", RPC)
def test_nmfcross_process_small(ctx, K, T, F, iters, rpc):
    """the small shapes and the tile / depth edges of each GEMM (M or N one below, at and above 64 / 128; a contraction of 1,
    15, 16, 17), at every count and constraint set: even r and c, r and c larger than T or K among them"""
    r, p, c = R.rpc_of(rpc, K)          # the client's min(srcWindows, polyphony)
    X, W0 = R.loop_inputs(K, T, F)
    W0c = W0.copy()
    H, rc = ctx.nmfcross_process(X, W0, r, p, c, iters, seed=R.H_SEED)
    assert rc == 0
    np.testing.assert_array_equal(W0, W0c)   # W0 is read only
    if iters == 0:
        assert CROSS_BAR[0] == 0.0 and np.array_equal(H, R.initial_h(K, T, R.H_SEED).T)     # the draw, bit for bit
    _compare_h(H, _loop_ref(K, T, F, rpc, iters), f"{K}x{T}x{F} rpc {(r, p, c)}", iters)


@pytest.mark.parametrize("iters", [1, 2, 50])
@pytest.mark.parametrize("rpc", RPC[:4])
def test_nmfcross_process_259x173(ctx, iters, rpc):
    K, T, F = 259, 173, 513
    r, p, c = R.rpc_of(rpc, K)
    X, W0 = R.audio_inputs_shared(K, T, F, 7)
    H, rc = ctx.nmfcross_process(X, W0, r, p, c, iters, seed=3)
    assert rc == 0
    _compare_h(H, R.nmfcross(X, W0, r, p, c, iters, 3), f"259x173x513 rpc {(r, p, c)}", iters)


def test_nmfcross_process_large(ctx):
    K, T, F = 1500, 700, 513
    X, W0 = _inputs(K, T, F, 11)
    H, rc = ctx.nmfcross_process(X, W0, 7, 11, 7, 5, seed=5)
    assert rc == 0
    _compare_h(H, R.nmfcross(X, W0, 7, 11, 7, 5, 5), "1500x700x513", 5)


def test_nmfcross_strided_inputs(ctx):
    (K, T, F), seed, rpc, iters, hseed = R.STRIDED
    X, W0 = R.audio_inputs_shared(K, T, F, seed)
    Xs = np.zeros((T, F + 15)); Xs[:, :F] = X
    Ws = np.zeros((K, F + 5)); Ws[:, :F] = W0
    H, _ = ctx.nmfcross_process(Xs[:, :F], Ws[:, :F], *rpc, iters, seed=hseed)
    _compare_h(H, R.nmfcross(X, W0, *rpc, iters, hseed), "strided", iters)


@pytest.mark.parametrize("iters", R.SILENCE_ITERS)
def test_digital_silence(ctx, iters):
    """all-zero target frames (0, 7 .. 9, T - 1) and all-zero source frames (3, K - 1: a dictionary clamped to eps): H1 finite,
    exact zeros where the restatement has them, every other entry under the bar"""
    X, W0 = R.silence_inputs()
    K, T, _ = R.SILENCE
    H, rc = ctx.nmfcross_process(X, W0, *R.SILENCE_RPC, iters, seed=R.H_SEED)
    assert rc == 0 and np.isfinite(H).all()
    ref = R.nmfcross(X, W0, *R.SILENCE_RPC, iters, R.H_SEED)
    assert not ref[[0, 7, 8, 9, T - 1]].any() and not H[[0, 7, 8, 9, T - 1]].any()
    _compare_h(H, ref, "silence", iters)


def test_frames_past_65535_through_the_loop(ctx):
    """T = 65541: the two stencils stride their frames over a grid of 65535 rows, and frames 65535 .. 65540 are the second lap"""
    K, T, F = R.LONG
    X, W0 = R.loop_inputs(K, T, F)
    H, rc = ctx.nmfcross_process(X, W0, *R.LONG_RPC, R.LONG_ITERS, seed=R.H_SEED)
    assert rc == 0
    ref = R.nmfcross(X, W0, *R.LONG_RPC, R.LONG_ITERS, R.H_SEED)
    assert ref[65535:].any()
    print(f"frames 65535 ..: elrel {R.elrel(H[65535:], ref[65535:]):.3e}")
    _compare_h(H, ref, "5x65541x3", R.LONG_ITERS)


def _griffinlim(ctx, n, win, fft, hop, iters):
    spec = R.gl_input(n, win, fft, hop)
    out = ctx.griffinlim(spec, n, win, fft, hop, iters=iters, seed=R.GL_SEED)
    ref = R.griffinlim(spec, n, iters, win, fft, hop, R.GL_SEED)
    e = R.gl_frame_err(out, ref)
    print(f"griffinlim {(n, win, fft, hop)} x {iters}: worst frame {e:.3e} (bar {GL_BAR[iters]:.1e}); "
          f"of the peak {np.abs(out - ref).max() / np.abs(ref).max():.3e}")
    assert e <= GL_BAR[iters]
    assert np.abs(out - ref).max() <= 1e-9 * np.abs(ref).max()


@pytest.mark.parametrize("n,win,fft,hop", R.GL_CASES)
def test_griffinlim(ctx, n, win, fft, hop):
    _griffinlim(ctx, n, win, fft, hop, 50)


@pytest.mark.parametrize("n,win,fft,hop", R.GL_CASES)
@pytest.mark.parametrize("iters", [0, 1, 2, 3])
def test_griffinlim_first_iterations(ctx, n, win, fft, hop, iters):
    """0: magnitude times the drawn phase alone; 1 .. 3: the momentum term from its first use on"""
    _griffinlim(ctx, n, win, fft, hop, iters)


CLIENT = R.CLIENT


def _e2e(y, ref, what):
    e = float(np.abs(y.astype(np.float64) - ref.astype(np.float64)).max() / np.abs(ref).max())
    print(f"bufnmfcross {what}: |got - want| / peak = {e:.3e} (bar {E2E_BAR:.3e})")
    assert E2E_BAR < 1e-6 and e <= E2E_BAR, (what, e)


@pytest.mark.parametrize("n_src,n_tgt,win,fft,hop", CLIENT)
def test_bufnmfcross_end_to_end(ctx, n_src, n_tgt, win, fft, hop):
    src, tgt = R.client_audio(n_src, n_tgt)
    r, p, c = R.client_rpc(n_tgt, hop)
    y, rc = ctx.bufnmfcross(src, tgt, win, fft, hop, r, p, c, 50, seed=42)
    assert rc == 0 and y.shape == (n_tgt,) and y.dtype == np.float32
    _e2e(y, R.bufnmfcross(src, tgt, win, fft, hop, r, p, c, 50, 42), str((n_src, n_tgt, win, fft, hop)))


def test_bufnmfcross_goldens(ctx):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nmfcross_v1.npz"))
    for n in ("a", "b", "c"):
        win, fft, hop, r, p, c, iters, seed = (int(v) for v in g[f"{n}_params"])
        y, rc = ctx.bufnmfcross(g[f"{n}_source"], g[f"{n}_target"], win, fft, hop, r, p, c, iters, seed)
        assert rc == 0
        _e2e(y, g[f"{n}_output"], f"golden {n}")


def test_bufnmfcross_messages(ctx):
    import fluhip
    x = oracle_np.synth_audio(4000, 1).astype(np.float32)
    cases = [((x[:0], x), "Empty source buffer"), ((x, x[:0]), "Empty target buffer"),
             ((x, x[:1000]), "Time Sparsity is larger than target frames")]
    for (s, t), msg in cases:
        with pytest.raises(fluhip.FluhipError) as e:
            ctx.bufnmfcross(s, t, 1024, 1024, 512, 7, 11, 7, 5, seed=1)
        assert str(e.value).endswith(msg) or msg in str(e.value)
    with pytest.raises(fluhip.FluhipError) as e:
        ctx.bufnmfcross(x, x[:1000], 1024, 1024, 512, 1, 11, 5, 5, seed=1)
    assert "Continuity is larger than target frames" in str(e.value)
    with pytest.raises(fluhip.FluhipError):
        ctx.nmfcross_process(np.ones((4, 5)), np.ones((3, 5)), 1, 4, 1, 2)   # p > K


def test_progress_numbering_and_cancellation(ctx):
    x = oracle_np.synth_audio(8000, 2).astype(np.float32)
    y = oracle_np.synth_audio(6000, 3).astype(np.float32)
    seen = []
    _, rc = ctx.bufnmfcross(x, y, 512, 512, 256, 7, 11, 7, 6, seed=4, progress=lambda i: seen.append(i) or True)
    assert rc == 0 and seen == list(range(1, 10))
    import fluhip
    ctx.set_progress_lag(1)
    try:
        seen.clear()
        _, rc = ctx.bufnmfcross(x, y, 512, 512, 256, 7, 11, 7, 6, seed=4, progress=lambda i: seen.append(i) or i < 3)
        assert rc == fluhip.CANCELLED and seen == [1, 2, 3]
        seen.clear()
        _, rc = ctx.bufnmfcross(x, y, 512, 512, 256, 7, 11, 7, 6, seed=4, progress=lambda i: seen.append(i) or i < 8)
        assert rc == fluhip.CANCELLED and seen == list(range(1, 9))
    finally:
        ctx.set_progress_lag(8)
    seen.clear()
    X, W0 = _inputs(10, 12, 33, 1)
    _, rc = ctx.nmfcross_process(X, W0, 3, 4, 3, 20, seed=1, progress=lambda i: seen.append(i) or i < 5)
    assert rc == fluhip.CANCELLED and seen[:5] == [1, 2, 3, 4, 5] and len(seen) == 5
    _, rc = ctx.bufnmfcross(x, y, 512, 512, 256, 7, 11, 7, 6, seed=4)   # the context is usable afterwards
    assert rc == 0


def test_two_runs_are_bit_identical(ctx):
    X, W0 = _inputs(300, 200, 513, 4)
    a, _ = ctx.nmfcross_process(X, W0, 7, 11, 7, 10, seed=2)
    b, _ = ctx.nmfcross_process(X, W0, 7, 11, 7, 10, seed=2)
    assert np.array_equal(a, b)
    x = oracle_np.synth_audio(20000, 5).astype(np.float32)
    y1, _ = ctx.bufnmfcross(x, x[::-1].copy(), 1024, 1024, 512, seed=6)
    y2, _ = ctx.bufnmfcross(x, x[::-1].copy(), 1024, 1024, 512, seed=6)
    assert np.array_equal(y1, y2)


def test_no_device_memory_is_left_behind(ctx):
    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipDeviceSynchronize() == 0
        assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
        return f.value

    x = oracle_np.synth_audio(30000, 6).astype(np.float32)

    def one_pass():
        _, rc = ctx.bufnmfcross(x, x[:20000], 1024, 1024, 512, iters=5, seed=1, progress=lambda i: True)
        assert rc == 0
        X, W0 = _inputs(700, 300, 513, 3)
        ctx.nmfcross_process(X, W0, 7, 11, 7, 3, seed=1)

    one_pass()
    before = free_bytes()
    for _ in range(5):
        one_pass()
    assert before - free_bytes() < (8 << 20)


# ---- every GEMM form against the restatement ------------------------------------------------------------------------------
def test_128_tile_forms_at_large_shapes(ctx):
    """the shapes that reach the 128 x 128 forms on this device in production: GEMM2 (TB = 0) at K = 2600, T = 1700, and the
    synthesis GEMM (TB = 1) at T >= 29 x 128 target frames; the test asserts the form the plan took"""
    K, T, F = 2600, 1700, 513
    assert ctx.cross_plan(T, K, F)[0], ctx.cross_plan(T, K, F)          # GEMM2: 128 x 128
    X, W0 = _inputs(K, T, F, 13)
    H, rc = ctx.nmfcross_process(X, W0, 7, 11, 7, 2, seed=6)
    assert rc == 0
    _compare_h(H, R.nmfcross(X, W0, 7, 11, 7, 2, 6), "2600x1700x513", 2)
    n_src, n_tgt = 20000, 3800 * 512
    Ks, Tt = (n_src + 512) // 512, (n_tgt + 512) // 512
    assert ctx.cross_plan(Tt, 2 * 513, Ks)[0], ctx.cross_plan(Tt, 2 * 513, Ks)   # synthesis: 128 x 128, TB = 1
    src = oracle_np.synth_audio(n_src, 41).astype(np.float32)
    tgt = oracle_np.synth_audio(n_tgt, 42).astype(np.float32)
    y, rc = ctx.bufnmfcross(src, tgt, 1024, 1024, 512, 7, 11, 7, 3, seed=9)
    assert rc == 0
    ref = R.bufnmfcross(src, tgt, 1024, 1024, 512, 7, 11, 7, 3, 9)
    assert np.abs(y - ref).max() <= 1e-6 * np.abs(ref).max()


@pytest.fixture(scope="module")
def ab_ctx():
    """the measurement build, whose FLUHIP_CROSS_TILE / FLUHIP_CROSS_SPLIT force the GEMM form (fluhip_env.h)"""
    import importlib.util
    import os
    import fluhip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fluhip_build_ab", os.path.join(root, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.LIB_AB):
        mod.build_ab()
    c = fluhip.Context(0, fluhip.load_library(mod.LIB_AB))
    yield c
    c.close()


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("split", [1, 3])
def test_every_gemm_form(ab_ctx, monkeypatch, tile, split):
    monkeypatch.setenv("FLUHIP_CROSS_TILE", str(tile))
    monkeypatch.setenv("FLUHIP_CROSS_SPLIT", str(split))
    K, T, F = 300, 200, 513
    for M, N, Kd in ((T, F, K), (T, K, F), (T, 2 * F, K)):
        big, ns, _ = ab_ctx.cross_plan(M, N, Kd)
        assert big == (tile == 128) and ns == split, (M, N, Kd, big, ns)
    X, W0 = _inputs(K, T, F, 17)
    for iters, rpc in ((3, (7, 11, 7)), (1, (3, 300, 5))):
        H, rc = ab_ctx.nmfcross_process(X, W0, *rpc, iters, seed=4)
        assert rc == 0
        _compare_h(H, R.nmfcross(X, W0, *rpc, iters, 4), f"300x200x513 tile {tile} split {split} rpc {rpc}", iters)
    src = oracle_np.synth_audio(30000, 51).astype(np.float32)
    tgt = oracle_np.synth_audio(25000, 52).astype(np.float32)
    y, rc = ab_ctx.bufnmfcross(src, tgt, 1024, 1024, 512, 7, 11, 7, 4, seed=2)
    assert rc == 0
    ref = R.bufnmfcross(src, tgt, 1024, 1024, 512, 7, 11, 7, 4, 2)
    assert np.abs(y - ref).max() <= 1e-6 * np.abs(ref).max()


def test_wide_baseline_computes_the_same_update(ab_ctx, monkeypatch):
    """the A/B baseline of tools/nmfcross_bench.py (FLUHIP_CROSS_WIDE=1: the any-rank NMF path's kernels) is the same loop"""
    monkeypatch.setenv("FLUHIP_CROSS_WIDE", "1")
    X, W0 = _inputs(150, 90, 257, 19)
    H, rc = ab_ctx.nmfcross_process(X, W0, 7, 11, 7, 5, seed=8)
    assert rc == 0
    _compare_h(H, R.nmfcross(X, W0, 7, 11, 7, 5, 8), "wide path", 5)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("shape", R.EDGE, ids=_shape_id)
def test_every_gemm_form_at_the_tile_and_depth_edges(ab_ctx, monkeypatch, tile, split, shape):
    """the forced forms at M or N one below, at and above the tile, contractions of 1, 15, 16, 17, and splits whose last chunk
    is short (65 = 32 + 32 + 1, 127 = 48 + 48 + 31, 129 = 48 + 48 + 33, 33 = 16 + 16 + 1)"""
    monkeypatch.setenv("FLUHIP_CROSS_TILE", str(tile))
    monkeypatch.setenv("FLUHIP_CROSS_SPLIT", str(split))
    K, T, F = shape
    for M, N, Kd in ((T, F, K), (T, K, F)):
        big, ns, chunk = ab_ctx.cross_plan(M, N, Kd)
        assert big == (tile == 128) and (ns, chunk) == R.forced_splits(Kd, split), (M, N, Kd, big, ns, chunk)
    X, W0 = R.loop_inputs(K, T, F)
    for iters, rpc in ((3, RPC[0]), (1, RPC[2])):
        H, rc = ab_ctx.nmfcross_process(X, W0, *R.rpc_of(rpc, K), iters, seed=R.H_SEED)
        assert rc == 0
        _compare_h(H, _loop_ref(K, T, F, rpc, iters), f"{_shape_id(shape)} tile {tile} split {split} rpc {R.rpc_of(rpc, K)}", iters)


# ---- the C++ client (include/flucoma_hip/NMFCrossClient.hpp) through tests/cpp/nmfcross_driver.cpp ------------------------
@pytest.mark.parametrize("async_", [0, 1])
def test_cpp_client(fluhip_lib_path, tmp_path, async_):
    import importlib.util
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fluhip_build_d", os.path.join(root, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    driver = mod.build_nmfcross_driver()
    src = oracle_np.synth_audio(24000, 61).astype(np.float32)
    tgt = np.stack([oracle_np.synth_audio(17000, 62), oracle_np.synth_audio(17000, 63)], axis=1).astype(np.float32)
    src.tofile(tmp_path / "src.f32")
    tgt.tofile(tmp_path / "tgt.f32")             # interleaved, two channels: the client reads channel 0
    out = tmp_path / "out.bin"
    # polyphony 12 -> 13 (Odd), iterations 20
    r = subprocess.run([driver, "run", str(tmp_path / "src.f32"), "24000", "1", "48000", str(tmp_path / "tgt.f32"), "17000", "2",
                        "44100", "1024", "-1", "-1", "7", "12", "7", "20", "5", str(async_), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-1] == "run|0|", r.stdout
    raw = out.read_bytes()
    frames, chans = np.frombuffer(raw[:16], dtype=np.int64)
    sr = np.frombuffer(raw[16:24], dtype=np.float64)[0]
    y = np.frombuffer(raw[24:], dtype=np.float32)
    assert (frames, chans, sr) == (17000, 1, 48000.0)     # tgtFrames x 1 at the SOURCE's sample rate (:133)
    _e2e(y, R.bufnmfcross(src, tgt[:, 0], 1024, 1024, 512, 7, 13, 7, 20, 5), f"C++ client async {async_}")
