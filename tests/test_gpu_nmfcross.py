"""BufNMFCross on the MI355X, through the C ABI, against the numpy restatement (tests/nmfcross_ref.py): the NMFCross H loop
(fluhip_nmfcross_process_f64), Griffin-Lim (fluhip_griffinlim_f64) and the client end to end (fluhip_bufnmfcross_f32)."""
import ctypes

import numpy as np
import pytest

import nmfcross_ref as R
import oracle_np

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(fluhip_lib_path):
    import fluhip
    c = fluhip.Context(0, fluhip.load_library(fluhip_lib_path))
    yield c
    c.close()


def _inputs(K, T, F, seed):
    # magnitudes of real audio: the constraint comparisons then see the value spread the client sees
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


def _compare_h(H, ref, what):
    zg, zr = H > 0, ref > 0
    if not np.array_equal(zg, zr):
        bad = np.argwhere(zg != zr)[:5]
        gaps = [(tuple(int(i) for i in b), float(H[tuple(b)]), float(ref[tuple(b)])) for b in bad]
        pytest.fail(f"{what}: zero patterns differ at {int((zg != zr).sum())} entries, e.g. (index, device, restatement) {gaps}")
    err = np.linalg.norm(H - ref) / max(np.linalg.norm(ref), 1e-300)
    assert err <= 1e-10, (what, err)


SMALL = [(1, 4, 33), (3, 5, 9), (37, 61, 129)]
RPC = [(7, 11, 7), (1, 1, 1), (3, None, 5), (9, 1, 3)]


@pytest.mark.parametrize("K,T,F", SMALL)
@pytest.mark.parametrize("iters", [1, 2, 50])
@pytest.mark.parametrize("rpc", RPC)
def test_nmfcross_process_small(ctx, K, T, F, iters, rpc):
    r, p, c = rpc
    p = K if p is None else min(p, K)   # the client's min(srcWindows, polyphony)
    X, W0 = _inputs(K, T, F, K + T + F)
    W0c = W0.copy()
    H, rc = ctx.nmfcross_process(X, W0, r, p, c, iters, seed=42)
    assert rc == 0
    np.testing.assert_array_equal(W0, W0c)   # W0 is read only
    _compare_h(H, R.nmfcross(X, W0, r, p, c, iters, 42), f"K={K} T={T} F={F} iters={iters} rpc={(r, p, c)}")


@pytest.mark.parametrize("iters", [1, 2, 50])
@pytest.mark.parametrize("rpc", RPC)
def test_nmfcross_process_259x173(ctx, iters, rpc):
    K, T, F = 259, 173, 513
    r, p, c = rpc
    p = K if p is None else min(p, K)
    X, W0 = _inputs(K, T, F, 7)
    H, rc = ctx.nmfcross_process(X, W0, r, p, c, iters, seed=3)
    assert rc == 0
    _compare_h(H, R.nmfcross(X, W0, r, p, c, iters, 3), f"259x173 iters={iters} rpc={(r, p, c)}")


def test_nmfcross_process_large(ctx):
    K, T, F = 1500, 700, 513
    X, W0 = _inputs(K, T, F, 11)
    H, rc = ctx.nmfcross_process(X, W0, 7, 11, 7, 5, seed=5)
    assert rc == 0
    _compare_h(H, R.nmfcross(X, W0, 7, 11, 7, 5, 5), "1500x700x513")


def test_nmfcross_strided_inputs(ctx):
    X, W0 = _inputs(20, 30, 65, 2)
    Xs = np.zeros((30, 80)); Xs[:, :65] = X
    Ws = np.zeros((20, 70)); Ws[:, :65] = W0
    H, _ = ctx.nmfcross_process(Xs[:, :65], Ws[:, :65], 3, 4, 3, 4, seed=9)
    _compare_h(H, R.nmfcross(X, W0, 3, 4, 3, 4, 9), "strided")


@pytest.mark.parametrize("n,win,fft,hop", [(3000, 256, 512, 64), (5000, 1024, 1024, 512), (2500, 200, 256, 100)])
def test_griffinlim(ctx, n, win, fft, hop):
    x = oracle_np.synth_audio(n, 21)
    spec = oracle_np.stft(x, win, fft, hop)[0] * (1.0 + 0.5j)
    out = ctx.griffinlim(spec, n, win, fft, hop, iters=50, seed=8)
    ref = R.griffinlim(spec, n, 50, win, fft, hop, 8)
    assert np.abs(out - ref).max() <= 1e-9 * np.abs(ref).max()


# (n_src, n_tgt, win, fft, hop): default FFT settings, win < fft, fft 2048, target shorter / longer than the source
CLIENT = [(22050, 22050, 1024, 1024, 512), (20000, 9000, 1000, 1024, 250), (30000, 26000, 2048, 2048, 512),
          (15000, 40000, 1024, 1024, 512), (26000, 3 * 512 + 100, 1024, 1024, 512)]


@pytest.mark.parametrize("n_src,n_tgt,win,fft,hop", CLIENT)
def test_bufnmfcross_end_to_end(ctx, n_src, n_tgt, win, fft, hop):
    src = oracle_np.synth_audio(n_src, 31).astype(np.float32)
    tgt = oracle_np.synth_audio(n_tgt, 32).astype(np.float32)
    c = min(7, (n_tgt + hop) // hop)    # the last case: target frames == continuity (the boundary of the check)
    r = min(7, c)
    y, rc = ctx.bufnmfcross(src, tgt, win, fft, hop, r, 11, c, 50, seed=42)
    assert rc == 0 and y.shape == (n_tgt,) and y.dtype == np.float32
    ref = R.bufnmfcross(src, tgt, win, fft, hop, r, 11, c, 50, 42)
    assert np.abs(y - ref).max() <= 1e-6 * np.abs(ref).max()


def test_bufnmfcross_goldens(ctx):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nmfcross_v1.npz"))
    for n in ("a", "b", "c"):
        win, fft, hop, r, p, c, iters, seed = (int(v) for v in g[f"{n}_params"])
        y, rc = ctx.bufnmfcross(g[f"{n}_source"], g[f"{n}_target"], win, fft, hop, r, p, c, iters, seed)
        assert rc == 0
        ref = g[f"{n}_output"]
        assert np.abs(y - ref).max() <= 1e-6 * np.abs(ref).max(), n


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
    _compare_h(H, R.nmfcross(X, W0, 7, 11, 7, 2, 6), "2600x1700x513")
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
        _compare_h(H, R.nmfcross(X, W0, *rpc, iters, 4), f"tile {tile} split {split} iters {iters}")
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
    _compare_h(H, R.nmfcross(X, W0, 7, 11, 7, 5, 8), "wide path")


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
    ref = R.bufnmfcross(src, tgt[:, 0], 1024, 1024, 512, 7, 13, 7, 20, 5)
    assert np.abs(y - ref).max() <= 1e-6 * np.abs(ref).max()
