"""CPU tests of BufNMFCross: the numpy restatement (tests/nmfcross_ref.py) against its loop-by-loop transcription of the
reference's constraint functions, the integer-division constraint factor, the random draws, the committed goldens, and the
C ABI's declarations / binding.  No GPU compute."""
import ctypes
import os
import re

import numpy as np
import pytest

import nmfcross_ref as R
import oracle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fluhip_nmfcross_process_f64", "fluhip_griffinlim_f64", "fluhip_bufnmfcross_f32")


def _random_h(K, T, seed, zeros=0.3):
    rng = np.random.default_rng(seed)
    H = rng.random((K, T))
    H[rng.random((K, T)) < zeros] = 0.0
    return H


@pytest.mark.parametrize("K,T", [(1, 1), (1, 6), (5, 8), (6, 7), (9, 4), (12, 13)])
@pytest.mark.parametrize("size", [1, 2, 3, 4, 7, 9, 15])
def test_constraints_vectorised_match_literal(K, T, size):
    H = _random_h(K, T, K * 100 + T)
    energy = np.random.default_rng(size).random(K)
    for it, iters in [(0, 1), (2, 5), (4, 5)]:
        np.testing.assert_array_equal(R.sparsity(H, size, it, iters), R.sparsity_literal(H, size, it, iters))
        for p in sorted({1, min(size, K), K}):
            np.testing.assert_array_equal(R.polyphony(H, energy, p, it, iters), R.polyphony_literal(H, energy, p, it, iters))
    np.testing.assert_allclose(R.continuity(H, size), R.continuity_literal(H, size), rtol=1e-15, atol=0)


def test_polyphony_ties_go_to_the_lower_row():
    H = np.array([[1.0], [2.0], [2.0], [0.5]])
    out = R.polyphony(H, np.ones(4), 1, 0, 1)
    assert out[:, 0].tolist() == [0.0, 2.0, 0.0, 0.0]
    np.testing.assert_array_equal(out, R.polyphony_literal(H, np.ones(4), 1, 0, 1))


def test_constraint_factor_is_integer_division():
    # 1 on every iteration but the last, 0 on the last (NMFCross.hpp:132, :150)
    assert [R.decay(i, 5) for i in range(5)] == [1, 1, 1, 1, 0]
    assert R.decay(0, 1) == 0
    H = _random_h(6, 9, 3)
    e = np.ones(6)
    np.testing.assert_array_equal(R.sparsity(H, 3, 3, 5), H)
    np.testing.assert_array_equal(R.polyphony(H, e, 2, 3, 5), H)
    assert (R.sparsity(H, 3, 4, 5) != H).any()
    assert ((R.polyphony(H, e, 2, 4, 5) > 0).sum(axis=0) <= 2).all()


def test_one_iteration_applies_the_constraints_at_iteration_zero():
    rng = np.random.default_rng(5)
    X, W0 = rng.random((12, 9)), rng.random((7, 9))
    H1 = R.nmfcross(X, W0, 3, 2, 1, 1, seed=11)
    # with c = 1 continuity is the identity: H1's zeros are exactly where sparsity and polyphony removed entries of H0
    H0 = R.initial_h(7, 12, 11)
    kept = R.polyphony(R.sparsity(H0, 3, 0, 1), (np.maximum(W0.T, R.EPS) ** 2).sum(axis=0), 2, 0, 1)
    np.testing.assert_array_equal(H1.T > 0, kept > 0)
    assert ((H1 > 0).sum(axis=1) <= 2).all()
    np.testing.assert_allclose(R.nmfcross(X, W0, 3, 2, 1, 1, seed=11, literal=True), H1, rtol=1e-15, atol=0)


def test_literal_and_vectorised_pipelines_agree():
    rng = np.random.default_rng(9)
    X, W0 = rng.random((15, 11)), rng.random((10, 11))
    for r, p, c, iters in [(7, 10, 7, 3), (1, 1, 1, 2), (3, 10, 5, 4), (9, 1, 3, 2)]:
        a = R.nmfcross(X, W0, r, p, c, iters, seed=1)
        b = R.nmfcross(X, W0, r, p, c, iters, seed=1, literal=True)
        np.testing.assert_array_equal(a > 0, b > 0)
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=0)


def test_initial_h_is_the_column_major_fill():
    u = oracle_np.rng_uniform01(42, 12)
    H = R.initial_h(3, 4, 42)            # K x T column-major: entry (k, t) is draw t K + k
    assert H[2, 1] == u[1 * 3 + 2] and H[0, 3] == u[9]


def test_griffinlim_phase_draws_are_column_major():
    T, F, seed = 5, 3, 77
    u = oracle_np.rng_uniform01(seed, T * F)
    ph = R.random_phase(T, F, seed)
    for t in range(T):
        for f in range(F):
            th = 2 * np.pi * u[f * T + t]
            assert ph[t, f] == np.cos(th) + 1j * np.sin(th)


def test_istft_of_stft_is_the_signal():
    x = oracle_np.synth_audio(3000, 5)
    spec, _ = oracle_np.stft(x, 256, 512, 64)
    np.testing.assert_allclose(R.istft(spec, len(x), 256, 512, 64), x, atol=1e-12)


def test_client_messages_in_the_reference_order():
    assert R.check_client(0, 0, 512, 100, 100) == "Empty source buffer"
    assert R.check_client(10, 0, 512, 100, 100) == "Empty target buffer"
    assert R.check_client(10, 1024, 512, 4, 4) == "Time Sparsity is larger than target frames"
    assert R.check_client(10, 1024, 512, 3, 4) == "Continuity is larger than target frames"
    assert R.check_client(10, 1024, 512, 3, 3) is None


def test_goldens_are_reproduced():
    g = np.load(os.path.join(ROOT, "tests", "golden", "nmfcross_v1.npz"))
    names = sorted({k.split("_")[0] for k in g.files})
    assert names == ["a", "b", "c"]
    for n in names:
        win, fft, hop, r, p, c, iters, seed = (int(v) for v in g[f"{n}_params"])
        y, H1 = R.bufnmfcross(g[f"{n}_source"], g[f"{n}_target"], win, fft, hop, r, p, c, iters, seed, return_h=True)
        np.testing.assert_array_equal(H1 > 0, g[f"{n}_H1"] > 0)
        np.testing.assert_allclose(H1, g[f"{n}_H1"], rtol=1e-12, atol=0)
        assert np.abs(y - g[f"{n}_output"]).max() <= 1e-6 * np.abs(g[f"{n}_output"]).max()


def test_header_declares_the_nmfcross_entries():
    text = open(os.path.join(ROOT, "include", "flucoma_hip.h")).read()
    assert re.search(r"#define FLUHIP_ABI_VERSION 5\b", text)
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", body), name


def test_binding_lists_the_nmfcross_entries():
    import fluhip
    for name in NEW_SYMBOLS:
        assert name in fluhip.EXPORTS
    for meth in ("nmfcross_process", "griffinlim", "bufnmfcross"):
        assert callable(getattr(fluhip.Context, meth))


def test_library_exports_the_nmfcross_entries(fluhip_lib_path):
    lib = ctypes.CDLL(fluhip_lib_path)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name


def test_build_lists_the_new_sources():
    import importlib.util
    spec = importlib.util.spec_from_file_location("fluhip_build_x", os.path.join(ROOT, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "kernels_nmfcross.hip" in mod.SOURCES and "api_cross.hip" in mod.SOURCES


# ---- the C++ client's host side (include/flucoma_hip/NMFCrossClient.hpp, tests/cpp/nmfcross_driver.cpp) ------------------
@pytest.fixture(scope="module")
def driver(fluhip_lib_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("fluhip_build_d", os.path.join(ROOT, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build_nmfcross_driver()


def _drive(driver, *args):
    import subprocess
    r = subprocess.run([driver, *[str(a) for a in args]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cpp_client_error_paths(driver):
    got = [l.split("|") for l in _drive(driver, "errors").splitlines()]
    assert got == [["no_source", "2", "Source Buffer Supplied But Invalid"], ["no_target", "2", "Target Buffer Supplied But Invalid"],
                   ["no_output", "2", "Output Buffer Supplied But Invalid"], ["empty_source", "2", "Empty source buffer"],
                   ["empty_target", "2", "Empty target buffer"],
                   ["sparsity_too_large", "2", "Time Sparsity is larger than target frames"],
                   ["continuity_too_large", "2", "Continuity is larger than target frames"]]


@pytest.mark.parametrize("args,want", [
    ((7, 11, 7, 50, 1024, -1, -1), "7 11 7 50"),
    ((4, 12, 6, 3, 1024, -1, -1), "5 13 7 3"),          # Odd(): an even value becomes the next odd one
    ((0, -4, -1, 0, 1024, -1, -1), "1 1 1 1"),          # Min(1) first
    ((3, 1200, 3, 5, 1024, -1, -1), "3 513 3 5"),       # FrameSizeUpperLimit<kFFT>: fft 1024 -> 513 bins
    ((3, 1200, 3, 5, 256, -1, -1), "3 129 3 5"),
    ((3, 600, 3, 5, 1000, -1, 2048), "3 601 3 5"),      # (601 <= 1025 bins of fft 2048)
])
def test_cpp_client_constraints(driver, args, want):
    assert _drive(driver, "constrain", *args).strip() == want


def test_cpp_client_descriptors_are_the_references_table(driver):
    import json
    mine = json.loads(_drive(driver, "descriptors"))
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "param_descriptors_nmfcross.json")))
    assert mine == want
    assert [d["name"] for d in mine["BufNMFCross"]] == ["source", "target", "output", "timeSparsity", "polyphony", "continuity",
                                                       "iterations", "seed", "fftSettings"]
    if os.path.isdir("/root/reference/include/flucoma"):
        import subprocess
        import sys
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_param_descriptor_fixture.py"), "--nmfcross"],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and json.loads(r.stdout) == want
