"""CPU tests of tests/hpss_ref.py, the numpy restatement of the reference's harmonic / percussive separation: the literal
streaming model against the closed form the GPU computes (which pins the off-by-one of the harmonic median and the
forward-looking percussive median), the medians against a brute-force sort, the reconstruction property of modes 1 and 2, the
distance of the GPU tests' inputs from a tie, the floor between two double STFTs that sets the GPU tests' bar, the parameter
table, the plan and the ABI symbols."""
import ctypes
import json
import os

import numpy as np
import pytest

import hpss_ref as R
import oracle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TIE_GUARD = 1e-9   # relative; about six orders above the ulp-level difference between two double FFTs
KNEE = (0.1, 3.0, 0.6, 9.0)          # a real knee: bins 12 .. 76 of 129
KNEE_ONE = (0.5, 2.0, 0.505, 6.0)    # floor(64.5) = 64, floor(65.145) = 65 of 129 bins: a knee of length 1 (LinSpaced yields y2)

# the largest |a - b| / peak between hpss_channel on numpy's FFT and on the project's C oracle STFT over AUDIO_CASES (peak: the
# largest |sample| of the input and of the expected output).  The constant is the measured figure (beside it) rounded up to two
# digits; test_audio_floor_between_two_double_stfts recomputes it on every host and allows 2 x.  The GPU bar
# (tests/test_gpu_hpss.py) is 64 x the constant, the factor the novelty and onset GPU tests use, plus 2^-24 of peak for the
# rounding of the float32 output.
AUDIO_FLOOR = 5.9e-16   # measured 5.829e-16 (the case with n below the window; the others 4.1e-16 .. 4.7e-16)

# ---- the inputs the GPU tests use: defined here so that the tie guard and the floor are proved on exactly them --------------
PLANE_SHAPE = (256, 256, 64)        # F = 129
PLANE_N = 17640                     # 0.4 s
# (hSize, vSize, mode, harmThresh, percThresh) of the GPU tests' mask comparisons in modes 1 and 2
MASK_CASES = [(17, 31, 1, R.DEFAULT_THRESH, R.DEFAULT_THRESH), (17, 31, 2, R.DEFAULT_THRESH, R.DEFAULT_THRESH),
              (3, 3, 2, KNEE, R.DEFAULT_THRESH), (33, 129, 1, KNEE, KNEE), (17, 31, 2, KNEE_ONE, KNEE),
              (65, 63, 2, R.DEFAULT_THRESH, KNEE_ONE), (63, 65, 1, KNEE_ONE, R.DEFAULT_THRESH)]
# name -> (n, seed, win, fft, hop, hSize, vSize, mode, harmThresh, percThresh) of the GPU tests' audio comparisons
AUDIO_CASES = {
    "block_mode0": (22050, 11, 1024, 1024, 512, 17, 31, 0, R.DEFAULT_THRESH, R.DEFAULT_THRESH),
    "block_mode1": (22050, 11, 1024, 1024, 512, 17, 31, 1, R.DEFAULT_THRESH, R.DEFAULT_THRESH),
    "block_mode2": (22050, 11, 1024, 1024, 512, 17, 31, 2, KNEE, R.DEFAULT_THRESH),
    "win_below_fft": (5003, 12, 256, 512, 48, 17, 31, 0, R.DEFAULT_THRESH, R.DEFAULT_THRESH),
    "fft4096": (44100, 13, 4096, 4096, 1024, 17, 31, 0, R.DEFAULT_THRESH, R.DEFAULT_THRESH),
    "n_below_win": (700, 14, 1024, 1024, 512, 5, 31, 0, R.DEFAULT_THRESH, R.DEFAULT_THRESH),
}

_cache = {}


def plane_mag():
    """the magnitude plane [T, 129] of 0.4 s of drum_like audio at (256, 256, 64), computed once"""
    if "plane" not in _cache:
        x = oracle_np.drum_like(PLANE_N, seed=7)
        _cache["plane"] = np.ascontiguousarray(np.abs(R.frame_spectra(x, *PLANE_SHAPE)))
    return _cache["plane"]


def audio_case(name, stft=None):
    """(audio float32, expected float64 [3, n]) of an AUDIO_CASES entry, computed once"""
    key = (name, stft is not None)
    if key not in _cache:
        n, seed, win, fft, hop, h, v, mode, ht, pt = AUDIO_CASES[name]
        x = oracle_np.drum_like(n, seed=seed).astype(np.float32)
        _cache[key] = (x, R.hpss_channel(x, win, fft, hop, h, v, mode, ht, pt, stft=stft))
    return _cache[key]


def peak_of(x, want):
    return max(float(np.abs(x).max()), float(np.abs(want).max()))


def stream_audio():
    if "stream" not in _cache:
        _cache["stream"] = oracle_np.drum_like(4000, seed=3).astype(np.float64)
    return _cache["stream"]


# ---- the literal model against the closed form ----------------------------------------------------------------------
@pytest.mark.parametrize("v_size", [3, 31])
@pytest.mark.parametrize("h_size", [3, 5, 17])
@pytest.mark.parametrize("shape", [(256, 256, 64), (256, 512, 48), (128, 128, 128)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_streaming_equals_the_closed_form(mode, shape, h_size, v_size):
    win, fft, hop = shape
    n = 1500 + 7 * h_size + v_size            # no multiple of hop or of 64
    assert n % hop and n % 64
    x = stream_audio()[:n]
    a = R.hpss_streaming(x, win, fft, hop, h_size, v_size, mode, KNEE if mode else R.DEFAULT_THRESH)
    b = R.hpss_channel(x, win, fft, hop, h_size, v_size, mode, KNEE if mode else R.DEFAULT_THRESH)
    assert a.shape == b.shape == (3, n) and np.abs(a[:2]).max() > 0.01
    assert np.abs(a - b).max() <= 1e-12 * np.abs(x).max()


def test_the_centred_variants_are_not_what_the_reference_computes():
    """an H median centred ON the masked frame, or a V median centred on the bin, misses the streaming model by far"""
    x = stream_audio()[:1601]
    for mode in (0, 1, 2):
        a = R.hpss_streaming(x, 256, 256, 64, 17, 31, mode)
        for variant in (dict(_h_back=0), dict(_v_centred=True)):
            b = R.hpss_channel(x, 256, 256, 64, 17, 31, mode, **variant)
            assert np.abs(a - b).max() > 1e-3 * np.abs(x).max(), (mode, variant)


def test_a_short_buffer_and_a_long_filter():
    """n below the window, and an H filter longer than the buffer has frames"""
    x = stream_audio()[:100]
    for h_size in (3, 33):
        a = R.hpss_streaming(x, 256, 256, 64, h_size, 31, 2)
        b = R.hpss_channel(x, 256, 256, 64, h_size, 31, 2)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(x).max()


def test_median_filter_model_is_a_selection_of_the_last_values():
    rng = np.random.default_rng(1)
    v = np.round(rng.standard_normal(60), 1)          # with ties
    for size in (3, 5, 17):
        f = R.MedianFilterModel(size)
        got = [f.process_sample(s) for s in v]
        zz = np.concatenate([np.zeros(size - 1), v])
        assert got == [np.sort(zz[i:i + size])[size // 2] for i in range(len(v))]


@pytest.mark.parametrize("h_size,v_size", [(3, 3), (17, 31), (33, 129), (5, 63)])
def test_plane_medians_equal_a_brute_force_sort(h_size, v_size):
    mag = plane_mag()[:60]
    T, F = mag.shape
    hmed, vmed, _ = R.hpss_planes(mag, h_size, v_size)
    h2 = (h_size - 1) // 2
    for t in range(T):
        for f in range(0, F, 7):
            rows = [mag[r, f] if 0 <= r < T else 0.0 for r in range(t - h2 - 1, t + h2)]        # frames m - h2 - 1 .. m + h2 - 1
            bins = [mag[t, g] if g < F else 0.0 for g in range(f, f + v_size)]                  # bins f .. f + vSize - 1
            assert len(rows) == h_size
            assert hmed[t, f] == np.sort(rows)[h_size // 2] and vmed[t, f] == np.sort(bins)[v_size // 2]


def test_threshold_table():
    assert (R.make_threshold(129, *R.DEFAULT_THRESH) == 10.0 ** 0.05).all()
    thr = R.make_threshold(129, *KNEE)
    assert (thr[:12] == 10.0 ** (3 / 20)).all() and (thr[77:] == 10.0 ** (9 / 20)).all()
    assert thr[12] == 10.0 ** (3 / 20) and thr[76] == 10.0 ** (9 / 20) and (np.diff(thr[12:77]) > 0).all()
    one = R.make_threshold(129, *KNEE_ONE)
    assert (one[:64] == 10.0 ** 0.1).all() and (one[64:] == 10.0 ** 0.3).all()     # length 1: Eigen's LinSpaced yields HIGH
    assert list(R.lin_spaced(1, 2.0, 6.0)) == [6.0] and list(R.lin_spaced(3, 1.0, 2.0)) == [1.0, 1.5, 2.0]
    assert list(R.lin_spaced(3, -4.0, 2.0)) == [-4.0, -1.0, 2.0]
    assert R.constrain_pairs((1.5, 3, -1, 9)) == (0.0, 9.0, 1.0, 3.0) and R.constrain_pairs(KNEE) == KNEE


def test_masks_on_zeros_and_infinities():
    z = np.zeros((2, 4))
    for mode, want in ((0, (0, 0, 0)), (1, (0, 1, 0)), (2, (0, 0, 1))):
        got = R.masks_of(z, z, mode, np.ones(4), np.ones(4))
        assert [float(g.max()) for g in got] == list(want) and [float(g.min()) for g in got] == list(want)
    hm, pm, rm = R.masks_of(np.array([1.0, 0.0, 2.0]), np.array([0.0, 1.0, 2.0]), 2, np.ones(3), np.ones(3))
    assert list(hm) == [1, 0, 0] and list(pm) == [0, 1, 0] and list(rm) == [0, 0, 1]          # x / 0 = +inf compares true
    hm, pm, rm = R.masks_of(np.array([3.0]), np.array([2.9]), 2, np.array([1.0]), np.array([0.5]))
    assert (hm[0], pm[0], rm[0]) == (0.5, 0.5, 0.0)                                           # both comparisons hold: 1 / 2


@pytest.mark.parametrize("mode", [1, 2])
def test_the_outputs_sum_to_the_input(mode):
    """mode 1: harmonic + percussive, mode 2: all three reproduce the input at every sample that window^2 covers"""
    x = stream_audio()[:3001]
    out = R.hpss_channel(x, 256, 256, 64, 17, 31, mode, KNEE, KNEE_ONE)
    ok = R.covered(len(x), 256, 64)
    assert ok.sum() >= len(x) - 2
    if mode == 1:
        assert not out[2].any()
    err = float(np.abs(out.sum(axis=0) - x)[ok].max() / np.abs(x).max())
    print(f"mode {mode}: reconstruction error {err:.3e} of peak (floor {AUDIO_FLOOR:.1e})")
    assert err <= AUDIO_FLOOR


# ---- the GPU tests' inputs keep clear of ties -----------------------------------------------------------------------
def test_the_gpu_mask_cases_keep_clear_of_ties():
    mag = plane_mag()
    for h, v, mode, ht, pt in MASK_CASES:
        m = R.tie_margin(mag, h, v, mode, ht, pt)
        print(f"planes h {h} v {v} mode {mode}: smallest relative distance from a threshold {m:.3e}")
        assert m >= TIE_GUARD          # zero bins excluded


def test_the_gpu_audio_cases_keep_clear_of_ties():
    for name, (n, seed, win, fft, hop, h, v, mode, ht, pt) in AUDIO_CASES.items():
        if mode == 0:
            continue
        x = audio_case(name)[0]
        m = R.tie_margin(np.abs(R.frame_spectra(x, win, fft, hop)), h, v, mode, ht, pt)
        print(f"{name}: smallest relative distance from a threshold {m:.3e}")
        assert m >= TIE_GUARD


def test_audio_floor_between_two_double_stfts(oracle):
    worst = 0.0
    for name in AUDIO_CASES:
        x, a = audio_case(name)
        b = audio_case(name, stft=oracle.stft)[1]
        e = float(np.abs(a - b).max()) / peak_of(x, a)
        print(f"{name}: |numpy - C oracle| / peak = {e:.3e}")
        worst = max(worst, e)
    print(f"audio floor {worst:.3e} (constant {AUDIO_FLOOR:.1e})")
    assert worst <= 2 * AUDIO_FLOOR


# ---- the plan, the ABI, the build list (pure host code of the built library) ------------------------------------------
@pytest.fixture(scope="module")
def lib(fluhip_lib_path):
    import fluhip
    return fluhip.load_library(fluhip_lib_path)


def plan(lib, h, v):
    out = (ctypes.c_int64 * 4)()
    return None if lib.fluhip_debug_hpss_plan(None, h, v, out) else tuple(int(x) for x in out)


def test_the_library_exports_the_hpss_entry_points(fluhip_lib_path):
    L = ctypes.CDLL(fluhip_lib_path)
    for name in ("fluhip_hpss_planes_f64", "fluhip_bufhpss_f32", "fluhip_debug_hpss_plan"):
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "flucoma_hip.h")).read()
    assert "#define FLUHIP_ABI_VERSION 5" in header and L.fluhip_abi_version() == 5


def test_plan_table(lib):
    """(form of H, form of V, LDS bytes, bins per workgroup): on chip up to size 63 for either filter, the LDS the kernel's own
    arithmetic ([hSize][256] doubles + 256 + vSize - 1 doubles), and never above what a workgroup may have"""
    assert plan(lib, 17, 31) == (0, 0, (17 * 256 + 256 + 30) * 8, 256)
    assert plan(lib, 3, 3) == (0, 0, (3 * 256 + 258) * 8, 256)
    assert plan(lib, 63, 63) == (0, 0, (63 * 256 + 256 + 62) * 8, 256) and plan(lib, 63, 63)[2] <= 160 * 1024
    assert plan(lib, 65, 63) == (1, 0, (256 + 62) * 8, 256) and plan(lib, 63, 65) == (0, 1, 63 * 256 * 8, 256)
    assert plan(lib, 65, 65) == (1, 1, 0, 256) and plan(lib, 101, 129) == (1, 1, 0, 256)
    for h in range(3, 131, 2):
        for v in (3, 63, 65, 1001):
            p = plan(lib, h, v)
            assert p[0] == (h > 63) and p[1] == (v > 63) and p[2] <= 160 * 1024


def test_plan_refusals(lib):
    for h, v in ((4, 31), (1, 31), (17, 30), (17, 1), (-3, 31), (1003, 31), (17, 1003)):
        assert plan(lib, h, v) is None
    assert lib.fluhip_debug_hpss_plan(None, 17, 31, None) != 0


def test_build_lists_the_hpss_sources():
    text = open(os.path.join(ROOT, "flucoma-core_amd", "build.py")).read()
    assert '"kernels_hpss.hip"' in text and '"api_hpss.hip"' in text and '"kernels_hpss.hip": ["-ffp-contract=off"]' in text


# ---- the C++ host client (include/flucoma_hip/HPSSClient.hpp) through tests/cpp/hpss_driver.cpp, without a device ------
@pytest.fixture(scope="module")
def hpss_driver(fluhip_lib_path):
    return R.build_driver()


def test_cpp_client_descriptors_are_the_references_table(hpss_driver):
    mine = json.loads(R.drive(hpss_driver, "descriptors"))
    want = json.load(open(os.path.join(GOLDEN, "param_descriptors_hpss.json")))
    assert mine == want
    assert [d["name"] for d in mine["BufHPSS"]] == ["source", "startFrame", "numFrames", "startChan", "numChans", "harmonic",
                                                   "percussive", "residual", "harmFilterSize", "percFilterSize", "maskingMode",
                                                   "harmThresh", "percThresh", "fftSettings"]
    ht = [d for d in mine["BufHPSS"] if d["name"] == "harmThresh"][0]
    assert (ht["kind"], ht["default"], ht["fixedSize"]) == ("FloatPairsArray", [0, 1, 1, 1], 4)


def test_cpp_client_error_paths(hpss_driver):
    got = [l.split("|") for l in R.drive(hpss_driver, "errors").splitlines()]
    assert got == [["no_source", "2", "Input buffer not set"], ["no_output", "2", "No valid output has been set"],
                   ["start_past_end", "2", "Input buffer  invalid start frame 5000"],
                   ["chan_past_end", "2", "Input buffer  invalid start channel 3"]]


@pytest.mark.parametrize("args,want", [
    ((4, 2, 7, 0.9, 3, 0.2, 9, 1000, -1, -1), "5 3 2 0.2 9 0.9 3 1000 500 1024"),     # Odd: 4 -> 5; Min(3); a pair in the wrong order
    ((17, 31, -1, -0.5, 1, 1.5, 2, 512, 256, 1024), "17 31 0 0 1 1 2 512 256 1024"),   # frequencies clipped to [0, 1]
])
def test_cpp_client_constraints(hpss_driver, args, want):
    assert R.drive(hpss_driver, "constrain", *args).strip() == want
