"""CPU tests of tests/onset_ref.py, the numpy restatement of the reference's onset detection: the slice positions the
reference's own TestOnsetSegmentation.cpp asserts (tests/golden/onset_reference_cases.json), the distance of those cases
from a tie, the floor between two double STFTs that sets the GPU tests' bar, and the quirks, each on a tiny case."""
import json
import os

import numpy as np
import pytest

import onset_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLDEN, "onset_reference_cases.json")))["cases"]
TIE_GUARD = 1e-7   # the novelty tests' guard

# the largest element-wise |a - b| / max(1, |a|) between the restatement on numpy's FFT and on the project's C oracle STFT, per
# metric, over floor_inputs() at win 512 / hop 128 / fft 512 under the harness framing.  Each constant is the measured figure
# (beside it) rounded UP to two digits; test_curve_floor_between_two_double_stfts asserts measured <= constant on every host
# it runs on, and the GPU bar is 64 x the constant (tests/test_gpu_onset.py).  No frame is left out.
CURVE_FLOOR = {
    0: 4.5e-16,   # measured 4.458e-16
    1: 4.5e-16,   # measured 4.453e-16
    2: 1.2e-16,   # measured 1.110e-16
    3: 1.3e-14,   # measured 1.230e-14
    4: 1.3e-12,   # measured 1.205e-12 (values up to 1.16e30 on the frame after silence)
    5: 4.5e-16,   # measured 4.441e-16
    6: 4.5e-16,   # measured 4.441e-16
    7: 4.5e-16,   # measured 4.441e-16
    8: 2.8e-16,   # measured 2.765e-16
    9: 2.8e-16,   # measured 2.765e-16
}

# thresholds of the GPU tests' detection comparison on floor_inputs(), one per metric, chosen on the restatement so that every
# frame of every filter size is further from the threshold than TIE_GUARD plus twice the GPU allowance of that frame
# (test_the_detection_thresholds_keep_clear_of_ties proves it): identity of the detections is then a fair demand
DETECT_THRESHOLDS = {0: 0.242, 1: 4.2, 2: 0.07, 3: 0.191, 4: 5.3, 5: 0.021, 6: 0.043, 7: 0.073, 8: 0.23, 9: 0.23}
DETECT_FILTERS = (1, 5, 29)
DETECT_MIN_SLICE = 3

_cache = {}


def filtered_allowance(want_raw, want_filtered, bar):
    """filtered = raw - median, and the median is one of the raw values: each of the two carries an error of at most
    bar x max(1, |itself|), so the difference is held to the sum of the two allowances"""
    med = want_raw - want_filtered
    return bar * (np.maximum(1.0, np.abs(want_raw)) + np.maximum(1.0, np.abs(med)))


def detection_inputs(function):
    """(name, padded signal, frames, raw curve of the restatement) of the floor inputs at win 512 / fft 512 / hop 128, computed once"""
    key = ("detect", function)
    if key not in _cache:
        out = []
        for name, x in floor_inputs().items():
            z, T = R.harness_signal(x, 512, 128)
            out.append((name, z, T, R.raw_curve(z, T, 512, 512, 128, function)))
        _cache[key] = out
    return _cache[key]


def floor_inputs():
    if "floor" not in _cache:
        noise = (0.1 * np.random.default_rng(7).standard_normal(20000)).astype(np.float32).astype(np.float64)
        _cache["floor"] = {"drums": R.mono_drums(GOLDEN)[:40000], "noise": noise}
    return _cache["floor"]


def case_run(case):
    """(positions, filtered curve) of a fixture case, computed once"""
    key = case["label"]
    if key not in _cache:
        _cache[key] = R.harness(R.signal(case["signal"], GOLDEN), case["window"], case["hop"], case["fft"], case["metric"],
                                case["minSliceLength"], case["filterSize"], case["threshold"], case["frameDelta"],
                                want_filtered=True)
    return _cache[key]


def test_the_fixture_holds_every_case_of_the_reference():
    assert len(CASES) == 7 + 1 + 9 + 3 + 1
    assert sorted({c["metric"] for c in CASES if c["label"].startswith("test_drums_")}) == [0, 1, 2, 3, 5, 6, 7, 8, 9]
    assert max((len(R.harness_signal(np.zeros(453932), c["window"], c["hop"])[0]) - c["window"]) // c["hop"] for c in CASES) == 11397


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_reference_held_positions(case):
    got = case_run(case)[0]
    assert len(got) == len(case["expected"])
    if case["margin"] <= 1:
        assert got == case["expected"]
    else:
        assert np.abs(np.array(got) - np.array(case["expected"])).max() <= case["margin"]


def test_the_drum_cases_keep_clear_of_ties():
    worst = min(float(np.abs(case_run(c)[1] - c["threshold"]).min()) for c in CASES if c["signal"] == "monoDrums")
    print(f"smallest |filtered - threshold| over the drum cases: {worst:.3e}")
    assert worst >= TIE_GUARD


@pytest.mark.parametrize("function", range(10))
def test_the_detection_thresholds_keep_clear_of_ties(function):
    thr, bar = DETECT_THRESHOLDS[function], 64 * CURVE_FLOOR[function]
    for name, z, T, raw in detection_inputs(function):
        for fs in DETECT_FILTERS:
            f = R.filter_curve(raw, fs)
            margin = np.abs(f - thr) - 2 * filtered_allowance(raw, f, bar)
            print(f"metric {function} {name} filter {fs}: smallest margin {margin.min():.3e}, {int(R.detect(f, thr, DETECT_MIN_SLICE).sum())} detections")
            assert margin.min() >= TIE_GUARD
            assert R.detect(f, thr, DETECT_MIN_SLICE).sum() >= 1


def test_curve_floor_between_two_double_stfts(oracle):
    for function in range(R.N_FUNCTIONS):
        worst = 0.0
        for x in floor_inputs().values():
            z, T = R.harness_signal(x, 512, 128)
            a = R.raw_curve(z, T, 512, 512, 128, function)
            b = R.raw_curve(z, T, 512, 512, 128, function, stft=oracle.stft)
            worst = max(worst, float((np.abs(a - b) / np.maximum(1.0, np.abs(a))).max()))
        print(f"metric {function}: floor {worst:.3e} (constant {CURVE_FLOOR[function]:.1e})")
        assert worst <= CURVE_FLOOR[function]


# ---- the quirks, each on a case small enough to compute by hand -------------------------------------------------------
def test_hfc_weights_are_linspaced_to_n_inclusive():
    assert list(R.hfc_weights(3)) == [0.0, 1.5, 3.0]          # LinSpaced(3, 0, 3), not the bin indices 0, 1, 2
    X = np.array([[1.0 + 0j, 2.0, 2.0j]])
    assert R.odf(1, X, X, X)[0] == (0 * 1 + 1.5 * 4 + 3 * 4) / 3
    assert R.odf(0, X, X, X)[0] == (1 + 4 + 4) / 3            # energy is the MEAN of |X|^2


def test_filter_size_one_returns_the_raw_value():
    raw = np.array([3.0, -1.0, 7.0, 2.0])
    assert (R.filter_curve(raw, 1) == raw).all()


def test_the_median_starts_from_zeros():
    raw = np.array([5.0, 6.0, 7.0, 1.0, 1.0])
    # windows (0 0 5) (0 5 6) (5 6 7) (6 7 1) (7 1 1) -> medians 0 5 6 6 1
    assert list(R.running_median(raw, 3)) == [0.0, 5.0, 6.0, 6.0, 1.0]
    assert list(R.filter_curve(raw, 3)) == [5.0, 1.0, 1.0, -5.0, 0.0]
    assert list(R.running_median(np.array([4.0, 4.0, 4.0]), 5)) == [0.0, 0.0, 4.0]   # sorted[5 / 2] of (0 0 0 0 4) ...


def test_detection_and_debounce():
    f = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    assert list(R.detect(f, 0.5, 0)) == [0, 1, 0, 1, 0, 0, 1, 0, 0, 1]
    assert list(R.detect(f, 0.5, 2)) == [0, 1, 0, 0, 0, 0, 1, 0, 0, 1]   # the counter is 2, 1, 0 on the three frames after
    assert list(R.detect(f, 0.5, 4)) == [0, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert list(R.detect(np.array([1.0, 1.0]), 0.5, 0)) == [1, 0]       # the previous value starts at 0


def test_frame_delta_has_no_effect_on_metric_5_and_one_on_metric_2():
    x = floor_inputs()["noise"][:6000]
    z, T = R.harness_signal(x, 512, 128)
    assert (R.raw_curve(z, T, 512, 512, 128, 5, 100) == R.raw_curve(z, T, 512, 512, 128, 5, 0)).all()
    assert not (R.raw_curve(z, T, 512, 512, 128, 2, 100) == R.raw_curve(z, T, 512, 512, 128, 2, 0)).all()


def test_metrics_8_and_9_are_bit_equal():
    x = floor_inputs()["drums"][:8000]
    z, T = R.harness_signal(x, 512, 128)
    assert (R.raw_curve(z, T, 512, 512, 128, 8) == R.raw_curve(z, T, 512, 512, 128, 9)).all()


def test_the_phase_is_the_complex_arctangent_and_the_wrap_is_kept_as_written():
    assert R.catan_re(np.array([2.0j]))[0] == np.pi / 2 and abs(np.angle(2.0j) - np.pi / 2) < 1e-15
    assert abs(R.catan_re(np.array([1.0 + 0j]))[0] - np.pi / 4) < 1e-15          # atan(1), where the angle of 1 is 0
    assert R.wrap_phase(4.0) == 4.0                                               # above pi: unchanged
    assert abs(R.wrap_phase(1.0) - (1.0 + 2 * np.pi * (1 + np.floor((-np.pi - 1.0) / (2 * np.pi))))) == 0
    assert abs(R.wrap_phase(1.0) - 1.0) < 1e-15 and abs(R.wrap_phase(-4.0) - (2 * np.pi - 4.0)) < 1e-15


def test_wrapper_framings_agree_with_the_harness_on_the_impulses():
    one = R.one_impulse().astype(np.float32)
    got = R.bufonsetslice(one, 0, 0.5, 2, 5, 0, 1024, 1024, 512)
    assert list(got) == [22016]   # the harness's position: same frames, same latency correction
    got = R.bufonsetslice(R.stereo_impulses().astype(np.float32), 9, 0.1, 2, 5, 0, 512, 512, 64, start_frame=100)
    assert list(got) == [1124, 12132, 23140, 34212]
    f = R.bufonsetfeature(one, 0, 5, 0, 1024, 1024, 512, padding_mode=1)
    assert f.dtype == np.float32 and len(f) == 1 + (44100 + 512 + 1024 - 1024) // 512 - 1


def test_build_lists_the_onset_sources():
    text = open(os.path.join(ROOT, "flucoma-core_amd", "build.py")).read()
    assert '"kernels_onset.hip"' in text and '"api_onset.hip"' in text


# ---- the C++ host clients (include/flucoma_hip/OnsetSliceClient.hpp) through tests/cpp/onset_driver.cpp, without a device
@pytest.fixture(scope="module")
def onset_driver(fluhip_lib_path):
    return R.build_driver()


def test_cpp_client_descriptors_are_the_references_tables(onset_driver):
    mine = json.loads(R.drive(onset_driver, "descriptors"))
    want = json.load(open(os.path.join(GOLDEN, "param_descriptors_onset.json")))
    assert mine == want
    assert [d["name"] for d in mine["BufOnsetSlice"]][5:] == ["indices", "metric", "threshold", "minSliceLength", "filterSize",
                                                             "frameDelta", "fftSettings"]
    assert [d["name"] for d in mine["BufOnsetFeature"]][5:] == ["features", "padding", "metric", "filterSize", "frameDelta",
                                                               "fftSettings"]
    fs = [d for d in mine["BufOnsetSlice"] if d["name"] == "filterSize"][0]
    assert (fs["default"], fs["min"], fs["max"], fs["relational"]) == (5, 1, 101, "Odd")
    if os.path.isdir("/root/reference/include/flucoma"):
        import subprocess
        import sys
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_param_descriptor_fixture.py"), "--onset"],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and json.loads(r.stdout) == want


def test_cpp_client_error_paths(onset_driver):
    got = [l.split("|") for l in R.drive(onset_driver, "errors").splitlines()]
    assert got == [["slice_no_source", "2", "Input buffer not set"], ["slice_no_output", "2", "No valid output has been set"],
                   ["slice_start_past_end", "2", "Input buffer  invalid start frame 5000"],
                   ["feature_no_source", "2", "Input buffer not set"], ["feature_no_output", "2", "No valid output has been set"]]


@pytest.mark.parametrize("args,want", [
    ((12, -1, -3, 4, 9000, 1000, -1, -1), "9 0 0 5 8192 1000 500 1024"),    # Odd(): 4 -> 5; Min() / Max() on the rest
    ((-2, 0.25, 10, 103, -5, 512, 256, 1024), "0 0.25 10 101 0 512 256 1024"),
    ((3, 2, 2, 0, 100, 800, 330, 1024), "3 2 2 1 100 800 330 1024"),
])
def test_cpp_client_constraints(onset_driver, args, want):
    assert R.drive(onset_driver, "constrain", *args).strip() == want
