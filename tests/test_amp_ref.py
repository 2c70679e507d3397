"""CPU tests of tests/amp_ref.py, the literal model of the reference's BufAmpSlice / BufAmpFeature, and of what the device
tests (tests/test_gpu_amp.py) rest on: the model gives the reference's own expected lists exactly, every behaviour a tidy
reader would write differently is shown to matter, the closed forms of the two offline clients equal the sample-by-sample
drive of the real-time clients, and every input the device's detections are compared on is clear of ties by a wide margin."""
import json
import os
import re

import numpy as np
import pytest

import amp_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FACTOR = 64          # the project's margin for two correct evaluations in different precision
CLEAR = 1000         # a threshold stays this many envelope bars away from every envelope value
SYMBOLS = ["fluhip_amp_envelope_f64", "fluhip_amp_slices_f64", "fluhip_bufampslice_f32", "fluhip_bufampfeature_f32",
           "fluhip_debug_amp_plan"]


@pytest.fixture(scope="module")
def amp_driver(fluhip_lib_path):
    return A.build_driver()


# ---- the reference's own cases ---------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_six_cases():
    cases = A.reference_cases()
    assert [c[0] for c in cases] == ["impulses", "sharp_sines", "schmitt", "debounce", "debounce_schmitt", "drums"]
    assert all(c[4] == 1 for c in cases)
    assert len(cases[-1][3]) == 23 and len(A.mono_drums()) == 453932


@pytest.mark.parametrize("case", A.reference_cases(), ids=lambda c: c[0])
def test_model_gives_the_reference_s_expected_positions_exactly(case):
    name, signal, p, expected, _ = case
    assert A.slices(A.reference_signal(signal), p) == expected


# ---- what a tidy reader would write differently ----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", A.VARIANTS)
def test_each_tidied_variant_gives_another_answer(variant):
    what, x, p = A.variant_inputs()[variant]
    pos, env = A.slices(x, p, want_values=True)
    vpos, venv = A.slices(x, p, variant=variant, want_values=True)
    if what == "positions":
        assert pos != vpos, (pos[:8], vpos[:8])
    else:
        assert not np.array_equal(env, venv)


def test_the_variants_are_all_named():
    assert set(A.variant_inputs()) == set(A.VARIANTS)


def test_behaviours_kept():
    # a zero gives -inf, which becomes the floor; both followers start there, so silence is exactly 0
    assert np.all(A.envelope(np.zeros(50), floor=-33.0, hipass=0.01) == 0.0)
    # 0 bypasses the filter: the level of a constant is its own, not the high-passed one
    lv = A.level(np.full(8, 0.5), -144.0, 0.0)
    assert lv == [20 * np.log10(0.5)] * 8
    # the cutoff is capped at half the sample rate
    assert A.hipass_fraction(30000.0) == 0.5 == A.hipass_fraction(22050.0) and A.hipass_fraction(0.0) == 0.0
    # a sample that is not finite repeats the last finite one, 0 before the first
    x = np.array([np.nan, np.inf, 0.25, np.nan, -np.inf, -0.5, np.nan])
    assert A.level(x, -144.0, 0.0) == A.level(np.array([0.0, 0.0, 0.25, 0.25, 0.25, -0.5, -0.5]), -144.0, 0.0)
    # minSliceLength 0 is legal: with the state falling at once a slice may start on every second sample
    x = np.tile([1.0, 0.001], 200)
    pos = A.slices(x, A.params(on=0.0, off=144.0, min_slice=0, high_pass_freq=0.0))
    assert len(pos) > 20 and set(np.diff(pos)) == {2}


# ---- the two offline clients ----------------------------------------------------------------------------------------------
CLIENT_PARAMS = A.params(fast_up=3, fast_down=80, slow_up=300, slow_down=300, on=12.0, off=6.0, floor=-70.0)


@pytest.mark.parametrize("chans,n,start", [(1, 1000, 0), (2, 1500, 7), (3, 64, 0), (1, 65, 3), (2, 1, 0)])
def test_slice_client_equals_the_literal_drive_of_the_real_time_client(chans, n, start):
    audio = np.stack([A.bursts(n, 20 + c) for c in range(chans)]).astype(np.float32)
    got = A.bufampslice(audio, CLIENT_PARAMS, start_frame=start)
    want = A.literal_bufampslice(audio, CLIENT_PARAMS, start_frame=start)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if n >= 1000:
        assert got[0] >= start   # a detection, not the -1 of silence


def test_slice_client_sums_the_channels_in_float_and_answers_silence_with_minus_one():
    a = np.array([[1e8, 1.0], [-1e8, 1.0], [1.0, 1e-9]], dtype=np.float32)
    assert np.array_equal(A.mono_sum(a), np.array([1.0, 2.0], dtype=np.float32))   # ((0 + 1e8) - 1e8) + 1, in float
    assert np.array_equal(A.bufampslice(np.zeros((2, 300), dtype=np.float32), CLIENT_PARAMS, start_frame=11), [-1])
    assert np.array_equal(A.literal_bufampslice(np.zeros((2, 300), dtype=np.float32), CLIENT_PARAMS, start_frame=11), [-1])


@pytest.mark.parametrize("chans,n", [(1, 700), (3, 130), (2, 64), (1, 1)])
def test_feature_client_equals_the_literal_drive_of_the_real_time_client(chans, n):
    audio = np.stack([A.bursts(n, 30 + c) for c in range(chans)]).astype(np.float32)
    got = A.bufampfeature(audio, CLIENT_PARAMS)
    want = A.literal_bufampfeature(audio, CLIENT_PARAMS)
    assert got.shape == (chans, n) and got.dtype == np.float32 and np.array_equal(got, want)
    for c in range(chans):   # every channel from a reset client: its own single call
        assert np.array_equal(got[c], A.bufampfeature(audio[c], CLIENT_PARAMS)[0])


# ---- clear of ties ---------------------------------------------------------------------------------------------------------
def detection_table():
    """every input whose detections tests/test_gpu_amp.py compares with the model: the six reference cases and
    amp_ref.detection_inputs()"""
    table = {"ref_" + name: (A.reference_signal(signal), p) for name, signal, p, _, _ in A.reference_cases()}
    table.update(A.detection_inputs())
    return table


@pytest.mark.parametrize("name", list(detection_table()))
def test_detection_inputs_are_clear_of_ties(name):
    """the smallest |value - on| and |value - off| over ALL samples of the input exceeds 1000 x the input's envelope bar
    (64 x the largest double-against-long-double difference of the model; taken on the first 60 000 samples of the drum
    loop, whose long double run is the only long one)"""
    x, p = detection_table()[name]
    _, values = A.slices(x, p, want_values=True)
    margin = A.threshold_margin(values, p["on"], p["off"])
    _, fmax, _ = A.precision_floor(("detect", name), x, p)
    bar = FACTOR * fmax
    print(f"{name}: margin {margin:.3e} dB, envelope bar {bar:.3e} dB, ratio {margin / bar if bar else np.inf:.3g}")
    assert margin > CLEAR * bar, (margin, bar)
    assert margin > 0


def test_reference_cases_margins_are_the_measured_ones():
    m = {}
    for name, signal, p, _, _ in A.reference_cases():
        _, values = A.slices(A.reference_signal(signal), p, want_values=True)
        m[name] = A.threshold_margin(values, p["on"], p["off"])
    assert 2.2e-5 < min(m.values()) < 2.4e-5 and 5.0e-3 < max(m.values()) < 5.2e-3, m


def test_front_end_chunk_of_the_table_is_the_kernels():
    text = open(os.path.join(ROOT, "flucoma-core_amd", "csrc", "fluhip_amp.h")).read()
    assert int(re.search(r"kAmpChunk\s*=\s*(\d+)", text).group(1)) == A.CHUNK


# ---- the host layers -------------------------------------------------------------------------------------------------------
def test_cpp_client_descriptors_are_the_references_tables(amp_driver):
    mine = json.loads(A.drive(amp_driver, "descriptors"))
    want = json.load(open(os.path.join(GOLDEN, "param_descriptors_amp.json")))
    assert mine == want
    ramps = ["fastRampUp", "fastRampDown", "slowRampUp", "slowRampDown"]
    assert [d["name"] for d in mine["BufAmpSlice"]][5:] == ["indices"] + ramps + ["onThreshold", "offThreshold", "floor",
                                                                                 "minSliceLength", "highPassFreq"]
    assert [d["name"] for d in mine["BufAmpFeature"]][5:] == ["features"] + ramps + ["floor", "highPassFreq"]
    on = [d for d in mine["BufAmpSlice"] if d["name"] == "onThreshold"][0]
    assert (on["default"], on["min"], on["max"]) == (144, -144, 144)


def test_cpp_client_validation_without_a_device(amp_driver):
    lines = dict(l.split("|", 1) for l in A.drive(amp_driver, "errors").splitlines())
    assert lines["slice_no_source"].startswith("2|") and lines["feature_no_source"].startswith("2|")
    assert lines["slice_no_output"] == "2|No valid output has been set" == lines["feature_no_output"]
    assert lines["slice_start_past_end"].startswith("2|")
    # the parameter table's constraints: Min(1) ramps, [-144, 144] thresholds and floor, Min(0) minSliceLength and highPassFreq
    assert A.drive(amp_driver, "constrain", 0, -3, 5, 0, 200, -200, 150, -1, -5).split() == \
        ["1", "1", "5", "1", "144", "-144", "144", "0", "0"]


def test_header_lists_the_new_symbols_under_version_5():
    text = open(os.path.join(ROOT, "include", "flucoma_hip.h")).read()
    comment = text[text.index("/* 5 (round 6)"):text.index("#define FLUHIP_ABI_VERSION 5")]
    for s in SYMBOLS:
        assert s in comment, s
        assert re.search(r"\bint\s+" + s + r"\s*\(", text), s
