"""CPU tests of the novelty restatement (tests/novelty_ref.py): the literal streaming form against the closed batch form,
the reference-held slice positions, the tie guard of every input the GPU tests use for detections, and the measured floor
behind the BufNoveltyFeature bar."""
import json
import os

import numpy as np
import pytest

import novelty_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = json.load(open(os.path.join(ROOT, "tests", "golden", "novelty_reference_cases.json")))["cases"]


@pytest.mark.parametrize("T,D,k,f", [(40, 13, 3, 1), (60, 7, 9, 4), (30, 40, 17, 12), (5, 13, 9, 1), (2, 3, 31, 4),
                                     (90, 5, 65, 12), (1, 4, 3, 1)])
def test_streaming_and_batch_forms_agree(T, D, k, f):
    rng = np.random.default_rng(T * 1000 + k)
    X = rng.standard_normal((T, D))
    if T > 12:
        X[T // 2:T // 2 + 3] = 0.0
    s, d = R.streaming(X, k, f, 0.05, 2)
    b = R.curve_batch(X, k, f)
    assert np.abs(s - b).max() < 1e-13
    assert (d == R.peaks_batch(b, 0.05, 2)).all()


def test_gaussian_sigma_is_an_integer_division():
    # WindowFuncs.hpp:66-73: k = 3 -> 1, 17 -> 5, 31 -> 10
    for k, sigma in ((3, 1), (17, 5), (31, 10)):
        h = (k - 1) // 2
        assert R.gaussian(k)[0] == np.exp(-(h * h) / (2.0 * sigma * sigma))


@pytest.mark.parametrize("case", CASES, ids=[c["signal"] for c in CASES])
def test_reference_held_positions(case):
    x = R.SIGNALS[case["signal"]]()
    args = (case["window"], case["fft"], case["hop"], case["threshold"], case["minSliceLength"], case["kernelSize"],
            case["filterSize"])
    got = R.harness(x, *args)
    assert len(got) == len(case["expected"])
    assert np.abs(np.array(got) - np.array(case["expected"])).max() <= case["margin"]
    # the offline wrapper's framing (Slicing / BufferedProcess / FluidSource) gives the harness's positions
    audio = R.mono_impulses() if case["signal"] == "monoImpulses" else x[None]
    client, curve = R.bufnoveltyslice(audio, 0, case["kernelSize"], case["threshold"], case["filterSize"],
                                      case["minSliceLength"], case["window"], case["fft"], case["hop"], want_curve=True)
    assert list(client) == got
    assert R.outcome_margin(curve, case["threshold"]) > 1e-7
    # ... and the MFCC curve of the same signal keeps clear of ties too (the GPU test compares its positions)
    _, curve1 = R.bufnoveltyslice(audio, 1, case["kernelSize"], case["threshold"], case["filterSize"],
                                  case["minSliceLength"], case["window"], case["fft"], case["hop"], want_curve=True)
    assert R.outcome_margin(curve1, case["threshold"]) > 1e-7


def test_client_level_restatement_on_multichannel_input_with_a_start_offset():
    x = R.sharp_sines()
    stereo = np.stack([0.25 * x, 0.75 * x]).astype(np.float32)
    got = R.bufnoveltyslice(stereo[:, 5000:], 0, 3, 0.38, 1, 4, 512, 1024, 256, start_frame=5000)
    base = R.bufnoveltyslice(stereo[:, 5000:], 0, 3, 0.38, 1, 4, 512, 1024, 256, start_frame=0)
    assert list(got) == [v + 5000 for v in base] and len(got) >= 3
    assert list(R.bufnoveltyslice(np.zeros((2, 9000), dtype=np.float32))) == [-1]
    # a detection inside the latency becomes one detection at the start offset
    assert R.bufnoveltyslice(R.smooth_sine()[None], 0, 3, 0.34, 1, 30, 512, 1024, 256, start_frame=77)[0] == 77


def test_the_gpu_sweeps_inputs_keep_clear_of_ties():
    import test_gpu_novelty as G
    worst = np.inf
    for seed, T, D, k, f in G.SWEEP:
        c = R.curve_batch(G.sweep_features(seed, T, D), k, f)
        worst = min(worst, R.comparison_margins(c, 0.05).min())
    for count, T, D, k, f in [(7, 90, 513, 17, 4), (128, 60, 13, 9, 1), (128, 40, 513, 3, 1), (7, 70, 40, 101, 4)]:
        for b in (0, count - 1):
            c = R.curve_batch(G.sweep_features(100 + b, T, D), k, f)
            worst = min(worst, R.comparison_margins(c, 0.05).min())
    print("smallest comparison margin of the sweep:", worst)
    assert worst > G.TIE_GUARD


def test_the_drum_loop_keeps_clear_of_ties():
    import test_gpu_novelty as G
    x = G.drum_loop()[:88200]
    stereo = np.stack([x, 0.5 * np.roll(x, 3)]).astype(np.float32)
    for algorithm, thr in ((0, 0.1), (1, 0.1)):
        pos, curve = R.bufnoveltyslice(stereo, algorithm, 9, thr, 4, 8, 1024, 1024, 512, start_frame=1234, want_curve=True)
        assert len(pos) > 1 and R.outcome_margin(curve, thr) > G.TIE_GUARD


def test_feature_floor_between_two_double_stfts(oracle):
    """the BufNoveltyFeature bar: the restatement on numpy's FFT against the same on the C oracle's STFT"""
    import test_gpu_novelty as G
    floor = 0.0
    for name, win, fft, hop in G.FEATURE_INPUTS:
        x = (G.drum_loop()[:30000] if name == "drums" else R.SIGNALS[name]()[:30000]).astype(np.float32)
        for algorithm in (0, 1):
            for pm in (0, 1, 2):
                for k, f in ((3, 1), (17, 4)):
                    a = R.bufnoveltyfeature(x, algorithm, k, f, win, fft, hop, padding_mode=pm, as_double=True)
                    b = R.bufnoveltyfeature(x, algorithm, k, f, win, fft, hop, padding_mode=pm, as_double=True, stft=oracle.stft)
                    floor = max(floor, float(np.abs(a - b).max()))
    print(f"feature floor between the two double STFTs: {floor:.3e}; bar 64 x = {64 * floor:.3e}")
    assert floor <= G.FEATURE_FLOOR and G.FEATURE_BAR == 64 * G.FEATURE_FLOOR


def test_build_lists_the_novelty_sources():
    import importlib.util
    spec = importlib.util.spec_from_file_location("fluhip_build_n", os.path.join(ROOT, "flucoma-core_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "kernels_novelty.hip" in mod.SOURCES and "api_novelty.hip" in mod.SOURCES


# ---- the C++ clients' host side (include/flucoma_hip/NoveltySliceClient.hpp, tests/cpp/novelty_driver.cpp) ---------------
@pytest.fixture(scope="module")
def novelty_driver(fluhip_lib_path):
    return R.build_driver()


_drive = R.drive


def test_cpp_client_descriptors_are_the_references_tables(novelty_driver):
    mine = json.loads(_drive(novelty_driver, "descriptors"))
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "param_descriptors_novelty.json")))
    assert mine == want
    assert [d["name"] for d in mine["BufNoveltySlice"]][5:] == ["indices", "algorithm", "kernelSize", "threshold", "filterSize",
                                                               "minSliceLength", "fftSettings"]
    assert [d["name"] for d in mine["BufNoveltyFeature"]][5:] == ["features", "padding", "algorithm", "kernelSize", "filterSize",
                                                                 "fftSettings"]
    if os.path.isdir("/root/reference/include/flucoma"):
        import subprocess
        import sys
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_param_descriptor_fixture.py"), "--novelty"],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and json.loads(r.stdout) == want


def test_cpp_client_error_paths(novelty_driver):
    got = [l.split("|") for l in _drive(novelty_driver, "errors").splitlines()]
    assert got == [["slice_no_source", "2", "Input buffer not set"], ["slice_no_output", "2", "No valid output has been set"],
                   ["slice_start_past_end", "2", "Input buffer  invalid start frame 5000"],
                   ["feature_no_source", "2", "Input buffer not set"], ["feature_no_output", "2", "No valid output has been set"]]


@pytest.mark.parametrize("args,want", [
    ((7, 4, -1, 0, -3, 1000, -1, -1), "4 5 0 1 0 1000 500 1024"),    # Odd(): 4 -> 5; Min() on the rest
    ((1, 1, 0.25, 3, 10, 512, 256, 1024), "1 3 0.25 3 10 512 256 1024"),
])
def test_cpp_client_constraints(novelty_driver, args, want):
    assert _drive(novelty_driver, "constrain", *args).strip() == want


def test_the_novelty_entry_points_take_no_event_and_no_stream():
    """A tripwire, not a measurement: every event or stream the library hands out comes from take_event / the context's
    create calls, and the text of the novelty layer names none of them (its device memory is DevBuf objects of the call).
    It would not see an event taken through a helper defined elsewhere and it would trip on a rename; what is measured
    is the free device memory over 200 calls, tests/test_gpu_novelty.py."""
    import re
    for f in ("api_novelty.hip", "kernels_novelty.hip", "fluhip_novelty.h"):
        text = open(os.path.join(ROOT, "flucoma-core_amd", "csrc", f)).read()
        text = re.sub(r"//[^\n]*", "", text)
        assert not re.search(r"take_event|hipEventCreate|hipStreamCreate|hipEventRecord|eventPool|hipMalloc\b|hipFree\b", text), f
