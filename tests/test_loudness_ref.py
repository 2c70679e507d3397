"""CPU tests of tests/loudness_ref.py, the literal model of the reference's BufLoudness: hand-computed cases, every kept
behaviour against its tidied variant (which must give another answer), the filter against scipy and the BS.1770 table, the
floors between the double and the long double model that set the GPU tests' bars (tests/test_gpu_loudness.py), the
frame-parallel decomposition the device runs restated in numpy, and the C++ client without a device."""
import json
import os

import numpy as np
import pytest

import loudness_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# The largest difference in dB between the literal model in double and in long double (the same double coefficients and
# samples) over every frame of the three buffers of each case of L.CASES: (loudness with kWeighting on, peak with truePeak on,
# loudness with kWeighting off, peak with truePeak off).  Each constant is the measured figure rounded UP to two digits, and
# never below one ulp of the largest |dB| of its column: a double result cannot be told apart more finely, and with truePeak
# off the two models see the same max |x| and can differ by nothing but log10's last bit.  test_the_floors asserts
# measured <= constant; the CPU restatement of the decomposition stays within 8 x, the GPU bars are 64 x.
FLOORS = {
    "noise_1024_512": (7.1e-12, 3.4e-15, 3.3e-15, 1.0e-15),        # measured 7.009e-12 3.303e-15 3.245e-15 9.975e-16
    "noise_256_64": (2.1e-11, 3.0e-15, 2.9e-15, 9.9e-16),          # measured 2.097e-11 2.957e-15 2.816e-15 9.810e-16
    "sine_dc_1024_512": (4.2e-11, 3.7e-15, 1.5e-15, 6.2e-17),      # measured 4.150e-11 3.649e-15 1.491e-15 6.109e-17
    "sine_dc_256_64": (2.5e-10, 2.2e-15, 1.5e-15, 6.2e-17),        # measured 2.406e-10 2.131e-15 1.471e-15 6.112e-17
    "noise32_1024_512": (7.4e-12, 4.1e-15, 3.3e-15, 1.0e-15),      # measured 7.376e-12 4.016e-15 3.253e-15 9.901e-16
    "noise32_256_64": (2.5e-11, 3.7e-15, 3.1e-15, 9.9e-16),        # measured 2.407e-11 3.695e-15 3.043e-15 9.879e-16
    "noise_2048_300": (6.6e-12, 3.0e-15, 3.2e-15, 8.9e-16),        # measured 6.502e-12 2.957e-15 3.121e-15 7.373e-16
    "noise_5_2": (4.8e-10, 7.2e-15, 3.6e-15, 3.6e-15),             # measured 4.791e-10 4.351e-15 3.176e-15 1.808e-15
    "noise_1_1": (4.9e-07, 2.3e-14, 1.5e-14, 1.5e-14),             # measured 4.841e-07 2.219e-14 6.918e-15 9.534e-15
    "noise_3_7": (7.4e-10, 1.5e-14, 3.6e-15, 3.6e-15),             # measured 7.300e-10 3.845e-15 3.521e-15 2.564e-15
    "noise_32768_8192": (3.4e-13, 2.0e-15, 2.1e-15, 8.9e-16),      # measured 3.344e-13 1.907e-15 2.076e-15 3.760e-16
    "noise_96k": (5.1e-10, 3.3e-15, 2.9e-15, 9.9e-16),             # measured 5.041e-10 3.204e-15 2.816e-15 9.810e-16
    "noise_192k": (8.2e-09, 9.9e-16, 2.9e-15, 9.9e-16),            # measured 8.197e-09 9.810e-16 2.816e-15 9.810e-16
    "noise_8k": (2.6e-14, 3.0e-15, 2.9e-15, 9.9e-16),              # measured 2.558e-14 2.957e-15 2.816e-15 9.810e-16
    "sine_dc_2048_300": (1.9e-11, 2.9e-15, 1.3e-15, 5.6e-17),      # measured 1.863e-11 2.861e-15 1.220e-15 4.803e-17
    "sine_dc_5_2": (3.6e-09, 3.8e-15, 1.6e-15, 9.8e-16),           # measured 3.599e-09 3.754e-15 1.504e-15 9.775e-16
    "sine_dc_1_1": (4.6e-06, 7.2e-15, 1.4e-15, 9.9e-16),           # measured 4.504e-06 3.747e-15 1.306e-15 9.853e-16
    "sine_dc_3_7": (4.7e-09, 7.2e-15, 1.6e-15, 9.9e-16),           # measured 4.619e-09 3.247e-15 1.507e-15 9.853e-16
    "sine_dc_32768_8192": (3.0e-12, 2.6e-15, 9.8e-16, 5.6e-17),    # measured 2.905e-12 2.546e-15 9.725e-16 4.556e-17
    "sine_dc_96k": (1.0e-08, 3.6e-15, 1.4e-15, 5.6e-17),           # measured 9.968e-09 3.545e-15 1.340e-15 5.104e-17
    "sine_dc_192k": (2.7e-07, 4.5e-16, 1.3e-15, 4.5e-16),          # measured 2.670e-07 2.121e-16 1.288e-15 2.121e-16
    "sine_dc_8k": (8.1e-14, 3.3e-15, 1.4e-15, 5.7e-17),            # measured 8.018e-14 3.275e-15 1.374e-15 5.651e-17
}


def floor_of(name, column, switch):
    """the stored floor of a case: column 0 loudness / 1 peak, switch = kWeighting resp. truePeak"""
    return FLOORS[name][column + (0 if switch else 2)]


def measured_floors(name):
    row = []
    for sw in (True, False):
        d = L.case_model(name, sw, sw)
        ld = L.case_model(name, sw, sw, np.longdouble)
        diff = np.abs(d - ld).max(axis=(0, 1)).astype(np.float64)
        ulp = np.spacing(np.abs(d).max(axis=(0, 1)))
        row += [float(diff[0]), float(diff[1]), float(ulp[0]), float(ulp[1])]
    return row


# ---- hand-computed cases ---------------------------------------------------------------------------------------------------
def test_the_coefficients_are_the_bs1770_table_at_48_khz():
    # ITU-R BS.1770-4, annex 1, tables 1 and 2 (48 kHz), as printed: 14 digits
    shelf_b = [1.53512485958697, -2.69169618940638, 1.19839281085285]
    shelf_a = [1.0, -1.69065929318241, 0.73248077421585]
    hp_b = [1.0, -2.0, 1.0]
    hp_a = [1.0, -1.99004745483398, 0.99007225036621]
    b, a = L.kweighting_coefficients(48000.0)
    want_b, want_a = np.convolve(shelf_b, hp_b), np.convolve(shelf_a, hp_a)
    # the reference computes the biquads from (f0, G, Q) as libebur128 does, and those constants were fitted to the table: the
    # multiplied-out coefficients agree with the table's 14 printed digits
    eb, ea = np.abs(np.array(b) - want_b).max(), np.abs(np.array(a) - want_a).max()
    print("b", eb, "a", ea)
    assert eb < 2e-14       # measured 1.8e-15: half a unit of the 14th printed digit of 2.69 is 5e-15, doubled by the high-pass
    assert ea < 2e-14       # measured 4.4e-16
    assert len(b) == 5 and len(a) == 5 and a[0] == 1.0


def test_the_filter_is_scipy_lfilter_with_carried_state():
    signal = pytest.importorskip("scipy.signal")
    b, a = L.kweighting_coefficients(44100.0)
    x = L.material("noise", 3000)
    # two frames, the state carried: lfilter's zi is the transposed direct form II state, so it is carried as lfilter
    # returns it; the model carries mX / mY
    y_ref, zi = signal.lfilter(b, a, x[:1700], zi=np.zeros(4))
    y_ref2, _ = signal.lfilter(b, a, x[1700:], zi=zi)
    y1, st = L.filter_run(x[:1700].tolist(), L.zero_state(), b, a)
    y2, _ = L.filter_run(x[1700:].tolist(), st, b, a)
    err = np.abs(np.array(y1 + y2) - np.concatenate([y_ref, y_ref2])).max()
    print("model vs lfilter:", err)
    # two double realisations (direct form I vs transposed direct form II) of a filter whose high-pass poles sit at
    # 1 - 2.7e-3: rounding noise of 1e-16 is amplified by ~ 1 / (1 - |p|)^2 ~ 1e5; measured 2.2e-11 on +-0.5 noise
    assert err < 1e-10
    # ... and restarting the second frame from zero state is another filter
    y2r, _ = L.filter_run(x[1700:].tolist(), L.zero_state(), b, a)
    assert np.abs(np.array(y2r) - y_ref2).max() > 1e-3


def test_a_full_scale_square_wave_s_frame():
    # kWeighting off, truePeak off: mean square 1 -> -0.691 dB, peak 0 dB; epsilon adds 10 log10(1 + eps) = 9.6e-16 resp.
    # 20 log10(1 + eps) = 1.9e-15
    x = np.tile([1.0, -1.0], 512)
    out = L.loudness_frames(x, 1024, 512, k_weighting=False, true_peak=False)
    assert out.shape == (1, 2)
    assert abs(out[0, 0] - L.OFFSET) < 2e-15 and abs(out[0, 1]) < 3e-15


def test_digital_silence():
    out = L.loudness_frames(np.zeros(4096), 1024, 512)
    assert np.all(out[:, 0] == L.OFFSET + 10 * np.log10(L.EPSILON))
    assert np.all(out[:, 1] == 20 * np.log10(L.EPSILON))


def test_the_interpolator_s_taps():
    for factor, ring in ((4, 13), (2, 25)):
        assert L.ring_size(factor) == ring
        ph = L.interpolator_filters(factor)
        flat = [(d * factor + f, c) for f, taps in enumerate(ph) for d, c in taps]
        # taps 0 and 48 are the Hann window's zeros, and every factor-th tap from the centre is a zero of the sinc: dropped
        kept = sorted(i for i, _ in flat)
        assert 0 not in kept and 48 not in kept and 24 in kept
        assert all((i - 24) % factor != 0 or i == 24 for i in kept)
        assert max(d for taps in ph for d, _ in taps) <= ring - 1
        assert dict(flat)[24] == 1.0
    assert [L.interpolation_factor(sr) for sr in (8000, 44100, 88199, 88200, 96000, 176399, 176400, 192000)] == [4, 4, 4, 2, 2, 2, 1, 1]


def test_true_peak_sees_between_the_samples():
    # a sine at fs / 4 sampled 45 degrees off its crests: every sample is 0.7071, the waveform peaks at 1
    n = np.arange(1024)
    x = np.sin(2 * np.pi * n / 4 + np.pi / 4)
    out = L.loudness_frames(x, 1024, 512, k_weighting=False, true_peak=True)
    plain = L.loudness_frames(x, 1024, 512, k_weighting=False, true_peak=False)
    assert abs(plain[0, 1] - 20 * np.log10(np.sqrt(0.5))) < 1e-9
    assert abs(out[0, 1]) < 0.2                          # (0.10 dB over: the ripple of a 49-tap windowed sinc at fs / 4)
    # at 176400 Hz and above the interpolator is not run
    hi = L.loudness_frames(x, 1024, 512, k_weighting=False, true_peak=True, sr=176400.0)
    assert np.array_equal(hi[:, 1], plain[:, 1])


# ---- kept behaviours: the tidied variant must differ -----------------------------------------------------------------------
TIDY_MATERIAL = [("noise", 256, 64), ("sine_dc", 256, 64), ("noise", 5, 2)]


def differs(a, b, col, tol=1e-6):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a[..., col] - b[..., col]).max() > tol


@pytest.mark.parametrize("kind,win,hop", TIDY_MATERIAL)
def test_kept_1_the_filter_is_never_reset(kind, win, hop):
    x = L.material(kind, 20 * hop + win)
    kept = L.loudness_frames(x, win, hop)
    tidy = L.loudness_frames(x, win, hop, variant="filter_reset")
    assert np.array_equal(kept[0], tidy[0])            # (frame 0 starts from zero state either way)
    assert differs(kept[1:], tidy[1:], 0, 1e-3)
    assert np.array_equal(kept[:, 1], tidy[:, 1])


@pytest.mark.parametrize("kind,win,hop", TIDY_MATERIAL)
def test_kept_2_the_peak_is_the_unfiltered_frame_s(kind, win, hop):
    x = L.material(kind, 20 * hop + win)
    for tp in (True, False):
        kept = L.loudness_frames(x, win, hop, true_peak=tp)
        tidy = L.loudness_frames(x, win, hop, true_peak=tp, variant="peak_filtered")
        assert differs(kept, tidy, 1, 1e-2)
        assert np.array_equal(kept[:, 0], tidy[:, 0])


@pytest.mark.parametrize("kind,win,hop", TIDY_MATERIAL)
def test_kept_3_the_latency_frames_move_both_states(kind, win, hop):
    x = L.material(kind, 20 * hop + win)
    for padding in (0, 1, 2):
        kept = L.bufloudness(x, win, hop, padding, as_double=True)
        tidy = L.bufloudness(x, win, hop, padding, variant="latency_skipped", as_double=True)
        assert kept.shape == tidy.shape
        # dropped frame j ends at sample j hop - padding of the input: with padding 0 every one behind the first holds input
        pad, _, drop = L.control_geometry(len(x), win, hop, padding)
        if (drop - 1) * hop > pad:
            assert differs(kept.T, tidy.T, 0, 1e-6)
            # (the interpolator's history is 12 samples: it moves a frame's peak where the window is no longer than that)
            assert differs(kept.T, tidy.T, 1, 1e-6) == (win < 13)
        else:
            assert np.array_equal(kept, tidy)               # (nothing but zeros went through: both states are still zero)
        assert padding != 0 or (drop - 1) * hop > pad


@pytest.mark.parametrize("kind,win,hop", TIDY_MATERIAL)
def test_kept_4_the_ring_buffer_outlives_the_frame(kind, win, hop):
    x = L.material(kind, 20 * hop + win)
    kept = L.loudness_frames(x, win, hop)
    tidy = L.loudness_frames(x, win, hop, variant="history_zeroed")
    assert np.array_equal(kept[0], tidy[0])
    assert differs(kept[1:], tidy[1:], 1, 1e-4)
    assert np.array_equal(kept[:, 0], tidy[:, 0])


def test_kept_4b_a_short_window_s_ring_holds_several_frames():
    # win 1 at factor 4: twelve frames back are still in the ring
    x = np.zeros(40)
    x[3] = 1.0
    out = L.loudness_frames(x, 1, 1, k_weighting=False)
    audible = np.nonzero(out[:, 1] > 20 * np.log10(1e-5))[0]
    assert audible.min() == 3 and audible.max() >= 3 + 10


@pytest.mark.parametrize("kind,win,hop", TIDY_MATERIAL)
def test_kept_5_the_offset_stays_without_weighting(kind, win, hop):
    x = L.material(kind, 20 * hop + win)
    kept = L.loudness_frames(x, win, hop, k_weighting=False)
    tidy = L.loudness_frames(x, win, hop, k_weighting=False, variant="no_offset")
    assert np.abs((tidy[:, 0] - kept[:, 0]) - 0.691).max() < 1e-12


def test_hop_above_window_and_the_paddings():
    x = L.material("noise", 100)
    for padding, want in ((0, (100 + 3 - 3) // 7 + 1), (1, (100 + 3 + 2 - 3) // 7 + 1)):
        out = L.bufloudness(x, 3, 7, padding)
        pad, T, drop = L.control_geometry(100, 3, 7, padding)
        assert drop == 0 and out.shape == (2, T) and out.dtype == np.float32 and T == want
    # Full mode with hop > win: win - hop is negative and the reference copies its input to a negative offset; refused here
    assert L.user_padding(3, 7, 2) == -4
    with pytest.raises(ValueError):
        L.bufloudness(x, 3, 7, 2)
    assert L.bufloudness(x, 7, 3, 2).shape == (2, 1 + (-(-(100 + 7 + 8) // 3) * 3 - 7) // 3 - 2)
    assert L.bufloudness(x, 1024, 512, 1, select=2).shape[0] == 1
    a, b = L.bufloudness(x, 16, 4, 1, select=3), L.bufloudness(x, 16, 4, 1, select=2)
    assert np.array_equal(a[1], b[0])


# ---- the floors ------------------------------------------------------------------------------------------------------------
def test_the_floors():
    assert set(FLOORS) == set(L.CASES)
    bad = []
    for name in L.CASES:
        m = measured_floors(name)
        print(f'    "{name}": ' + " ".join(f"{v:.3e}" for v in m[:2] + m[4:6]) + "   ulps " + " ".join(f"{v:.3e}" for v in m[2:4] + m[6:]))
        want = FLOORS[name]
        for got, ulp, const in zip(m[:2] + m[4:6], m[2:4] + m[6:], want):
            if not (got <= const and ulp <= const * 1.0000001):
                bad.append((name, got, ulp, const))
    assert not bad, bad


# ---- the decomposition the device runs ---------------------------------------------------------------------------------------
def test_the_frame_transition_is_the_filter_s_own_response():
    # M s is the state behind a frame of zeros entered with state s
    b, a = L.kweighting_coefficients(44100.0)
    M = np.array(L.frame_transition(37, 44100.0), dtype=np.float64)
    rng = np.random.default_rng(5)
    s = rng.uniform(-1, 1, 8)
    _, end = L.filter_run([0.0] * 37, s.tolist(), b, a)
    assert np.abs(np.array(end) - M @ s).max() < 1e-9
    assert np.all(M[:4] == 0)                              # (a window of four samples or more forgets the input history)
    M256 = np.array(L.frame_transition(256, 44100.0), dtype=np.float64)
    assert np.abs(M256).max() > 1e3                        # the conditioning K14 speaks of: entries in the thousands ...
    assert M256[4:, 4:].min() < -1e3                       # ... with alternating signs


def decomposition_error(name, precision):
    _, win, hop, _, sr = L.CASES[name]
    ref = L.case_model(name, True, True)
    return max(float(np.abs(L.decomposed_loudness(x, win, hop, sr, precision) - want[:, 0]).max())
               for x, want in zip(L.case_signals(name), ref))


@pytest.mark.parametrize("name", list(L.CASES))
def test_the_decomposition_stays_within_8_floors(name):
    worst = decomposition_error(name, "dd")
    print(f"{name}: decomposition {worst:.3e} dB, floor {floor_of(name, 0, True):.1e}")
    assert worst <= 8 * floor_of(name, 0, True)


@pytest.mark.parametrize("name", ["noise_256_64", "sine_dc_256_64"])
def test_the_decomposition_with_m_rounded_to_double_does_not(name):
    worst = decomposition_error(name, "double_m")
    print(f"{name}: decomposition with M rounded to double {worst:.3e} dB, floor {floor_of(name, 0, True):.1e}")
    assert worst > 8 * floor_of(name, 0, True)              # measured 109 x (noise), 139 x (sine on DC)


@pytest.mark.parametrize("name", ["noise_256_64", "sine_dc_256_64", "sine_dc_192k"])
def test_the_scan_itself_holds_in_long_double_once_m_is_exact(name):
    # M's entries reach 5.5e3 at (256, 44100 Hz), 5.3e4 at 96 kHz and 2.8e5 at 192 kHz (the poles move towards z = 1 with the
    # sample rate).  Built by 256 successive long double steps, M missed 8 floors from 96 kHz on (63 floors at 192 kHz);
    # built in 32 digits and THEN rounded to long double it holds, the scan in long double too (3.4 floors at 192 kHz).
    # The device carries both as double-doubles
    worst = decomposition_error(name, "longdouble")
    print(f"{name}: decomposition, M and scan rounded to long double {worst:.3e} dB, floor {floor_of(name, 0, True):.1e}")
    assert worst <= 8 * floor_of(name, 0, True)


# ---- the C++ host client through tests/cpp/loudness_driver.cpp, without a device -----------------------------------------
@pytest.fixture(scope="module")
def loudness_driver(fluhip_lib_path):
    return L.build_driver()


def test_cpp_client_descriptors_are_the_reference_s_table(loudness_driver):
    mine = json.loads(L.drive(loudness_driver, "descriptors"))
    want = json.load(open(os.path.join(GOLDEN, "param_descriptors_loudness.json")))
    assert mine == want
    wrapper = ["source", "startFrame", "numFrames", "startChan", "numChans", "features", "padding"]
    assert [d["name"] for d in mine["BufLoudness"]] == wrapper + ["select", "kWeighting", "truePeak", "windowSize", "hopSize",
                                                                 "maxWindowSize"]
    sel = [d for d in mine["BufLoudness"] if d["name"] == "select"][0]
    assert (sel["kind"], sel["default"], sel["strings"]) == ("Choices", 3, ["loudness", "peak"])
    mw = mine["BufLoudness"][-1]
    assert (mw["default"], mw["min"], mw["max"], mw["relational"], mw["fixed"]) == (16384, 4, 32768, "PowerOfTwo", True)


def test_the_fixture_is_what_the_tool_mints_from_the_reference():
    ref = "/root/reference"
    if not os.path.isdir(ref):
        return   # the fixture is data; the reference's text is not everywhere
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_param_descriptor_fixture.py"), "--loudness", ref],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == json.load(open(os.path.join(GOLDEN, "param_descriptors_loudness.json")))


def test_cpp_client_defaults(loudness_driver):
    # both outputs, both switches on, 1024 / 512, maxWindowSize 16384, padding Default
    assert L.drive(loudness_driver, "defaults").strip() == "3 1 1 1024 512 16384 1"


def test_cpp_client_error_paths(loudness_driver):
    got = [l.split("|") for l in L.drive(loudness_driver, "errors").splitlines()]
    assert got == [["no_source", "2", "Input buffer not set"], ["no_output", "2", "No valid output has been set"],
                   ["start_past_end", "2", "Input buffer  invalid start frame 5000"],
                   ["chan_past_end", "2", "Input buffer  invalid start channel 3"],
                   ["hop_zero", "2", "hopSize must be at least 1"],
                   ["window_zero", "2", "windowSize must be in [1, maxWindowSize]"],
                   ["window_above_max", "2", "windowSize must be in [1, maxWindowSize]"],
                   ["max_window_not_a_power_of_two", "2", "maxWindowSize must be a power of two from 4 to 32768"],
                   ["max_window_too_large", "2", "maxWindowSize must be a power of two from 4 to 32768"]]


@pytest.mark.parametrize("args,want", [
    ((7, 5, -1, 0, 0, 16384), "3 1 0 1 1 16384"),               # select bits, enums, Min(1), Min(1)
    ((1, 0, 1, 40000, 3, 3000), "1 0 1 4096 3 4096"),           # PowerOfTwo rounds up; UpperLimit<maxWindowSize>
    ((2, 1, 1, 5, 9, 2), "2 1 1 4 9 4"),                        # Min(4); hop > win is legal
    ((3, 1, 1, 32768, 8192, 100000), "3 1 1 32768 8192 32768"),  # Max(32768)
])
def test_cpp_client_constraints(loudness_driver, args, want):
    assert L.drive(loudness_driver, "constrain", *args).strip() == want
