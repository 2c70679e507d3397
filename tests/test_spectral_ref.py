"""CPU tests of tests/spectral_ref.py, the numpy restatement of the reference's SpectralShape and ChromaFilterBank: hand-computed
cases, every kept behaviour against its tidied variant (which must give another answer), and the floors between two double
STFTs that set the GPU tests' bars (tests/test_gpu_spectral.py)."""
import json
import os

import numpy as np
import pytest

import pitch_ref as R
import spectral_ref as S
from test_pitch_ref import shape_mags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
UNIT_POWER = [(0, 0), (1, 0), (0, 1), (1, 1)]
NORMALIZE = (0, 1, 2)

# The largest difference between the restatement on numpy's FFT and on the project's C oracle STFT over every shape of
# R.SHAPES on R.material(shape) under the client's framing, every frame.  SpectralShape: per descriptor, |a - b| /
# max(1, |b|), the largest over unit 0 / 1 and power 0 / 1.  Chroma: per normalize mode, |a - b| relative to the frame's
# peak, numChroma 12, ref 440.  Each constant is the measured figure (beside it) rounded UP to two digits;
# test_floors_between_two_double_stfts asserts measured <= constant, and the GPU bars are 64 x the constants.
SHAPE_FLOOR = {"centroid": 2.4e-15,    # measured 2.321e-15
               "spread": 1.1e-14,      # measured 1.062e-14
               "skew": 2.1e-14,        # measured 2.076e-14
               "kurtosis": 3.6e-14,    # measured 3.542e-14
               "rolloff": 4.7e-13,     # measured 4.647e-13
               "flatness": 1.5e-14,    # measured 1.469e-14
               "crest": 4.5e-16}       # measured 4.426e-16
CHROMA_FLOOR = {0: 7.4e-16,            # measured 7.348e-16
                1: 5.1e-16,            # measured 5.041e-16
                2: 5.6e-16}            # measured 5.551e-16
# the filter table has no STFT in front of it: its floor is the restatement in double against the restatement in long
# double, the largest over the tables the GPU tests read (the conditioning of nChroma log2(f / (ref / 16)), up to ~ 300, times
# the rounding of a double)
FILTER_FLOOR = 1.1e-13                 # measured 1.032e-13
FILTER_CASES = [(12, 129, 440.0, 44100.0), (7, 257, 440.0, 44100.0), (24, 513, 440.0, 44100.0), (12, 2049, 22000.0, 44100.0),
                (12, 2049, 22000.0, 8000.0), (12, 3, 440.0, 44100.0), (12, 5, 440.0, 44100.0)]


def mags1024():
    return shape_mags((1024, 1024, 512))[0]


# ---- hand-computed cases ---------------------------------------------------------------------------------------------
def test_a_flat_spectrum():
    # amp = 1 on the bins 0 .. 511 (bin 512 is never read): flatness and crest are 0 dB, the centroid is the mean of the
    # axis, which LinSpaced stretches to end at 512 binHz = sr / 2: its mean is sr / 4
    d = S.spectral_shape(np.ones(513))
    assert d[5] == 0 and d[6] == 0
    assert abs(d[0] - 11025.0) < 1e-9
    ax = S.shape_axis(0, 512, 44100 / 1024)
    assert abs(d[0] - ax.mean()) < 1e-9
    assert abs(d[1] - np.sqrt(((ax - ax.mean()) ** 2).mean())) < 1e-9
    assert abs(d[2]) < 1e-12                               # symmetric
    assert abs(d[3] - 1.8) < 1e-4                          # a uniform distribution's kurtosis, 9/5 (1 - O(1 / n^2))
    # 95 % of 512 equal bins: the running sum reaches 486.4 inside bin 486, 0.4 of the way from axis[485] to axis[486]
    assert abs(d[4] - (ax[486] - (ax[486] - ax[485]) * 0.6)) < 1e-8


def test_a_single_hot_bin():
    mag = np.zeros(513)
    mag[100] = 1.0
    d = S.spectral_shape(mag)
    ax = S.shape_axis(0, 512, 44100 / 1024)
    # everything else is epsilon: the centroid is the hot bin's frequency to 512 epsilon, the rolloff lies inside that bin
    assert abs(d[0] - ax[100]) < 1e-7
    assert ax[99] < d[4] <= ax[100]
    assert abs(d[6] - 20 * np.log10(512.0)) < 1e-9         # crest: max / mean = 512 / (1 + 511 eps)
    assert d[5] < -250                                     # flatness: exp(mean(log)) ~ eps^(511 / 512)
    assert d[2] > 0 or d[2] < 0                            # (finite)


@pytest.mark.parametrize("n_bins", (3, 5))
def test_the_smallest_transforms(n_bins):
    # fft 4: bins 0, 1 at 0 and 2 binHz (the axis of two bins ends at maxBin binHz); fft 8: four bins at 0, 4/3, 8/3, 4 binHz
    sr = 44100.0
    bin_hz = sr / (2 * (n_bins - 1))
    mag = np.arange(1, n_bins + 1, dtype=np.float64)
    d = S.spectral_shape(mag, sr=sr)
    size = n_bins - 1
    ax = np.linspace(0, size * bin_hz, size)
    amp = mag[:size]
    c = (amp * ax).sum() / amp.sum()
    assert abs(d[0] - c) < 1e-9
    assert abs(d[1] - np.sqrt((amp * (ax - c) ** 2).sum() / amp.sum())) < 1e-9
    assert abs(d[6] - 20 * np.log10(amp.max() / amp.mean())) < 1e-12
    # the MIDI axis at fft 4 leaves one bin (1, with 0 folded in): it sits at maxBin binHz, spread 0, skewness 0 / 0
    m = S.spectral_shape(mag, unit=1, sr=sr)
    if n_bins == 3:
        assert abs(m[0] - (69 + 12 * np.log2(2 * bin_hz / 440))) < 1e-9 and m[1] == 0 and np.isnan(m[2]) and np.isnan(m[3])
        assert m[4] == m[0] and abs(m[5]) < 1e-12 and abs(m[6]) < 1e-12
    # ... and with maxBin 1 nothing is left: seven zeros (defined; the reference reads an empty array)
    assert np.all(S.spectral_shape(mag, max_freq=1.5 * bin_hz, unit=1, sr=sr) == 0)


def test_an_empty_range_gives_seven_zeros():
    m = mags1024()[3]
    assert np.all(S.spectral_shape(m, min_freq=5000.0, max_freq=5000.0) == 0)      # maxBin 116 <= minBin 117
    assert np.all(S.spectral_shape(m, min_freq=6000.0, max_freq=5000.0) == 0)
    assert np.all(S.spectral_shape(m, min_freq=30000.0) == 0)                       # beyond Nyquist
    assert np.any(S.spectral_shape(m, min_freq=5000.0, max_freq=5100.0) != 0)       # bins 117, 118: one bin is read
    assert S.shape_bins(513, 0.0, 1e300, 44100.0)[:2] == (0, 512)
    assert S.shape_bins(513, 1e300, -1.0, 44100.0)[:2] == (513, 512)


def test_filter_columns_have_unit_norm():
    for nc, n_bins in ((12, 513), (7, 257), (24, 2049), (2, 3), (128, 5)):
        w, scale = S.chroma_filters(nc, n_bins)
        assert w.shape == (nc, n_bins)
        assert np.abs(np.sqrt((w * w).sum(axis=0)) - 1).max() < 1e-14
        assert scale == 2.0 / (2 * (n_bins - 1) * nc)


def test_chroma_of_a_440_hz_tone_peaks_at_a():
    # class 0 is ref / 16 = 27.5 Hz and its octaves: A
    c = S.bufchroma(R.tone(6000, 440.0), as_double=True)
    assert np.all(c[:, 2:-2].argmax(axis=0) == 0)
    # ... and with ref = 440 2^(3 / 12) (a C), A is class 9
    c = S.bufchroma(R.tone(6000, 440.0), ref=440.0 * 2 ** 0.25, as_double=True)
    assert np.all(c[:, 2:-2].argmax(axis=0) == 9)
    for normalize, red in ((1, np.sum), (2, np.max)):
        n = S.bufchroma(R.tone(6000, 440.0), normalize=normalize, as_double=True)
        assert np.abs(red(n, axis=0) - 1).max() < 1e-12


def test_chroma_leaves_its_input_alone():
    m = mags1024().copy()
    keep = m.copy()
    S.chroma_frames(m, min_freq=100.0, max_freq=5000.0)
    assert np.array_equal(m, keep)


# ---- kept behaviours: the tidied variant must differ -------------------------------------------------------------------
def differs(a, b, cols=range(7)):
    a, b = np.asarray(a), np.asarray(b)
    return all(not np.allclose(a[..., c], b[..., c], rtol=1e-9, atol=0) for c in cols)


def test_shape_1_the_clamp_comes_first():
    # with unit 1 and minBin 0 the clamped bin 0 is folded into bin 1: clamping afterwards adds a raw 0 instead of epsilon
    mag = np.zeros(513)
    mag[1] = 1e-16
    kept = S.spectral_shape(mag, unit=1)
    tidy = S.spectral_shape(mag, unit=1, clamp_first=False)
    assert kept[6] != tidy[6] and abs(kept[6] - tidy[6]) > 1e-3


def test_shape_2_bins_and_max_freq():
    assert S.shape_bins(513, 100.0, 1000.0, 44100.0)[:2] == (3, 23)        # ceil(2.32), floor(23.2)
    assert S.shape_bins(513, 0.0, -1.0, 44100.0)[:2] == (0, 512)
    assert S.shape_bins(513, 0.0, 30000.0, 44100.0)[:2] == (0, 512)        # capped at sr / 2
    assert S.shape_bins(513, 0.0, -1.0, 44100.0)[2] == 44100.0 / 1024


def test_shape_3_the_midi_axis_folds_bin_0_into_bin_1():
    m = mags1024()[3].copy()
    m[0] = 10 * m.max()
    kept = S.spectral_shape(m, unit=1)
    tidy = S.spectral_shape(m, unit=1, fold_dc=False)
    assert differs(kept, tidy)
    assert np.array_equal(S.spectral_shape(m, min_freq=50.0, unit=1), S.spectral_shape(m, min_freq=50.0, unit=1, fold_dc=False))


def test_shape_4_bin_maxbin_is_never_read_and_the_axis_is_stretched():
    m = mags1024()[3].copy()
    kept = S.spectral_shape(m)
    assert differs(kept, S.spectral_shape(m, axis_step_is_bin=True), cols=(0, 1, 4))
    m2 = m.copy()
    m2[512] = 100 * m.max()
    assert np.array_equal(S.spectral_shape(m2), kept)
    assert differs(S.spectral_shape(m2, include_max_bin=True), kept)
    ax = S.shape_axis(3, 23, 44100 / 1024)
    assert len(ax) == 20 and ax[0] == 3 * 44100 / 1024 and ax[-1] == 23 * 44100 / 1024
    assert abs((ax[1] - ax[0]) - 20 * (44100 / 1024) / 19) < 1e-12
    assert list(S.shape_axis(7, 8, 10.0)) == [80.0]                        # size 1 yields the high end


def test_shape_5_the_midi_axis():
    ax = S.shape_axis(1, 512, 44100 / 1024, unit=1)
    hz = S.shape_axis(1, 512, 44100 / 1024)
    assert np.allclose(ax, 69 + 12 * np.log2(hz / 440), rtol=0, atol=1e-11)
    assert differs(S.spectral_shape(mags1024()[3], unit=1), S.spectral_shape(mags1024()[3], unit=0), cols=(0, 1, 2, 3, 4))


def test_shape_6_central_moments_and_the_unrooted_spread():
    m = mags1024()[3]
    kept = S.spectral_shape(m)
    raw = S.spectral_shape(m, raw_moments=True)
    # expanded raw moments agree to rounding only -- and not to the last place: the cancellation costs digits
    assert np.allclose(kept[:4], raw[:4], rtol=1e-6) and not np.array_equal(kept[1:4], raw[1:4])
    rooted = S.spectral_shape(m, rooted_spread=True)
    assert differs(kept, rooted, cols=(2, 3))
    spread = kept[1] ** 2
    assert abs(rooted[2] / kept[2] - spread ** 0.75) < 1e-6 * spread ** 0.75


def test_shape_7_the_rolloff():
    m = mags1024()[3]
    kept = S.spectral_shape(m, rolloff_percent=50.0)
    assert differs(kept, S.spectral_shape(m, rolloff_percent=50.0, rolloff_interpolates=False), cols=(4,))
    ax = S.shape_axis(0, 512, 44100 / 1024)
    assert S.spectral_shape(m, rolloff_percent=0.0)[4] == ax[0]            # i == 0: freqs[0]
    # a frame whose running sum never crosses (NaN fails every comparison): maxBin - 1, a bin index, not a frequency
    bad = m.copy()
    bad[7] = np.nan
    assert S.spectral_shape(bad)[4] == 511.0
    assert S.spectral_shape(bad, rolloff_miss_is_frequency=True)[4] == ax[-1]
    # 100 %: unpinned -- within the last frequency step, or the miss value
    r = S.spectral_shape(m, rolloff_percent=100.0)[4]
    assert r == 511.0 or ax[-2] <= r <= ax[-1]


def test_shape_8_decibels_with_a_floor_and_power():
    mag = np.zeros(513)
    mag[100] = 1e300                                       # flatness ~ 1e-313: the floor holds it at 20 log10(eps)
    kept = S.spectral_shape(mag)
    assert kept[5] == 20 * np.log10(S.EPSILON)
    assert S.spectral_shape(mag, db_floor=False)[5] < -6000
    m = mags1024()[3]
    assert differs(S.spectral_shape(m, power=1), S.spectral_shape(m, power=0))
    assert np.allclose(S.spectral_shape(m, power=1), S.spectral_shape(np.maximum(m, S.EPSILON) ** 2), rtol=1e-12)


def test_chroma_init_the_axis_has_fft_points_over_the_sample_rate():
    kept, _ = S.chroma_filters(12, 513)
    tidy, _ = S.chroma_filters(12, 513, axis_over_fft=True)
    assert np.abs(kept - tidy).max() > 1e-4
    # freqs[0] = freqs[1] - 1.5 nChroma: column 0 peaks one and a half octaves = 18 classes below column 1
    assert kept[:, 0].argmax() == (kept[:, 1].argmax() - 18) % 12


def test_chroma_init_half_chroma_is_an_integer_quotient():
    kept, _ = S.chroma_filters(7, 257)
    tidy, _ = S.chroma_filters(7, 257, half_rounds_up=True)
    assert np.abs(kept - tidy).max() > 1e-3
    assert np.array_equal(S.chroma_filters(12, 257)[0], S.chroma_filters(12, 257, half_rounds_up=True)[0])


def test_chroma_init_the_remainder_is_c_fmod():
    # ref 22000: ref / 16 = 1375 Hz; at fft 16384 the first points lie more than 10.5 octaves below it and the argument
    # of fmod is negative: C's fmod keeps the sign, Python's % does not.  (At fft 4096 and 44.1 kHz it stays positive; at
    # 8 kHz it does not.)
    kept, _ = S.chroma_filters(12, 8193, 22000.0)
    tidy, _ = S.chroma_filters(12, 8193, 22000.0, c_fmod=False)
    assert np.abs(kept - tidy).max() > 1e-3
    assert np.array_equal(S.chroma_filters(12, 2049, 22000.0)[0], S.chroma_filters(12, 2049, 22000.0, c_fmod=False)[0])
    assert np.abs(S.chroma_filters(12, 2049, 22000.0, 8000.0)[0] - S.chroma_filters(12, 2049, 22000.0, 8000.0, c_fmod=False)[0]).max() > 1e-3
    assert np.array_equal(S.chroma_filters(12, 513)[0], S.chroma_filters(12, 513, c_fmod=False)[0])


def test_chroma_init_columns_are_normalised_and_the_scale():
    kept, scale = S.chroma_filters(12, 513)
    raw, _ = S.chroma_filters(12, 513, unit_columns=False)
    assert np.abs(kept - raw).max() > 1e-2
    assert scale == 2.0 / (1024 * 12)
    m = mags1024()[:4]
    assert np.allclose(S.chroma_frames(m), (m * m) @ kept.T * scale, rtol=1e-15)


def test_chroma_frame_the_range_branch():
    m = mags1024()[:6]
    full = S.chroma_frames(m)
    assert S.chroma_range(513, 0.0, -1.0, 44100.0) == (-1, 513)
    # min_freq 0 with max_freq set: the branch runs, minBin is 0 and bin 0 IS zeroed (0 .. minBin inclusive)
    assert S.chroma_range(513, 0.0, 30000.0, 44100.0) == (0, 512)
    assert S.chroma_range(513, 0.0, 30000.0, 44100.0, min_zero_keeps_all=False) == (-1, 512)
    m0 = m.copy()
    m0[:, 0] = 10 * m.max()
    kept = S.chroma_frames(m0, max_freq=5000.0)
    tidy = S.chroma_frames(m0, max_freq=5000.0, min_zero_keeps_all=False)
    assert np.abs(kept - tidy).max() > 1e-3 * np.abs(kept).max()
    # both set: bins 0 .. ceil(100 / binHz) = 3 and floor(5000 / binHz) = 116 .. 512 are zeroed
    assert S.chroma_range(513, 100.0, 5000.0, 44100.0) == (3, 116)
    w, scale = S.chroma_filters(12, 513)
    cut = m.copy()
    cut[:, :4] = 0
    cut[:, 116:] = 0
    assert np.array_equal(S.chroma_frames(m, min_freq=100.0, max_freq=5000.0), (cut * cut) @ w.T * scale)
    assert np.abs(full - S.chroma_frames(m, min_freq=100.0, max_freq=5000.0)).max() > 0
    # clamped where the reference would index past the frame
    assert S.chroma_range(513, 30000.0, -1.0, 44100.0) == (512, 512)
    assert np.all(S.chroma_frames(m, min_freq=30000.0) == 0)
    assert np.all(S.chroma_frames(m, max_freq=0.0) == 0)


def test_chroma_frame_normalize():
    m = mags1024()[:6]
    raw = S.chroma_frames(m)
    assert np.allclose(S.chroma_frames(m, normalize=1), raw / raw.sum(axis=1)[:, None], rtol=1e-15)
    assert np.allclose(S.chroma_frames(m, normalize=2), raw / raw.max(axis=1)[:, None], rtol=1e-15)
    z = np.zeros((2, 513))
    for normalize in NORMALIZE:                           # max(norm, epsilon): silence is 0, not 0 / 0
        assert np.all(S.chroma_frames(z, normalize=normalize) == 0)


def test_select_orders_the_channels():
    mags = mags1024()
    allsel = S.bufspectralshape(None, mags=mags, as_double=True)
    assert allsel.shape == (7, len(mags))
    some = S.bufspectralshape(None, select=0b1010010, mags=mags, as_double=True)
    assert np.array_equal(some, allsel[[1, 4, 6]])


# ---- the floors --------------------------------------------------------------------------------------------------------
def shape_err(a, b):
    """per descriptor: the largest |a - b| / max(1, |b|); NaNs must coincide"""
    assert np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore"):
        e = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    return np.nan_to_num(e, nan=0.0).reshape(-1, 7).max(axis=0)


def chroma_err(a, b):
    """the largest |a - b| relative to the frame's peak (frames of zeros: absolute)"""
    peak = np.abs(b).max(axis=-1, keepdims=True)
    return float((np.abs(a - b) / np.where(peak == 0, 1.0, peak)).max())


def test_floors_between_two_double_stfts(oracle):
    worst = np.zeros(7)
    cworst = {n: 0.0 for n in NORMALIZE}
    for shape in R.SHAPES:
        a, sr = shape_mags(shape)
        b, _ = shape_mags(shape, stft=oracle.stft)
        for unit, power in UNIT_POWER:
            worst = np.maximum(worst, shape_err(S.shape_frames(a, unit=unit, power=power, sr=sr),
                                                S.shape_frames(b, unit=unit, power=power, sr=sr)))
        for n in NORMALIZE:
            cworst[n] = max(cworst[n], chroma_err(S.chroma_frames(a, normalize=n, sr=sr), S.chroma_frames(b, normalize=n, sr=sr)))
    for name, w in zip(S.DESCRIPTORS, worst):
        print(f"{name}: {w:.3e} (constant {SHAPE_FLOOR[name]:.1e})")
    for n in NORMALIZE:
        print(f"chroma normalize {n}: {cworst[n]:.3e} (constant {CHROMA_FLOOR[n]:.1e})")
    assert all(w <= SHAPE_FLOOR[name] for name, w in zip(S.DESCRIPTORS, worst))
    assert all(cworst[n] <= CHROMA_FLOOR[n] for n in NORMALIZE)


def test_the_filter_table_s_floor():
    worst = 0.0
    for nc, n_bins, ref, sr in FILTER_CASES:
        w, _ = S.chroma_filters(nc, n_bins, ref, sr)
        wl, _ = S.chroma_filters(nc, n_bins, ref, sr, dtype=np.longdouble)
        worst = max(worst, float(np.abs(w - wl).max()))
    print(f"filter table: {worst:.3e} (constant {FILTER_FLOOR:.1e})")
    assert worst <= FILTER_FLOOR


# ---- the C++ host clients through tests/cpp/spectral_driver.cpp, without a device -----------------------------------------
@pytest.fixture(scope="module")
def spectral_driver(fluhip_lib_path):
    return S.build_driver()


def test_cpp_client_descriptors_are_the_references_tables(spectral_driver):
    mine = json.loads(R.drive(spectral_driver, "descriptors"))
    want = json.load(open(os.path.join(GOLDEN, "param_descriptors_spectral.json")))
    assert mine == want
    wrapper = ["source", "startFrame", "numFrames", "startChan", "numChans", "features", "padding"]
    assert [d["name"] for d in mine["BufSpectralShape"]] == wrapper + ["select", "minFreq", "maxFreq", "rolloffPercent", "unit",
                                                                      "power", "fftSettings"]
    assert [d["name"] for d in mine["BufChroma"]] == wrapper + ["numChroma", "ref", "normalize", "minFreq", "maxFreq", "fftSettings"]
    sel = [d for d in mine["BufSpectralShape"] if d["name"] == "select"][0]
    assert (sel["kind"], sel["default"], sel["strings"]) == ("Choices", 127, list(S.DESCRIPTORS))


def test_the_fixture_is_what_the_tool_mints_from_the_reference():
    ref = "/root/reference"
    if not os.path.isdir(ref):
        return   # the fixture is data; the reference's text is not everywhere
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_param_descriptor_fixture.py"), "--spectral", ref],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == json.load(open(os.path.join(GOLDEN, "param_descriptors_spectral.json")))


def test_cpp_client_defaults(spectral_driver):
    # select all on, 0 .. -1 Hz, 95 %, Hz, magnitudes, fft 1024 / -1 / -1, padding Default; 12 classes, 440 Hz, no normalisation
    assert R.drive(spectral_driver, "defaults").splitlines() == ["shape 127 0 -1 95 0 0 1024 512 1024 1",
                                                                 "chroma 12 440 0 0 -1 1024 512 1024 1"]


def test_cpp_client_error_paths(spectral_driver):
    got = [l.split("|") for l in R.drive(spectral_driver, "errors").splitlines()]
    want = [["no_source", "2", "Input buffer not set"], ["no_output", "2", "No valid output has been set"],
            ["start_past_end", "2", "Input buffer  invalid start frame 5000"],
            ["chan_past_end", "2", "Input buffer  invalid start channel 3"]]
    assert got == [[f"shape_{w[0]}"] + w[1:] for w in want] + [[f"chroma_{w[0]}"] + w[1:] for w in want]


@pytest.mark.parametrize("args,want", [
    (("shape", 255, -3, -7, 150, 4, -1, 1000, 250, -1), "127 0 -1 100 1 0 1000 250 1024"),   # select bits, Min(0), Min(-1), Max(100), enums
    (("shape", 5, 100, 50, 20, 1, 1, 512, 256, 2048), "5 100 50 20 1 1 512 256 2048"),        # (no relation between the bounds)
    (("chroma", 1, -5, 7, -2, -0.5, 1024, -1, -1), "2 0 2 0 -0.5 1024 512 1024"),             # Min(2), Min(0), enum, Min(0), Min(-1)
    (("chroma", 500, 30000, 1, 20, 2000, 1024, -1, -1), "500 22000 1 20 2000 1024 512 1024"),  # (numChroma: no static Max), Max(22000)
])
def test_cpp_client_constraints(spectral_driver, args, want):
    assert R.drive(spectral_driver, "constrain", *args).strip() == want
