"""CPU tests of tests/pitch_ref.py, the numpy restatement of the reference's pitch analysis (YinFFT, harmonic product
spectrum, cepstrum): closed forms with their analytic bounds, the kept quirks (each with a tidied variant that must fail),
the distance of the GPU tests' inputs from a tie, and the floor between two double STFTs that sets the GPU tests' bars."""
import json
import os

import numpy as np
import pytest

import pitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ALGORITHMS = (R.CEPSTRUM, R.HPS, R.YINFFT)
TIE_GUARD = 1e-5

# The largest difference between the restatement on numpy's FFT and on the project's C oracle STFT, per algorithm, over
# every shape of R.SHAPES on R.material(shape) under the client's framing: the curve element-wise relative to max(1, |want|),
# the pitch relative, the confidence absolute.  Each constant is the measured figure (beside it) rounded UP to two digits;
# test_floors_between_two_double_stfts asserts measured <= constant on every host it runs on, and the GPU bars are 64 x the
# constants (tests/test_gpu_pitch.py).  No frame is left out.
CURVE_FLOOR = {R.CEPSTRUM: 1.3e-12,   # measured 1.201e-12
               R.HPS: 1.2e-12,        # measured 1.152e-12
               R.YINFFT: 9.4e-14}     # measured 9.335e-14
PITCH_FLOOR = {R.CEPSTRUM: 7.5e-14,   # measured 7.486e-14
               R.HPS: 0.0,            # measured 0: a bin index times the bin width
               R.YINFFT: 1.7e-15}     # measured 1.659e-15
CONF_FLOOR = {R.CEPSTRUM: 1.2e-14,    # measured 1.123e-14
              R.HPS: 3.4e-16,         # measured 3.331e-16
              R.YINFFT: 5.6e-16}      # measured 5.551e-16

# (minFreq, maxFreq, sample rate) of the GPU tests' edge cases on the (1024, 1024, 512) input: equal bounds (an empty search),
# minFreq 0, and 8 kHz with a maxFreq beyond it, where every clamp bites -- once with a segment left, once with none for YinFFT
EDGE_BOUNDS = [(300.0, 300.0, 44100.0), (0.0, 10000.0, 44100.0), (20.0, 20000.0, 8000.0), (10.0, 20.0, 8000.0)]

_cache = {}


def shape_mags(shape, stft=None):
    """(magnitudes [T, F] of the client's frames, sample rate) of a test shape, computed once"""
    key = (shape, stft is not None)
    if key not in _cache:
        x, sr = R.material(shape)
        _cache[key] = (R.client_magnitudes(x, *shape, stft=stft), sr)
    return _cache[key]


def sine_frame(period, fft, harmonics=1):
    n = np.arange(fft)
    x = sum(np.sin(2 * np.pi * k * n / period) / k for k in range(1, harmonics + 1))
    return np.abs(np.fft.rfft(x * R.hann(fft)))


# ---- closed forms ----------------------------------------------------------------------------------------------------
def test_yinfft_finds_an_integer_period():
    # the difference function of a periodic signal dips at its period; the Hann window keeps the dip above zero, so the
    # rising factor i / tmpSum of the normalisation moves its minimum towards shorter lags, by less than the one lag the
    # search resolves before it interpolates
    sr, period = 44100.0, 100
    pitch, conf = R.yinfft(sine_frame(period, 1024), 20.0, 10000.0, sr)
    assert abs(sr / pitch - period) < 1.0
    assert conf > 0.9


def test_cepstrum_finds_an_integer_period():
    # a harmonic comb of spacing fft / period bins is a cosine of 2 nBins / (fft / period) half cycles over the nBins =
    # fft / 2 + 1 sample points of the DCT-II, and row i of the table is i half cycles: the peak lies within one row of
    # period (fft + 2) / fft
    sr, period, fft = 44100.0, 64, 2048
    mag = sine_frame(period, fft, harmonics=20) + 1e-3
    pitch, conf = R.cepstrum(mag, sr / (period * 1.5), sr / (period * 0.6), sr)
    assert abs(sr / pitch - period * (fft + 2) / fft) <= 1.0
    assert 0 < conf <= 1


def test_hps_finds_the_dominant_product():
    mag = np.full(513, 1e-3)
    j = 37
    mag[[j, 2 * j, 3 * j]] = 1.0
    pitch, conf = R.hps(mag, 20.0, 10000.0, 44100.0)
    assert pitch == j * 44100.0 / 1024
    assert conf > 0.99


@pytest.mark.parametrize("algorithm", (R.HPS, R.YINFFT))
def test_an_all_zero_frame_gives_zero_without_a_nan(algorithm):
    out = R.frame(np.zeros(513), algorithm)
    assert out == (0.0, 0.0)
    assert list(R.to_unit(np.array([0.0, 440.0]), 1)) == [-999.0, 69.0]


# ---- kept quirks: the tidied variant must differ ---------------------------------------------------------------------
def test_hps_multiplies_three_factors_not_four():
    mag = np.abs(np.random.default_rng(1).standard_normal(513)) + 0.1
    kept = R.hps_curve(mag)
    assert np.array_equal(kept[:10], (mag * np.r_[mag[0:513:2], np.zeros(256)][:513] * np.r_[mag[0:513:3], np.zeros(342)][:513])[:10])
    assert np.all(kept[513 // 3:] == 0)
    through4 = R.hps_curve(mag, n_harmonics=5)
    assert not np.allclose(kept[1:100], through4[1:100])


def test_yinfft_clamps_the_upper_lag_to_size_minus_minbin():
    # at 8 kHz with maxFreq 20: minBin = 400, so the clamp cuts maxBin from nBins to 513 - 400 - 1 = 112 < minBin: no search
    mags, _ = shape_mags((1024, 1024, 512))
    m = mags[3]
    assert R.bins(R.YINFFT, 513, 10.0, 20.0, 8000.0) == (400, 112)
    assert R.yinfft(m, 10.0, 20.0, 8000.0) == (0.0, 0.0)
    assert R.yinfft(m, 10.0, 20.0, 8000.0, clamp=False)[0] > 0
    # ... and where both survive, the clamp shortens the segment: lo = 2, hi = 513 - 2 - 1
    assert R.bins(R.YINFFT, 513, 0.0, 20000.0, 44100.0) == (2, 510)
    assert R.bins(R.YINFFT, 513, 0.0, 20000.0, 44100.0, yin_clamp=False) == (2, 513)


def test_the_dct_scales_row_zero_on_its_own():
    mags, sr = shape_mags((1024, 1024, 512))
    kept = R.cepstrum(mags[3], 50.0, 2000.0, sr)
    tidy = R.cepstrum(mags[3], 50.0, 2000.0, sr, row0_like_others=True)
    assert kept[0] == tidy[0]
    assert abs(kept[1] * 2 ** -0.5 - tidy[1]) < 1e-12 and kept[1] != tidy[1]
    t = R.dct_table(8)
    assert np.allclose(t @ t.T, np.eye(8))   # orthonormal only with the kept scale


def test_peak_detection_orders_by_interpolated_height():
    seg = np.array([0.0, 1.0, 0.9, 0.0, 1.0, 0.2, 0.0])   # equal raw heights; the first peak's parabola is higher
    pk = R.peaks(seg)
    assert [round(p[0]) for p in pk] == [1, 4]
    assert pk[0][1] > pk[1][1] > 1.0
    assert R.peaks(np.array([0.0, np.nan, 0.0, 1.0, 0.0]))[0][0] == 3.0   # a NaN fails every comparison


def test_unbounded_quotients_count_as_the_bin_count():
    assert R.bins(R.CEPSTRUM, 513, 0.0, 10000.0, 44100.0) == (4, 513)
    assert R.bins(R.HPS, 129, 20.0, 20000.0, 8000.0) == (1, 129)
    assert R.hps(np.ones(129), 9000.0, 10000.0, 8000.0) == (0.0, 0.0)     # minBin >= nBins


# ---- the client ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding_mode", (0, 1, 2))
@pytest.mark.parametrize("shape", R.SHAPES[:4])
def test_frame_positions_are_the_streaming_wrapper_s(shape, padding_mode):
    # FluidSource model: the input sits latency + pad into the padded signal; frame j is the win samples ending at (j + 1) hop
    win, fft, hop = shape
    n = 5000
    pad = (0, win >> 1, win - hop)[padding_mode]
    padded = n + win + 2 * pad
    if padding_mode == 2:
        padded = -(-padded // hop) * hop
    start, T = R.client_frames(n, win, hop, padding_mode)
    total = 1 + (padded - win) // hop
    assert T == total - win // hop
    assert start == (win // hop) * hop - win - pad
    assert start + (T - 1) * hop < n


def test_select_and_unit():
    mags, sr = shape_mags((1024, 1024, 512))
    both = R.bufpitch(None, R.YINFFT, mags=mags, as_double=True)
    assert both.shape == (2, len(mags))
    assert np.array_equal(R.bufpitch(None, R.YINFFT, select=2, mags=mags, as_double=True)[0], both[1])
    midi = R.bufpitch(None, R.YINFFT, unit=1, select=1, mags=mags, as_double=True)[0]
    assert np.allclose(midi, 69 + 12 * np.log2(both[0] / 440))
    with pytest.raises(ValueError):
        R.bufpitch(None, select=0, mags=mags)


# ---- the GPU tests' inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ALGORITHMS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=[str(s) for s in R.SHAPES])
def test_the_inputs_keep_clear_of_ties(shape, algorithm):
    mags, sr = shape_mags(shape)
    leads = np.array([R.lead(m, algorithm, sr=sr) for m in mags])
    res = R.frames(mags, algorithm, sr=sr)
    loud = mags.max(axis=1) > 1e-3
    print(f"{shape} algorithm {algorithm}: smallest lead {leads.min():.3e}, {int((res[loud, 0] != 0).sum())} of {int(loud.sum())} loud frames with a pitch")
    assert leads.min() >= TIE_GUARD
    assert (res[loud, 0] != 0).sum() * 2 >= loud.sum()


def test_the_clamps_bite_at_8_khz():
    mags, _ = shape_mags((1024, 1024, 512))
    for lo, hi, sr in EDGE_BOUNDS:
        for algorithm in ALGORITHMS:
            leads = np.array([R.lead(m, algorithm, lo, hi, sr) for m in mags])
            print(f"bounds ({lo}, {hi}) at {sr} Hz, algorithm {algorithm}: smallest lead {leads.min():.3e}")
            assert leads.min() >= TIE_GUARD
    assert R.bins(R.YINFFT, 513, 20.0, 20000.0, 8000.0) == (0, 400)
    assert R.bins(R.HPS, 513, 20.0, 20000.0, 8000.0) == (3, 513)
    assert R.bins(R.CEPSTRUM, 513, 20.0, 20000.0, 8000.0) == (0, 400)


def test_floors_between_two_double_stfts(oracle):
    worst = {a: [0.0, 0.0, 0.0] for a in ALGORITHMS}
    for shape in R.SHAPES:
        a, sr = shape_mags(shape)
        b, _ = shape_mags(shape, stft=oracle.stft)
        for alg in ALGORITHMS:
            ca, cb = R.curves(a, alg), R.curves(b, alg)
            ra, rb = R.frames(a, alg, sr=sr), R.frames(b, alg, sr=sr)
            assert np.array_equal(ra[:, 0] != 0, rb[:, 0] != 0)
            nz = ra[:, 0] != 0
            w = worst[alg]
            w[0] = max(w[0], float(np.nanmax(np.abs(ca - cb) / np.maximum(1.0, np.abs(ca)))))
            w[1] = max(w[1], float((np.abs(ra[nz, 0] - rb[nz, 0]) / ra[nz, 0]).max()) if nz.any() else 0.0)
            w[2] = max(w[2], float(np.abs(ra[:, 1] - rb[:, 1]).max()))
    for alg in ALGORITHMS:
        c, p, k = worst[alg]
        print(f"algorithm {alg}: curve {c:.3e} (constant {CURVE_FLOOR[alg]:.1e}), pitch {p:.3e} ({PITCH_FLOOR[alg]:.1e}), "
              f"confidence {k:.3e} ({CONF_FLOOR[alg]:.1e})")
        assert c <= CURVE_FLOOR[alg] and p <= PITCH_FLOOR[alg] and k <= CONF_FLOOR[alg]


EXTRA = R.extra_inputs()


def extra_mags(i):
    if ("extra", i) not in _cache:
        _, x, shape, mode, lo, hi, sr = EXTRA[i]
        _cache[("extra", i)] = R.client_magnitudes(x, *shape, padding_mode=mode)
    return _cache[("extra", i)]


@pytest.mark.parametrize("i", range(len(EXTRA)), ids=[e[0] for e in EXTRA])
def test_the_extra_inputs_keep_clear_of_ties(i):
    _, x, shape, mode, lo, hi, sr = EXTRA[i]
    mags = extra_mags(i)
    for algorithm in ALGORITHMS:
        leads = np.array([R.lead(m, algorithm, lo, hi, sr) for m in mags])
        print(f"{EXTRA[i][0]} algorithm {algorithm}: smallest lead {leads.min():.3e}")
        assert leads.min() >= TIE_GUARD


# ---- the C++ host client (include/flucoma_hip/PitchClient.hpp) through tests/cpp/pitch_driver.cpp, without a device -----
@pytest.fixture(scope="module")
def pitch_driver(fluhip_lib_path):
    return R.build_driver()


def test_cpp_client_descriptors_are_the_references_table(pitch_driver):
    mine = json.loads(R.drive(pitch_driver, "descriptors"))
    want = json.load(open(os.path.join(GOLDEN, "param_descriptors_pitch.json")))
    assert mine == want
    assert [d["name"] for d in mine["BufPitch"]] == ["source", "startFrame", "numFrames", "startChan", "numChans", "features",
                                                    "padding", "select", "algorithm", "minFreq", "maxFreq", "unit", "fftSettings"]
    sel = [d for d in mine["BufPitch"] if d["name"] == "select"][0]
    assert (sel["kind"], sel["default"], sel["strings"]) == ("Choices", 3, ["pitch", "confidence"])


def test_the_fixture_is_what_the_tool_mints_from_the_reference():
    ref = "/root/reference"
    if not os.path.isdir(ref):
        return   # the fixture is data; the reference's text is not everywhere
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_param_descriptor_fixture.py"), "--pitch", ref],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == json.load(open(os.path.join(GOLDEN, "param_descriptors_pitch.json")))


def test_cpp_client_defaults(pitch_driver):
    # select all on, YinFFT, 20 .. 10000 Hz, Hz, fft 1024 / -1 / -1 (hop 512, fft 1024), padding Default
    assert R.drive(pitch_driver, "defaults").strip() == "3 2 20 10000 0 1024 512 1024 1"


def test_cpp_client_error_paths(pitch_driver):
    got = [l.split("|") for l in R.drive(pitch_driver, "errors").splitlines()]
    assert got == [["no_source", "2", "Input buffer not set"], ["no_output", "2", "No valid output has been set"],
                   ["start_past_end", "2", "Input buffer  invalid start frame 5000"],
                   ["chan_past_end", "2", "Input buffer  invalid start channel 3"]]


@pytest.mark.parametrize("args,want", [
    ((3, 2, 500, 100, 0, 1024, -1, -1), "3 2 100 100 0 1024 512 1024"),          # minFreq capped at maxFreq
    ((7, 5, -3, 0.5, 4, 1000, 250, -1), "3 2 0 1 1 1000 250 1024"),              # ranges: select bits, enums, Min(0), Min(1)
    ((1, 0, 20000, 30000, 1, 512, 256, 2048), "1 0 10000 20000 1 512 256 2048"),  # Max(10000), Max(20000)
])
def test_cpp_client_constraints(pitch_driver, args, want):
    assert R.drive(pitch_driver, "constrain", *args).strip() == want
