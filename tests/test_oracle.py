"""CPU tests: the C oracle against the committed golden vectors (minted by the independent numpy
restatement) and against the pins the reference's own tests provide for this path.

Reference tests mirrored here:
  tests/algorithms/public/TestNMF.cpp:11-46          same seed => identical output, other seed differs
  tests/algorithms/util/TestEigenRandom.cpp:92-114   seed repeatability, range
  tests/clients/common/TestBufferedProcess.cpp:42-44 Hann formula 0.5 - 0.5 cos(2 pi i / N), COLA
"""
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from helpers import rel_err

RNG_CPP = r"""
#include <random>
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  unsigned long seed = strtoul(argv[1], 0, 10); int n = atoi(argv[2]);
  std::mt19937_64 g{seed}; std::uniform_real_distribution<double> d{0.0, 1.0};
  for (int i = 0; i < n; i++) printf("%.17g\n", d(g));
}
"""


def test_rng_matches_libstdcxx(oracle, onp):
    """util/EigenRandom.hpp:73-101 uses libstdc++'s <random> verbatim: compile it and compare."""
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "r.cpp"), os.path.join(td, "r")
        open(src, "w").write(RNG_CPP)
        subprocess.run(["g++", "-O1", "-o", exe, src], check=True)
        for seed in (0, 42, 5063, 2**31 + 7):
            out = subprocess.run([exe, str(seed), "1000"], check=True, capture_output=True, text=True).stdout
            ref = np.array([float(x) for x in out.split()])
            assert np.array_equal(oracle.rng_uniform01(seed, 1000), ref)
            assert np.array_equal(onp.rng_uniform01(seed, 1000), ref)


def test_rng_golden(oracle, golden):
    for seed in (42, 5063):
        r = oracle.rng_uniform01(seed, 16)
        assert np.array_equal(r, golden[f"g3_rng{seed}"])
        assert (r >= 0).all() and (r < 1).all()
    # SURVEY 8 a6 known values
    assert oracle.rng_uniform01(42, 1)[0] == 0.75515553295453897
    assert oracle.rng_uniform01(5063, 1)[0] == 0.05300292112151906


def test_hann_window(oracle, golden):
    for win in (1024, 2048, 4096):
        w = oracle.hann(win)
        assert np.array_equal(w[:8], golden[f"g1_hann{win}_head"])
        assert np.array_equal(w[-8:], golden[f"g1_hann{win}_tail"])
        assert abs(w.sum() - golden[f"g1_hann{win}_sum"][0]) < 1e-9
    # TestBufferedProcess.cpp:42-44 + COLA of the periodic Hann at overlap 2
    N = 1024
    w = oracle.hann(N)
    i = np.arange(N)
    assert np.allclose(w, 0.5 - 0.5 * np.cos(2 * np.pi * i / N), atol=1e-15)
    assert np.allclose(w[: N // 2] + w[N // 2:], 1.0, atol=1e-12)


@pytest.mark.parametrize("n,win,hop", [(453932, 1024, 512), (2646000, 2048, 512), (441000, 2048, 512),
                                       (88200, 1024, 512), (1, 1024, 512), (511, 1024, 512), (512, 1024, 512)])
def test_frame_count(oracle, n, win, hop):
    """nrt/NMFClient.hpp:111-112 / alg/STFT.hpp:98-99 -- integer arithmetic, exact."""
    assert oracle.num_frames(n, win, hop) == (n + hop) // hop == n // hop + 1


def test_frame_counts_of_baseline_configs(oracle):
    assert oracle.num_frames(453932, 1024, 512) == 887
    assert oracle.num_frames(2646000, 2048, 512) == 5168
    assert oracle.num_frames(26460000, 4096, 1024) == 25840
    assert oracle.num_frames(441000, 2048, 512) == 862


@pytest.mark.parametrize("wfh", [(1024, 1024, 512), (2048, 2048, 512), (512, 1024, 256)])
def test_stft_golden(oracle, golden, wfh):
    win, fft, hop = wfh
    sig = golden["g2_signal"]
    spec, mag = oracle.stft_f32(sig, win, fft, hop)
    key = f"g2_{win}_{fft}_{hop}"
    assert spec.shape[0] == int(golden[key + "_T"][0])
    rows = golden[key + "_rows"]
    scale = np.abs(golden[key + "_spec"]).max()
    assert np.abs(spec[rows] - golden[key + "_spec"]).max() / scale < 1e-12
    assert np.abs(mag[rows] - golden[key + "_mag"]).max() / scale < 1e-12
    assert abs(mag.sum() - golden[key + "_magsum"][0]) / golden[key + "_magsum"][0] < 1e-12
    # DC and Nyquist purely real (util/FFT.hpp:99-101)
    assert np.all(spec[:, 0].imag == 0) and np.all(spec[:, -1].imag == 0)


def test_stft_against_naive_dft(oracle):
    """the hand-rolled FFT against a long-double direct DFT on one frame"""
    rs = np.random.RandomState(0)
    x = rs.standard_normal(300)
    win, fft, hop = 64, 128, 16
    spec, mag = oracle.stft(x, win, fft, hop)
    t = 7
    padded = np.zeros(len(x) + win + hop, dtype=np.longdouble)
    padded[win // 2: win // 2 + len(x)] = x
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)).astype(np.longdouble)
    fr = np.zeros(fft, dtype=np.longdouble)
    fr[:win] = padded[t * hop: t * hop + win] * w
    k = np.arange(fft // 2 + 1)[:, None].astype(np.longdouble)
    nn = np.arange(fft)[None, :].astype(np.longdouble)
    ang = -2 * np.pi * k * nn / fft
    re = (fr[None, :] * np.cos(ang)).sum(axis=1)
    im = (fr[None, :] * np.sin(ang)).sum(axis=1)
    assert np.abs(spec[t].real - re.astype(np.float64)).max() < 1e-13
    assert np.abs(spec[t].imag[1:-1] - im.astype(np.float64)[1:-1]).max() < 1e-13


def test_nmf_repeatable_with_seed(oracle):
    """tests/algorithms/public/TestNMF.cpp:11-46"""
    X = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9.0]])
    a = oracle.nmf_process(X, 2, 1, True, True, 42)
    b = oracle.nmf_process(X, 2, 1, True, True, 42)
    c = oracle.nmf_process(X, 2, 1, True, True, 5063)
    d = oracle.nmf_process(X, 2, 1, True, True, 5063)
    for i in range(3):
        assert np.array_equal(a[i], b[i]) and np.array_equal(c[i], d[i])
        assert not np.array_equal(a[i], c[i])
        assert np.isfinite(a[i]).all()


@pytest.mark.parametrize("seed", [42, 5063])
@pytest.mark.parametrize("iters", [1, 50])
def test_nmf_tiny_golden(oracle, golden, seed, iters):
    W1, H1, V1, rc = oracle.nmf_process(golden["g4_X"], 2, iters, True, True, seed)
    assert rc == 0
    assert rel_err(W1, golden[f"g4_s{seed}_i{iters}_W"]) < 1e-12
    assert rel_err(H1, golden[f"g4_s{seed}_i{iters}_H"]) < 1e-12
    assert rel_err(V1, golden[f"g4_s{seed}_i{iters}_V"]) < 1e-12


@pytest.mark.parametrize("faithful", [False, True])
@pytest.mark.parametrize("mode", ["u11", "u10", "u01", "u00", "seeded"])
def test_nmf_g5_golden(oracle, golden, mode, faithful):
    X, W0, H0 = golden["g5_X"], golden["g5_W0"], golden["g5_H0"]
    if mode == "seeded":
        uw, uh, iters, w0, h0 = True, True, 200, W0, H0
    else:
        uw, uh = mode[1] == "1", mode[2] == "1"
        iters = 200 if (uw or uh) else 0
        w0, h0 = (None if uw else W0), (None if uh else H0)
    W1, H1, V1, rc = oracle.nmf_process(X, 4, iters, uw, uh, 42, w0, h0, faithful=faithful)
    assert rc == 0
    assert rel_err(W1, golden[f"g5_{mode}_W"]) < 1e-11
    assert rel_err(H1, golden[f"g5_{mode}_H"]) < 1e-11
    assert rel_err(V1, golden[f"g5_{mode}_V"]) < 1e-11


def test_nmf_cancel(oracle):
    X = np.abs(np.random.RandomState(1).standard_normal((20, 9)))
    calls = []

    def cb(it):
        calls.append(it)
        return it < 3

    W1, H1, V1, rc = oracle.nmf_process(X, 2, 10, True, True, 1, progress=cb)
    assert rc == 1 and calls == [1, 2, 3]
    assert np.array_equal(V1, X)  # alg/NMF.hpp:175-176: early return leaves V untouched


def test_writeback(oracle, onp):
    rs = np.random.RandomState(2)
    W1, H1 = rs.uniform(0, 1, (3, 17)), rs.uniform(0, 2, (29, 3))
    b, a = oracle.bufnmf_writeback(W1, H1)
    b2, a2 = onp.bufnmf_writeback(W1, H1)
    assert np.array_equal(b, b2) and np.array_equal(a, a2)
    assert a.max() == pytest.approx(1.0, abs=1e-6)


def test_c1_shape_end_to_end_golden(oracle, onp, golden):
    """BASELINE config 1 shape (453932 samples, rank 3, 1024/512, 50 iterations) on the
    synthetic drum-like stand-in for Nicol-LoopE-M.wav."""
    x = onp.drum_like(453932)
    sha = np.frombuffer(hashlib.sha256(x.tobytes()).digest(), dtype=np.uint8)
    if not np.array_equal(sha, golden["g6_input_sha256"]):
        pytest.skip("numpy RandomState stream differs from the one the fixture was minted with")
    bases, acts, mag = oracle.bufnmf_channel(x, 1024, 1024, 512, 3, 50, 42, want_mag=True)
    assert mag.shape == tuple(golden["g6_TF"])
    pb, pa = golden["g6_probe_bases_idx"], golden["g6_probe_acts_idx"]
    assert np.allclose(bases[pb[:, 0], pb[:, 1]], golden["g6_probe_bases"], rtol=1e-5, atol=1e-7)
    assert np.allclose(acts[pa[:, 0], pa[:, 1]], golden["g6_probe_acts"], rtol=1e-5, atol=1e-7)
    sums = golden["g6_sums"]
    assert abs(mag.sum() - sums[2]) / sums[2] < 1e-12
    assert abs(bases.astype(np.float64).sum() - sums[0]) / sums[0] < 1e-6


def test_resynth_oracles_agree(oracle, onp):
    x = onp.synth_audio(6000, 5)
    win, fft, hop, K = 256, 256, 64, 3
    spec, mag = onp.stft(x.astype(np.float64), win, fft, hop)
    W1, H1, V1 = onp.nmf_process(mag, K, 20, True, True, 42)
    tot = np.zeros(len(x))
    for k in range(K):
        a = oracle.resynth_component(spec, W1, H1, V1, k, win, fft, hop, len(x))
        b = onp.resynth_component(spec, W1, H1, V1, k, win, fft, hop, len(x))
        assert np.abs(a - b).max() < 1e-12
        tot += a
    # the masks sum to ~1 so the components add back up to (almost) the input
    assert np.abs(tot - x).max() < 0.05


def test_reference_wav_c1_when_available(oracle, onp):
    """Plumbing config c1 on the bundled WAV's samples (Nicol-LoopE-M.wav, 16-bit mono 44.1 kHz: all of them travel in
    tests/golden/reference_c1.npz, tools/make_reference_c1_fixture.py): both oracles on the whole spectrogram and factors."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_c1.npz"))
    assert float(g["sample_rate"]) == 44100 and g["pcm16"].dtype == np.int16 and g["pcm16"].ndim == 1
    n = len(g["pcm16"])
    assert n == 453932
    x = (g["pcm16"].astype(np.float32) / 32768.0)
    bases, acts, mag = oracle.bufnmf_channel(x, 1024, 1024, 512, 3, 50, 42, want_mag=True)
    b2, a2, m2, *_ = onp.bufnmf_channel(x, 1024, 1024, 512, 3, 50, 42)
    assert mag.shape == (887, 513)
    assert rel_err(mag, m2) < 1e-12
    assert rel_err(bases, b2) < 1e-6 and rel_err(acts, a2) < 1e-6


def test_c1_fixture_both_oracles(oracle, onp):
    """tests/golden/reference_c1.npz (tools/make_reference_c1_fixture.py): BASELINE config 1 on its named input -- the
    bundled loop's own samples travel as data -- and what both restatements make of it (T = 887, F = 513, rank 3,
    50 iterations, seed 42): the C oracle and the numpy oracle reproduce the stored probes here, the HIP path on the GPU
    (tests/test_gpu_parity.py::test_c1_on_the_named_input)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_c1.npz"))
    win, fft, hop, K, iters, seed = (int(v) for v in g["params"])
    x = g["pcm16"].astype(np.float32) / 32768.0
    assert len(x) == 453932 and (win, fft, hop, K, iters, seed) == (1024, 1024, 512, 3, 50, 42)
    bases, acts, mag = oracle.bufnmf_channel(x, win, fft, hop, K, iters, seed, want_mag=True)
    assert mag.shape == tuple(g["frames_bins"]) == (887, 513)
    pb, pa = g["probe_bases_idx"], g["probe_acts_idx"]
    assert np.array_equal(bases[pb[:, 0], pb[:, 1]], g["probe_bases_c"])
    assert np.array_equal(acts[pa[:, 0], pa[:, 1]], g["probe_acts_c"])
    assert rel_err(mag[::97, ::31], g["mag_probe"]) < 1e-14
    assert np.allclose(g["probe_bases_c"], g["probe_bases_np"], rtol=1e-6, atol=1e-9)
    assert np.allclose(g["probe_acts_c"], g["probe_acts_np"], rtol=1e-6, atol=1e-9)
    assert np.allclose(g["sums_c"], g["sums_np"], rtol=1e-6)


def test_process_frame_c_vs_numpy():
    """alg/NMF.hpp:45-89 restated twice (C and numpy) must agree; and the update must not move a frame
    that the dictionary already explains exactly (fixed point of the KL multiplicative update)."""
    import oracle_c, oracle_np
    o = oracle_c.get("native")
    rng = np.random.default_rng(3)
    K, F = 4, 65
    W0 = rng.random((K, F))
    X = rng.random((6, F))
    X[1, :5] = 0.0
    H, V = o.nmf_process_frames(X, W0, 10, 42)
    for t in range(X.shape[0]):
        h, v = oracle_np.nmf_process_frame(X[t], W0, 10, 42)
        assert np.allclose(H[t], h, rtol=1e-12, atol=0) and np.allclose(V[t], v, rtol=1e-12, atol=0)
    # same seed => same start for every frame (a fresh generator per call, util/EigenRandom.hpp:80)
    H0, _ = o.nmf_process_frames(np.vstack([X[2], X[2]]), W0, 0, 42)
    assert np.array_equal(H0[0], H0[1]) and np.array_equal(H0[0], np.maximum(oracle_np.rng_uniform01(42, K), 2.220446049250313e-16))
    Wn = W0 / np.sqrt((W0 * W0).sum(axis=1, keepdims=True))
    htrue = np.array([0.5, 1.5, 0.25, 2.0])
    hfit, vfit = oracle_np.nmf_process_frame(htrue @ Wn, W0, 2000, 7)
    assert np.allclose(vfit, htrue @ Wn, rtol=1e-6)


@pytest.mark.parametrize("seed,iters", [(42, 10), (5063, 10), (42, 0), (7, 100)])
def test_process_frame_golden(seed, iters):
    """G7: the C restatement of NMF::processFrame against the committed vectors (tools/make_golden.py --frames)"""
    import oracle_c
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_frames_v1.npz"))
    H, V = oracle_c.get("native").nmf_process_frames(g["g7_X"], g["g7_W0"], iters, seed)
    assert rel_err(H, g[f"g7_s{seed}_i{iters}_H"]) < 1e-12 and rel_err(V, g[f"g7_s{seed}_i{iters}_V"]) < 1e-12


def test_nndsvd_oracle_properties():
    """the numpy restatement of NNDSVD (alg/NNDSVD.hpp:30-132): rank rule, non-negativity, method 0
    reproduces |U S V^T| term by term, the lazily sampled random fill of method 1 consumes one draw per
    sub-epsilon coefficient in column-major order"""
    import oracle_np as onp
    rs = np.random.RandomState(4)
    X = np.abs(rs.standard_normal((50, 6))) @ np.abs(rs.standard_normal((6, 33))) + 1e-3
    W, H, k, U, s, VT = onp.nndsvd(X, 10, 0, 10, 0.9, 0, 42)
    assert k == onp.nndsvd_rank(s, 0, 10, 0.9) and 1 <= k <= 10
    assert (W >= 0).all() and (H >= 0).all() and (W[k:] == 0).all() and (H[:, k:] == 0).all()
    assert np.allclose(W[:k], np.abs(U[:, :k].T)) and np.allclose(H[:, :k], np.abs((s[:k, None] * VT[:k]).T))
    assert onp.nndsvd_rank(s, 3, 10, 0.0) == 3 and onp.nndsvd_rank(s, 0, 2, 0.999) == 2
    W3, H3, _ = onp.nndsvd_from_svd(U, s, VT, X, 10, 4, 4, 0.0, 3, 42)
    W1, H1, _ = onp.nndsvd_from_svd(U, s, VT, X, 10, 4, 4, 0.0, 1, 42)
    eps = 2.220446049250313e-16
    holes = np.flatnonzero(W3.reshape(-1) < eps)            # W3 [rows, F] row-major == WT column-major
    draws = (X.mean() * 0.001 - eps) * onp.rng_uniform01(42, holes.size) + eps
    assert np.array_equal(W1.reshape(-1)[holes], draws)
    assert np.array_equal(W1.reshape(-1)[W3.reshape(-1) >= eps], W3.reshape(-1)[W3.reshape(-1) >= eps])


@pytest.mark.parametrize("frame", [32, 64, 256, 1024, 8192])
def test_hann_cola_like_reference_buffered_process(oracle, frame):
    """tests/clients/common/TestBufferedProcess.cpp:20-70: the reference checks that its Hann window
    (0.5 - 0.5 cos(2 pi i / N), the formula the oracle's window must be) overlap-adds to the input at hop = N/2
    to 1e-12.  Same property, same sizes, on the oracle's table; and at hop = N/4 the squared window sums to 1.5
    (the normaliser the ISTFT divides by, alg/STFT.hpp:196)."""
    w = oracle.hann(frame)
    i = np.arange(frame)
    assert np.array_equal(w, 0.5 - 0.5 * np.cos((2 * np.pi * i) / frame))
    hop = frame // 2
    ola = w[:hop] + w[hop:]
    assert np.abs(ola - 1.0).max() < 1e-12
    q = frame // 4
    sq = sum((w[j * q:(j + 1) * q]) ** 2 for j in range(4))
    assert np.abs(sq - 1.5).max() < 1e-12


def test_reference_testnmf_processframe_case(oracle):
    """tests/algorithms/public/TestNMF.cpp:48-73, same inputs: processFrame with 0 iterations returns the seeded
    start; same seed => same output, another seed => another output"""
    x = np.array([1.0, 0, 1, 0])
    bases = np.array([[0.0, 0, 1, 0], [1, 0, 0, 0]])
    a, _ = oracle.nmf_process_frames(x[None, :], bases, 0, 42)
    b, _ = oracle.nmf_process_frames(x[None, :], bases, 0, 42)
    c, _ = oracle.nmf_process_frames(x[None, :], bases, 0, 7863)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


# ---- the reference's own known answers for the framing of the buffered clients ------------------------------
@pytest.mark.parametrize("dtype", [np.int64, np.float64])
@pytest.mark.parametrize("overlap", [4, 3, 2, 1])
@pytest.mark.parametrize("frame_size", [32, 43, 64, 96, 128, 512])
def test_reference_testfluidsource_known_delay(onp, frame_size, overlap, dtype):
    """tests/clients/common/TestFluidSource.cpp:17-59 replayed on the restated FluidSource (oracle_np.FluidSourceModel):
    host blocks of 64 samples of an iota signal, max frame 1024; every frame pulled at hop = frameSize / overlap
    equals the input delayed by frameSize -- the reference's known answer, same sizes, same loop."""
    host, max_frame = 64, 1024
    framer = onp.FluidSourceModel(max_frame, host, dtype=dtype)
    data = np.arange(2 * max_frame, dtype=dtype)
    hop = frame_size // overlap
    expected = np.zeros(data.size + frame_size, dtype=dtype)
    expected[frame_size:] = data                                  # :41-43
    j = k = 0
    pulled = 0
    for i in range(0, data.size - host, host):                    # :45
        framer.push(data[i:i + host])
        while j < host:                                           # :52-56
            out = framer.pull(frame_size, j)
            assert np.array_equal(out, expected[k:k + frame_size]), (i, j, k)
            j += hop
            k += hop
            pulled += 1
        j = j if j < host else j - host                           # :58
    assert pulled >= (data.size - host) // hop - 1


@pytest.mark.parametrize("frame_size", [32, 64, 256, 1024, 8192])
def test_reference_testbufferedprocess_cola(onp, frame_size):
    """tests/clients/common/TestBufferedProcess.cpp:20-70 replayed on the restated FluidSource + FluidSink:
    a step signal pushed in host blocks of 64, Hann-windowed frames at hop = frameSize / 2 overlap-added back;
    the output is the input delayed by frameSize to 1e-12 (:60-68)."""
    host = 64
    hop = frame_size // 2
    src = onp.FluidSourceModel(frame_size, host)
    snk = onp.FluidSinkModel(frame_size, host)
    total = min(128 * frame_size, 16 * frame_size + 4096)         # the reference runs 128 frames; the tail repeats
    x = np.zeros(total)
    x[frame_size:] = 1.0                                          # :33
    w = onp.hann(frame_size)
    frame_time = 0
    for i in range(frame_size, total - host, host):               # :45
        src.push(x[i:i + host])
        while frame_time < host:                                  # BufferedProcess::process, cc/BufferedProcess.hpp:52-67
            snk.push(src.pull(frame_size, frame_time) * w, frame_time)
            frame_time += hop
        frame_time = frame_time if frame_time < host else frame_time - host
        actual = snk.pull(host)
        assert np.abs(actual - x[i - frame_size:i - frame_size + host]).max() <= 1e-12, i


@pytest.mark.parametrize("n,win,hop", [(88200, 1024, 512), (20000, 1024, 256), (9999, 512, 100), (5000, 2048, 300),
                                       (777, 64, 64), (4096, 1024, 1024), (30000, 4096, 1000), (5001, 301, 75),
                                       (5024, 301, 75), (999, 33, 11)])
@pytest.mark.parametrize("padding_mode", [0, 1, 2])
def test_feature_framing_follows_from_fluidsource(oracle, onp, n, win, hop, padding_mode):
    """The closed form both oracles (and the HIP path's frameOffset) use for the frames BufMFCC / BufMelBands keep --
    T = 1 + (n + 2 (win / 2)) / hop - win / hop, frame k starts at (win / hop) hop - win - win / 2 + k hop -- derived by
    running the restated StreamingControl -> BufferedProcess -> FluidSource chain on a signal of sample indices."""
    if padding_mode != 1 and hop > win:
        pytest.skip("FFTParams keeps hop <= win")
    T, start0 = onp.feature_frames(n, win, hop, padding_mode)
    Tm, starts = onp.streaming_control_frame_starts(n, win, hop, padding_mode)
    assert Tm == T
    seen = 0
    for k, s in enumerate(starts):
        if s is not None:
            assert s == start0 + k * hop, (k, s)
            seen += 1
    assert seen >= T - 2 - win // hop


# ---- a pin on the REAL reference's outputs: its pre-analysed demo corpus -----------------------------------------------
def _mfcc_stats(m):
    """BufStats' mean and standard deviation per coefficient (algorithms/util/WeightedStats.hpp:34-35: uniform weights
    1 / N, i.e. the population form), flattened as the corpus rows are: 13 means, then 13 deviations"""
    m = m.astype(np.float64)
    return np.concatenate([m.mean(axis=1), m.std(axis=1)])


def test_oracles_reproduce_the_references_pre_analysed_corpus(oracle, onp):
    """flucoma-core ships the output of a FluCoMa build: Resources/Data/flucoma_corpus_mfcc.json holds, for 1086 slices of
    its concatenated demo files, the mean and deviation over the slice's frames of BufMFCC's coefficients 1..13 (info.txt:
    "pre-analysed MFCCs of the FluCoMa demo audio files in small slices"; slice points in flucoma_corpus_slices.wav, file
    order in flucoma_corpus_files.json).  299 slices lie inside the first three files; 27 of them travel with their rows in
    tests/golden/reference_corpus_mfcc_sample.npz (tools/make_reference_corpus_sample_fixture.py: slice 0, the two that
    straddle a file boundary, 8 short ones per file, seeded) and are recomputed: both oracles -- sample read, Hann window, the buffered clients' framing and padding, the unnormalised FFT,
    magnitude, 40 mel bands, 20 log10, DCT-II, startCoeff -- land on the reference's numbers to the float32 the JSON
    stores (3.6e-6 on values up to 60), on 16-bit 44.1 kHz and 24-bit 48 kHz material.  None / Full padding or startCoeff 0
    miss by 0.3 .. 240.  This is the one place where the restatements meet outputs of the reference itself; the STFT half of
    it (a1 - a5 of SURVEY 8) is the BufNMF path's own."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_corpus_mfcc_sample.npz"))
    slices, off = g["slices"], g["offsets"]
    seg = lambda j: (g["pcm24"][off[j]:off[j + 1]].astype(np.float64) / 8388608.0).astype(np.float32)
    assert set(g["source_file"].tolist()) == {0, 1, 2} and slices[0] == 0
    checked, worst = 0, 0.0
    for j in range(len(slices)):
        ref = g["expected"][j]
        got_np = _mfcc_stats(onp.bufmfcc_channel(seg(j), 1024, 1024, 512, 40, 13, 1))
        got_c = _mfcc_stats(oracle.bufmfcc_channel(seg(j), 1024, 1024, 512, 40, 13, 1))
        worst = max(worst, np.abs(got_np - ref).max(), np.abs(got_c - ref).max())
        checked += 1
    assert checked == len(slices) == 27, checked
    assert worst < 2e-5, worst
    # and the parameters are not a coincidence: slice 0 with the neighbouring choices
    ref0 = g["expected"][0]
    assert np.abs(_mfcc_stats(onp.bufmfcc_channel(seg(0), 1024, 1024, 512, 40, 13, 0)) - ref0).max() > 100      # startCoeff 0
    assert np.abs(_mfcc_stats(onp.bufmfcc_channel(seg(0), 1024, 1024, 512, 40, 13, 1, padding_mode=0)) - ref0).max() > 0.1


def test_reference_corpus_fixture_is_what_the_oracles_give(oracle, onp):
    """tests/golden/reference_corpus_mfcc.npz (tools/make_reference_mfcc_fixture.py: four slices of the corpus above with
    the reference's rows) -- the copy that travels to the GPU box -- against both oracles"""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_corpus_mfcc.npz"))
    x = (g["pcm16"].astype(np.float64) / 32768.0).astype(np.float32)
    pts = g["points"]
    for j in range(len(pts) - 1):
        seg = x[int(pts[j]):int(pts[j + 1])]
        for o in (onp, oracle):
            assert np.abs(_mfcc_stats(o.bufmfcc_channel(seg, 1024, 1024, 512, 40, 13, 1)) - g["expected"][j]).max() < 2e-5



@pytest.mark.parametrize("n,win,fft,hop,K,mode", [(3000, 256, 256, 64, 3, 1), (2500, 256, 512, 100, 2, 0),
                                                  (4100, 128, 128, 128, 4, 2), (1000, 64, 64, 96, 2, 1), (700, 255, 256, 60, 2, 1)])
def test_nmfmatch_and_nmffilter_closed_forms_against_the_literal_clients(onp, n, win, fft, hop, K, mode):
    """The users of NMF::processFrame (clients/rt/NMFMatchClient.hpp:76-118, NMFFilterClient.hpp:69-118): oracle_np holds a
    LITERAL model of each real-time client -- host vector in, host vector out, FluidSource / FluidSink rings, the output
    written before the call's frame is processed (NMFMatch), the window^2 normalisation channel (NMFFilter) -- driven the
    way the reference's offline wrappers drive a real-time client (StreamingControl with host vectors of one hop;
    Streaming with host vectors of 64 samples), and the closed forms the HIP entry points compute in one batch.  They must
    be the same floats: hop dividing the window or not, hop = window, hop > window (NMFMatch), odd window, win < fft."""
    rs = np.random.RandomState(n)
    x = onp.synth_audio(n, 5).astype(np.float32)
    bases = rs.uniform(0.01, 1, (K, fft // 2 + 1)).astype(np.float32)
    a = onp.nmfmatch_streaming_control(x, bases, win, fft, hop, 42, mode)
    b = onp.nmfmatch_channel(x, bases, win, fft, hop, 42, mode)
    assert a.shape == b.shape == (K, onp.feature_frames(n, win, hop, mode)[0]) and np.array_equal(a, b)
    if win // hop >= 1:
        assert np.any(a[:, 0] != 0)            # a frame precedes the first kept column
    else:
        assert not a[:, 0].any()               # ... or it holds the activations as constructed
    if hop <= win:
        c = onp.nmffilter_streaming(x, bases, win, fft, hop, 7, 42)
        d = onp.nmffilter_channel(x, bases, win, fft, hop, 7, 42)
        assert c.shape == d.shape == (K, n) and np.array_equal(c, d)
        if hop < win and win % hop == 0:
            assert np.abs(c.sum(axis=0) - x).max() < 1e-5   # the masks add up to one: the components add up to the input
    # a maxComponents below the buffer's channel count takes the first components only (:93)
    a2 = onp.nmfmatch_streaming_control(x, bases, win, fft, hop, 42, mode, max_rank=1)
    assert a2.shape[0] == 1 and np.array_equal(a2, onp.nmfmatch_channel(x, bases[:1], win, fft, hop, 42, mode))


@pytest.mark.parametrize("faithful", [False, True])
def test_update_arithmetic_against_scikit_learns_multiplicative_updates(oracle, onp, faithful):
    """The NMF arithmetic has no reference-held answer (tests/algorithms/public/TestNMF.cpp:11-46 asserts determinism only,
    and alg/NMF.hpp needs Eigen to compile).  A third implementation by an unrelated party stands in as a cross-check of
    the two update formulas: scikit-learn's `_multiplicative_update_w / _h` with beta_loss = 1 are the KL multiplicative
    updates of alg/NMF.hpp:158-161 and :165-170 (numerator (V / WH) H^T over the row sums of H; W^T (V / WH) over the
    column sums of W).  Driven from the oracle's own start (libstdc++ RNG, clamp, normalise: :149-153) in the reference's
    order -- W update, column-normalise W (:162), H update with the new W -- they must land where both oracles land.
    scikit-learn clamps WH at float32 epsilon where the reference clamps at double epsilon, so the input is strictly
    positive and no clamp is active; what is left is summation order."""
    nmf = pytest.importorskip("sklearn.decomposition._nmf")
    rs = np.random.RandomState(11)
    T, F, K, iters = 60, 33, 5, 40
    X = np.abs(rs.standard_normal((T, F))) + 0.05                # [T, F] as the oracles take it
    W1, H1, V1, rc = oracle.nmf_process(X, K, iters, True, True, 42, faithful=faithful)
    assert rc == 0
    Wn, Hn, Vn = onp.nmf_process(X, K, iters, seed=42)
    # the same start as oracle_np.nmf_process (alg/NMF.hpp:118-153)
    W = onp.rng_uniform01(42, F * K).reshape(K, F).T.copy()
    H = onp.rng_uniform01(42, K * T).reshape(T, K).T.copy()
    W = np.maximum(W, onp.EPS); H = np.maximum(H, onp.EPS)
    W = W / np.sqrt((W * W).sum(axis=0, keepdims=True))
    H = H / np.sqrt((H * H).sum(axis=1, keepdims=True))
    V = X.T.copy()                                                # F x T = W (F x K) H (K x T)
    for _ in range(iters):
        W = nmf._multiplicative_update_w(V, W, H, beta_loss=1, l1_reg_W=0, l2_reg_W=0, gamma=1.0)[0]
        W = W / np.sqrt((W * W).sum(axis=0, keepdims=True))
        H = nmf._multiplicative_update_h(V, W, H, beta_loss=1, l1_reg_H=0, l2_reg_H=0, gamma=1.0)
    assert (W @ H).min() > 1e-4                                   # no clamp of either implementation was ever near
    for got_w, got_h in ((W1, H1), (Wn, Hn)):
        assert rel_err(got_w, W.T) < 1e-11
        assert rel_err(got_h, H.T) < 1e-11
    assert rel_err(V1, (W @ H).T) < 1e-11
