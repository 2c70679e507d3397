"""CPU tests of tests/stft_ref.py, and the derivation of the bars tests/test_gpu_stft.py holds the forward STFT to, frame by
frame:

  STFT_BAR[fft]    8 x the larger of the distances (stft_ref.frame_err: every frame relative to its own peak, spectrum and
                   magnitudes alike) from the long double restatement of two independent float64 transforms -- numpy's rfft
                   and the C oracle's hand-rolled FFT -- on the inputs the GPU file runs (dynamics and tones, as float32 and
                   as float64), at every fft size the GPU file uses.  The factor 8 is the one the NMF, frames and resynthesis
                   files give a float64 implementation over its own floor.  Nothing is added for float32 input: the samples
                   are exact in double and the comparison is of doubles.

What the measure buys is shown on deliberate breaks of a float64 numpy STFT (built here, nothing committed as a kernel): each
misses STFT_BAR under frame_err, and for each the old measure -- max |a - b| / max |b| over the spectrogram < 1e-12 -- is
recorded.  Rounding one pass's twiddles to float32 in the quietest tenth of the frames PASSES the old bar (2e-13) and misses
the new one by seven decades; stale padding columns of the bin-major copy are seen by no read-out the old tests had.

The shape table of the GPU file is pinned to K1's dispatch: block form, generic kernel with each LDS variant, global-memory
passes, a second round of a workgroup, the prefetched-samples path -- from the launchers' own arithmetic restated in
stft_ref.py, so that a change of a launcher that moves a shape out of its branch fails here, on the CPU.
"""
import functools

import numpy as np
import pytest

import oracle_np
import stft_ref as R

OLD_BAR = 1e-12
# How a bar follows from the figures (test_the_bars_cover_the_measured_floor recomputes them and prints every one): 8 x the
# worst frame_err of the two float64 transforms at that size, plus 3 % for another libm / pocketfft build, rounded up to two
# digits.  Measured (numpy rfft / C oracle, worst of spectrum and magnitudes over the four inputs):
#   fft     4  1.71e-16 / 1.44e-16       8  2.14e-16 / 1.98e-16      16  2.30e-16 / 2.84e-16      32  2.19e-16 / 4.22e-16
#          64  3.53e-16 / 5.41e-16     128  3.01e-16 / 4.94e-16     256  2.99e-16 / 6.77e-16     512  3.62e-16 / 6.10e-16
#        1024  3.20e-16 / 7.60e-16    2048  3.80e-16 / 6.84e-16    4096  4.13e-16 / 8.69e-16    8192  3.77e-16 / 9.13e-16
#       16384  3.59e-16 / 9.63e-16   32768  4.21e-16 / 1.02e-15   65536  3.94e-16 / 9.87e-16
# (numpy's pocketfft sits at 2 - 4e-16 at every size; the C oracle's radix-2 passes grow with log2 of the size and set the bar)
STFT_BAR = {4: 1.5e-15, 8: 1.8e-15, 16: 2.4e-15, 32: 3.5e-15, 64: 4.5e-15, 128: 4.1e-15, 256: 5.6e-15, 512: 5.1e-15, 1024: 6.3e-15,
            2048: 5.7e-15, 4096: 7.2e-15, 8192: 7.6e-15, 16384: 8.0e-15, 32768: 8.5e-15, 65536: 8.2e-15}
HEADROOM = 1.03
FLOAT32_ULP = 2.0 ** -24       # BufSTFT writes float32: one rounding of a double within STFT_BAR of the reference


def round_up_two_digits(x):
    e = int(np.floor(np.log10(x))) - 1
    return float(f"{np.ceil(x / 10.0 ** e * (1 - 1e-12)) * 10.0 ** e:.1e}")


def floor_inputs(fft):
    """[(name, x, win, hop)] the bar of `fft` is measured on: both families, float32 and float64, a handful of frames (the
    C oracle transforms every frame of what it is given)"""
    hop = max(1, fft // 4)
    n = R.n_for(9 if fft <= 8192 else 4, hop)
    return [(f"{fam} {dt}", R.INPUTS[fam](n, 100 + fft % 97, dt), fft, hop) for fam in ("dynamics", "tones") for dt in ("float32", "float64")]


@functools.lru_cache(maxsize=None)
def measured_floor(fft):
    """(numpy rfft, C oracle): the worst frame_err of either float64 transform from the long double restatement"""
    import oracle_c
    oc = oracle_c.get("native")
    worst = [0.0, 0.0]
    for name, x, win, hop in floor_inputs(fft):
        ref = R.stft_ld(x, win, fft, hop)
        for i, got in enumerate((R.stft_f64(x, win, fft, hop), oc.stft(x.astype(np.float64), win, fft, hop))):
            worst[i] = max(worst[i], R.frame_err(got[0], ref[0])[0], R.frame_err(got[1], ref[1])[0])
    return tuple(worst)


# ---- the bars ----------------------------------------------------------------------------------------------------------------
def test_the_bars_cover_the_measured_floor():
    assert sorted(STFT_BAR) == R.all_fft_sizes()
    for fft in sorted(STFT_BAR):
        a, b = measured_floor(fft)
        want = round_up_two_digits(8 * max(a, b) * HEADROOM)
        print(f"fft {fft}: numpy rfft {a:.2e}, C oracle {b:.2e}, x 8 + 3 % rounded up {want:.1e} (bar {STFT_BAR[fft]:.1e})")
        assert 8 * max(a, b) <= STFT_BAR[fft] <= 1.25 * want, (fft, a, b)       # covers, and is not looser than the rule
        assert STFT_BAR[fft] < 1e-14


# ---- the restatement against the oracles, the goldens and numpy ------------------------------------------------------------------
GEOMETRIES = [(5000, 1024, 1024, 256), (4999, 512, 1024, 256), (3000, 301, 512, 75), (700, 64, 64, 16), (1, 64, 64, 16), (31, 64, 64, 16)]


@pytest.mark.parametrize("n,win,fft,hop", GEOMETRIES)
def test_against_both_oracles_and_numpy(oracle, n, win, fft, hop):
    x = R.dynamics(n, 3)
    spec, mag = R.stft_ld(x, win, fft, hop)
    T = R.num_frames(n, hop)
    assert spec.shape == mag.shape == (T, fft // 2 + 1) and T == oracle.num_frames(n, win, hop)
    assert not spec[:, 0].imag.any() and not spec[:, -1].imag.any()            # DC and Nyquist purely real
    for name, (s, m) in (("oracle_np", oracle_np.stft(x, win, fft, hop)), ("C oracle f32", oracle.stft_f32(x, win, fft, hop)),
                         ("C oracle", oracle.stft(x.astype(np.float64), win, fft, hop))):
        old = max(R.rel_err(s, spec), R.rel_err(m, mag))
        new = max(R.frame_err(s, spec)[0], R.frame_err(m, mag)[0])
        print(f"{name} {n} {win} {fft} {hop}: old measure {old:.2e}, frame by frame {new:.2e}")
        assert old < OLD_BAR and new <= STFT_BAR[fft]
    # numpy's rfft of the SAME windowed frames, under the new measure
    fr = R.frames_of(x, win, fft, hop, np.arange(T), dtype=np.float64)
    s = np.fft.rfft(fr, axis=1)
    assert R.frame_err(s[:, 1:-1], spec[:, 1:-1])[0] <= STFT_BAR[fft] and R.frame_err(np.abs(s), mag)[0] <= STFT_BAR[fft]


@pytest.mark.parametrize("wfh", [(1024, 1024, 512), (2048, 2048, 512), (512, 1024, 256)])
def test_against_the_committed_goldens(golden, wfh):
    win, fft, hop = wfh
    sig, key = golden["g2_signal"], f"g2_{win}_{fft}_{hop}"
    rows = golden[key + "_rows"]
    spec, mag = R.stft_ld(sig, win, fft, hop, frames=rows)
    assert R.num_frames(len(sig), hop) == int(golden[key + "_T"][0])
    assert R.rel_err(golden[key + "_spec"], spec) < OLD_BAR and R.rel_err(golden[key + "_mag"], mag) < OLD_BAR
    assert R.frame_err(golden[key + "_spec"], spec)[0] <= STFT_BAR[fft] and R.frame_err(golden[key + "_mag"], mag)[0] <= STFT_BAR[fft]


def test_the_window_tables_and_the_framing():
    assert np.abs(R.window(0, 1024) - oracle_np.hann(1024)).max() <= 2.0 ** -52
    assert np.abs(R.window(0, 1023) - oracle_np.hann(1023)).max() <= 2.0 ** -52
    assert R.window(0, 8)[0] == 0 and R.window(2, 8)[0] == pytest.approx(0.08) and R.window(4, 7)[3] == 1.0
    assert R.window(3, 8)[0] == pytest.approx(0.35875 - 0.48829 + 0.14128 + 0.01168)
    # a named subset of frames is those frames of the whole
    x = R.tones(3001, 5)
    whole = R.stft_ld(x, 256, 256, 64)[0]
    assert np.array_equal(R.stft_ld(x, 256, 256, 64, frames=[0, 7, 46])[0], whole[[0, 7, 46]])
    # BufSTFT's three padding modes: frame counts and offsets of oracle_np.bufstft_forward
    for mode in (0, 1, 2):
        for n, win, fft, hop in R.BUFSTFT_SHAPES:
            T, off = R.bufstft_geometry(n, win, hop, mode)
            m32 = oracle_np.bufstft_forward(R.dynamics(n, 9), win, fft, hop, mode)[0]
            assert m32.shape == (fft // 2 + 1, T) and off == -oracle_np.bufstft_padding(win, hop, mode)
            mag = R.stft_ld(R.dynamics(n, 9), win, fft, hop, offset=off, T=T)[1]
            assert R.frame_err(m32.T.astype(np.float64), mag)[0] <= FLOAT32_ULP + STFT_BAR[fft]
    # a window shorter than the transform is zero padded at its tail; one sample gives one frame with its sample at win / 2
    fr = R.frames_of(np.ones(1, dtype=np.float32), 6, 8, 4, [0], dtype=np.float64)
    assert R.num_frames(1, 4) == 1 and np.array_equal(fr[0], [0, 0, 0, R.window(0, 6)[3], 0, 0, 0, 0])


def test_the_inputs_are_what_they_claim():
    n, win, hop = 40000, 1024, 256
    for dt in ("float32", "float64"):
        x = R.dynamics(n, 1, dt)
        assert x.dtype == np.dtype(dt)
        peak = np.abs(R.stft_f64(x, win, win, hop)[0]).max(axis=1)
        assert peak.min() > 0 and peak[-3] / peak[2] > 1e5                 # every frame at a scale of its own, six decades
        assert len(np.unique(np.round(np.log10(peak), 2))) > len(peak) // 2
        y = R.tones(n, 1, dt)
        m = R.stft_f64(y, win, win, hop)[1][5:-5]
        assert (m.max(axis=1) / np.median(m, axis=1)).min() > 300           # peaks well above the floor
    assert R.dynamics(1, 1).shape == (1,) and R.dynamics(1, 1)[0] != 0


def test_frame_err_exempts_nothing():
    ref = np.array([[1.0, 2.0], [1e-30, 3e-30], [0.0, 0.0]])
    assert R.frame_err(ref, ref) == (0.0, 0)
    got = ref.copy()
    got[1, 0] = 2.5e-30                          # the old measure reads 7.5e-31
    assert R.frame_err(got, ref) == (pytest.approx(0.5), 1) and R.rel_err(got, ref.astype(R.LD)) < 1e-30
    got = ref.copy()
    got[2, 1] = 1e-300
    with pytest.raises(AssertionError):
        R.frame_err(got, ref)                    # not zero where the reference is exactly zero
    spec = np.array([[3 + 4j, 0j, 1e-200 + 0j]])
    assert R.mag_of_spec_err(np.array([[5.0, 0.0, 1e-200]]), spec) == 0.0
    assert R.mag_of_spec_err(np.array([[5.0 * (1 + 2.0 ** -50), 0.0, 1e-200]]), spec) > R.MAG_OF_SPEC_BAR
    with pytest.raises(AssertionError):
        R.mag_of_spec_err(np.array([[5.0, 1e-154, 1e-200]]), spec)


# ---- what the measure buys: deliberate breaks of a float64 STFT ------------------------------------------------------------------
BREAK = dict(n=40000, win=1024, fft=1024, hop=256)


def numpy_stft(x, win, fft, hop, frames_hook=None, fft_hook=None):
    T = R.num_frames(len(x), hop)
    fr = R.frames_of(x, win, fft, hop, np.arange(T), dtype=np.float64)
    if frames_hook is not None:
        fr = frames_hook(fr)
    spec = np.fft.rfft(fr, axis=1) if fft_hook is None else fft_hook(fr)
    spec[:, 0] = spec[:, 0].real
    spec[:, -1] = spec[:, -1].real
    return spec


def fft_r2_f64(fr, stage32=None, rows=None):
    """stft_ref.fft_ld's passes at float64; pass `stage32`'s twiddles rounded to float32 in the frames `rows`"""
    M, N = fr.shape
    tw = R._twiddles_ld(N).astype(np.complex128)
    X = fr.astype(np.complex128)[:, R._bitrev(N)]
    size, stage = 2, 0
    while size <= N:
        w = tw[:: N // size]
        wb = np.broadcast_to(w, (M, len(w))).copy()
        if stage == stage32:
            wb[rows] = w.astype(np.complex64).astype(np.complex128)
        X = X.reshape(M, N // size, 2, size // 2)
        o = X[:, :, 1, :] * wb[:, None, :]
        X = np.concatenate([X[:, :, 0, :] + o, X[:, :, 0, :] - o], axis=-1)
        size, stage = size * 2, stage + 1
    return X.reshape(M, N)[:, :N // 2 + 1].copy()


def test_the_measure_sees_what_the_old_one_cannot():
    n, win, fft, hop = (BREAK[k] for k in ("n", "win", "fft", "hop"))
    x = R.dynamics(n, 11)
    T = R.num_frames(n, hop)
    ref = R.stft_ld(x, win, fft, hop)[0]
    good = numpy_stft(x, win, fft, hop)
    assert R.frame_err(good, ref)[0] <= STFT_BAR[fft] and R.frame_err(fft_r2_f64(R.frames_of(x, win, fft, hop, np.arange(T), dtype=np.float64))[:, 1:-1], ref[:, 1:-1])[0] <= STFT_BAR[fft]
    quiet = np.arange(T) < T // 10                                            # the envelope rises: the first tenth

    def neighbour(fr):
        fr = fr.copy()
        fr[6] = fr[7]                                                         # a quiet frame from its neighbour's samples
        return fr

    def short_hi(fr):
        fr = fr.copy()
        last = n - 1 - ((T - 1) * hop - win // 2)                             # the last valid sample of the last frame
        assert fr[T - 1, last] != 0 and not fr[T - 1, last + 1:].any()
        fr[T - 1, last] = 0.0
        return fr

    def swapped_pair(fr):
        w = R.window(0, win)
        m = 2 * 137                                                           # the two window values of one point swapped
        raw = fr[:, [m, m + 1]] / w[[m, m + 1]]
        fr = fr.copy()
        fr[:, m], fr[:, m + 1] = raw[:, 0] * w[m + 1], raw[:, 1] * w[m]
        return fr

    breaks = {
        "a quiet frame from its neighbour's samples": numpy_stft(x, win, fft, hop, frames_hook=neighbour),
        "the last sample of the last frame dropped": numpy_stft(x, win, fft, hop, frames_hook=short_hi),
        "a pair of window values swapped": numpy_stft(x, win, fft, hop, frames_hook=swapped_pair),
        "one pass's twiddles at float32 in the quiet frames": numpy_stft(x, win, fft, hop, fft_hook=lambda fr: fft_r2_f64(fr, 5, quiet)),
    }
    old_passes = {}
    for name, got in breaks.items():
        new, t = R.frame_err(got, ref)
        old = R.rel_err(got, ref)
        old_passes[name] = old < OLD_BAR
        print(f"{name}: frame by frame {new:.2e} at frame {t} (bar {STFT_BAR[fft]:.1e}); old measure {old:.2e}: "
              f"{'PASSES' if old_passes[name] else 'fails'} 1e-12")
        assert new > STFT_BAR[fft], name
        assert R.frame_err(np.abs(got), np.abs(ref))[0] > STFT_BAR[fft], name   # ... and in the magnitudes alike
    assert old_passes["one pass's twiddles at float32 in the quiet frames"]
    # the padding columns of the bin-major copy left non-zero: no read-out of the old tests returns them
    mag = np.abs(good)
    F, Tp, Fp = fft // 2 + 1, -(-T // 32) * 32, -(-(fft // 2 + 1) // 32) * 32
    magT = np.zeros((1, Fp, Tp))
    magT[0, :F, :T] = mag.T
    lay = np.zeros((1, Tp, Fp))
    lay[0, :T, :F] = mag
    R.check_layouts(lay, magT, [T], F)
    stale = magT.copy()
    stale[0, 5, T] = 1e-9
    with pytest.raises(AssertionError):
        R.check_layouts(lay, stale, [T], F)
    off = magT.copy()
    off[0, 7, 3] = np.nextafter(off[0, 7, 3], 1.0)
    with pytest.raises(AssertionError):
        R.check_layouts(lay, off, [T], F)


# ---- the GPU shapes reach the branches they are meant to -----------------------------------------------------------------------
def test_the_restated_constants_are_the_launchers():
    """stft_ref.dispatch restates the launchers' arithmetic; the constants it restates are read here from the launchers' text, so
    that a change there fails on the CPU before a GPU shape silently leaves its branch"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flucoma-core_amd", "csrc")
    block = open(os.path.join(csrc, "kernels_stft_block.hip")).read()
    generic = open(os.path.join(csrc, "kernels_stft.hip")).read()
    core = open(os.path.join(csrc, "fft_core.h")).read()
    # the production instantiations: R1, R2, R3, NW, WINLDS (, FPW, DB)
    prod = re.sub(r"#ifdef FLUHIP_AB_SWITCHES.*?#endif", "", block, flags=re.S)
    inst = re.findall(r"return launch_block_t<([\d, a-z]+)>\(k, s\);", prod)
    assert inst == ["16, 8, 8, 8, 0, 2", "16, 8, 8, 8, 0, 1, true", "16, 8, 8, 8, 1", "16, 8, 16, 4, 1", "8, 8, 8, 16, 1"], inst
    assert "if (db == 1 && magT) return launch_block_t<16, 8, 8, 8, 0, 1, true>" in prod and "if (fpw == 2)" in prod
    assert {f: v[:4] for f, v in R.BLOCK_FORMS.items()} == {2048: (16, 8, 8, 8), 4096: (16, 8, 16, 4), 1024: (8, 8, 8, 16)}
    for text in ("((size_t) Core::TW + (WINLDS ? Core::N : 0)) * 16 + (size_t) (DB ? 2 : 1) * NW * FPW * Core::BUFD * 8",
                 "const int perCu = (int) ((160 * 1024) / shmem);", "const int64_t cap = 256 * (int64_t) (perCu < 1 ? 1 : perCu);",
                 "const int64_t chunk = (k.totalBlocks + 7) / 8;", "int64_t grid = 8 * chunk;",
                 "k.blocksPerBuf = (k.T + NW * FPW - 1) / (NW * FPW);", "const int64_t blk = (L & 7) * chunk + slot;",
                 "constexpr bool PREFETCH = FPW == 1 && PPL == 16 && NW <= 12;"):
        assert text in block, text
    for text in ("static constexpr int BUFD = N + N / 16 + (XL ? 34 : 2);", "static constexpr int T2 = (R2 - 1) * NS2, T3 = (R3 - 1) * NS3, TW = T2 + T3;",
                 "static constexpr bool XL = FLUHIP_SPLIT_VIA_LDS != 0 && NB3 == 1;",
                 "return (win % 2) == 0 && win <= fft && (fft == 1024 || fft == 2048 || fft == 4096);"):
        assert text in core, text
    for text in ("return ((twInLds ? 3 : 2) * nc * 2 + (winInLds ? (size_t) win : 0)) * sizeof(double);",
                 "return stft_lds_bytes(win, fft, false, false) > 160 * 1024;",
                 "k.twInLds = stft_lds_bytes(a.win, a.fft, true, false) <= 160 * 1024 ? 1 : 0;",
                 "k.winInLds = (k.twInLds && stft_lds_bytes(a.win, a.fft, true, true) <= 80 * 1024) ? 1 : 0;",
                 "const int64_t cap = 256 * 8;", "int64_t cf = std::max<int64_t>(1, ((int64_t) 512 << 20) / perFrame);",
                 "const int radix = (nc / Ns >= 4) ? 4 : 2;"):
        assert text in generic, text


def test_the_shapes_reach_every_branch():
    # block form, one buffer: one block minus one, exactly one, plus one, two and a half
    assert {f: R.block_T(f) for f in R.BLOCK_FFTS} == {1024: (15, 16, 17, 40), 2048: (7, 8, 9, 20), 4096: (3, 4, 5, 10)}
    for fft in R.BLOCK_FFTS:
        for magT in (False, True):
            d = R.dispatch(fft, fft, 1, R.block_T(fft)[3], magT)
            assert d["branch"] == "block" and d["rounds"] == 1 and d["cap"] == 256 and d["FPB"] == {1024: 16, 2048: 8, 4096: 4}[fft]
            assert d["DB"] == (fft == 2048 and magT) and d["WINLDS"] != d["DB"] and d["PREFETCH"] == (fft == 2048)
        win = R.SHORT_EVEN_WINDOWS[fft]
        assert win % 2 == 0 and win < fft and R.dispatch(win, fft, 1, 9)["branch"] == "block"
    assert {f: R.block_form(f, f, True)["shmem"] for f in R.BLOCK_FFTS} == {1024: 90240, 2048: 155648, 4096: 134976}
    assert R.block_form(2048, 2048, False)["shmem"] == 102272
    # generic kernel: the powers of two without a block form, and the odd windows with each LDS variant
    assert sorted(f for _, f, _ in R.GENERIC_POW2) == [4, 8, 16, 32, 64, 128, 256, 512, 8192]
    for win, fft, hop in R.GENERIC_POW2 + R.GENERIC_ODD:
        d = R.dispatch(win, fft, 1, 9)
        assert d["branch"] == "generic" and not d["strided"], (win, fft)
        if fft >= 1024:
            assert (d["twInLds"], d["winInLds"]) == R.GENERIC_LDS[fft], (win, fft, d)
    assert [w % 2 for w, _, _ in R.GENERIC_ODD] == [1, 1, 1, 1]
    assert {(R.dispatch(f, f, 1, 9)["twInLds"], R.dispatch(f, f, 1, 9)["winInLds"]) for _, f, _ in R.GENERIC_POW2 if f <= 512} == {(True, True)}
    assert {(f.bit_length() - 1) % 2 for _, f, _ in R.GENERIC_POW2} == {0, 1}                 # odd and even log2: with and without a radix-2 pass
    win, fft, hop, T = R.GENERIC_STRIDE_CASE
    d = R.dispatch(win, fft, 1, T)
    assert d["branch"] == "generic" and d["strided"] and d["grid"] == 2048 < T
    # global-memory passes; 32768 ends in a radix-2 pass; one case across the chunk boundary
    # (a radix-2 last pass where log2(fft / 2) is odd: 16384 and 65536; 32768 is radix 4 throughout)
    assert {f: R.dispatch(f, f, 1, R.BIG_T)["last_radix"] for f in R.BIG_FFTS} == {16384: 2, 32768: 4, 65536: 2}
    for f in R.BIG_FFTS:
        d = R.dispatch(f, f, 1, R.BIG_T)
        assert d["branch"] == "big" and d["chunks"] == 1
    win, fft, hop, n = R.CHUNK_CASE
    d = R.dispatch(win, fft, 1, R.num_frames(n, hop))
    assert R.num_frames(n, hop) == 1032 and d["chunk_frames"] == 1024 and d["chunks"] == 2
    named = R.chunk_frames_named()
    assert {0, 3, 1020, 1023, 1024, 1028, 1028, 1031, 64, 960} <= set(named) and len(named) < 40
    # corpora in one round: three buffers, a ragged last block, odd n
    for fft in R.BLOCK_FFTS:
        B, n, win, _, hop = R.corpus_one_round(fft)
        T = R.num_frames(n, hop)
        d = R.dispatch(win, fft, B, T, True, True, n, hop)
        assert B == 3 and n % 2 == 1 and T % d["FPB"] not in (0,) and d["rounds"] == 1 and d["prefetched"] == 0
    # more than one round: the staging sets alternate, and at fft 2048 the prefetched samples are used
    blocks = {2048: (264, 270), 1024: (260, 260), 4096: (260, 260)}
    for fft, cases in R.MULTI_ROUND.items():
        for i, (B, n, win, _, hop) in enumerate(cases):
            T = R.num_frames(n, hop)
            d = R.dispatch(win, fft, B, T, True, True, n, hop)
            assert d["branch"] == "block" and len(d["dealing"]) == blocks[fft][i] > d["cap"] and d["rounds"] == 2
            assert (hop % 2, n % 2) == ((0, 0), (1, 1))[i]
            assert (d["prefetched"] > 0) == (fft == 2048), (fft, i, d["prefetched"])
            picked = R.round_blocks(d["dealing"])
            assert len(picked) == 4 and len(set(picked)) == 4
            # every block of every buffer is dealt exactly once
            assert sorted((b, t0) for _, _, b, t0 in d["dealing"]) == [(b, t0) for b in range(B) for t0 in range(0, T, d["FPB"])]
    # at fft 2048 with an odd hop the frames alternate between the prefetched and the clamped gather
    B, n, win, fft, hop = R.MULTI_ROUND[2048][1]
    d = R.dispatch(win, fft, B, R.num_frames(n, hop), True, True, n, hop)
    in_round_two = sum(min(d["FPB"], R.num_frames(n, hop) - t0) for r, _, _, t0 in d["dealing"] if r == 1)
    assert 0 < d["prefetched"] < in_round_two
    # ragged corpora: one sample, below one hop, one block exactly, the longest
    for fft in R.BLOCK_FFTS:
        lens, hop, fpb = R.ragged_lengths(fft), fft // 4, R.BLOCK_FORMS[fft][3]
        assert lens[0] == 1 and lens[1] < hop and R.num_frames(lens[2], hop) == fpb and max(lens) == lens[3]
        assert [R.num_frames(v, hop) for v in lens[:2]] == [1, 1]
    # shapes without a block form
    assert [R.dispatch(w, f, B, R.num_frames(n, h), True)["branch"] for B, n, w, f, h in R.NO_BLOCK_CORPORA] == ["generic"] * 3 + ["big"]
    assert [R.dispatch(w, f, 1, 21)["branch"] for _, w, f, _ in R.BUFSTFT_SHAPES] == ["block", "generic"]


def test_the_frames_outside_the_buffer_reach_every_form_and_every_edge():
    """the shape table of test_gpu_stft.py's frames outside their buffer: every kernel form is met, the frames run from more than
    two transforms before the buffer to at least one behind it, and the shifts put a frame on each edge -- s0 = -fft (no sample of
    the buffer) and -fft + 1 (one) in front, n - 1 (one) and n (none) behind -- with the guards reaching past every frame"""
    forms = {}
    for win, fft, dtypes in R.OUTSIDE_CASES:
        for odd_hop in (False, True):
            n, hop, frame0, T, guard = R.outside_geometry(fft, odd_hop, 0)
            assert n == fft + fft // 2 + 5 and hop == fft // 4 - odd_hop and frame0 == -(2 * fft + hop) and 20 <= T <= 26
            d = R.dispatch(win, fft, R.OUTSIDE_B, T, False, True, n, hop)
            forms.setdefault(d["branch"], set()).add((win, fft))
            starts = R.outside_starts(fft, odd_hop)
            assert {-fft, -fft + 1, n - 1, n} <= starts, (win, fft, odd_hop)
            assert min(starts) < -2 * fft and max(starts) >= n + fft
            assert {-1, 0, 1} <= set(R.outside_shifts(fft, odd_hop)) and len(R.outside_shifts(fft, odd_hop)) <= 7
            for sh in R.outside_shifts(fft, odd_hop):
                n, hop, frame0, T, guard = R.outside_geometry(fft, odd_hop, sh)
                assert guard >= -frame0 + fft and guard >= frame0 + (T - 1) * hop + fft - n + fft
            # frames wholly inside, on even and odd bases: the float gather's aligned and clamped interior paths both
            inside = [s for s in starts if 0 <= s and s + fft <= n]
            assert {s % 2 for s in inside} == {0, 1}
        assert dtypes == (("float32",) if fft > 8192 else ("float32", "float64"))
    assert forms["block"] == {(f, f) for f in R.BLOCK_FFTS} | {(R.SHORT_EVEN_WINDOWS[f], f) for f in R.BLOCK_FFTS}
    assert forms["generic"] == {(64, 64), (1023, 1024), (8192, 8192)} and forms["big"] == {(16384, 16384)}
    assert all(f in STFT_BAR for _, f, _ in R.OUTSIDE_CASES)
