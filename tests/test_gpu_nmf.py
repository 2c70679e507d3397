"""GPU tests of the whole NMF update loop -- fluhip_nmf_process_f64 on one buffer of doubles, fluhip_corpus_nmf on corpora of
float audio -- ENTRY BY ENTRY against tests/nmf_ref.py.

The loop carries state from launch to launch (the deferred normalisation, the side column's partials, the column sums a W
update leaves for the H update, split contractions, work lists, the progress-lag window), and an error there lands in one
bin, one component or one buffer's last frames: the only error measure is nmf_ref.elrel -- every entry of W1 and H1 relative
to ITSELF, exact zeros where the reference has exact zeros, no entry exempted -- and every buffer of every corpus is
compared.  The bars are derived on the CPU (tests/test_nmf_ref.py): 8 x what the device's documented quotient (relative
error <= 2^-46) and float64's own rounding cost on the reference, one set per input family -- NMF_BAR[iterations] for one
buffer of doubles, NMF_BAR_AUDIO[iterations] for corpora of audio, whose sparser factors cost more -- and every quotient
times (1 + 2^-40) misses them at every input.  Audio runs up to 10 iterations: at 30, float64 itself is 7.2e-13 from long
double on it and no bar 8 x above that could refuse what a quotient error of 2^-40 costs (9.1e-13).  The shapes reach every regime of the
planner (test_nmf_ref.py asserts which); every test prints what it measures (rowrel: W per component / per bin, H per frame
/ per component, each relative to its own peak, for context).

Measured on an MI355X when the file was written (elrel of W1 / of H1 / of V1; every test prints its own):
  one buffer, 10 iterations, bar 3.3e-13 (T x F x K):
    87x129x3 5.1e-15 / 3.5e-15 / 2.7e-15, 33x100x16 7.3e-15 / 6.7e-15 / 1.7e-15, 1040x3x2 7.0e-16 / 2.1e-15 / 2.2e-15,
    12288x33x3 3.7e-15 / 8.6e-15 / 3.9e-15, 12289x33x3 6.2e-15 / 6.4e-15 / 5.4e-15, 33x33x32 4.3e-15 / 4.5e-15 / 1.2e-15,
    87x33x128 2.6e-15 / 5.3e-15 / 1.5e-15, 173x33x20 3.3e-15 / 4.3e-15 / 1.2e-15, 1x513x32 3.0e-15 / 5.8e-15 / 1.7e-15,
    31x513x32 9.2e-15 / 7.4e-15 / 2.1e-15, 32x513x32 9.7e-15 / 9.9e-15 / 2.6e-15, 33x513x32 1.1e-14 / 9.2e-15 / 2.0e-15,
    4200x33x32 2.4e-15 / 4.8e-15 / 1.1e-15, 87x129x130 4.5e-15 / 3.8e-15 / 1.3e-15; 33x100 at ranks 17, 24, 25, 32, 33, 40,
    41, 64, 65, 128: 2.6e-15 .. 6.4e-15 / 3.7e-15 .. 5.5e-15 / 1.2e-15 .. 1.8e-15
  corpora, 10 iterations, bar 7.0e-13, the worst buffer (W1 / H1): 512x87x257x32 5.4e-14 / 8.0e-14, 128x257x129x100 3.5e-14 / 3.2e-14,
    8x173x513x32 5.7e-14 / 6.6e-14, 8x173x513x20 4.7e-14 / 3.3e-14, 512x87x129x100 6.2e-14 / 1.0e-13, 2x87x129x200 6.4e-15 /
    7.4e-15; the ragged corpus 2.0e-14 / 2.7e-14 at rank 5, 2.7e-14 / 2.6e-14 at rank 32
  iteration counts (strip 87x129x3, uniform 33x33x32, work lists 8x173x513x20; the larger of W1 and H1):
    0 (bars 2.7e-15 doubles, 8.2e-15 audio): 4.4e-16, 4.3e-16, 1.1e-15;  1 (1.4e-13, 1.4e-13): 1.2e-15, 1.4e-15, 4.2e-15;
    2 (1.4e-13, 1.4e-13): 1.4e-15, 1.7e-15, 6.1e-15;  7 (1.7e-13, 4.6e-13): 4.3e-15, 2.9e-15, 2.3e-14;
    8 (2.3e-13, 4.6e-13): 4.2e-15, 3.4e-15, 2.9e-14;  9 (2.4e-13, 6.3e-13): 5.0e-15, 4.3e-15, 4.0e-14;
    30 (7.0e-13, doubles only): 3.1e-14, 1.4e-14 -- with a callback the same figures to the last digit
  a fixed factor: 0 .. 2.0e-15 of the normalised seed (bar 1.4e-13); cancelled at 5: 2.5e-15 / 2.2e-15
  -- on doubles the device sits where the float64 reference sits against its own long double form; on audio both sit
  higher (entries that decayed many decades under their frame's peak), the device no higher than the reference (run once at
  30 iterations, before that count was dropped for audio: 7.2e-13, the reference's own distance from long double).
  The writeback: every base is the float32 rounding of the device's own double, every activation within one rounding.

What the file catches -- five deliberate breaks, each built once in a scratch copy (none committed), the break in the fourth
iteration of a call where it is one of sequencing; beside each what max|a - b| / max|b|, the measure of the 1e-9 assertions of
test_gpu_parity.py, reads on the same run:
  the side column's partials of one H update not handed to the W update behind it (it reads the generation before):
    test_one_buffer_every_entry[1x33x33x32] and nine more fail -- W1's last bin is off by 7.3e-2 of itself, H1 by 2.2e-11;
    of the peak that is 1.3e-11 and 9.6e-13, a pass at 1e-9.  test_ragged_corpus_many_buffers_whole_contractions and
    test_corpus_side_column_wide_ranks still pass; test_two_launch_iteration_at_every_strip_width, whose audio has a loud
    enough last bin, fails too
  the column sums of W' not left in the H update's denominator slots, the H update told they are (ranks 105 .. 128):
    test_one_buffer_every_entry[1x87x33x128] and [1x33x100x128] fail (H1 off by 0.8); gross, test_gpu_parity.py sees it too
  the last 16 bins of one W update left out: 49 tests here fail (W1 off by 0.1 .. 0.4); gross, 89 existing tests fail too
  the Newton step of the shared reciprocal dropped in the MFMA update kernels: every MFMA shape here fails at 1.9e-8 .. 5.3e-8;
    of the peak 5e-9 .. 1.7e-8, so the 1e-9 bar sees it as well, by a factor of ten (the strip kernel was left whole and passes)
  the deferred normalisation never applied at the end: the unit-norm assertion and elrel of W1 fail everywhere (1e-2 .. 9e-2),
    as do the existing tests
  -- four of the five are too coarse to need this file; the side column on a quiet Nyquist bin is what only it sees.
"""
import numpy as np
import pytest

import nmf_ref as R
import oracle_np
from test_nmf_ref import NMF_BAR, NMF_BAR_AUDIO

pytestmark = pytest.mark.gpu


def check(got, want, iters, label, bars=None):
    """elrel of W1, H1 (and V1 when given) against the reference, printed and held to the bar"""
    bars = bars or (NMF_BAR[iters],) * 3
    names = ("W", "H", "V")
    errs = [R.elrel(g, w) for g, w in zip(got, want) if g is not None]
    rr = R.rowrels(got[0], want[0], got[1], want[1])
    print(f"nmf {label} x {iters}: elrel " + " ".join(f"{n} {e:.3e}" for n, e in zip(names, errs)) +
          f" (bar {' / '.join(f'{b:.1e}' for b in bars[:len(errs)])}); rowrel W {rr[0]:.1e} / {rr[1]:.1e} H {rr[2]:.1e} / {rr[3]:.1e}")
    for n, e, b in zip(names, errs, bars):
        assert e <= b, (label, n, e, b)
    return errs


def unit_norms(W1, iters, bars=NMF_BAR):
    """every component of W1 has L2 norm 1 within the bar (the deferred normalisation's final application)"""
    nrm = np.sqrt((W1 * W1).sum(axis=1))
    assert np.abs(nrm - 1.0).max() <= bars[iters], nrm


def run_one(ctx, shape, iters, X=None, **kw):
    _, T, F, K = shape
    W1, H1, V1, rc = ctx.nmf_process(R.nmf_input(T, F, K) if X is None else X, K, iters, seed=R.SEED, **kw)
    return (W1, H1, V1), rc


class CorpusRun:
    """a corpus of nmf_ref.corpus_audio with its spectrogram on the device; magnitudes read back once"""

    def __init__(self, ctx, shape):
        import fluhip
        B, T, F, K = shape
        n, win, fft, hop = R.corpus_geometry(T, F)
        self.shape, self.seeds = shape, R.corpus_seeds(B)
        self.c = fluhip.Corpus(ctx, B, n, win, fft, hop, K)
        assert (self.c.T, self.c.F) == (T, F)
        self.c.set_audio(R.corpus_audio(B, T, F))
        self.c.stft()
        self.mag = self.c.read_f64(factors=False)[0]
        self._refs = {}

    def factors(self):
        _, W1, H1 = self.c.read_f64(mag=False)
        return W1, H1

    def reference(self, b, iters, uw=True, uh=True, W0=None, H0=None):
        """the reference of buffer b on the DEVICE's own magnitudes: the STFT is no part of the comparison"""
        key = (b, iters, uw, uh, W0 is not None, H0 is not None)
        if key not in self._refs:
            self._refs[key] = R.nmf_process(self.mag[b], self.shape[3], iters, uw, uh, self.seeds[b], W0, H0)
        return self._refs[key]

    def check(self, iters, label, buffers=None, uw=True, uh=True, W0=None, H0=None, bars=None):
        W1, H1 = self.factors()
        bars = bars or (NMF_BAR_AUDIO[iters],) * 2
        worst = [0.0, 0.0]
        for b in range(self.shape[0]) if buffers is None else buffers:
            want = self.reference(b, iters, uw, uh, None if W0 is None else W0[b], None if H0 is None else H0[b])
            for i, (g, w) in enumerate(((W1[b], want[0]), (H1[b], want[1]))):
                e = R.elrel(g, w)
                assert e <= bars[i], (label, b, "WH"[i], e, bars[i])
                worst[i] = max(worst[i], e)
        print(f"corpus {label} x {iters}: elrel W {worst[0]:.3e} H {worst[1]:.3e} over "
              f"{self.shape[0] if buffers is None else len(buffers)} buffers (bar {bars[0]:.1e} / {bars[1]:.1e})")
        return W1, H1

    def close(self):
        self.c.close()


# ---- one buffer of doubles: every regime, every rank edge ------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.ONE_BUFFER_SHAPES, ids=R.shape_id)
def test_one_buffer_every_entry(ctx, shape):
    _, T, F, K = shape
    got, rc = run_one(ctx, shape, 10)
    assert rc == 0
    check(got, R.reference(T, F, K, 10), 10, R.shape_id(shape))
    unit_norms(got[0], 10)


# ---- iteration counts: around the progress-lag window of 8, with and without a callback --------------------------------------
@pytest.mark.parametrize("iters", R.ITER_COUNTS)
@pytest.mark.parametrize("shape", [s for s in R.ITER_SHAPES if s[0] == 1], ids=R.shape_id)
def test_iteration_counts_one_buffer(ctx, shape, iters):
    _, T, F, K = shape
    want = R.reference(T, F, K, iters)
    got, rc = run_one(ctx, shape, iters)
    assert rc == 0
    check(got, want, iters, R.shape_id(shape))
    unit_norms(got[0], iters)
    if iters in (7, 8, 9):
        seen = []
        got, rc = run_one(ctx, shape, iters, progress=lambda it: seen.append(it) or True)
        assert rc == 0 and seen == list(range(1, iters + 1))
        check(got, want, iters, R.shape_id(shape) + " with a callback")


@pytest.mark.parametrize("shape", [s for s in R.ITER_SHAPES if s[0] > 1], ids=R.shape_id)
def test_iteration_counts_corpus(ctx, shape):
    run = CorpusRun(ctx, shape)
    try:
        for iters in R.AUDIO_ITER_COUNTS:
            assert run.c.nmf(iters, seeds=run.seeds) == 0
            run.check(iters, R.shape_id(shape))
            if iters in (7, 8, 9):
                seen = []
                assert run.c.nmf(iters, seeds=run.seeds, progress=lambda it: seen.append(it) or True) == 0
                assert seen == list(range(1, iters + 1))
                run.check(iters, R.shape_id(shape) + " with a callback")
    finally:
        run.close()


# ---- update modes, drawn and seeded factors -------------------------------------------------------------------------------------
def mode_bars(uw, uh, iters, bars=NMF_BAR):
    """an updated factor: the bar of the run; a fixed one is the normalised seed: the bar of one iteration"""
    return (bars[iters] if uw else bars[1], bars[iters] if uh else bars[1], bars[iters] if (uw or uh) else bars[1])


@pytest.mark.parametrize("seeded", [False, True], ids=["drawn", "seeded"])
@pytest.mark.parametrize("uw,uh", R.MODES)
@pytest.mark.parametrize("shape", R.MODE_SHAPES, ids=R.shape_id)
def test_update_modes_one_buffer(ctx, shape, uw, uh, seeded):
    _, T, F, K = shape
    kw = {}
    if seeded:
        W0, H0 = R.seed_factors(T, F, K)
        kw = dict(W0=W0.astype(np.float64), H0=H0.astype(np.float64))
    got, rc = run_one(ctx, shape, 10, updateW=uw, updateH=uh, **kw)
    assert rc == 0
    want = R.reference(T, F, K, 10, uw, uh, seeded)
    check(got, want, 10, f"{R.shape_id(shape)} W {uw} H {uh} {'seeded' if seeded else 'drawn'}", bars=mode_bars(uw, uh, 10))
    zero = R.reference(T, F, K, 0, True, True, seeded)
    if not uw:
        assert R.elrel(got[0], zero[0]) <= NMF_BAR[1]                # the normalised seed, untouched
    if not uh:
        assert R.elrel(got[1], zero[1]) <= NMF_BAR[1]


@pytest.mark.parametrize("uw,uh", R.MODES)
def test_update_modes_corpus_with_set_factors(ctx, uw, uh):
    """the work lists; the seeds go in as floats (Corpus.set_factors), per buffer: the reference takes the same floats"""
    shape = R.MODE_CORPUS_SHAPE
    B, T, F, K = shape
    run = CorpusRun(ctx, shape)
    try:
        seeds = [R.seed_factors(T, F, K, which=b) for b in range(B)]
        sW = np.stack([s[0] for s in seeds])                                   # [B, K, F]
        sH = np.stack([s[1].T for s in seeds])                                 # [B, K, T]
        W0 = [s[0].astype(np.float64) for s in seeds]
        H0 = [s[1].astype(np.float64) for s in seeds]
        run.c.set_factors(sW, sH)
        assert run.c.nmf(10, seed=R.SEED, updateW=uw, updateH=uh) == 0
        run.check(10, f"{R.shape_id(shape)} W {uw} H {uh} set_factors", uw=uw, uh=uh, W0=W0, H0=H0, bars=mode_bars(uw, uh, 10, NMF_BAR_AUDIO)[:2])
        # seeds cleared: drawn factors again, per-buffer seeds
        run.c.set_factors(None, None)
        assert run.c.nmf(10, seeds=run.seeds, updateW=uw, updateH=uh) == 0
        run.check(10, f"{R.shape_id(shape)} W {uw} H {uh} drawn", uw=uw, uh=uh, bars=mode_bars(uw, uh, 10, NMF_BAR_AUDIO)[:2])
    finally:
        run.close()


# ---- corpora: every buffer, per-buffer seeds, no state from call to call ----------------------------------------------------------
@pytest.mark.parametrize("shape", R.CORPUS_SHAPES, ids=R.shape_id)
def test_corpus_every_buffer_every_entry(ctx, shape):
    B, T, F, K = shape
    run = CorpusRun(ctx, shape)
    try:
        assert run.c.nmf(10, seeds=run.seeds) == 0
        W1, H1 = run.check(10, R.shape_id(shape))
        for b in range(B):
            unit_norms(W1[b], 10, NMF_BAR_AUDIO)
        # another schedule in between, then the same call again: the same bits as on the fresh corpus -- nothing a call leaves
        # behind (the side column's partials, the column sums, the deferred norms) reaches the next
        some = sorted({0, 1, B // 2, B - 1})
        assert run.c.nmf(10, seeds=run.seeds, updateW=False) == 0
        run.check(10, R.shape_id(shape) + " W fixed after a full run", buffers=some, uw=False, bars=(NMF_BAR_AUDIO[1], NMF_BAR_AUDIO[10]))
        assert run.c.nmf(10, seeds=run.seeds) == 0
        W2, H2 = run.factors()
        assert np.array_equal(W1, W2) and np.array_equal(H1, H2)
    finally:
        run.close()


# ---- a ragged corpus: frame counts around 32, one apart ------------------------------------------------------------------------
@pytest.mark.parametrize("K", R.RAGGED_RANKS)
def test_ragged_corpus_each_buffer_over_its_own_frames(ctx, K):
    import fluhip
    audios = R.ragged_audio()
    c = fluhip.RaggedCorpus(ctx, R.RAGGED_LENS, 1024, 1024, 256, K)
    try:
        assert c.Ts == [31, 32, 32, 33, 34] and c.T == 34
        c.set_audio(audios)
        c.stft()
        seeds = R.corpus_seeds(len(audios))
        assert c.nmf(10, seeds=seeds) == 0
        mag, W1, H1 = c.read_f64()
    finally:
        c.close()
    worst = [0.0, 0.0]
    for b, T in enumerate(c.Ts):
        assert not mag[b, T:].any() and not H1[b, T:].any()                    # frames past a buffer's own are zero
        rW, rH, _ = R.nmf_process(mag[b, :T], K, 10, seed=seeds[b])
        worst = [max(worst[0], R.elrel(W1[b], rW)), max(worst[1], R.elrel(H1[b, :T], rH))]
        unit_norms(W1[b], 10, NMF_BAR_AUDIO)
    print(f"ragged corpus rank {K} x 10: elrel W {worst[0]:.3e} H {worst[1]:.3e} (bar {NMF_BAR_AUDIO[10]:.1e})")
    assert max(worst) <= NMF_BAR_AUDIO[10]


# ---- cancellation ---------------------------------------------------------------------------------------------------------------
def test_cancel_at_iteration_five_returns_iteration_five(ctx):
    """progress lag 1: the callback of iteration 5 refuses, the factors handed back are those of iteration 5 -- held to
    NMF_BAR[7] = 1.7e-13, the next larger derived bar (no bar is derived for 5 itself)"""
    import fluhip
    shape = R.CANCEL_SHAPE
    _, T, F, K = shape
    bar_at = min(i for i in NMF_BAR if i >= R.CANCEL_AT)
    assert bar_at == 7
    ctx.set_progress_lag(1)
    try:
        seen = []
        got, rc = run_one(ctx, shape, 200, progress=lambda it: seen.append(it) or it < R.CANCEL_AT)
        assert rc == fluhip.CANCELLED and seen == list(range(1, R.CANCEL_AT + 1))
    finally:
        ctx.set_progress_lag(8)
    want = R.reference(T, F, K, R.CANCEL_AT)
    check(got[:2], want[:2], bar_at, f"{R.shape_id(shape)} cancelled at {R.CANCEL_AT}")


# ---- strided input ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.STRIDED_SHAPES, ids=R.shape_id)
def test_strided_input(ctx, shape):
    """ldx > F: the padding behind every row holds 7.0, must not reach a bin and must be there afterwards"""
    _, T, F, K = shape
    Xc = R.nmf_input(T, F, K)
    buf = np.full((T, F + 5), 7.0)
    buf[:, :F] = Xc
    X = buf[:, :F]
    assert X.strides == (8 * (F + 5), 8)
    got, rc = run_one(ctx, shape, 10, X=X)
    assert rc == 0
    check(got, R.reference(T, F, K, 10), 10, R.shape_id(shape) + " strided")
    assert (buf[:, F:] == 7.0).all() and np.array_equal(buf[:, :F], Xc)


# ---- the client's writeback ---------------------------------------------------------------------------------------------------
def test_writeback_is_the_rounding_of_the_devices_own_factors(ctx):
    """every float of Corpus.writeback() against oracle_np.bufnmf_writeback of the device's own double factors: within one
    float32 rounding of each value (bases: the rounding itself; activations: scaled by the buffer's largest)"""
    shape = R.MODE_CORPUS_SHAPE
    run = CorpusRun(ctx, shape)
    try:
        assert run.c.nmf(10, seeds=run.seeds) == 0
        W1, H1 = run.factors()
        bases, acts = run.c.writeback()
    finally:
        run.close()
    assert bases.dtype == np.float32 and acts.dtype == np.float32
    same = 0
    for b in range(shape[0]):
        rb, ra = oracle_np.bufnmf_writeback(W1[b], H1[b])
        assert bases[b].shape == rb.shape and acts[b].shape == ra.shape
        for got, want in ((bases[b], rb), (acts[b], ra)):
            ulp = np.maximum(np.spacing(np.abs(want)), np.float32(2.0 ** -149))
            assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), b
            assert not got[want == 0].any()
        same += int((bases[b] == rb).sum())
    print(f"writeback {R.shape_id(shape)}: {same} of {bases.size} bases identical to the rounded factors")
