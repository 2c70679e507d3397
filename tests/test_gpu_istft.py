"""GPU tests of the inverse STFT and the ratio-masked resynthesis at double precision: fluhip_debug_resynth_f64 (the clients'
frame + overlap-add kernels, on-chip and through the global-memory passes) and the corpus' batched kernel against
tests/istft_ref.py.  The bar is 64 x the floor tests/test_istft_ref.py measures between the C oracle and that restatement on
the CPU -- the factor the onset, novelty, pitch and HPSS GPU tests put over such a floor: the device's transform is a third
double implementation and differs from both in the last places."""
import time

import numpy as np
import pytest

import istft_ref as R
import oracle_np
from test_istft_ref import BATCH_EXTRA, BATCH_SHAPES, BATCH_SIZES, ISTFT_BAR, PER_BUFFER, RAGGED

pytestmark = pytest.mark.gpu


def check_plain(ctx, case, spec):
    n, win, fft, hop, trim = case
    T = R.num_frames(n, hop)
    assert spec.shape == (T, fft // 2 + 1)
    got = ctx.resynth_f64(spec, win, fft, hop, n, trim)
    ref = R.istft(spec, win, fft, hop, n, trim)
    w = R.weights(T, win, hop, n, trim)
    e = R.err(got, ref, w)
    print(f"inverse {R.case_id(case)}: err {e:.2e} (bar {ISTFT_BAR:.2e}), peak {np.abs(ref).max():.3f}")
    assert got.shape == (n,) and not np.isnan(got).any()
    assert np.abs(ref).max() > 0.01
    assert e <= ISTFT_BAR
    return got, ref, w


# ---- a. the plain inverse in every kernel form -----------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PLAIN_CASES + R.SHORT_CASES, ids=R.case_id)
def test_plain_inverse(ctx, case):
    n, win, fft, hop, trim = case
    got, _, _ = check_plain(ctx, case, R.plain_spec(n, win, fft, hop))
    if hop > win:
        uncovered = (np.arange(n) + trim) % hop >= win
        assert uncovered.any() and not got[uncovered].any()


def test_bad_arguments_are_named_and_leave_the_output_alone(ctx):
    import fluhip
    n, win, fft, hop, trim = 1500, 64, 64, 16, 32
    spec = np.ascontiguousarray(R.plain_spec(n, win, fft, hop)).view(np.float64)
    T, F = R.num_frames(n, hop), fft // 2 + 1
    W, H = (np.ascontiguousarray(a) for a in R.factors(T, F, 3))
    out = np.full((3, n), -7.0)
    good = dict(spec=spec, T=T, win=win, fft=fft, hop=hop, n=n, trim=trim, W=W, H=H, K=3, out=out)

    def call(**kw):
        a = dict(good, **kw)
        ptr = lambda v: None if v is None else v.ctypes.data_as(fluhip._dp)  # noqa: E731
        return ctx.lib.fluhip_debug_resynth_f64(ctx.h, ptr(a["spec"]), a["T"], a["win"], a["fft"], a["hop"], a["n"], a["trim"],
                                                ptr(a["W"]), ptr(a["H"]), a["K"], ptr(a["out"]))

    for kw, word in ((dict(spec=None), "spec"), (dict(T=0), "T must"), (dict(win=0), "win"), (dict(hop=0), "hop"),
                     (dict(fft=48), "fft"), (dict(fft=32), "fft"), (dict(fft=131072), "fft"), (dict(n=0), "n must"),
                     (dict(trim=-1), "trim"), (dict(H=None), "W and H"), (dict(W=None), "W and H"), (dict(K=0), "K must")):
        assert call(**kw) == fluhip.ERROR, kw
        msg = ctx.lib.fluhip_last_error(ctx.h).decode()
        assert msg.startswith("fluhip_debug_resynth_f64: ") and word in msg, (kw, msg)
        assert (out == -7.0).all(), kw
    assert call(out=None) == fluhip.ERROR and "out" in ctx.lib.fluhip_last_error(ctx.h).decode()
    assert call() == fluhip.OK and not (out == -7.0).any()


# ---- b. across a chunk of the global-memory passes -------------------------------------------------------------------
def test_inverse_across_a_chunk_boundary(ctx):
    """fft 65536: 1032 frames against the 1024 one 512 MB chunk of the global-memory passes holds; any spectrum is a valid
    input, so it is drawn (no forward transform on the CPU).  The samples the last frames of the first chunk and the first
    frames of the second reach are held to the bar on their own as well, so that a failure names its side."""
    n, win, fft, hop, trim = R.CHUNK_CASE
    spec = R.chunk_spec()
    assert spec.shape[0] == 1032 > R.CHUNK_FRAMES
    t0 = time.perf_counter()
    got = ctx.resynth_f64(spec, win, fft, hop, n, trim)
    t1 = time.perf_counter()
    ref = R.istft(spec, win, fft, hop, n, trim)
    w = R.weights(spec.shape[0], win, hop, n, trim)
    print(f"chunk boundary: device call {t1 - t0:.2f} s, reference {time.perf_counter() - t1:.2f} s")
    e = R.err(got, ref, w)
    print(f"inverse {R.case_id(R.CHUNK_CASE)}: err {e:.2e} (bar {ISTFT_BAR:.2e}), peak {np.abs(ref).max():.4f}")
    # (a unit-variance spectrum of 32769 bins is a signal of deviation 1 / 256: the measure is relative, the peak only not 0)
    assert not np.isnan(got).any() and np.abs(ref).max() > 1e-3
    edge = R.CHUNK_FRAMES * hop - trim
    for name, lo, hi in (("before", edge - 4 * hop, edge), ("behind", edge, edge + 4 * hop)):
        es = float((np.abs(got[lo:hi] - ref[lo:hi]) * w[lo:hi]).max()) / R.peak(ref, w)
        print(f"  samples [{lo}, {hi}) {name} the boundary: err {es:.2e}")
        assert es <= ISTFT_BAR, name
    assert e <= ISTFT_BAR


# ---- c. the ratio-masked resynthesis, every component in one launch --------------------------------------------------
@pytest.mark.parametrize("case", R.MASKED_CASES, ids=R.case_id)
def test_masked_resynthesis(ctx, case):
    """all K outputs come from one call and are held component by component (a wrong stride between the components of a
    launch shows as component 1 holding component 0's samples); they add up to the inverse of the spectrum where V-hat is
    positive -- the zero rows of H and the zero column of W take their frames and their bin out of every component"""
    n, win, fft, hop, K = case
    trim = win // 2
    spec = R.plain_spec(n, win, fft, hop)
    T, F = spec.shape
    W, H = R.factors(T, F, K)
    got = ctx.resynth_f64(spec, win, fft, hop, n, trim, W, H)
    assert got.shape == (K, n) and not np.isnan(got).any()
    w = R.weights(T, win, hop, n, trim)
    for k in range(K):
        ref = R.istft(spec, win, fft, hop, n, trim, R.ratio_mask(W, H, k))
        e = R.err(got[k], ref, w)
        print(f"masked {R.case_id(case)} component {k}: err {e:.2e} (bar {ISTFT_BAR:.2e}), peak {np.abs(ref).max():.3f}")
        assert np.abs(ref).max() > 0.01
        assert e <= ISTFT_BAR, k
    whole = R.istft(spec * ((H @ W) > 0), win, fft, hop, n, trim)
    e = R.err(got.sum(axis=0), whole, w)
    print(f"masked {R.case_id(case)}: the components add up within {e:.2e} (bar {K * ISTFT_BAR:.2e})")
    assert e <= K * ISTFT_BAR


def test_a_launch_of_one_component_gives_the_bits_of_a_launch_of_nine(ctx):
    """A launch of nine components against launches of one, bit for bit.  The mask of a component divides by the V-hat of
    ALL the factors a call is given, so a call with row k alone does not have the mask component k has among nine.  Held
    here is what both can share: nine components of which only k is non-zero -- V-hat is then h_k w_k plus exact zeros, the
    K = 1 call's own -- must put the K = 1 call's samples in slot k and exact zeros in the other eight."""
    n, win, fft, hop, K = R.MASKED_CASES[2]
    assert K == 9
    trim = win // 2
    spec = R.plain_spec(n, win, fft, hop)
    T, F = spec.shape
    W, H = R.factors(T, F, K)
    w = R.weights(T, win, hop, n, trim)
    for k in (0, 4, 8):
        one = ctx.resynth_f64(spec, win, fft, hop, n, trim, W[k:k + 1], H[:, k:k + 1])
        Wk, Hk = np.zeros_like(W), np.zeros_like(H)
        Wk[k], Hk[:, k] = W[k], H[:, k]
        nine = ctx.resynth_f64(spec, win, fft, hop, n, trim, Wk, Hk)
        assert np.array_equal(nine[k], one[0]), k
        assert not np.delete(nine, k, axis=0).any()
        ref = R.istft(spec, win, fft, hop, n, trim, R.ratio_mask(W[k:k + 1], H[:, k:k + 1], 0))
        assert np.abs(ref).max() > 0.01 and R.err(one[0], ref, w) <= ISTFT_BAR


# ---- d. the batched kernel (and the per-buffer form) through a corpus ------------------------------------------------
def check_corpus_buffer(ctx, name, x, got, W1, H1, win, fft, hop):
    """every float sample within half a float32 ulp of the restatement's value plus the double bar, the restatement run
    from the device's own factors and the device's own double spectrum"""
    K, n = got.shape
    T = R.num_frames(n, hop)
    spec = ctx.stft(x, win, fft, hop, want_mag=False)[0]
    assert spec.shape[0] == T and H1.shape == (T, K)
    w = R.weights(T, win, hop, n, win // 2)
    worst = 0.0
    for k in range(K):
        ref = R.istft(spec, win, fft, hop, n, win // 2, R.ratio_mask(W1, H1, k))
        bound = 2.0 ** -24 * np.abs(ref) + ISTFT_BAR * R.peak(ref, w) / w
        d = np.abs(got[k].astype(np.float64) - ref)
        worst = max(worst, float((d / bound).max()))
        assert (d <= bound).all(), (name, k, int(np.argmax(d / bound)), float((d / bound).max()))
    print(f"corpus {name}: worst |got - ref| / (2^-24 |ref| + bar peak / w) = {worst:.3f}")
    assert np.isfinite(got).all() and np.abs(got).max() > 0.01


def run_corpus(ctx, win, fft, hop, B, n, K, seed):
    import fluhip
    audio = np.stack([oracle_np.synth_audio(n, seed + b) for b in range(B)])
    c = fluhip.Corpus(ctx, B, n, win, fft, hop, K)
    c.keep_spectrum(True)
    c.set_audio(audio); c.stft(); c.nmf(4, seed=42)
    out = c.resynth()
    _, W1, H1 = c.read_f64(mag=False)
    c.close()
    assert out.shape == (B, K, n) and out.dtype == np.float32
    for b in range(B):
        check_corpus_buffer(ctx, f"{win}_{fft}_{hop} B{B} n{n} K{K} buffer {b}", audio[b], out[b], W1[b], H1[b], win, fft, hop)


# Which form a corpus' resynthesis takes is resynth_batch_supported's rule (kernels_resynth_batch.hip), which no entry point reports:
# an even window that is a multiple of the hop, fft 2048 with a hop of 256 / 512 / 1024 or fft 1024 with 128 / 256 / 512 --
# every shape below but PER_BUFFER's fft 512.  Rank 3 packs two (buffer, run) pairs into a workgroup, rank 8 takes the rows
# shared through the LDS, rank 9 leaves seven idle wavefronts at the barriers; the odd n puts every other component's
# output on a 4-byte boundary only; 59 slots in runs of 8 give several run boundaries.
BATCH_CASES = [shape + size for shape in BATCH_SHAPES for size in BATCH_SIZES] + [BATCH_EXTRA]


@pytest.mark.parametrize("win,fft,hop,B,n,K", BATCH_CASES, ids=[R.case_id(c) for c in BATCH_CASES])
def test_batched_resynthesis_per_sample(ctx, win, fft, hop, B, n, K):
    assert win % hop == 0 and win % 2 == 0 and hop in {2048: (256, 512, 1024), 1024: (128, 256, 512)}[fft]
    run_corpus(ctx, win, fft, hop, B, n, K, 8100)


def test_ragged_batched_resynthesis_per_sample(ctx):
    import fluhip
    lens, win, fft, hop, K = RAGGED
    audios = [oracle_np.synth_audio(n, 8300 + i) for i, n in enumerate(lens)]
    c = fluhip.RaggedCorpus(ctx, lens, win, fft, hop, K)
    c.keep_spectrum(True)
    c.set_audio(audios); c.stft(); c.nmf(4, seed=42)
    out = c.resynth()
    _, W1, H1 = c.read_f64(mag=False)
    Ts = list(c.Ts)
    c.close()
    for b, n in enumerate(lens):
        assert out[b].shape == (K, n) and Ts[b] == R.num_frames(n, hop)
        assert not H1[b][Ts[b]:].any()
        check_corpus_buffer(ctx, f"ragged buffer {b} n{n}", audios[b], out[b], W1[b], H1[b][:Ts[b]], win, fft, hop)


def test_per_buffer_resynthesis_per_sample(ctx):
    """fft 512 has no batched form: the corpus falls through to the frame + overlap-add kernels with the float output"""
    win, fft, hop, B, n, K = PER_BUFFER
    assert fft not in (1024, 2048)
    run_corpus(ctx, win, fft, hop, B, n, K, 8500)
