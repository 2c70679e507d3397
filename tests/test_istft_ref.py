"""CPU tests of tests/istft_ref.py: the restatement inverts the forward transform, leaves the samples no frame covers at
exactly 0, and lies within FLOOR of the native C oracle's resynthesis on every case the GPU tests (tests/test_gpu_istft.py)
run at trim = win / 2 -- the floor their bar is 64 times."""
import numpy as np
import pytest

import istft_ref as R
import oracle_np

# The largest err (istft_ref.err: normaliser-weighted, relative to the weighted peak) between the C oracle's
# resynth_component and the restatement over FLOOR_CASES, measured (6.01e-16, at fft 2048 / hop 1024 / rank 8; from fft 16
# up every case lies between 2.1e-16 and that) and rounded up to one digit.  Two double implementations of one inverse -- the
# oracle's own FFT with a double overlap-add, numpy's irfft with a long double one -- differ by this much; the device's is a
# third.
FLOOR = 7e-16
ISTFT_BAR = 64 * FLOOR

# the shapes of the batched kernel's tests (test_gpu_istft.py part d) and of the per-buffer form beside them
BATCH_SHAPES = [(fft, fft, hop) for fft, hops in ((2048, (256, 512, 1024)), (1024, (128, 256, 512))) for hop in hops]
BATCH_SIZES = [(2, 30001, 3), (1, 9000, 8), (2, 9000, 9)]    # (B, n, K)
BATCH_EXTRA = (1024, 2048, 256, 2, 9000, 5)                  # an even window shorter than the transform
RAGGED = ((30000, 700, 4100), 2048, 2048, 512, 6)
PER_BUFFER = (512, 512, 128, 2, 5000, 4)                     # no batched form at fft 512

# (n, win, fft, hop, K): K = 0 is the plain inverse (the oracle gets the factors 1, 1 and V = 1: a mask of exactly 1)
FLOOR_CASES = ([c[:4] + (0,) for c in R.PLAIN_CASES + R.SHORT_CASES + [R.CHUNK_CASE] if c[4] == c[1] // 2] + R.MASKED_CASES +
               [(n, win, fft, hop, K) for win, fft, hop in BATCH_SHAPES for _, n, K in BATCH_SIZES] +
               [(BATCH_EXTRA[4],) + BATCH_EXTRA[:3] + (BATCH_EXTRA[5],), (PER_BUFFER[4],) + PER_BUFFER[:3] + (PER_BUFFER[5],)] +
               [(n,) + RAGGED[1:] for n in RAGGED[0]])


def floor_case_err(oracle, case):
    n, win, fft, hop, K = case
    trim = win // 2
    T, F = R.num_frames(n, hop), fft // 2 + 1
    w = R.weights(T, win, hop, n, trim)
    if K == 0:
        spec = R.chunk_spec() if case[:4] == R.CHUNK_CASE[:4] else R.plain_spec(n, win, fft, hop)
        got = oracle.resynth_component(spec, np.ones((1, F)), np.ones((T, 1)), np.ones((T, F)), 0, win, fft, hop, n)
        return R.err(got, R.istft(spec, win, fft, hop, n, trim), w)
    spec = R.plain_spec(n, win, fft, hop)
    W, H = R.factors(T, F, K)
    V = H @ W
    worst = 0.0
    for k in range(K):
        got = oracle.resynth_component(spec, W, H, V, k, win, fft, hop, n)
        worst = max(worst, R.err(got, R.istft(spec, win, fft, hop, n, trim, R.ratio_mask(W, H, k)), w))
    return worst


def test_the_floor_between_the_oracle_and_the_restatement(oracle):
    errs = {R.case_id(c): floor_case_err(oracle, c) for c in FLOOR_CASES}
    for name, e in errs.items():
        print(f"{name}: oracle vs restatement {e:.2e}")
    worst = max(errs.values())
    print(f"floor {worst:.3e} (FLOOR {FLOOR:.1e}, ISTFT_BAR {ISTFT_BAR:.2e})")
    assert 0 < worst <= FLOOR


@pytest.mark.parametrize("n,win,fft,hop", [(9000, 1024, 1024, 512), (9000, 1024, 1024, 256), (2500, 200, 256, 100),
                                           (6000, 301, 512, 75)])
def test_the_restatement_inverts_the_forward_transform(n, win, fft, hop):
    x = oracle_np.synth_audio(n, 77).astype(np.float64)
    spec = oracle_np.stft(x, win, fft, hop)[0]
    y = R.istft(spec, win, fft, hop, n, win // 2)
    assert np.abs(x).max() > 0.01
    assert np.abs(y[win:-win] - x[win:-win]).max() <= 1e-12
    # a trim is a shift: the same samples, `d` positions later
    d = win // 2 - hop // 2
    assert np.array_equal(R.istft(spec, win, fft, hop, n - d, win // 2 - d)[d:], y[: n - 2 * d])


def test_samples_no_frame_covers_are_exactly_zero():
    n, win, fft, hop, trim = 5000, 256, 256, 384, 128
    spec = R.plain_spec(n, win, fft, hop)
    y = R.istft(spec, win, fft, hop, n, trim)
    uncovered = (np.arange(n) + trim) % hop >= win
    assert uncovered.sum() > n // 4 and np.abs(y[~uncovered]).max() > 0.01
    assert not y[uncovered].any() and not np.signbit(y[uncovered]).any()
    assert not R.normaliser(R.num_frames(n, hop), win, hop, n, trim)[uncovered].any()


def test_the_mask_clamps_and_vanishes_where_the_estimate_does():
    T, F, K = 30, 33, 3
    W, H = R.factors(T, F, K)
    m = np.stack([R.ratio_mask(W, H, k) for k in range(K)])
    assert m.min() == 0.0 and m.max() <= 1.0
    assert not m[:, [0, T // 2, T - 2]].any() and not m[:, :, F // 3].any()
    live = (H @ W) > 0
    assert np.abs(m.sum(axis=0)[live] - 1).max() < 1e-15
    one = R.ratio_mask(W[:1], H[:, :1], 0)          # a single component: est / est, clamped at 1
    assert set(np.unique(one[live])) <= {1.0, np.nextafter(1.0, 0)}
