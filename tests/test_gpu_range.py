"""The double-precision entry points over the double range (fluhip_stft_f64, fluhip_nmf_process_f64 / _views_f64 / _frames_f64,
fluhip_nndsvd_f64).  The reference does its arithmetic in double precision and works at any magnitude (std::abs of
std::complex for the magnitudes, alg/STFT.hpp:61-66; element-by-element quotients, alg/NMF.hpp:158-168; BDCSVD, which
scales first, alg/NNDSVD.hpp:42).  A float32 input reaches none of these scales, so the rest of the suite cannot see what
happens there: here every case is the GPU entry point against the CPU restatement of the same operation, at scales where a
kernel's intermediate values leave the double range (products of several W H values in one reciprocal, sums of squares)
or where the epsilon clamp of the factor updates is partly active.
"""
import ctypes

import numpy as np
import pytest

from helpers import TOL_FACTORS_TIGHT, TOL_STFT, elementwise_rel_err, rel_err

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
ITERS = 6
UPDATES = [(True, True), (True, False), (False, True)]

# the update schedules a single buffer reaches, by the planner's answer (fluhip_debug_plan_shape: slot 0 family, 1 W-update
# splits, 7 computed rank, 8 frame strip, 23 norm-combine form)
SCHEDULES = {
    "strip_k8": (300, 513, 8),         # frame-strip kernel: six quotients per reciprocal
    "batched_k32": (300, 513, 32),     # fused kernel, four per reciprocal
    "batched_k40": (300, 513, 40),
    "inplace_k128": (200, 257, 128),   # rank 128: the in-place pipeline with its norm-combine form
    "any_rank_k144": (60, 65, 144),    # above 128: the un-fused any-rank path
    "split_k16": (700, 1025, 16),      # a single buffer large enough for split contractions
}


def _plan(lib, T, F, K):
    out = (ctypes.c_int64 * 32)()
    assert lib.fluhip_debug_plan_shape(1, T, F, K, out) == 0
    return [int(v) for v in out]


def test_range_schedules_are_the_ones_named(ctx):
    """the cases below cover what they say they cover: a planner change that moves a shape to another schedule fails here"""
    p = {name: _plan(ctx.lib, *shape) for name, shape in SCHEDULES.items()}
    assert (p["strip_k8"][0], p["strip_k8"][8], p["strip_k8"][7]) == (5, 1, 16)
    assert (p["batched_k32"][0], p["batched_k32"][8], p["batched_k32"][7]) == (5, 0, 32)
    assert (p["batched_k40"][0], p["batched_k40"][8], p["batched_k40"][7]) == (5, 0, 40)
    assert (p["inplace_k128"][0], p["inplace_k128"][8], p["inplace_k128"][7]) == (5, 0, 128) and p["inplace_k128"][23] >= 0
    assert (p["any_rank_k144"][0], p["any_rank_k144"][7]) == (0, 144)
    assert (p["split_k16"][0], p["split_k16"][8]) == (5, 1) and p["split_k16"][1] > 1


def _matrix(T, F, K, scale):
    rs = np.random.RandomState(T + F + K)
    X = (np.abs(rs.standard_normal((T, 5)) @ rs.standard_normal((5, F))) + 0.01 * rs.uniform(0, 1, (T, F))) * scale
    W0, H0 = rs.uniform(0, 1, (K, F)), rs.uniform(0, 1, (T, K))
    return X, W0, H0


def _nontrivial(*arrays):
    return all(np.isfinite(a).all() and np.abs(a).max() > 0 for a in arrays)


def _check_both_entries(ctx, oracle, X, K, uw, uh, W0=None, H0=None, label=()):
    """fluhip_nmf_process_f64 and fluhip_nmf_process_views_f64 (X as a transposed view) against the oracle"""
    T, F = X.shape
    rW, rH, rV, _ = oracle.nmf_process(X, K, ITERS, uw, uh, 42, W0=W0, H0=H0)
    assert _nontrivial(rW, rH, rV), ("the oracle itself has no result here", label)
    W1, H1, V1, rc = ctx.nmf_process(X, K, ITERS, uw, uh, 42, W0=W0, H0=H0)
    assert rc == 0 and np.isfinite(W1).all() and np.isfinite(H1).all() and np.isfinite(V1).all(), label
    errs = (rel_err(W1, rW), rel_err(H1, rH), rel_err(V1, rV))
    assert max(errs) < TOL_FACTORS_TIGHT, (label, errs)
    Xv = np.ascontiguousarray(X.T).T
    W2, H2, V2 = np.empty((K, F)), np.empty((T, K)), np.empty((T, F))
    rc = ctx.nmf_process_views(Xv, K, ITERS, uw, uh, 42, W0=W0, H0=H0, W1=W2, H1=H2, V1=V2)
    assert rc == 0
    errs = (rel_err(W2, rW), rel_err(H2, rH), rel_err(V2, rV))
    assert max(errs) < TOL_FACTORS_TIGHT, ("views", label, errs)


@pytest.mark.parametrize("scale", [1e40, 1e60, 1e100, 1e140])
@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_nmf_f64_over_the_double_range(ctx, oracle, schedule, scale):
    """magnitudes no float input reaches: the products of four / six clamped W H values behind one reciprocal leave the
    double range from ~1e51 / ~1e77 on unless the input is brought into range first"""
    T, F, K = SCHEDULES[schedule]
    X, W0, H0 = _matrix(T, F, K, scale)
    for uw, uh in UPDATES:
        _check_both_entries(ctx, oracle, X, K, uw, uh, label=(schedule, scale, uw, uh))
    _check_both_entries(ctx, oracle, X, K, True, True, W0=W0, H0=H0, label=(schedule, scale, "seeded"))


@pytest.mark.parametrize("scale", [3e-16, 1e-16, 5e-17])
@pytest.mark.parametrize("schedule", ["strip_k8", "batched_k32", "inplace_k128"])
def test_nmf_f64_where_the_epsilon_clamp_is_partly_active(ctx, oracle, schedule, scale):
    """around 1e-16 most of W H sits below epsilon while the factors are still non-zero: max(W H, eps) must clamp
    exactly where the reference clamps (at 1e-30 everything collapses to epsilon and says nothing about it)"""
    T, F, K = SCHEDULES[schedule]
    X, _, _ = _matrix(T, F, K, scale)
    for uw, uh in UPDATES:
        _check_both_entries(ctx, oracle, X, K, uw, uh, label=(schedule, scale, uw, uh))


@pytest.mark.parametrize("scale", [1e160, 1e250])
@pytest.mark.parametrize("schedule", ["strip_k8", "batched_k32", "inplace_k128", "any_rank_k144"])
def test_nmf_f64_beyond_the_references_range_never_returns_non_finite_factors(ctx, schedule, scale):
    """past ~1e154 the reference's own W.colwise().normalize() overflows to zeros, so there is no parity to ask for; but a
    call that reports success must not hand back NaN or inf"""
    import fluhip
    T, F, K = SCHEDULES[schedule]
    X, _, _ = _matrix(T, F, K, scale)
    for uw, uh in UPDATES:
        try:
            W1, H1, V1, rc = ctx.nmf_process(X, K, ITERS, uw, uh, 42)
        except fluhip.FluhipError as e:
            assert str(e).strip(), (schedule, scale, uw, uh)
            continue
        assert rc == 0
        assert np.isfinite(W1).all() and np.isfinite(H1).all() and np.isfinite(V1).all(), (schedule, scale, uw, uh)


@pytest.mark.parametrize("scale", [1e-16, 1e60, 1e140])
@pytest.mark.parametrize("K", [8, 32])
def test_nmf_frames_f64_over_the_double_range(ctx, oracle, K, scale):
    T, F = 120, 513
    X, W0, _ = _matrix(T, F, K, scale)
    rH, rV = oracle.nmf_process_frames(X, W0, ITERS, 42)
    assert _nontrivial(rH, rV)
    H, V = ctx.nmf_process_frames(X, W0, ITERS, 42)
    assert np.isfinite(H).all() and np.isfinite(V).all()
    assert rel_err(H, rH) < TOL_FACTORS_TIGHT and rel_err(V, rV) < TOL_FACTORS_TIGHT, (K, scale, rel_err(H, rH), rel_err(V, rV))


# the size classes of test_stft_vs_oracle: in-LDS (512, 2048), the largest in-LDS one (8192), global-memory passes
STFT_SHAPES = [(5000, 512, 512, 128), (12000, 2048, 2048, 512), (20000, 8192, 8192, 2048), (60000, 16384, 16384, 4096),
               (140000, 65536, 65536, 16384)]


@pytest.mark.parametrize("scale", [1e-300, 1e-200, 1e-160, 1e160, 1e200, 1e300])
@pytest.mark.parametrize("n,win,fft,hop", STFT_SHAPES)
def test_stft_f64_over_the_double_range(ctx, oracle, onp, n, win, fft, hop, scale):
    x = onp.synth_audio(n, 3000 + fft % 97).astype(np.float64) * scale
    spec, mag = ctx.stft(x, win, fft, hop)
    rspec, rmag = oracle.stft(x, win, fft, hop)
    assert np.isfinite(spec).all() and np.isfinite(mag).all()
    assert rel_err(spec, rspec) < TOL_STFT and rel_err(mag, rmag) < TOL_STFT, (rel_err(spec, rspec), rel_err(mag, rmag))
    # bin by bin: the magnitude is |spectrum| with all its digits (np.abs of a complex is hypot) -- a bin clamped to a floor
    # or computed from an underflowed sum of squares fails this
    assert elementwise_rel_err(mag, np.abs(spec)) < 1e-12
    # and against the oracle's: two double FFTs already differ by ~5e-12 relative in bins 1e-6 below the peak, so the
    # element-wise comparison across implementations looks at bins within 1e-3 of it
    assert elementwise_rel_err(mag, rmag, floor=1e-3) < 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stft_silence_has_magnitude_exactly_zero(ctx, onp, dtype):
    """std::abs(0) is 0 (alg/STFT.hpp:61-66): all-zero audio, and the frames wholly inside a run of zeros longer than a window"""
    win, fft, hop = 1024, 1024, 256
    _, mag = ctx.stft(np.zeros(20000, dtype=dtype), win, fft, hop)
    assert (mag == 0).all(), mag.max()
    x = onp.synth_audio(20000, 11).astype(dtype)
    x[6000:14000] = 0
    _, mag = ctx.stft(x, win, fft, hop)
    # frame t covers samples [t hop - win / 2, t hop + win / 2) of the input (the reference's centred framing)
    quiet = [t for t in range(mag.shape[0]) if t * hop - win // 2 >= 6000 and t * hop + win // 2 <= 14000]
    assert len(quiet) > 10
    assert (mag[quiet] == 0).all(), np.abs(mag[quiet]).max()
    assert (mag[: quiet[0] - 4] > 0).any()


def _lowrank_spectrogram(T, F, r, seed):
    rs = np.random.RandomState(seed)
    scales = np.linspace(3.0, 0.3, r)
    return (np.abs(rs.standard_normal((T, r))) * scales) @ np.abs(rs.standard_normal((r, F))) + 1e-3 * rs.uniform(0, 1, (T, F))


@pytest.mark.parametrize("scale", [1e-250, 1e-160, 1e160, 1e250])
@pytest.mark.parametrize("T,F,amount,min_rank,max_rank", [(60, 33, 0.8, 0, 10), (200, 129, 0.5, 2, 16), (40, 65, 0.0, 3, 8),
                                                           (300, 513, 0.9, 1, 24)])
def test_nndsvd_method0_over_the_double_range(ctx, onp, T, F, amount, min_rank, max_rank, scale):
    """the SVD's sums of squares leave the double range past 1e+-154 unless the matrix is scaled first (as BDCSVD and LAPACK do)"""
    X = _lowrank_spectrogram(T, F, 12, T + F) * scale
    W, H, k = ctx.nndsvd(X, max_rank, min_rank, max_rank, amount, 0, 42)
    rW, rH, rk, U, s, VT = onp.nndsvd(X, max_rank, min_rank, max_rank, amount, 0, 42)
    assert _nontrivial(rW, rH)
    assert k == rk
    assert np.isfinite(W).all() and np.isfinite(H).all()
    assert rel_err(W, rW) < 1e-8 and rel_err(H, rH) < 1e-8, (rel_err(W, rW), rel_err(H, rH))
    assert (W[k:] == 0).all() and (H[:, k:] == 0).all()


@pytest.mark.parametrize("scale", [1e-250, 1e250])
@pytest.mark.parametrize("method", [1, 2, 3])
def test_nndsvd_split_methods_over_the_double_range(ctx, onp, method, scale):
    """test_nndsvd_split_methods' sign-tolerant comparison at a large and a small scale: every component equals the
    oracle's un-filled construction for one of the two signs of its singular pair, wherever that is >= epsilon"""
    T, F, K = 120, 65, 8
    X = _lowrank_spectrogram(T, F, 10, 5) * scale
    W, H, k = ctx.nndsvd(X, K, K, K, 0.0, method, 42)
    assert k == K and np.isfinite(W).all() and np.isfinite(H).all()
    U, s, VT = np.linalg.svd(X.T, full_matrices=False)
    assert np.isfinite(s).all() and s[K - 1] > 0
    mean = float(X.mean())
    for j in range(K):
        best = np.inf
        for sign in (1.0, -1.0):
            Uj, VTj = U.copy(), VT.copy()
            Uj[:, j] *= sign
            VTj[j] *= sign
            cW, cH, _ = onp.nndsvd_from_svd(Uj, s, VTj, X, K, K, K, 0.0, 3, 42)
            mw, mh = cW[j] >= EPS, cH[:, j] >= EPS
            ew = np.abs(W[j][mw] - cW[j][mw]).max() / np.abs(cW[j]).max() if mw.any() else 0.0
            eh = np.abs(H[:, j][mh] - cH[:, j][mh]).max() / np.abs(cH[:, j]).max() if mh.any() else 0.0
            if max(ew, eh) < best:
                best, zw, zh = max(ew, eh), ~mw, ~mh
        assert best < 1e-8, (j, best)
        if method == 2:
            assert np.allclose(W[j][zw], mean, rtol=1e-12) and np.allclose(H[:, j][zh], mean, rtol=1e-12)
        elif method == 3:
            assert (W[j][zw] < EPS).all() and (H[:, j][zh] < EPS).all()
        elif mean * 0.001 > EPS:
            assert ((W[j][zw] >= EPS) & (W[j][zw] <= mean * 0.001)).all()
            assert ((H[:, j][zh] >= EPS) & (H[:, j][zh] <= mean * 0.001)).all()
