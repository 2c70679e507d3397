"""The one-sided Jacobi SVD behind NNDSVD / BufNMFSeed (kernels_svd.hip) against LAPACK in float64, at the shapes
the kernel's header names and on spectra that are hard for Jacobi: tails of close values, exact zeros, exact low rank,
repeated values, thirteen decades of grading.

fluhip_debug_jacobi_svd_f64 hands back what production computes (all r = min(F, T) pairs and the sweep count of the same
nndsvd_device call fluhip_nndsvd_f64 and fluhip_bufnmfseed_f32 make), so the factorisation itself is tested: values,
orthonormality of both factors, reconstruction, singular SUBSPACES (clusters closer than 1e-6 s_0 are compared through
their projectors), dead pairs, the sweep count.  Then the two public entry points at the same inputs.

Tolerances.  No bar here comes from the kernel.  For every case the test measures the same quantity on LAPACK's own
factors (`_lapack_side`): orthonormality and reconstruction of numpy.linalg.svd's output, and for the singular values
gesdd against gesvd (scipy) or, without scipy, numpy's SVD of X against that of X^T.  The bar is
max(64 x LAPACK's figure, 64 eps sqrt(max(T, F))): Jacobi is at least as accurate as bidiagonalisation, 64 is room for
the summation order.  `graded` is asserted RELATIVE per value against 50-digit mpmath values (or, without mpmath, the
values the matrix was built from), the bar being 64 x LAPACK's own worst relative error against the same reference.

MEASURED (MI355X; the full table shape x input -> sweeps is in DESIGN.md, "Jacobi SVD: sweeps and accuracy").  Wall
time of one ctx.jacobi_svd call (upload, sweeps, 2 r row downloads, host sort and normalisation: not device time): < 10 ms up to 64 x 64, 28 - 104 ms at 300 x 513, 38 - 174 ms at 100 x 1025, 91 - 285 ms at 862 x 1025,
61 - 137 ms at 3000 x 513, 68 - 141 ms at 10000 x 257; the whole file runs in 25 s.  Sweeps: at most 17 on magnitudes, 24
(of 40) on `graded` 64 x 64.  Kernel figure / bar, worst case per quantity:
  s       5.8e-15  / 4.55e-13  (100x1025 tonal; LAPACK gesdd vs gesvd 2.4e-16)
  orth U  6.9e-15  / 7.78e-13  (3000x513 stft_chord; LAPACK 3.2e-15);  6.2e-15 / 4.55e-13 at 862x1025 stft_chord
  orth V  3.3e-15  / 7.78e-13  (3000x513 tonal)
  rec     1.74e-13 / 5.21e-13  (100x1025 lowrank_noise; LAPACK 8.1e-15)                       within 4x of its bar
          7.3e-14  / 8.65e-13  (300x513 lowrank_noise), 7.1e-14 / 5.02e-12 (862x1025 lowrank_noise), 3.9e-14 / 2.38e-13
          (40x65 noise); every other case below 2e-14
  subspace: worst ratio to its bar 2.3e-2
  graded, relative per value against mpmath: 64x64 5.84e-6 / 1.01e-4 (LAPACK 1.58e-6); 7x33 3.1e-7 / 2.6e-6 (LAPACK 4.1e-8)
These tests found a defect, fixed with them: with the rotation applied as c x - s y, s x + c y, max |U U^T - I| was
5.02e-13 at 862x1025 stft_chord (bar 4.55e-13), 4.54e-13 at 862x1025 lowrank_noise, s off by 2.0e-13 s_0 (kernels_svd.hip,
DESIGN.md).  Public entry points: method 0 at 1e-8 measured <= 2e-12; BufNMFSeed at 1e-5 measured <= 2e-11.

Silence (test_silence_*), the reading of the reference: NNDSVD.hpp:49-58 forms `current / total` with total = 0, and
`NaN < amount` is false, so the loop does not run and k = minRank.  Method 0 then writes |U_k| (some orthonormal
vectors) and |S_k V_k^T| = 0.  NMFSeedClient.hpp:120-128 takes maxH = 0 and multiplies the envelopes by 1 / 0: every
activation the reference writes is 0 * inf = NaN.  Methods 1..3 divide a zero vector by its zero norm (:90-100): NaN as
well.  The library reproduces what is defined (the rank, the zero H of method 0) and refuses what is not:
FLUHIP_ERROR with a message, no output written, instead of NaN with FLUHIP_OK.
"""
import time

import numpy as np
import pytest

from conftest import rel_err

EPS = float(np.finfo(np.float64).eps)
LIVE = 1e-10        # pairs with s_i > LIVE s_0 are "live"
CLUSTER = 1e-6      # neighbours closer than CLUSTER s_0 share a cluster
COVERAGES = (0.3, 0.5, 0.8, 0.95, 0.999)


# ---------------------------------------------------------------------------------------------------------------------
# inputs: seeded generators, T x F, non-negative (graded excepted)
# ---------------------------------------------------------------------------------------------------------------------
def gen_lowrank_noise(T, F, seed):
    """tests/test_gpu_parity.py's helper: well separated leading values over a 1e-3 noise floor"""
    rs = np.random.RandomState(seed)
    r = 12
    scales = np.linspace(3.0, 0.3, r)
    return (np.abs(rs.standard_normal((T, r))) * scales) @ np.abs(rs.standard_normal((r, F))) + 1e-3 * rs.uniform(0, 1, (T, F))


def gen_noise(T, F, seed):
    return np.random.RandomState(seed).uniform(0, 1, (T, F))


def gen_tonal(T, F, seed):
    """up to 20 partials of three bins each with on/off envelopes; exact zeros everywhere else"""
    rs = np.random.RandomState(seed)
    X = np.zeros((T, F))
    n_part = min(20, max(1, F // 4))
    centres = rs.choice(np.arange(1, max(2, F - 1)), size=n_part, replace=False) if F > 2 else np.zeros(1, dtype=int)
    for c in centres:
        env = np.zeros(T)
        t = 0
        while t < T:
            seg = int(rs.randint(1, max(2, T // 6 + 1)))
            if rs.uniform() < 0.5:
                env[t:t + seg] = rs.uniform(0.2, 1.0)
            t += seg
        if not env.any():
            env[int(rs.randint(0, T))] = 1.0
        amp = rs.uniform(0.3, 3.0)
        for db, g in ((-1, 0.25), (0, 1.0), (1, 0.25)):
            if 0 <= c + db < F:
                X[:, c + db] += amp * g * env
    return X


def gen_exact_rank_5(T, F, seed):
    rs = np.random.RandomState(seed)
    k = min(5, T, F)
    return rs.uniform(0, 1, (T, k)) @ rs.uniform(0, 1, (k, F))


def gen_equal_blocks(T, F, seed=0):
    """8 disjoint all-ones blocks of one size: 8 equal singular values sqrt(T//8 * F//8), then exact zeros"""
    assert T >= 8 and F >= 8
    X = np.zeros((T, F))
    tb, fb = T // 8, F // 8
    for i in range(8):
        X[i * tb:(i + 1) * tb, i * fb:(i + 1) * fb] = 1.0
    return X


def graded_values(r):
    return 10.0 ** np.linspace(0.0, -12.0, r)


def gen_graded(T, F, seed):
    """U diag(10^0 .. 10^-12) V^T with orthonormal U, V from a QR of seeded noise; signed"""
    assert max(T, F) <= 64
    rs = np.random.RandomState(seed)
    r = min(T, F)
    Qt, _ = np.linalg.qr(rs.standard_normal((T, r)))
    Qf, _ = np.linalg.qr(rs.standard_normal((F, r)))
    return (Qt * graded_values(r)) @ Qf.T


GENERATORS = {"lowrank_noise": gen_lowrank_noise, "noise": gen_noise, "tonal": gen_tonal,
              "exact_rank_5": gen_exact_rank_5, "equal_blocks": gen_equal_blocks, "graded": gen_graded}

# (T, F, input, seed).  The full-size shapes take lowrank_noise, tonal and stft_chord; the small ones take everything
# that is defined there (equal_blocks needs 8 x 8, graded at most 64 x 64).
SMALL_SHAPES = [(1, 33), (33, 1), (2, 2), (7, 33), (64, 64), (40, 65)]
FULL_SHAPES = [(300, 513), (100, 1025), (862, 1025), (3000, 513), (10000, 257)]
# stft_chord: (samples, window, fft, hop) giving the shape
CHORD = {(40, 65): (4992, 128, 128, 128), (300, 513): (76544, 1024, 1024, 256), (100, 1025): (50688, 2048, 2048, 512),
         (862, 1025): (441000, 2048, 2048, 512), (3000, 513): (767744, 1024, 1024, 256), (10000, 257): (1279872, 512, 512, 128)}


def _cases():
    out = []
    for T, F in SMALL_SHAPES:
        names = ["lowrank_noise", "noise", "tonal", "exact_rank_5"]
        if T >= 8 and F >= 8:
            names.append("equal_blocks")
        if max(T, F) <= 64:
            names.append("graded")
        if (T, F) in CHORD:
            names.append("stft_chord")
        out += [(T, F, n) for n in names]
    for T, F in FULL_SHAPES:
        out += [(T, F, n) for n in ("lowrank_noise", "tonal", "stft_chord")]
    return out


CASES = _cases()


def make_input(name, T, F, ctx=None, onp=None):
    """the input of a case; the seed is a function of the case alone"""
    if name == "stft_chord":
        n, win, fft, hop = CHORD[(T, F)]
        x = onp.synth_audio(n, 900 + T)
        _, mag = ctx.stft(x.astype(np.float64), win, fft, hop, want_spec=False)
        assert mag.shape == (T, F), mag.shape
        return np.ascontiguousarray(mag)
    return GENERATORS[name](T, F, 1000 + 7 * T + F)


# ---------------------------------------------------------------------------------------------------------------------
# the reference side
# ---------------------------------------------------------------------------------------------------------------------
def clusters_of(s_ref, live):
    """index lists of the live values, neighbours closer than CLUSTER s_0 sharing a list"""
    out, cur = [], []
    for i in range(live):
        if cur and s_ref[cur[-1]] - s_ref[i] >= CLUSTER * s_ref[0]:
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


def n_live(s):
    return int(np.sum(s > LIVE * s[0])) if s[0] > 0 else 0


def _orth(M):
    return float(np.abs(M @ M.T - np.eye(M.shape[0])).max()) if M.shape[0] else 0.0


def _lapack_side(X):
    """LAPACK's factors of X^T and LAPACK's own residuals, the figures every bar is derived from"""
    T, F = X.shape
    U, s, VT = np.linalg.svd(X.T, full_matrices=False)          # U [F, r], VT [r, T]
    floor = 64 * EPS * np.sqrt(max(T, F))
    live = n_live(s)
    orth = max(_orth(U[:, :live].T), _orth(VT[:live]))
    xmax = float(np.abs(X).max())
    rec = float(np.abs((U * s) @ VT - X.T).max()) / xmax if xmax > 0 else 0.0
    try:
        import scipy.linalg
        s_other = scipy.linalg.svd(X.T, full_matrices=False, compute_uv=False, lapack_driver="gesvd")
    except ImportError:
        s_other = np.linalg.svd(X, compute_uv=False)
    ds = float(np.abs(s - s_other).max()) / s[0] if s[0] > 0 else 0.0
    return dict(U=U, s=s, VT=VT, live=live, orth_ref=orth, rec_ref=rec, s_ref_err=ds,
                tol_orth=max(64 * orth, floor), tol_rec=max(64 * rec, floor), tol_s=max(64 * ds, floor))


_GRADED_REF = {}


def graded_reference(X):
    """singular values of the stored matrix at 50 digits (mpmath), or the values it was built from"""
    key = X.shape
    if key not in _GRADED_REF:
        try:
            import mpmath
            with mpmath.workdps(50):
                sv = mpmath.svd_r(mpmath.matrix(X.T.tolist()), compute_uv=False)
                ref = np.sort(np.array([float(v) for v in sv]))[::-1]
            _GRADED_REF[key] = (ref, "mpmath")
        except ImportError:
            _GRADED_REF[key] = (graded_values(min(X.shape)), "construction")
    return _GRADED_REF[key]


def crossing_margin(s_ref, amount):
    """distance of LAPACK's cumulative coverage from `amount` on either side of the step where it crosses"""
    cov = np.cumsum(s_ref) / np.sum(s_ref)
    k = int(np.searchsorted(cov, amount, side="left")) + 1     # first k with cov[k-1] >= amount
    k = min(k, len(s_ref))
    below = amount - (cov[k - 2] if k >= 2 else 0.0)
    above = cov[k - 1] - amount
    return min(abs(below), abs(above))


# ---------------------------------------------------------------------------------------------------------------------
# fluhip_debug_jacobi_svd_f64
# ---------------------------------------------------------------------------------------------------------------------
def check_factors(X, s, U, VT, sweeps, ref, tag, graded=False):
    """every assertion on (s, U, VT) of X^T; returns the measured figures"""
    T, F = X.shape
    r = min(T, F)
    s_ref, s0 = ref["s"], ref["s"][0]
    assert s.shape == (r,) and U.shape == (r, F) and VT.shape == (r, T)
    assert np.isfinite(s).all() and np.isfinite(U).all() and np.isfinite(VT).all(), tag
    assert (s >= 0).all() and (np.diff(s) <= 0).all(), tag
    assert 1 <= sweeps <= 40, tag
    err_s = float(np.abs(s - s_ref).max()) / s0
    live = r if graded else ref["live"]
    orth_u, orth_v = _orth(U[:live]), _orth(VT[:live])
    orth = max(orth_u, orth_v)
    rec = float(np.abs((U.T * s) @ VT - X.T).max()) / float(np.abs(X).max())
    # subspaces: per cluster of the reference's live values, the projector onto span(u_i); a single vector up to sign
    sub_worst, sub_ratio = 0.0, 0.0
    Ur = ref["U"]
    for c in clusters_of(s_ref, live):
        lo, hi = c[0], c[-1]
        gap = min(s_ref[lo - 1] - s_ref[lo] if lo > 0 else np.inf, s_ref[hi] - s_ref[hi + 1] if hi + 1 < r else s_ref[hi])
        bar = ref["tol_rec"] * s0 / gap
        if len(c) == 1:
            u, v = U[lo], Ur[:, lo]
            d = min(float(np.abs(u - v).max()), float(np.abs(u + v).max()))
        else:
            d = float(np.abs(U[c].T @ U[c] - Ur[:, c] @ Ur[:, c].T).max())
        if bar < 1.0:                      # a bar above 1 says nothing about unit vectors
            sub_worst = max(sub_worst, d)
            sub_ratio = max(sub_ratio, d / bar)
    fig = dict(err_s=err_s, orth=orth, rec=rec, sub=sub_worst, sub_ratio=sub_ratio, sweeps=sweeps)
    msg = (f"{tag}: sweeps {sweeps}  s {err_s:.2e} (bar {ref['tol_s']:.2e}, LAPACK {ref['s_ref_err']:.2e})  "
           f"orth U {orth_u:.2e} V {orth_v:.2e} (bar {ref['tol_orth']:.2e}, LAPACK {ref['orth_ref']:.2e})  "
           f"rec {rec:.2e} (bar {ref['tol_rec']:.2e}, LAPACK {ref['rec_ref']:.2e})  "
           f"subspace {sub_worst:.2e} (worst ratio to its bar {sub_ratio:.2e})")
    print(msg)
    assert err_s <= ref["tol_s"], msg
    assert orth <= ref["tol_orth"], msg
    assert rec <= ref["tol_rec"], msg
    assert sub_ratio <= 1.0, msg
    dead = np.zeros(r, dtype=bool) if graded else s_ref <= LIVE * s0
    assert (s[dead] <= ref["tol_s"] * s0).all(), msg
    return fig


@pytest.mark.gpu
@pytest.mark.parametrize("T,F,name", CASES, ids=[f"{T}x{F}-{n}" for T, F, n in CASES])
def test_jacobi_svd_vs_lapack(ctx, onp, T, F, name):
    """values, orthonormality, reconstruction, subspaces, dead pairs and the sweep count of the production SVD"""
    X = make_input(name, T, F, ctx, onp)
    ref = _lapack_side(X)
    t0 = time.perf_counter()
    s, U, VT, sweeps = ctx.jacobi_svd(X)
    ms = (time.perf_counter() - t0) * 1e3
    tag = f"{T}x{F} {name} ({ms:.0f} ms)"
    if max(T, F) <= 65:                                  # the numpy model's count: informative, the sums differ
        import jacobi_model
        tag += f" model sweeps {jacobi_model.jacobi_svd(X, vectors=False)[3]}"
    if name == "graded":
        g_ref, how = graded_reference(X)
        ok = g_ref >= 1e-12 * g_ref[0] * (1 - 1e-9)
        rel = float((np.abs(s - g_ref) / g_ref)[ok].max())
        rel_lapack = float((np.abs(ref["s"] - g_ref) / g_ref)[ok].max())
        tol_rel = max(64 * rel_lapack, 64 * EPS * np.sqrt(max(T, F)))
        tag += f" graded rel {rel:.2e} (bar {tol_rel:.2e}, LAPACK {rel_lapack:.2e}, reference: {how})"
        check_factors(X, s, U, VT, sweeps, ref, tag, graded=True)
        assert rel <= tol_rel, tag
    else:
        check_factors(X, s, U, VT, sweeps, ref, tag)


@pytest.mark.gpu
def test_jacobi_svd_strided_and_repeatable(ctx):
    """ldx > F reads the same matrix; a second run on the same context gives the same bits"""
    big = gen_lowrank_noise(60, 80, 3)
    X = big[:, :33]
    a = ctx.jacobi_svd(X)
    b = ctx.jacobi_svd(np.ascontiguousarray(X))
    c = ctx.jacobi_svd(X)
    for p, q, r_ in zip(a, b, c):
        assert np.array_equal(p, q) and np.array_equal(p, r_)


# ---------------------------------------------------------------------------------------------------------------------
# fluhip_nndsvd_f64
# ---------------------------------------------------------------------------------------------------------------------
# every shape and every magnitude input of CASES (graded is signed: it is no spectrogram and goes through jacobi_svd only)
NNDSVD_CASES = [c for c in CASES if c[2] != "graded"]
# components a case may leave out of the vector comparison because their singular value shares a cluster
CLUSTER_CAP = {"lowrank_noise": 0, "tonal": 0, "stft_chord": 0, "graded": 0, "equal_blocks": 8}
# components asked for: the structure each generator has (12 factors over a noise floor, at most 20 partials, rank 5,
# 8 blocks), never more than the reference calls live
N_COMPONENTS = {"lowrank_noise": 12, "noise": 24, "tonal": 16, "exact_rank_5": 5, "equal_blocks": 8, "stft_chord": 24}


def components_of(name, s_ref):
    return max(1, min(len(s_ref), N_COMPONENTS[name], n_live(s_ref)))


def _clustered(s_ref, k):
    live = n_live(s_ref)
    member = np.zeros(len(s_ref), dtype=bool)
    groups = []
    for c in clusters_of(s_ref, live):
        if len(c) > 1:
            member[c] = True
            groups.append(c)
    member[live:] = True                                  # dead pairs: vectors unspecified
    return member[:k], [g for g in groups if g[-1] < k]


@pytest.mark.gpu
@pytest.mark.parametrize("T,F,name", NNDSVD_CASES, ids=[f"{T}x{F}-{n}" for T, F, n in NNDSVD_CASES])
def test_nndsvd_method0_new_shapes(ctx, onp, T, F, name):
    """method 0 against oracle_np.nndsvd at 1e-8 over the components whose value is alone in its cluster; clustered
    components through sum_c W_j^2 / sum_c H_j^2 (the diagonal of the cluster's projector, basis-free); the rank rule at
    five coverages and at amount == 0, after asserting that the reference is not at a tie there"""
    X = make_input(name, T, F, ctx, onp)
    r = min(T, F)
    U, s_ref, VT = np.linalg.svd(X.T, full_matrices=False)
    K = components_of(name, s_ref)
    W, H, k = ctx.nndsvd(X, K, K, K, 0.0, 0, 42)
    rW, rH, rk = onp.nndsvd_from_svd(U, s_ref, VT, X, K, K, K, 0.0, 0, 42)
    assert k == rk == K
    assert np.isfinite(W).all() and np.isfinite(H).all()
    out, groups = _clustered(s_ref, K)
    n_out = int(out[:n_live(s_ref)].sum())
    if name in CLUSTER_CAP:
        assert n_out <= CLUSTER_CAP[name], (name, n_out)
    assert n_out <= max(K // 2, CLUSTER_CAP.get(name, 0)), (name, n_out)
    keep = ~out
    if keep.any():
        ew = np.abs(W[keep] - rW[keep]).max() / np.abs(rW).max()
        eh = np.abs(H[:, keep] - rH[:, keep]).max() / np.abs(rH).max()
        print(f"{T}x{F} {name}: method 0 W {ew:.2e} H {eh:.2e} over {int(keep.sum())} of {K} components")
        assert ew < 1e-8 and eh < 1e-8, (ew, eh)
    for g in groups:
        pw, rpw = (W[g] ** 2).sum(0), (rW[g] ** 2).sum(0)
        ph, rph = (H[:, g] ** 2).sum(1), (rH[:, g] ** 2).sum(1)
        assert np.abs(pw - rpw).max() < 1e-8 * max(rpw.max(), 1e-300), (g, np.abs(pw - rpw).max())
        assert np.abs(ph - rph).max() < 1e-8 * max(rph.max(), 1e-300), (g, np.abs(ph - rph).max())
    # the rank rule
    for amount in COVERAGES:
        rk = onp.nndsvd_rank(s_ref, 0, r, amount)
        margin = crossing_margin(s_ref, amount)
        _, _, k = ctx.nndsvd(X, r, 0, r, amount, 0, 42)
        if name == "equal_blocks" and amount == 0.5:
            # the one structural tie: 4 of 8 EQUAL values are exactly half of the sum, `current / total < 0.5` is
            # decided by the last bit of either SVD
            assert margin < 1e-9 and k in (4, 5), (k, margin)
            continue
        assert margin > 1e-9, f"the reference itself is at a tie: coverage {amount}, margin {margin:.2e}"
        assert k == rk, (amount, k, rk)
    _, _, k = ctx.nndsvd(X, r, min(3, r), r, 0.0, 0, 42)
    assert k == min(3, r)


def _signed_reference(onp, Wg, Hg, U, s, VT, X, k, w_rows, method):
    """the oracle's construction from LAPACK's SVD with each pair's sign chosen as the device's SVD chose it (a pair
    is defined up to a common sign; methods 1..3 follow it, in the reference as well).  Wg [k.., F], Hg [T, k..]: the
    device's factors; both decide, because with the reference's `yNNorm = xN.norm()` (:85) the two signs can select
    the same part of u and still scale v differently."""
    Uk, sk, VTk = U[:, :k].copy(), s[:k].copy(), VT[:k].copy()
    for j in range(1, k):
        best = None
        for sign in (1.0, -1.0):
            Uj, VTj = Uk.copy(), VTk.copy()
            Uj[:, j] *= sign
            VTj[j] *= sign
            cW, cH, _ = onp.nndsvd_from_svd(Uj, sk, VTj, X, w_rows, k, k, 0.0, 3, 42)
            mw, mh = cW[j] >= EPS, cH[:, j] >= EPS
            err = max(np.abs(Wg[j][mw] - cW[j][mw]).max() / np.abs(cW[j]).max(),
                      np.abs(Hg[:, j][mh] - cH[:, j][mh]).max() / np.abs(cH[:, j]).max())
            if best is None or err < best[0]:
                best = (err, sign)
        Uk[:, j] *= best[1]
        VTk[j] *= best[1]
    return onp.nndsvd_from_svd(Uk, sk, VTk, X, w_rows, k, k, 0.0, method, 42)


@pytest.mark.gpu
@pytest.mark.parametrize("method", [1, 2, 3])
@pytest.mark.parametrize("T,F", [(120, 65), (100, 1025), (862, 1025)])
def test_nndsvd_split_methods_new_shapes(ctx, onp, T, F, method):
    """test_nndsvd_split_methods' sign-tolerant comparison at the short-buffer and the config-1 shape"""
    K = 8
    X = gen_lowrank_noise(T, F, 5)
    W, H, k = ctx.nndsvd(X, K, K, K, 0.0, method, 42)
    assert k == K
    U, s, VT = np.linalg.svd(X.T, full_matrices=False)
    cW, cH, _ = _signed_reference(onp, W, H, U, s, VT, X, K, K, 3)
    mean = float(X.mean())
    for j in range(K):
        mw, mh = cW[j] >= EPS, cH[:, j] >= EPS
        err = max(np.abs(W[j][mw] - cW[j][mw]).max() / np.abs(cW[j]).max(),
                  np.abs(H[:, j][mh] - cH[:, j][mh]).max() / np.abs(cH[:, j]).max())
        assert err < 1e-8, (j, err)
        zw, zh = ~mw, ~mh
        if method == 1:
            assert ((W[j][zw] >= EPS) & (W[j][zw] <= mean * 0.001)).all() and ((H[:, j][zh] >= EPS) & (H[:, j][zh] <= mean * 0.001)).all()
        elif method == 2:
            assert np.allclose(W[j][zw], mean, rtol=1e-12) and np.allclose(H[:, j][zh], mean, rtol=1e-12)
        else:
            assert (W[j][zw] < EPS).all() and (H[:, j][zh] < EPS).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T,F,pad", [(60, 33, 1), (7, 33, 31), (300, 513, 7)])
def test_nndsvd_strided_input(ctx, onp, T, F, pad):
    """ldx > F: the rows of X sit `ldx` apart; the columns beyond F hold values that must not be read"""
    big = np.full((T, F + pad), 1e6)
    big[:, :F] = gen_lowrank_noise(T, F, T + F)
    X = big[:, :F]
    assert X.strides[0] == (F + pad) * 8
    K = min(T, F, 10)
    W, H, k = ctx.nndsvd(X, K, 0, K, 0.8, 0, 42)
    W2, H2, k2 = ctx.nndsvd(np.ascontiguousarray(X), K, 0, K, 0.8, 0, 42)
    assert k == k2 and np.array_equal(W, W2) and np.array_equal(H, H2)
    rW, rH, rk, *_ = onp.nndsvd(np.ascontiguousarray(X), K, 0, K, 0.8, 0, 42)
    assert k == rk and rel_err(W, rW) < 1e-8 and rel_err(H, rH) < 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# fluhip_bufnmfseed_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("coverage", [0.5, 0.9])
@pytest.mark.parametrize("n,win,fft,hop", [(441000, 2048, 2048, 512), (50000, 1024, 1024, 256)])
def test_bufnmfseed_padded_rows(ctx, oracle, onp, n, win, fft, hop, coverage, method):
    """BufNMFSeed at config 1's shape (862 frames in rows padded to 864) and at 196 frames (padded to 224): the sweeps
    work on rows of length T inside a leading dimension Tp > T.  Against oracle.stft_f32 + the oracle's NNDSVD at 1e-5;
    a second call on the same context gives the same bits (the sweeps work in place on the corpus' transposed copy)"""
    x = onp.synth_audio(n, 77)
    max_rank = 32
    bases, acts, k = ctx.bufnmfseed(x, win, fft, hop, 1, max_rank, coverage, method, 42)
    _, mag = oracle.stft_f32(x, win, fft, hop)
    T, F = mag.shape
    assert T % 32 != 0 and bases.shape == (max_rank, F) and acts.shape == (max_rank, T)
    U, s, VT = np.linalg.svd(mag.T, full_matrices=False)
    rk = min(max(onp.nndsvd_rank(s, 1, max_rank, coverage), 1), max_rank)
    assert crossing_margin(s, coverage) > 1e-9
    assert k == rk
    if method == 0:
        rW, rH, _ = onp.nndsvd_from_svd(U, s, VT, mag, max_rank, k, k, 0.0, 0, 42)
    else:
        # the envelopes before the client's 1 / max(H): component 0 does not depend on the sign, it gives the scale
        g = float(acts[0].max()) / float((np.sqrt(s[0]) * np.abs(VT[0])).max())
        rW, rH, _ = _signed_reference(onp, bases.astype(np.float64), acts.T.astype(np.float64) / g, U, s, VT, mag, k,
                                      max_rank, method)
    ra = rH.T.astype(np.float32) * np.float32(1.0 / rH.max())
    eb, ea = rel_err(bases[:k], rW[:k].astype(np.float32)), rel_err(acts[:k], ra[:k])
    print(f"bufnmfseed {T}x{F} coverage {coverage} method {method}: k {k} bases {eb:.2e} acts {ea:.2e}")
    assert eb < 1e-5 and ea < 1e-5, (eb, ea)
    assert (bases[k:] == 0).all() and (acts[k:] == 0).all()
    assert abs(float(acts.max()) - 1.0) < 1e-6
    b2, a2, k2 = ctx.bufnmfseed(x, win, fft, hop, 1, max_rank, coverage, method, 42)
    assert k2 == k and np.array_equal(b2, bases) and np.array_equal(a2, acts)


# ---------------------------------------------------------------------------------------------------------------------
# silence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_silence_nndsvd(ctx):
    """all-zero X (see the module docstring): 0 / 0 < amount is false, k = minRank; method 0 gives orthonormal |U_k| and
    H = 0 like the reference; methods 1..3 are 0 / 0 in the reference and an announced error here"""
    import fluhip
    X = np.zeros((20, 33))
    for min_rank in (0, 1, 3):
        W, H, k = ctx.nndsvd(X, 4, min_rank, 4, 0.8, 0, 42)
        assert k == min_rank
        assert np.isfinite(W).all() and (H == 0).all() and (W[k:] == 0).all()
        assert np.allclose(W[:k] @ W[:k].T, np.eye(k), atol=1e-14)
    s, U, VT, sweeps = ctx.jacobi_svd(X)
    assert (s == 0).all() and np.isfinite(U).all() and np.isfinite(VT).all() and sweeps == 1
    for method in (1, 2, 3):
        with pytest.raises(fluhip.FluhipError, match="not finite"):
            ctx.nndsvd(X, 4, 3, 4, 0.8, method, 42)
        # the error writes nothing: W, H and the rank keep what they held
        import ctypes
        dp = ctypes.POINTER(ctypes.c_double)
        W, H, k = np.full((4, 33), 7.0), np.full((20, 4), 7.0), ctypes.c_int64(-1)
        rc = ctx.lib.fluhip_nndsvd_f64(ctx.h, X.ctypes.data_as(dp), 20, 33, 33, 4, 3, 4, 0.8, method, 42,
                                       W.ctypes.data_as(dp), H.ctypes.data_as(dp), ctypes.byref(k))
        assert rc == fluhip.ERROR and (W == 7.0).all() and (H == 7.0).all() and k.value == -1


@pytest.mark.gpu
def test_silence_bufnmfseed(ctx, oracle, onp):
    """zero audio: the reference's client scales by 1 / max(H) = 1 / 0 and writes NaN (module docstring); the library
    says so instead -- FLUHIP_ERROR, outputs untouched (also with minimum rank 0, where the
    reference's rank is 0 and it writes nothing: the corpus path's silent bins are 1.5e-154, not 0, so the rank rule sees
    one component; the error is the same "no output").  Audio at 1e-30 is ordinary audio at a small scale: same bases
    and the same max-normalised activations as at full scale."""
    import fluhip
    win, fft, hop, max_rank = 1024, 1024, 256, 6
    n = 20000
    T, F = (n + hop) // hop, fft // 2 + 1
    lib, h = ctx.lib, ctx.h
    bases = np.full((max_rank, F), 7.0, dtype=np.float32)
    acts = np.full((max_rank, T), 7.0, dtype=np.float32)
    import ctypes
    fp = ctypes.POINTER(ctypes.c_float)
    k = ctypes.c_int64(-1)
    zero = np.zeros(n, dtype=np.float32)
    rc = lib.fluhip_bufnmfseed_f32(h, zero.ctypes.data_as(fp), n, 1, win, fft, hop, 1, max_rank, 0.5, 0, 42,
                                   bases.ctypes.data_as(fp), acts.ctypes.data_as(fp), ctypes.byref(k))
    assert rc == fluhip.ERROR and b"silent" in lib.fluhip_last_error(h)
    assert (bases == 7.0).all() and (acts == 7.0).all() and k.value == -1
    # bases alone (acts_out == NULL) need no 1 / max: silence gives one finite, unit-norm basis as before
    rc = lib.fluhip_bufnmfseed_f32(h, zero.ctypes.data_as(fp), n, 1, win, fft, hop, 1, max_rank, 0.5, 0, 42,
                                   bases.ctypes.data_as(fp), None, ctypes.byref(k))
    assert rc == fluhip.OK and k.value == 1 and np.isfinite(bases).all() and (bases[1:] == 0).all()
    assert abs(float(np.linalg.norm(bases[0].astype(np.float64))) - 1.0) < 1e-6
    for method, min_rank in ((2, 1), (0, 0), (3, 2)):
        with pytest.raises(fluhip.FluhipError, match="silent|not finite"):
            ctx.bufnmfseed(zero, win, fft, hop, min_rank, max_rank, 0.5, method, 42)
    x = onp.synth_audio(n, 31)
    tiny = (x.astype(np.float64) * 1e-30).astype(np.float32)
    bt, at, kt = ctx.bufnmfseed(tiny, win, fft, hop, 1, max_rank, 0.5, 0, 42)
    assert np.isfinite(bt).all() and np.isfinite(at).all()
    _, mag = oracle.stft_f32(tiny, win, fft, hop)
    rW, rH, rk, *_ = onp.nndsvd(mag, max_rank, 1, max_rank, 0.5, 0, 42)
    assert kt == rk
    ra = rH.T.astype(np.float32) * np.float32(1.0 / rH.max())
    assert rel_err(bt[:kt], rW[:kt].astype(np.float32)) < 1e-5 and rel_err(at[:kt], ra[:kt]) < 1e-5
    assert abs(float(at.max()) - 1.0) < 1e-6
    const = np.full(n, 1e-30, dtype=np.float32)
    bc, ac, kc = ctx.bufnmfseed(const, win, fft, hop, 1, max_rank, 0.5, 0, 42)
    _, mag = oracle.stft_f32(const, win, fft, hop)
    rW, rH, rk, *_ = onp.nndsvd(mag, max_rank, 1, max_rank, 0.5, 0, 42)
    assert kc == rk and np.isfinite(bc).all() and np.isfinite(ac).all()
    ra = rH.T.astype(np.float32) * np.float32(1.0 / rH.max())
    assert rel_err(bc[:1], rW[:1].astype(np.float32)) < 1e-5 and rel_err(ac[:1], ra[:1]) < 1e-5
