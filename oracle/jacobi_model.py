"""numpy model of the one-sided Jacobi SVD of flucoma-core_amd/csrc/kernels_svd.hip (test infrastructure).

It restates the driver's logic, not its arithmetic order: the round-robin tournament that pairs the rows
(`tournament_pair`), the power-of-two scaling to max|G| in [0.5, 1), the dead-row rule (`zero2 = 2e-29 |G|_F^2`), the
rotation test `|x.y| > 1e-15 |x||y|`, "a sweep that rotates no pair ends the iteration", the cap of 40 sweeps, the
stable descending sort of the row norms and the normalisation of the rows.  The sums are numpy's pairwise sums, the
kernel's are 256 strided lanes and a tree, so the sweep COUNT of the model is a guide to the kernel's and no more.

    s, U, VT, sweeps = jacobi_svd(X)        # X: [T, F]; the SVD of X^T (F x T) like fluhip_debug_jacobi_svd_f64
"""
from __future__ import annotations

import numpy as np

JACOBI_TOL = 1e-15      # kJacobiTol
ZERO2_FACTOR = 2.0e-29  # zero2 = ZERO2_FACTOR * |G|_F^2
MAX_SWEEPS = 40


def tournament_pair(m: int, r: int, i: int):
    """round-robin tournament on m (even) players: round r in [0, m-1), pair i in [0, m/2) -> (p, q), p < q"""
    mm = m - 1
    if i == 0:
        p, q = mm, r % mm
    else:
        p, q = (r + i) % mm, (r - i + mm) % mm
    return (q, p) if p > q else (p, q)


def round_pairs(n: int, r: int):
    """the pairs of round r for n rows (m = n rounded up to even; pairs with the padding player are dropped)"""
    m = (n + 1) & ~1
    pq = [tournament_pair(m, r, i) for i in range(m // 2)]
    pq = [(p, q) for p, q in pq if q < n]
    return np.array([p for p, _ in pq], dtype=np.int64), np.array([q for _, q in pq], dtype=np.int64)


def range_exponent(max_abs: float) -> int:
    """svd_range_exponent (range_scale.h): e with max_abs * 2^-e in [0.5, 1); 0 for zero or non-finite"""
    if not (max_abs > 0 and np.isfinite(max_abs)):
        return 0
    return int(np.frexp(max_abs)[1])


def jacobi_svd(X, max_sweeps: int = MAX_SWEEPS, tol: float = JACOBI_TOL, zero2_factor: float = ZERO2_FACTOR,
               vectors: bool = True):
    """SVD of X^T for X [T, F]: s [r] descending, U [r, F] (row j = u_j), VT [r, T], sweeps; r = min(F, T).
    sweeps is -1 when max_sweeps did not reach "no rotation in a whole sweep".  vectors=False skips the accumulated
    rotations (U is None): the singular values and the count only."""
    X = np.asarray(X, dtype=np.float64)
    T, n = X.shape
    e = range_exponent(float(np.abs(X).max()) if X.size else 0.0)
    G = np.ldexp(X.T.copy(), -e)                                 # [n, T], one bin per row
    J = np.eye(n) if vectors else None
    zero2 = float((G * G).sum()) * zero2_factor
    m = (n + 1) & ~1
    rounds = [round_pairs(n, r) for r in range(m - 1)]
    sweeps = -1
    for sw in range(max_sweeps):
        rotated = False
        for P, Q in rounds:
            if P.size == 0:
                continue
            x, y = G[P], G[Q]
            a = np.einsum("ij,ij->i", x, x)
            b = np.einsum("ij,ij->i", y, y)
            d = np.einsum("ij,ij->i", x, y)
            lim = np.sqrt(a) * np.sqrt(b)
            rot = (a > zero2) & (b > zero2) & (np.abs(d) > tol * lim)
            if not rot.any():
                continue
            rotated = True
            dd = np.where(rot, d, 1.0)
            with np.errstate(over="ignore"):                     # zeta^2 = inf gives t = 0, as in the kernel
                zeta = (b - a) / (2.0 * dd)
                t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = np.where(rot, c * t, 0.0)
            tau = (s / (1.0 + c))[:, None]                       # the kernel's form: c = 1 - s tau is never stored
            s = s[:, None]
            G[P], G[Q] = x - s * (y + tau * x), y + s * (x - tau * y)
            if vectors:
                jx, jy = J[P], J[Q]
                J[P], J[Q] = jx - s * (jy + tau * jx), jy + s * (jx - tau * jy)
        if not rotated:
            sweeps = sw + 1
            break
    norms = np.sqrt(np.einsum("ij,ij->i", G, G))
    order = np.argsort(-norms, kind="stable")
    r = min(n, T)
    order = order[:r]
    sv = norms[order]
    VT = G[order].copy()
    live = sv > 0
    VT[live] /= sv[live, None]
    return np.ldexp(sv, e), (J[order].copy() if vectors else None), VT, sweeps
