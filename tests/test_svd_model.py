"""CPU tests of oracle/jacobi_model.py, the numpy restatement of the driver of kernels_svd.hip (tournament pairing,
dead-row rule, 1e-15 rotation test, sweep count), and of what tests/test_gpu_svd.py takes for granted about its own
generators (cluster caps, no coverage threshold at a tie) -- from LAPACK's values alone, no GPU."""
import itertools
import re
import os

import numpy as np
import pytest

import jacobi_model as jm
import test_gpu_svd as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", range(1, 67))
def test_tournament_visits_every_pair_once(n):
    """a sweep = m - 1 rounds (m = n rounded up to even); the pairs of a round are disjoint (one workgroup each, no row
    shared) and the rounds together hold every pair of the n rows exactly once, odd n included (padding player m - 1)"""
    m = (n + 1) & ~1
    seen = []
    for r in range(m - 1):
        raw = [jm.tournament_pair(m, r, i) for i in range(m // 2)]
        players = [x for pq in raw for x in pq]
        assert sorted(players) == list(range(m)), (n, r)            # a perfect matching of the m players
        assert all(p < q for p, q in raw)
        P, Q = jm.round_pairs(n, r)
        assert len(P) == (m // 2 if n == m else m // 2 - 1) or n == 1
        seen += list(zip(P.tolist(), Q.tolist()))
    assert sorted(seen) == list(itertools.combinations(range(n), 2))


def test_model_constants_are_the_kernel_s():
    """the model's tolerance, dead-row factor and sweep cap are the ones in the sources"""
    k = open(os.path.join(ROOT, "flucoma-core_amd", "csrc", "kernels_svd.hip")).read()
    a = open(os.path.join(ROOT, "flucoma-core_amd", "csrc", "api_algorithms.hip")).read()
    assert float(re.search(r"kJacobiTol\s*=\s*([0-9.eE+-]+)", k).group(1)) == jm.JACOBI_TOL
    assert float(re.search(r"zero2\s*=\s*fro2\s*\*\s*([0-9.eE+-]+)", k).group(1)) == jm.ZERO2_FACTOR
    assert int(re.search(r"dFlag\.as<unsigned>\(\),\s*(\d+),", a).group(1)) == jm.MAX_SWEEPS


SMALL = [(T, F, n) for T, F, n in gs.CASES if max(T, F) <= 65 and n != "stft_chord"]


@pytest.mark.parametrize("T,F,name", SMALL, ids=[f"{T}x{F}-{n}" for T, F, n in SMALL])
def test_model_against_lapack(T, F, name):
    """the model passes the assertions the device SVD is held to (values, orthonormality, reconstruction, subspaces,
    dead pairs, 1 <= sweeps <= 40), with the same LAPACK-derived bars"""
    X = gs.make_input(name, T, F)
    ref = gs._lapack_side(X)
    s, U, VT, sweeps = jm.jacobi_svd(X)
    gs.check_factors(X, s, U, VT, sweeps, ref, f"model {T}x{F} {name}", graded=(name == "graded"))


def test_model_dead_row_rule_is_needed():
    """without zero2 the rows of an exactly rank-deficient input rotate among themselves until the cap"""
    X = gs.gen_exact_rank_5(40, 65, 3)
    assert jm.jacobi_svd(X, vectors=False)[3] > 0
    assert jm.jacobi_svd(X, vectors=False, zero2_factor=0.0)[3] == -1


GEN_CASES = [c for c in gs.NNDSVD_CASES if c[2] != "stft_chord"]


@pytest.mark.parametrize("T,F,name", GEN_CASES, ids=[f"{T}x{F}-{n}" for T, F, n in GEN_CASES])
def test_generators_meet_their_caps(T, F, name):
    """from LAPACK's singular values alone: the share of the leading components a case leaves out of the vector
    comparison is within its cap, and no coverage threshold sits within 1e-9 of a step of the cumulative coverage
    (equal_blocks at 0.5 excepted: 4 of 8 equal values)"""
    X = gs.make_input(name, T, F)
    s = np.linalg.svd(X.T, compute_uv=False)
    K = gs.components_of(name, s)
    out, _ = gs._clustered(s, K)
    n_out = int(out[:gs.n_live(s)].sum())
    if name in gs.CLUSTER_CAP:
        assert n_out <= gs.CLUSTER_CAP[name], n_out
    assert n_out <= max(K // 2, gs.CLUSTER_CAP.get(name, 0))
    for amount in gs.COVERAGES:
        margin = gs.crossing_margin(s, amount)
        if name == "equal_blocks" and amount == 0.5:
            assert margin < 1e-9
        else:
            assert margin > 1e-9, (amount, margin)


def test_graded_reference_is_graded():
    X = gs.make_input("graded", 64, 64)
    ref, how = gs.graded_reference(X)
    assert ref.shape == (64,) and (np.diff(ref) < 0).all()
    assert np.abs(ref - gs.graded_values(64)).max() < 1e-14            # Weyl: the stored matrix is within rounding of the design
