"""A corpus runs the plan the planner reports: `fluhip_corpus_plan` (what corpus_loop.hip launches from) against the same
projection of `fluhip_debug_plan_shape` (corpus_plan.hip decide_update_plan, no device), slot by slot, for one small shape of
every schedule regime.  The corpus holds ONE UpdatePlan and both calls read it; a second copy of the plan's fields on the corpus
-- as there was up to round 6 -- shows here the moment the two disagree.

Creation only allocates and zero-fills: no audio goes up, no iteration runs.  The shapes are the smallest found of each regime at
real transform sizes (129 bins and up); which regime a shape is in comes from the debug call's own answer, so a planner change
cannot silently move a shape out of its regime and leave that regime unchecked.
"""
import ctypes

import pytest

# name -> (buffers, frames, bins, rank)
SHAPES = {
    "frame_strip": (1, 87, 129, 3),
    "uniform_side_column": (512, 87, 257, 32),        # the two-launch iteration of rank 32: the H update takes everything over
    "split_contraction": (1, 862, 2049, 100),
    "lists_compute_rank": (8, 173, 513, 20),          # arrays of rank 32, the updates compute 24
    "lists_plain_rank": (8, 173, 513, 32),
    "two_launch_h": (128, 257, 129, 100),
    "uniform_off_size": (512, 87, 129, 100),          # arrays of rank 128, the updates compute 104; runs in round-major windows
    "any_rank": (2, 87, 129, 200),
}


def _uniform(p):
    return p[0] == 5 and not p[9] and not p[8] and p[1] == 1 and p[2] == 1 and p[10] <= 1


# what puts a plan (the 32 slots of fluhip_debug_plan_shape) into a regime
REGIMES = {
    "frame_strip": lambda p: p[8] > 0,
    "uniform_side_column": lambda p: _uniform(p) and p[4] == 1,
    "split_contraction": lambda p: p[0] == 5 and not p[9] and not p[8] and (p[1] > 1 or p[2] > 1),
    "lists_compute_rank": lambda p: p[9] == 1 and p[7] != p[6],
    "lists_plain_rank": lambda p: p[9] == 1 and p[7] == p[6],
    "two_launch_h": lambda p: p[10] > 1,
    "uniform_off_size": lambda p: _uniform(p) and p[7] != p[6],
    "any_rank": lambda p: p[0] == 0 and p[6] > 128,
}


def _debug_plan(lib, B, T, F, K):
    out = (ctypes.c_int64 * 32)()
    assert lib.fluhip_debug_plan_shape(B, T, F, K, out) == 0, (B, T, F, K)
    return [int(v) for v in out]


def test_every_regime_is_in_the_list(fluhip_lib_path):
    """pure host code: the planner still puts each shape into the regime it stands for"""
    import fluhip
    lib = fluhip.load_library(fluhip_lib_path)
    assert set(SHAPES) == set(REGIMES)
    for name, shape in SHAPES.items():
        p = _debug_plan(lib, *shape)
        assert REGIMES[name](p), (name, shape, p[:15])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_corpus_runs_the_plan_the_planner_reports(ctx, name):
    import fluhip
    B, T, F, K = SHAPES[name]
    fft = 2 * (F - 1)
    hop = fft // 4
    n = (T - 1) * hop + hop // 2                      # T = (n + hop) / hop frames (alg/STFT.hpp:98-99)
    c = fluhip.Corpus(ctx, B, n, fft, fft, hop, K)
    try:
        assert (c.T, c.F) == (T, F)                   # the shape the debug call is asked about
        got = (ctypes.c_int64 * 8)()
        ctx._check(ctx.lib.fluhip_corpus_plan(c.h, got))
    finally:
        c.close()
    p = _debug_plan(ctx.lib, B, T, F, K)
    assert REGIMES[name](p), (name, p[:15])
    # variant, nsplitW, nsplitH | tailSplitH << 16, lazy, sideW, stripsW, Kp | Kc << 16, strip kind
    want = [p[0], p[1], p[2] | p[10] << 16, p[3], p[4], p[5], p[6] | (p[7] if p[7] > 0 else p[6]) << 16, p[8]]
    assert [int(v) for v in got] == want, (name, list(got), want, p[:15])
