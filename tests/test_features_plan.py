"""fluhip_debug_features_plan without a device: the form and layout of every shape tests/test_gpu_features.py runs
(tests/features_cases.py), the LDS arithmetic at its boundaries, and the refusals.  Pure host code: no GPU."""
import ctypes

import pytest

from features_cases import (FALLBACK, FUSED, FUSED_DEFAULT, FUSED_MFCC, RANGE_CASES, TWO_BEYOND, TWO_MFCC, TWO_TODAY)

LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def lib(fluhip_lib_path):
    import fluhip
    return fluhip.load_library(fluhip_lib_path)


def plan(lib, mfcc, win, fft, bands, n_coefs=13, start=0, lo=20.0, hi=20000.0, sr=44100.0):
    out = (ctypes.c_int64 * 5)()
    rc = lib.fluhip_debug_features_plan(None, int(mfcc), win, fft, bands, n_coefs, start, lo, hi, sr, out)
    return None if rc else tuple(int(v) for v in out)


def plan_of(lib, c, mfcc=False, n_coefs=13, start=0):
    p = plan(lib, mfcc, c.win, c.fft, c.bands, n_coefs, start, c.lo, c.hi, c.sr)
    return (p[0], p[1], p[2], p[4])


def test_mel_band_cases_take_the_form_their_table_states(lib):
    for c in TWO_TODAY + TWO_BEYOND + FUSED_DEFAULT + RANGE_CASES + FALLBACK:
        assert plan_of(lib, c) == c.plan, c


def test_mfcc_cases_take_the_form_their_table_states(lib):
    for c, n_coefs, start in TWO_MFCC + FUSED_MFCC:
        assert plan_of(lib, c, True, n_coefs, start) == c.plan, (c, n_coefs, start)
    for c in TWO_TODAY + TWO_BEYOND + FALLBACK:
        assert plan_of(lib, c, True) == c.plan, c


def test_the_layout_never_asks_for_more_lds_than_the_kernel_may_have(lib):
    """every fft size with its smallest, a mid and its largest band count: the request is the layout's own arithmetic and
    stays within 160 KB, or the plan refuses"""
    for fft in (64, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
        F = fft // 2 + 1
        for bands in sorted({min(F, b) for b in (2, 40, 64, 65, 960, 1000, 4097, 20480, F)}):
            p = plan(lib, False, fft - 1, fft, bands)   # (an odd window: never the fused form)
            if p is None:
                assert bands > 20480
                continue
            form, nw, ft, lds, rows = p
            bands_pad = -(-bands // 64) * 64
            assert form == 1 and nw in (1, 2, 4) and ft in (1, 2, 4) and rows in (0, 1)
            assert lds == nw * ft * (bands_pad + F * rows) * 8 <= LDS_LIMIT
            # nothing is given up before it has to be: four frames while they fit, the rows on chip while one fits
            if ft < 4:
                assert nw == 1 and 2 * ft * (bands_pad + F * rows) * 8 > LDS_LIMIT
            if not rows:
                assert (bands_pad + F) * 8 > LDS_LIMIT


def test_layout_boundaries(lib):
    assert plan(lib, False, 8192, 8192, 960) == (1, 1, 4, 161824, 1)        # the last of four frames at fft 8192
    assert plan(lib, False, 8192, 8192, 961) == (1, 1, 2, 81936, 1)
    assert plan(lib, False, 16384, 16384, 40) == (1, 1, 2, 132112, 1)
    assert plan(lib, False, 32768, 32768, 40) == (1, 1, 1, 131592, 1)
    assert plan(lib, False, 65536, 65536, 40) == (1, 4, 4, 8192, 0)
    assert plan(lib, False, 65536, 65536, 20480) == (1, 1, 1, 163840, 0)
    assert plan(lib, True, 1024, 1024, 40) == (0, 0, 0, 0, 0)               # BASELINE config 5
    assert plan(lib, True, 1024, 1024, 64, 26) == (0, 0, 0, 0, 0) and plan(lib, True, 1024, 1024, 64, 27)[0] == 1
    assert plan(lib, True, 2048, 2048, 64, 40) == (0, 0, 0, 0, 0) and plan(lib, True, 2048, 2048, 64, 41)[0] == 1


def test_refusals(lib):
    assert plan(lib, False, 65536, 65536, 20481) is None                    # the band energies of one frame pass the LDS
    assert plan(lib, False, 1024, 1024, 1) is None and plan(lib, False, 1024, 1024, 514) is None
    assert plan(lib, True, 1024, 1024, 40, 41) is None and plan(lib, True, 1024, 1024, 40, 13, 2) is None
    assert plan(lib, False, 1024, 1000, 40) is None and plan(lib, False, 1025, 2048, 40, lo=50.0, hi=50.0) is None
    assert lib.fluhip_debug_features_plan(None, 0, 1024, 1024, 40, 13, 0, 20.0, 20000.0, 44100.0, None) != 0
