"""GPU tests of BufHPSS through the C ABI and the C++ client, against tests/hpss_ref.py.  The inputs, their distance from a
tie and the floor behind the audio bar are those tests/test_hpss_ref.py proves on the CPU."""
import ctypes

import numpy as np
import pytest

import hpss_ref as R
from test_hpss_ref import AUDIO_CASES, AUDIO_FLOOR, KNEE, KNEE_ONE, MASK_CASES, audio_case, peak_of, plane_mag

pytestmark = pytest.mark.gpu

# |got - want| <= AUDIO_BAR x peak: 64 x the floor between two double STFTs on the CPU (the factor the novelty and onset GPU
# tests use: the device's transform differs from both in the last places) plus 2^-24 of peak, which covers the rounding of
# the double result to the float32 output (half an ulp of a value no larger than peak is 2^-25 of it)
AUDIO_BAR = 64 * AUDIO_FLOOR + 2.0 ** -24
LIMIT = 63   # the on-chip limit fluhip_debug_hpss_plan reports (test_the_plan_reports_the_limit)


def ulps(got, want):
    return float((np.abs(got - want) / np.spacing(np.maximum(np.abs(want), np.finfo(np.float64).tiny))).max())


def audio_err(got, x, want):
    return float(np.abs(got.astype(np.float64) - want).max()) / peak_of(x, want)


def test_the_plan_reports_the_limit(ctx):
    assert ctx.hpss_plan(LIMIT, LIMIT)[:2] == (0, 0) and ctx.hpss_plan(LIMIT + 2, LIMIT + 2)[:2] == (1, 1)
    assert ctx.hpss_plan(17, 31) == (0, 0, (17 * 256 + 256 + 30) * 8, 256)


@pytest.mark.parametrize("h_size", [3, 17, 33, LIMIT, LIMIT + 2])
@pytest.mark.parametrize("v_size", [3, 31, 129, LIMIT, LIMIT + 2])
def test_medians_are_the_bits_of_the_restatement(ctx, h_size, v_size):
    """every kernel form: both medians array_equal, the mode 0 masks within 4 ulp (one reciprocal and one product)"""
    mag = plane_mag()
    wh, wv, wm = R.hpss_planes(mag, h_size, v_size, 0)
    hmed, vmed, masks = ctx.hpss_planes(mag, h_size, v_size, 0)
    assert np.array_equal(hmed[0], wh) and np.array_equal(vmed[0], wv)
    assert wh.max() > 0 and wv.max() > 0
    worst = max(ulps(masks[i, 0], wm[i]) for i in range(3))
    print(f"h {h_size} v {v_size} plan {ctx.hpss_plan(h_size, v_size)}: mode 0 masks within {worst:.1f} ulp")
    assert worst <= 4
    assert not masks[2].any()


@pytest.mark.parametrize("case", MASK_CASES, ids=[f"h{c[0]}_v{c[1]}_m{c[2]}_{i}" for i, c in enumerate(MASK_CASES)])
def test_mode_1_and_2_masks_are_identical(ctx, case):
    h_size, v_size, mode, ht, pt = case
    mag = plane_mag()
    wh, wv, wm = R.hpss_planes(mag, h_size, v_size, mode, ht, pt)
    hmed, vmed, masks = ctx.hpss_planes(mag, h_size, v_size, mode, ht, pt)
    assert np.array_equal(hmed[0], wh) and np.array_equal(vmed[0], wv)
    for i in range(3):
        assert np.array_equal(masks[i, 0], wm[i]), i
    assert 0 < wm[0].mean() < 1     # both outcomes of the comparison occur


def test_an_all_zero_plane(ctx):
    z = np.zeros((40, 129))
    for mode, want in ((0, (0, 0, 0)), (1, (0, 1, 0)), (2, (0, 0, 1))):
        hmed, vmed, masks = ctx.hpss_planes(z, 17, 31, mode)
        assert np.isfinite(masks).all() and not hmed.any() and not vmed.any()
        assert [float(masks[i].min()) for i in range(3)] == list(want) == [float(masks[i].max()) for i in range(3)]
        wm = R.hpss_planes(z, 17, 31, mode)[2]
        assert all(np.array_equal(masks[i, 0], wm[i]) for i in range(3))


def test_a_batch_of_planes_gives_the_bits_of_single_calls(ctx):
    mag = plane_mag()
    three = np.stack([mag, mag[::-1], 0.5 * mag])
    for h_size, v_size, mode in ((17, 31, 0), (65, 65, 2)):
        got = ctx.hpss_planes(three, h_size, v_size, mode, KNEE, KNEE_ONE)
        for b in range(3):
            one = ctx.hpss_planes(three[b], h_size, v_size, mode, KNEE, KNEE_ONE)
            assert np.array_equal(got[0][b], one[0][0]) and np.array_equal(got[1][b], one[1][0])
            assert np.array_equal(got[2][:, b], one[2][:, 0])


def test_planes_with_a_row_stride_and_null_outputs(ctx):
    lib, h = ctx.lib, ctx.h
    mag = plane_mag()[:50]
    T, F = mag.shape
    wide = np.full((T, F + 5), 9.0)
    wide[:, :F] = mag
    dp = ctypes.POINTER(ctypes.c_double)
    thr = (ctypes.c_double * 4)(*R.DEFAULT_THRESH)
    vmed = np.full((T, F), -7.0)
    assert lib.fluhip_hpss_planes_f64(h, wide.ctypes.data_as(dp), 1, T, F, F + 5, 5, 7, 0, thr, thr, None, vmed.ctypes.data_as(dp), None) == 0
    assert np.array_equal(vmed, R.hpss_planes(mag, 5, 7)[1])
    pm = np.full((T, F), -7.0)
    mp = (dp * 3)(None, pm.ctypes.data_as(dp), None)
    assert lib.fluhip_hpss_planes_f64(h, wide.ctypes.data_as(dp), 1, T, F, F + 5, 5, 7, 1, thr, thr, None, None, mp) == 0
    assert np.array_equal(pm, R.hpss_planes(mag, 5, 7, 1)[2][1])


@pytest.mark.parametrize("name", list(AUDIO_CASES))
def test_bufhpss_against_the_closed_form(ctx, name):
    n, seed, win, fft, hop, h_size, v_size, mode, ht, pt = AUDIO_CASES[name]
    x, want = audio_case(name)
    got = ctx.bufhpss(x, win, fft, hop, h_size, v_size, mode, ht, pt)[0]
    assert got.shape == (3, n) and got.dtype == np.float32
    e = audio_err(got, x, want)
    print(f"bufhpss {name}: |got - want| / peak = {e:.3e} (bar {AUDIO_BAR:.3e})")
    assert e <= AUDIO_BAR
    assert np.abs(want[:2]).max() > 0.01
    if mode != 2:
        assert not got[2].any()
    else:
        assert got[2].any()


def test_bufhpss_batch_gives_the_bits_of_single_calls(ctx):
    a = audio_case("block_mode2")[0][:9000]
    b = audio_case("fft4096")[0][:9000]
    for mode in (0, 2):
        both = ctx.bufhpss(np.stack([a, b]), 1024, 1024, 512, 17, 31, mode, KNEE, KNEE_ONE)
        assert np.array_equal(both[0], ctx.bufhpss(a, 1024, 1024, 512, 17, 31, mode, KNEE, KNEE_ONE)[0])
        assert np.array_equal(both[1], ctx.bufhpss(b, 1024, 1024, 512, 17, 31, mode, KNEE, KNEE_ONE)[0])


def test_bad_parameters_are_errors_that_name_them(ctx):
    lib, h = ctx.lib, ctx.h
    dp, fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    x = np.zeros(4000, dtype=np.float32)
    mag = np.zeros((20, 129))

    def calls(hs=17, vs=31, mode=0, win=256, fft=256, hop=64, count=1, ht=R.DEFAULT_THRESH, audio=True):
        thr, dflt = (ctypes.c_double * 4)(*ht), (ctypes.c_double * 4)(*R.DEFAULT_THRESH)
        out = np.full((3, 4000), -7, dtype=np.float32)
        rc = lib.fluhip_bufhpss_f32(h, x.ctypes.data_as(fp) if audio else None, count, 4000, win, fft, hop, hs, vs, mode, thr, dflt,
                                    out.ctypes.data_as(fp))
        res = [(rc, lib.fluhip_last_error(h).decode(), bool((out == -7).all()))]
        hm = np.full((20, 129), -7.0)
        rc = lib.fluhip_hpss_planes_f64(h, mag.ctypes.data_as(dp) if audio else None, count, 20, 129, 129, hs, vs, mode, thr, dflt,
                                        hm.ctypes.data_as(dp), None, None)
        res.append((rc, lib.fluhip_last_error(h).decode(), bool((hm == -7).all())))
        return res

    for kw, word in ((dict(hs=16), "harmFilterSize"), (dict(hs=1), "harmFilterSize"), (dict(vs=30), "percFilterSize"),
                     (dict(vs=1), "percFilterSize"), (dict(vs=131), "percFilterSize"), (dict(mode=3), "maskingMode"),
                     (dict(mode=-1), "maskingMode"), (dict(count=0), "at least one"), (dict(audio=False), "null buffer"),
                     (dict(ht=(0.7, 1, 0.2, 1)), "harmThresh"), (dict(ht=(0.0, 1, 1.5, 1)), "harmThresh")):
        for rc, msg, untouched in calls(**kw):
            assert rc == 2 and word in msg and untouched, (kw, msg)
    rc, msg, untouched = calls(hop=300)[0]
    assert rc == 2 and "hop" in msg and untouched
    rc, msg, untouched = calls(fft=300)[0]
    assert rc == 2 and "fft" in msg and untouched
    assert all(rc == 0 for rc, _, _ in calls())


# ---- the C++ host client (include/flucoma_hip/HPSSClient.hpp) through tests/cpp/hpss_driver.cpp ------------------------
@pytest.fixture(scope="module")
def hpss_driver(fluhip_lib_path):
    return R.build_driver()


def _run(driver, path, outp, n, chans, h_size=17, v_size=31, mode=0, ht=R.DEFAULT_THRESH, pt=R.DEFAULT_THRESH, win=1024, hop=512,
         fft=1024, residual=1, asynchronous=0, rate=48000):
    out = R.drive(driver, "run", path, n, chans, rate, h_size, v_size, mode, *ht, *pt, win, hop, fft, residual, asynchronous, outp)
    return [l for l in out.splitlines() if not l.startswith("process|")]


def test_cpp_client_equals_the_c_abi(ctx, hpss_driver, tmp_path):
    a = audio_case("block_mode2")[0][:12000]
    x = np.stack([a, 0.5 * a[::-1]]).astype(np.float32)
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    np.ascontiguousarray(x.T).tofile(path)                   # the memory buffer is frames x channels
    for mode, residual, asynchronous in ((2, 1, 0), (0, 0, 1)):
        lines = _run(hpss_driver, path, outp, 12000, 2, 17, 31, mode, KNEE, KNEE_ONE, residual=residual, asynchronous=asynchronous)
        want = ctx.bufhpss(x, 1024, 1024, 512, 17, 31, mode, KNEE, KNEE_ONE)          # [2, 3, n]
        assert lines[0] == "run|0|"
        assert lines[1] == "shape|harmonic|12000|2|48000" and lines[2] == "shape|percussive|12000|2|48000"
        assert lines[3] == ("shape|residual|12000|2|48000" if residual else "shape|residual|absent")   # an omitted buffer is accepted
        got = np.fromfile(outp, dtype=np.float32).reshape(3 if residual else 2, 2, 12000)
        for o in range(got.shape[0]):
            assert np.array_equal(got[o], want[:, o]), (mode, o)


def test_cpp_client_returns_the_announced_errors(ctx, hpss_driver, tmp_path):
    x = np.zeros(3000, dtype=np.float32)
    path, outp = tmp_path / "in.f32", tmp_path / "out.f32"
    x.tofile(path)
    for kw, word in ((dict(h_size=16), "harmFilterSize"), (dict(v_size=2), "percFilterSize"),
                     (dict(v_size=131, win=256, hop=64, fft=256), "percFilterSize"), (dict(mode=3), "maskingMode"),
                     (dict(win=256, hop=300, fft=256), "hop"), (dict(ht=(0.9, 1, 0.1, 1)), "harmThresh")):
        lines = _run(hpss_driver, path, outp, 3000, 1, **kw)
        status, code, msg = lines[0].split("|", 2)
        assert (status, code) == ("run", "2") and word in msg, (kw, lines[0])
        assert lines[1] == "shape|harmonic|7|3|44100"           # nothing was resized
