"""GPU tests of BufMelBands / BufMFCC through the C ABI in every form the feature pipeline has, against the f64 numpy
restatement (oracle_np: bufmelbands_channel, bufmfcc_channel, mel_filters -- held against the compiled reference in
tests/test_oracle.py).  The shapes and the form each must take are tests/features_cases.py; every run asserts its form
through Context.features_plan first.

Bars (none of them fitted to what the kernels give):
  * linear mel bands, element by element: |got - ref| <= 1e-5 ref + floor.  1e-5 is the project's bar for features; it
    holds per element because a band is a sum of non-negative terms, so a per-bin relative error carries through to the
    band.  floor = 1e-5 x the smallest non-zero reference value of the case: it is there for bands that are exactly zero in
    the reference, nothing looser.
  * dB mel bands and MFCCs: 2e-3 absolute (relative error means nothing on coefficients that are ~1e-13 for silence);
    MFCCs also max|err| / max|ref| < 1e-5.
"""
import os

import numpy as np
import pytest

import novelty_ref as R
from conftest import rel_err
from features_cases import (EMPTY_BANDS, FALLBACK, FUSED, FUSED_DEFAULT, FUSED_MFCC, FUSED_NW, PAIRS, RAGGED, RANGE_CASES,
                            TWO_BEYOND, TWO_MFCC, TWO_TODAY, case, ragged_frames, samples_for)

pytestmark = pytest.mark.gpu

REL_BAR = 1e-5      # linear bands per element, MFCCs against their largest
DB_BAR = 2e-3       # dB bands and MFCCs, absolute
DB_EPS = np.float32(20.0 * np.log10(2.220446049250313e-16))   # a band no bin falls into, in dB
# tests/test_gpu_novelty.py's bar for bufnoveltyfeature (64 x the floor between two double STFTs, see there)
NOVELTY_BAR = 64 * 3.8e-13

WORST = {}          # (form, quantity) -> largest error / bar seen in this session, printed by the last test


def note(plan, what, ratio):
    if plan is None:
        return
    form = "fused" if plan[0] == 0 else "two-kernel"
    WORST[(form, what)] = max(WORST.get((form, what), 0.0), float(ratio))


def audio_of(onp, c, T=None, seed=0):
    n = samples_for(c.T if T is None else T, c.win, c.hop)
    return np.stack([onp.synth_audio(n, 7000 + 13 * seed + ch, c.sr) for ch in range(c.channels)])


def plan_of(ctx, c, mfcc=False, n_coefs=13, start_coeff=0):
    form, nw, ft, lds, rows = ctx.features_plan(mfcc, c.win, c.fft, c.bands, n_coefs, start_coeff, c.lo, c.hi, c.sr)
    if form == 1:
        bands_pad = -(-c.bands // 64) * 64
        assert lds == nw * ft * (bands_pad + (c.fft // 2 + 1) * rows) * 8 <= 160 * 1024
    return (form, nw, ft, rows)


def check_linear(got, ref, plan, tag):
    ref = ref.astype(np.float64)
    nz = ref[ref > 0]
    floor = REL_BAR * (nz.min() if nz.size else 0.0)
    allow = REL_BAR * ref + floor
    err = np.abs(got.astype(np.float64) - ref)
    ratio = (err / np.maximum(allow, 1e-300)).max() if allow.max() > 0 else float(err.max() > 0)
    print(f"{tag}: linear bands worst err / allowance {ratio:.3e}")
    note(plan, "linear bands, per element", ratio)
    assert np.isfinite(got).all() and (err <= allow).all(), tag


def check_db(got, ref, plan, tag, bar=DB_BAR):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
    print(f"{tag}: dB bands max abs err {err:.3e}")
    note(plan, "dB bands, absolute", err / DB_BAR)
    assert np.isfinite(got).all() and err <= bar, tag


def check_mfcc(got, ref, plan, tag, bar=DB_BAR, rel=REL_BAR):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()
    r = rel_err(got, ref)
    print(f"{tag}: MFCC max abs err {err:.3e}, / max|ref| {r:.3e}")
    note(plan, "MFCC, absolute", err / DB_BAR)
    note(plan, "MFCC, relative to the largest", r / REL_BAR)
    assert np.isfinite(got).all() and err <= bar and r < rel, tag


def run_mel(ctx, onp, c, audio, pairs=PAIRS, want=None):
    """bufmelbands of every channel at once against the restatement channel by channel; returns the outputs"""
    plan = plan_of(ctx, c)
    assert plan == (c.plan if want is None else want), (c, plan)
    T = onp.feature_frames(audio.shape[1], c.win, c.hop)[0]
    outs = {}
    for normalize, db in pairs:
        got = ctx.bufmelbands(audio, c.win, c.fft, c.hop, c.bands, c.lo, c.hi, c.sr, normalize, db)
        assert got.shape == (audio.shape[0], c.bands, T)
        for ch in range(audio.shape[0]):
            ref = onp.bufmelbands_channel(audio[ch], c.win, c.fft, c.hop, c.bands, c.lo, c.hi, c.sr, normalize, db)
            assert ref.shape == got[ch].shape
            tag = f"{c.win}/{c.fft}/{c.hop} {c.bands} bands T {T} norm {int(normalize)} dB {int(db)} ch {ch}"
            (check_db if db else check_linear)(got[ch], ref, plan, tag)
        outs[(normalize, db)] = got
    return outs


def run_mfcc(ctx, onp, c, audio, n_coefs=13, start_coeff=0, want=None):
    plan = plan_of(ctx, c, True, n_coefs, start_coeff)
    assert plan == (c.plan if want is None else want), (c, plan)
    T = onp.feature_frames(audio.shape[1], c.win, c.hop)[0]
    got = ctx.bufmfcc(audio, c.win, c.fft, c.hop, c.bands, n_coefs, start_coeff, c.lo, c.hi, c.sr)
    assert got.shape == (audio.shape[0], n_coefs, T)
    for ch in range(audio.shape[0]):
        ref = onp.bufmfcc_channel(audio[ch], c.win, c.fft, c.hop, c.bands, n_coefs, start_coeff, c.lo, c.hi, c.sr)
        assert ref.shape == got[ch].shape
        check_mfcc(got[ch], ref, plan, f"{c.win}/{c.fft}/{c.hop} {c.bands} bands {n_coefs} coefs from {start_coeff} T {T} ch {ch}")
    return got


def ids(cases):
    return [f"{c.win}-{c.fft}-{c.hop}-{c.bands}b-{c.lo:g}-{c.hi:g}-{c.sr:g}-T{c.T}x{c.channels}" for c in cases]


# ---- two-kernel form -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TWO_TODAY, ids=ids(TWO_TODAY))
def test_two_kernel_layouts_of_four_frames(ctx, onp, c):
    """mel_kernel at 4, 2 and 1 wavefronts per workgroup, one and several chunks of 64 bands: all four
    (normalize, scale_db) pairs and the default MFCC"""
    audio = audio_of(onp, c)
    run_mel(ctx, onp, c, audio)
    run_mfcc(ctx, onp, c, audio)


@pytest.mark.parametrize("c", TWO_BEYOND, ids=ids(TWO_BEYOND))
def test_two_kernel_beyond_four_frames(ctx, onp, c):
    """shapes whose four magnitude rows and band energies pass 160 KB of LDS: 2 and 1 frames per wavefront, then the rows
    read from memory (fft 65536).  The launch asked for up to 1 MB of LDS here before and failed."""
    audio = audio_of(onp, c)
    run_mfcc(ctx, onp, c, audio)
    run_mel(ctx, onp, c, audio, pairs=[(True, False)])


@pytest.mark.parametrize("c", RAGGED, ids=ids(RAGGED))
def test_two_kernel_ragged_frame_counts(ctx, onp, c):
    """frame counts around a full workgroup at every layout: the clamped loads of dead frames, the store guards"""
    _, nw, ft, _ = c.plan
    for T in ragged_frames(nw, ft):
        audio = audio_of(onp, c, T, seed=T)
        run_mfcc(ctx, onp, c, audio)
        run_mel(ctx, onp, c, audio, pairs=[(True, False)])


@pytest.mark.parametrize("c,n_coefs,start", TWO_MFCC, ids=[f"{c.fft}-{c.bands}b-{k}c-from{s}" for c, k, s in TWO_MFCC])
def test_two_kernel_mfcc_options(ctx, onp, c, n_coefs, start):
    got = run_mfcc(ctx, onp, c, audio_of(onp, c), n_coefs, start)
    if n_coefs + start > c.bands:
        assert (got[:, -1, :] == 0.0).all()   # the row past the DCT table


# ---- fused form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FUSED_DEFAULT, ids=ids(FUSED_DEFAULT))
def test_fused_shapes_and_band_counts(ctx, onp, c):
    audio = audio_of(onp, c)
    run_mel(ctx, onp, c, audio)
    run_mfcc(ctx, onp, c, audio, n_coefs=2)


@pytest.mark.parametrize("c", RANGE_CASES, ids=ids(RANGE_CASES))
def test_frequency_ranges_move_the_boundary_tables(ctx, onp, c):
    """empty intervals below the first band, the last falling edge at Nyquist, another sample rate; the ranges whose bands
    are narrower than a bin take the two-kernel form (the table says which) and are held to the same bars"""
    audio = audio_of(onp, c)
    run_mel(ctx, onp, c, audio)
    run_mfcc(ctx, onp, c, audio, n_coefs=min(13, c.bands))


@pytest.mark.parametrize("win,fft,hop,bands", [(1024, 1024, 512, 64), (1000, 1024, 300, 13), (2048, 2048, 512, 13),
                                               (600, 2048, 150, 64)])
def test_fused_block_and_chunk_arithmetic(ctx, onp, win, fft, hop, bands):
    """the grid is 8 x chunk workgroups of NW frames, handed out dynamically: T = 1, NW - 1, NW, NW + 1 frames, and nine
    channels of three frames (a block count that is no multiple of 8)"""
    NW = FUSED_NW[fft]
    for T, channels in ((1, 2), (NW - 1, 2), (NW, 3), (NW + 1, 2), (3, 9)):
        c = case(win, fft, hop, bands, FUSED, T=T, channels=channels)
        audio = audio_of(onp, c, seed=T)
        run_mel(ctx, onp, c, audio, pairs=[(True, False), (False, True)])
        run_mfcc(ctx, onp, c, audio, n_coefs=min(13, bands))


@pytest.mark.parametrize("c,n_coefs,start", FUSED_MFCC, ids=[f"{c.win}-{c.fft}-{c.bands}b-{k}c-from{s}" for c, k, s in FUSED_MFCC])
def test_mfcc_up_to_the_fused_kernels_dct_capacity(ctx, onp, c, n_coefs, start):
    """the DCT options on the fused form up to the last row count its LDS holds, and one past it (two-kernel).
    64 coefficients of 64 bands sit on the table bound nDct * nBands = 4096 but not in the kernel's LDS (183 568 bytes at
    fft 1024, 175 888 at fft 2048, of 163 840): launch_feat_t has always declined them, and the plan says two-kernel."""
    got = run_mfcc(ctx, onp, c, audio_of(onp, c), n_coefs, start)
    if n_coefs + start > c.bands:
        assert (got[:, -1, :] == 0.0).all()


# ---- fallbacks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FALLBACK, ids=ids(FALLBACK))
def test_shapes_that_fall_back_to_two_kernels(ctx, onp, c):
    audio = audio_of(onp, c)
    outs = run_mel(ctx, onp, c, audio)
    run_mfcc(ctx, onp, c, audio)
    empty = onp.mel_filters(c.lo, c.hi, c.bands, c.fft // 2 + 1, c.sr).sum(axis=1) == 0.0
    if (c.fft, c.bands, c.hi) in EMPTY_BANDS:
        assert int(empty.sum()) == EMPTY_BANDS[(c.fft, c.bands, c.hi)]
    if empty.any():   # a band no bin falls into: 20 log10(eps) in dB, equal and not merely close; 0 in linear
        for normalize in (True, False):
            assert (outs[(normalize, True)][:, empty, :] == DB_EPS).all()
            assert (outs[(normalize, False)][:, empty, :] == 0.0).all()


# ---- both forms on the same input ------------------------------------------------------------------------------------------
def forced_two_kernel(fn):
    old = os.environ.get("FLUHIP_FEAT_FUSED")
    os.environ["FLUHIP_FEAT_FUSED"] = "0"
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop("FLUHIP_FEAT_FUSED", None)
        else:
            os.environ["FLUHIP_FEAT_FUSED"] = old


@pytest.mark.parametrize("c", [case(1024, 1024, 512, 40, FUSED, T=19, channels=3),
                               case(2048, 2048, 512, 13, FUSED, T=9, channels=2, lo=300.0, hi=3000.0),
                               case(1000, 1024, 300, 64, FUSED, T=17, channels=2)],
                         ids=["c5-shape", "fft2048-300-3000", "win1000-64b"])
def test_both_forms_on_the_same_input(ab_ctx, onp, c):
    """each form against the restatement by the bars above, the two against each other by twice those bars"""
    audio = audio_of(onp, c)
    two = (1, 4, 4, 1)
    fm = run_mel(ab_ctx, onp, c, audio)
    fc = run_mfcc(ab_ctx, onp, c, audio)
    tm = forced_two_kernel(lambda: run_mel(ab_ctx, onp, c, audio, want=two))
    tc = forced_two_kernel(lambda: run_mfcc(ab_ctx, onp, c, audio, want=two))
    for (normalize, db), a in fm.items():
        b = tm[(normalize, db)]
        for ch in range(audio.shape[0]):
            if db:
                check_db(a[ch], b[ch], None, "fused against two-kernel", bar=2 * DB_BAR)
            else:
                ref = onp.bufmelbands_channel(audio[ch], c.win, c.fft, c.hop, c.bands, c.lo, c.hi, c.sr, normalize, db).astype(np.float64)
                allow = 2 * (REL_BAR * ref + REL_BAR * ref[ref > 0].min())
                assert (np.abs(a[ch].astype(np.float64) - b[ch]) <= allow).all()
    for ch in range(audio.shape[0]):
        check_mfcc(fc[ch], tc[ch], None, "fused against two-kernel", bar=2 * DB_BAR, rel=2 * REL_BAR)


# ---- range and degenerate input, on one fused and one two-kernel shape -----------------------------------------------------
EDGE = [case(1024, 1024, 512, 40, FUSED, T=6, channels=1), case(4096, 4096, 1024, 40, (1, 2, 4, 1), T=6, channels=1)]


@pytest.mark.parametrize("c", EDGE, ids=["fused", "two-kernel"])
def test_silence(ctx, onp, c):
    zeros = np.zeros((2, samples_for(c.T, c.win, c.hop)), dtype=np.float32)
    coefs = run_mfcc(ctx, onp, c, zeros)
    assert np.abs(coefs[:, 0, :].astype(np.float64) - np.sqrt(c.bands) * 20.0 * np.log10(2.220446049250313e-16)).max() <= DB_BAR
    assert np.abs(coefs[:, 1:, :]).max() <= 1e-9
    outs = run_mel(ctx, onp, c, zeros)
    assert (outs[(True, False)] == 0.0).all() and (outs[(False, False)] == 0.0).all()


@pytest.mark.parametrize("c", EDGE, ids=["fused", "two-kernel"])
def test_a_silent_channel_leaves_its_neighbours_untouched(ctx, onp, c):
    n = samples_for(c.T, c.win, c.hop)
    a, b = onp.synth_audio(n, 7101), onp.synth_audio(n, 7102)
    three = np.stack([a, np.zeros(n, dtype=np.float32), b])
    assert plan_of(ctx, c, True) == c.plan and plan_of(ctx, c) == c.plan
    got = ctx.bufmfcc(three, c.win, c.fft, c.hop)
    assert np.array_equal(got[0], ctx.bufmfcc(a, c.win, c.fft, c.hop)[0]) and np.array_equal(got[2], ctx.bufmfcc(b, c.win, c.fft, c.hop)[0])
    assert np.array_equal(got[1], ctx.bufmfcc(three[1], c.win, c.fft, c.hop)[0])
    for normalize, db in PAIRS:
        got = ctx.bufmelbands(three, c.win, c.fft, c.hop, normalize=normalize, scale_db=db)
        for ch in (0, 1, 2):
            assert np.array_equal(got[ch], ctx.bufmelbands(three[ch], c.win, c.fft, c.hop, normalize=normalize, scale_db=db)[0])


@pytest.mark.parametrize("scale", [1e-30, 1e30, 1e36, 3e38])
@pytest.mark.parametrize("c", EDGE, ids=["fused", "two-kernel"])
def test_very_quiet_and_very_loud_float_audio(ctx, onp, c, scale):
    """float audio at both ends of the float range: finite, and within the dB bar.  A band sums a window's worth of samples
    over its bins, so its energy passes FLT_MAX before the samples do: the fused kernel's single-precision logarithm made
    such a band infinite, and the DCT a frame of NaNs, before it split the exponent off on that branch.  These few frames
    of synth_audio stay below FLT_MAX in every band at 1e36 (both builds pass there); at 3e38 -- full scale of what a float
    buffer can hold -- bands pass it, which the case asserts of the reference's own band energies."""
    audio = (audio_of(onp, c).astype(np.float64) * scale).astype(np.float32)
    assert np.isfinite(audio).all() and np.abs(audio).max() > 0.1 * scale
    if scale == 3e38:
        mag = onp.framed_magnitude(audio[0].astype(np.float64), c.win, c.fft, c.hop)
        bands = onp.melbands(mag, onp.mel_filters(c.lo, c.hi, c.bands, c.fft // 2 + 1, c.sr), c.win, False, False, False)
        assert bands.max() > float(np.finfo(np.float32).max)
    run_mfcc(ctx, onp, c, audio)
    run_mel(ctx, onp, c, audio, pairs=[(False, True), (True, True)])


# ---- novelty on the same kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win,fft,hop,plan", [(16384, 16384, 4096, (1, 1, 2, 1)), (4096, 4096, 1024, (1, 2, 4, 1))])
def test_novelty_mfcc_rows_at_large_fft(ctx, onp, win, fft, hop, plan):
    """bufnoveltyfeature(algorithm = 1) takes its rows from mel_kernel's f64 frame-major output: the layouts of fft 4096 and
    of fft 16384 (which could not launch), by test_bufnoveltyfeature_against_the_restatement's bars"""
    assert ctx.features_plan(True, win, fft, 40, 13, 0)[:3] + ctx.features_plan(True, win, fft, 40, 13, 0)[4:] == plan
    x = onp.synth_audio(13 * hop, 7201)
    for k, f in ((3, 1), (5, 4)):
        want = R.bufnoveltyfeature(x, 1, k, f, win, fft, hop, as_double=True)
        got = ctx.bufnoveltyfeature(x, 1, k, f, win, fft, hop)[0]
        assert got.shape == want.shape and len(want) > 8
        err = np.abs(got.astype(np.float64) - want)
        allow = NOVELTY_BAR + np.maximum((np.abs(want) + NOVELTY_BAR) * 2.0 ** -24, 2.0 ** -149)
        print(f"bufnoveltyfeature MFCC fft {fft} k {k} f {f}: worst err / allowance {(err / allow).max():.3f}")
        assert (err <= allow).all()


# ---- what the cases above cover --------------------------------------------------------------------------------------------
def test_every_form_and_layout_is_exercised(ctx):
    """in the style of test_both_plan_forms_are_exercised: the tables reach the fused form at both fft sizes, the two-kernel
    form at 4, 2 and 1 wavefronts of four frames, and each of the fallbacks past that (2 frames, 1 frame, rows from
    memory) -- by what the library reports for them, not by what the tables claim"""
    seen = set()
    for c in TWO_TODAY + TWO_BEYOND + FUSED_DEFAULT + RANGE_CASES + FALLBACK:
        p = plan_of(ctx, c)
        assert p == c.plan
        seen.add((p, c.fft) if p == FUSED else p)
    assert {(FUSED, 1024), (FUSED, 2048), (1, 4, 4, 1), (1, 2, 4, 1), (1, 1, 4, 1), (1, 1, 2, 1), (1, 1, 1, 1), (1, 4, 4, 0)} <= seen
    # a band count whose energies alone pass the LDS is refused with a message, by the plan as by the call
    import fluhip
    with pytest.raises(fluhip.FluhipError, match="too many bands"):
        ctx.features_plan(False, 65536, 65536, 20481)
    with pytest.raises(fluhip.FluhipError, match="too many bands"):
        ctx.bufmelbands(np.zeros(70000, dtype=np.float32), 65536, 65536, 16384, 20481)
    assert ctx.features_plan(False, 65536, 65536, 20480) == (1, 1, 1, 20480 * 8, 0)
    for key in sorted(WORST):
        print(f"largest error / bar, {key[0]}, {key[1]}: {WORST[key]:.3e}")
