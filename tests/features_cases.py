"""The shapes of tests/test_gpu_features.py as data, with the form fluhip_debug_features_plan must report for each:
tests/test_features_plan.py pins the table without a device, the GPU tests assert it again in front of every run.

A plan is (form, wavefronts per workgroup, frames per wavefront, rows staged in the LDS); the fused form is (0, 0, 0, 0).
The mel kernel's dynamic LDS is nw * ft * (bandsPad + F * rows) * 8 bytes, bandsPad = bands rounded up to 64, against 160 KB
(144 KB while more than one wavefront is left)."""
from collections import namedtuple

FUSED = (0, 0, 0, 0)
PAIRS = [(True, False), (True, True), (False, False), (False, True)]   # (normalize, scale_db)

Case = namedtuple("Case", "win fft hop bands lo hi sr plan T channels")


def case(win, fft, hop, bands, plan, T=5, channels=2, lo=20.0, hi=20000.0, sr=44100.0):
    return Case(win, fft, hop, bands, lo, hi, sr, plan, T, channels)


def samples_for(T, win, hop):
    """a buffer length that gives T frames under the Default padding (oracle_np.feature_frames)"""
    n = max((T - 1 + win // hop) * hop - 2 * (win // 2) + (hop - 1) // 2, 1)
    assert 1 + (n + win + 2 * (win // 2) - win) // hop - win // hop == T, (T, win, hop)
    return n


def ragged_frames(nw, ft):
    """T = 1; one short of, exactly, and one past a full workgroup; and a last wavefront with exactly one live frame"""
    per = nw * ft
    return sorted({1, per - 1, per, per + 1, per + (ft if nw > 1 else 2 * ft) + 1} - {0})


# ---- two-kernel form: every layout of mel_kernel ---------------------------------------------------------------------------
# layouts that launched before the frames-per-wavefront / rows-from-memory fallbacks existed: 4 frames per wavefront
TWO_TODAY = [
    case(512, 512, 128, 40, (1, 4, 4, 1)),
    case(301, 512, 75, 40, (1, 4, 4, 1)),            # odd window
    case(1024, 1024, 512, 65, (1, 4, 4, 1)),         # one band past a chunk of 64
    case(1024, 1024, 512, 128, (1, 4, 4, 1)),        # two full chunks
    case(1024, 1024, 512, 513, (1, 4, 4, 1)),        # the maximum
    case(4096, 4096, 1024, 40, (1, 2, 4, 1)),
    case(3000, 4096, 700, 100, (1, 2, 4, 1)),
    case(4096, 4096, 2048, 2049, (1, 1, 4, 1)),      # the maximum at fft 4096: 133 152 bytes for one wavefront
    case(8192, 8192, 2048, 40, (1, 1, 4, 1)),
    case(8192, 8192, 2048, 960, (1, 1, 4, 1)),       # 161 824 bytes: the last band count of four frames at fft 8192
]
# past that limit: 2 or 1 frames per wavefront, then the magnitude rows from memory
TWO_BEYOND = [
    case(8192, 8192, 2048, 1000, (1, 1, 2, 1)),      # bandsPad 1024: four frames would be 163 872 bytes
    case(8192, 8192, 2048, 4097, (1, 1, 2, 1)),
    case(16384, 16384, 4096, 40, (1, 1, 2, 1)),
    case(20000, 32768, 8192, 40, (1, 1, 1, 1)),
    case(65536, 65536, 16384, 40, (1, 4, 4, 0)),     # one row is 262 152 bytes
]
# one shape per layout for the ragged frame counts
RAGGED = [c for c in TWO_TODAY + TWO_BEYOND if c.bands == 40 and c.win != 301]

# MFCC options on the two-kernel form: (case, n_coefs, start_coeff)
TWO_MFCC = [
    (case(512, 512, 128, 40, (1, 4, 4, 1)), 40, 1),      # the DCT row past the table: zero in the reference
    (case(512, 512, 128, 40, (1, 4, 4, 1)), 2, 0),
    (case(1024, 1024, 512, 100, (1, 4, 4, 1)), 100, 0),
    (case(4096, 4096, 1024, 40, (1, 2, 4, 1)), 40, 1),
]

# ---- fused form ------------------------------------------------------------------------------------------------------------
FUSED_SHAPES = [(1024, 1024, 512), (1000, 1024, 300), (2, 1024, 1), (2048, 2048, 512), (600, 2048, 150)]
FUSED_BANDS = [2, 13, 63, 64]
FUSED_DEFAULT = [case(w, f, h, b, FUSED) for (w, f, h) in FUSED_SHAPES for b in FUSED_BANDS]
# frequency ranges that move the boundary tables (empty intervals below the first band, the last falling edge at Nyquist).
# A range runs fused while every band owns a bin and no bin sees three bands: 64 bands over 300 .. 3000 Hz are narrower
# than the 43 Hz bins of fft 1024 (two-kernel there, fused at fft 2048), and so are the lowest of 64 bands at 96 kHz
RANGES = [(300.0, 3000.0, 44100.0), (20.0, 22050.0, 44100.0), (5000.0, 20000.0, 44100.0), (20.0, 20000.0, 96000.0)]
TWO4 = (1, 4, 4, 1)
RANGE_CASES = [case(w, f, h, b, plan, lo=lo, hi=hi, sr=sr) for (w, f, h, b, (lo, hi, sr), plan) in [
    (1024, 1024, 512, 13, RANGES[0], FUSED), (1024, 1024, 512, 64, RANGES[0], TWO4), (1000, 1024, 300, 2, RANGES[0], FUSED),
    (2048, 2048, 512, 13, RANGES[0], FUSED), (2048, 2048, 512, 64, RANGES[0], FUSED),
    (1024, 1024, 512, 13, RANGES[1], FUSED), (1024, 1024, 512, 64, RANGES[1], FUSED),
    (2048, 2048, 512, 13, RANGES[1], FUSED), (2048, 2048, 512, 64, RANGES[1], FUSED),
    (1024, 1024, 512, 13, RANGES[2], FUSED), (1024, 1024, 512, 64, RANGES[2], FUSED),
    (2048, 2048, 512, 13, RANGES[2], FUSED), (2048, 2048, 512, 64, RANGES[2], FUSED),
    (1024, 1024, 512, 13, RANGES[3], FUSED), (1024, 1024, 512, 64, RANGES[3], TWO4),
    (2048, 2048, 512, 13, RANGES[3], FUSED), (2048, 2048, 512, 64, RANGES[3], TWO4), (600, 2048, 150, 63, RANGES[3], FUSED),
]]
# NW frames per workgroup of the fused kernel: 16 at fft 1024, 8 at fft 2048
FUSED_NW = {1024: 16, 2048: 8}

# MFCC on the fused form: (case, n_coefs, start_coeff).  The kernel's LDS holds nDct rows of 4 ceil(bands / 4) + 1 doubles
# beside the transform's buffers: at 64 bands 26 rows at fft 1024 and 40 at fft 2048 are the last that fit, and
# 64 coefficients of 64 bands (nDct * nBands = 4096, the table's own bound) run two-kernel at both sizes
FUSED_MFCC = [
    (case(1024, 1024, 512, 40, FUSED), 13, 0),           # BASELINE config 5
    (case(1024, 1024, 512, 40, FUSED), 13, 1),
    (case(1024, 1024, 512, 64, FUSED), 26, 0),
    (case(1024, 1024, 512, 64, (1, 4, 4, 1)), 27, 0),
    (case(1000, 1024, 300, 13, FUSED), 13, 0),           # n_coefs = n_bands
    (case(1000, 1024, 300, 13, FUSED), 13, 1),           # ... and the row past the table
    (case(2, 1024, 1, 2, FUSED), 2, 0),
    (case(2048, 2048, 512, 64, FUSED), 40, 0),
    (case(2048, 2048, 512, 64, (1, 4, 4, 1)), 41, 0),
    (case(600, 2048, 150, 63, FUSED), 16, 1),
    (case(1024, 1024, 512, 64, (1, 4, 4, 1)), 64, 0),
    (case(2048, 2048, 512, 64, (1, 4, 4, 1)), 64, 0),
]

# ---- shapes that must fall back to the two-kernel form ----------------------------------------------------------------------
FALLBACK = [
    case(1024, 1024, 512, 64, (1, 4, 4, 1), lo=20.0, hi=2000.0),      # three bands own no bin
    case(1024, 1024, 512, 40, (1, 4, 4, 1), hi=30000.0),              # bands above Nyquist
    case(1024, 1024, 512, 40, (1, 4, 4, 1), sr=8000.0),
    case(1023, 1024, 512, 40, (1, 4, 4, 1)),                          # odd window
    case(1024, 1024, 512, 65, (1, 4, 4, 1)),
    case(64, 64, 16, 33, (1, 4, 4, 1)),                               # 8 empty bands
    case(256, 256, 64, 40, (1, 4, 4, 1)),                             # 1 empty band
]
EMPTY_BANDS = {(64, 33, 20000.0): 8, (256, 40, 20000.0): 1, (1024, 64, 2000.0): 3}   # (fft, bands, hi) -> bands without a bin
