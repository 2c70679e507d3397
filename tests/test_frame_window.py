"""csrc/frame_window.h on the host (no GPU): which offsets of an STFT frame lie inside their buffer and which address the
gathers load for the others (gather_points of fft_core.h, the wave kernel's gathers of kernels_stft.hip call it).  A kernel's
results cannot show a stray load -- its value is discarded -- so the addresses are checked here, on the code the kernels run:
tests/cpp/frame_window_host.cpp emulates a frame's gather over frames anywhere around their buffer and holds every load inside
[0, n); the selection the gather had before (`ok ? i : lo` from the frame's first sample) is run through the same sweep and
must be caught, in its two known classes only; and a build under AddressSanitizer performs the loads from blocks of exactly
n elements."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "frame_window_host.cpp")
SMALL_SPANS = (2, 4, 8, 16, 64)
# frames of the sweep, restated from the program's loops: an emptied sweep fails the count
SMALL = sum(n + 8 * span + 1 for span in SMALL_SPANS for n in range(3 * span + 1))
REAL = 3 * 7 * 6 * 7          # spans x buffer lengths x edges x (+-3)
EDGE = 4 * 7 * 15 * 5         # spans x buffer lengths x edges x (+-2)


def build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    return r.returncode, r.stdout.split(), r.stdout + r.stderr[-800:]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("frame_window"), "frame_window_host")


def test_every_load_of_a_frame_stays_inside_its_buffer(exe):
    rc, out, text = run(exe)
    assert rc == 0 and out[0] == "ok", text
    got = dict(zip(out[2::2], map(int, out[3::2][:3])))
    assert got == {"small": SMALL, "real": REAL, "edge": EDGE} and int(out[1]) == SMALL + REAL + EDGE, text


def test_the_sweep_catches_the_selection_the_gather_had_before(exe):
    """`ok ? i : lo`, offsets from the frame's first sample: out of range for a frame wholly before its buffer by more than a
    frame (lo is capped at the span: sample s0 + span < 0) and for one wholly behind it (lo = hi = 0: sample s0 >= n) -- and
    for any frame of an empty buffer -- and for no other"""
    rc, out, text = run(exe, "parent")
    assert rc == 0 and out[0] == "parent", text
    got = dict(zip(out[1::2], map(int, out[2::2])))
    assert got["frames"] == SMALL + REAL + EDGE, text
    assert got["before"] > 0 and got["behind"] > 0 and got["empty"] > 0 and got["other"] == 0, text
    # the small sweep alone: every s0 of [-4 span, -span) before, every s0 of [n, n + 4 span] behind, at each n >= 1
    assert got["before"] >= sum(3 * span * 3 * span for span in SMALL_SPANS), text
    assert got["behind"] >= sum((4 * span + 1) * 3 * span for span in SMALL_SPANS), text


def test_the_loads_themselves_under_address_sanitizer(tmp_path):
    """a stand-alone program with its own main: the loads of the small sweep from heap blocks of exactly n floats and n
    doubles, and the whole index sweep under UndefinedBehaviorSanitizer (no conversion or sum may overflow at the int32 edges).
    The runtimes are linked into the program, so it runs whatever else the environment loads into a process."""
    san = build(tmp_path, "frame_window_host_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                "-static-libasan", "-static-libubsan")
    rc, out, text = run(san, "loads")
    assert rc == 0 and out[0] == "ok" and int(out[1]) == SMALL, text
    assert float(out[-1]) > 0, text           # the loads were performed: their sum is in the output
    rc, out, text = run(san)
    assert rc == 0 and out[0] == "ok" and int(out[1]) == SMALL + REAL + EDGE, text
