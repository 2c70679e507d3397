"""csrc/range_scale.h on the host (no GPU): the power-of-two exponents the double-precision entry points scale their input by.
NMF: 0 for every maximum <= 2^128 (such input keeps its arithmetic bit for bit), otherwise the smallest exponent that brings the
maximum to <= 2^128; SVD: the maximum into [0.5, 1).  Exact from the smallest subnormal to DBL_MAX."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_exponents_over_the_whole_double_range(tmp_path):
    exe = str(tmp_path / "range_scale_host")
    src = os.path.join(ROOT, "tests", "cpp", "range_scale_host.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-800:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 2098 * 5
