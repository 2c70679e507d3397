"""Mint tests/golden/nmfcross_v1.npz: small BufNMFCross jobs through the numpy restatement (tests/nmfcross_ref.py).

    python tools/make_nmfcross_golden.py

Per case: the source / target float audio, the parameters, H1 (T x K) and the float output.  The inputs come from the
package's synthetic-audio generator, so the file is reproducible bit for bit."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "flucoma-core_amd"))
import nmfcross_ref  # noqa: E402
from synth import synth_audio  # noqa: E402

# (name, n_src, n_tgt, win, fft, hop, r, p, c, iters, seed)
CASES = [
    ("a", 3000, 2500, 256, 256, 128, 7, 11, 7, 10, 42),
    ("b", 2000, 3300, 128, 256, 64, 3, 4, 5, 3, 7),
    ("c", 1500, 1500, 256, 256, 128, 9, 1, 3, 1, 3),
]


def main():
    out = {}
    for name, n_src, n_tgt, win, fft, hop, r, p, c, iters, seed in CASES:
        src = synth_audio(n_src, 100 + seed).astype(np.float32)
        tgt = synth_audio(n_tgt, 200 + seed).astype(np.float32)
        y, H1 = nmfcross_ref.bufnmfcross(src, tgt, win, fft, hop, r, p, c, iters, seed, return_h=True)
        out[f"{name}_source"], out[f"{name}_target"] = src, tgt
        out[f"{name}_params"] = np.array([win, fft, hop, r, p, c, iters, seed], dtype=np.int64)
        out[f"{name}_H1"], out[f"{name}_output"] = H1, y
    path = os.path.join(ROOT, "tests", "golden", "nmfcross_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
