"""Device time of BufLoudness at the client defaults (window 1024, hop 512, kWeighting and truePeak on), for DESIGN K14.

    python tools/loudness_time.py [--reps 5] [--shapes 128x10,8192x2]

Not a test: nothing in `pytest -m gpu` depends on a clock.  Each shape is `count` mono buffers of `seconds` at 44100 Hz from
host float32 buffers through fluhip_bufloudness_f32.  The figure is the device time of the call's kernel launches -- the
zero-state pass, the scan, the second pass and the peak kernel of every round, bracketed by HIP events on the context stream
(fluhip_prof_read, class 2) -- the minimum of `reps` calls; the host wall time of the whole call (uploads and the copy back
included) stands beside it.  `serial_steps` is what the reference's recurrence costs literally: frames x window dependent
filter steps per buffer, one after the other.  Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flucoma-core_amd"))
import fluhip  # noqa: E402
import synth  # noqa: E402

SR = 44100
WIN, HOP = 1024, 512


def row(ctx, count, seconds, reps):
    n = int(seconds * SR)
    base = np.stack([synth.synth_audio(n, 1000 + b) for b in range(min(count, 16))]).astype(np.float32)
    x = np.tile(base, (-(-count // len(base)), 1))[:count]
    out = ctx.bufloudness(x, win=WIN, hop=HOP, sample_rate=float(SR))   # warm
    ctx.synchronize()
    dev, wall, launches = [], [], 0
    ctx.prof_enable(True)
    for _ in range(reps):
        ctx.prof_reset()
        t0 = time.perf_counter()
        ctx.bufloudness(x, win=WIN, hop=HOP, sample_rate=float(SR))
        wall.append((time.perf_counter() - t0) * 1e3)
        launches, ms = ctx.prof_read(2)
        dev.append(ms)
    ctx.prof_enable(False)
    frames_all = out.shape[2] + WIN // HOP     # (the latency frames are run too)
    return {"shape": {"buffers": count, "seconds": seconds, "win": WIN, "hop": HOP, "frames_kept": int(out.shape[2])},
            "device_ms": min(dev), "device_ms_all": dev, "rounds": int(launches), "wall_ms": min(wall),
            "serial_steps_per_buffer": frames_all * WIN, "serial_steps": frames_all * WIN * count,
            "plan": ctx.loudness_plan(WIN, HOP, float(SR))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="128x10,8192x2")
    a = ap.parse_args()
    ctx = fluhip.Context(0)
    for s in a.shapes.split(","):
        count, seconds = s.split("x")
        print(json.dumps(row(ctx, int(count), float(seconds), a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
