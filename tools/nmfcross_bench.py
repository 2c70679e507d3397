"""BufNMFCross timing on one GPU: one JSON line per shape (fft 1024 / hop 512, 44.1 kHz synthetic audio).

    python tools/nmfcross_bench.py [--shapes 3x3,30x30,120x60] [--iters 10]

Device times come from rocprofv3 --kernel-trace --stats, one profiled child process per measurement (the child makes one
call of `iters` iterations; its set-up -- the host's draw of the T K initial values, the uploads -- launches no kernel and
so is not in any figure).  Per shape (source seconds x target seconds; K = source frames, T = target frames, F = 513):
  loop_us_per_iter     the NMFCross H loop: the GEMM kernels with their reduce launches + the continuity stencil (+ the
                       last iteration's sparsity / polyphony, spread over the iterations), summed kernel time / iters
  gemm_us_per_iter     the two GEMMs alone (cross_gemm_kernel + cross_reduce_kernel)
  tflops, peak_frac    4 F K T flop per iteration over gemm_us_per_iter, and its fraction of the 78.6 TFLOP/s FP64-matrix
                       datasheet peak (bench.py's constant)
  wide_us_per_iter     the same H update on the any-rank path of the plain NMF (kernels_nmf_wide.hip: dgemm_tile_kernel, the
                       in-place ratio, the apply and column-sum launches), run by the measurement build
                       (lib_ab, FLUHIP_CROSS_WIDE=1) in the same call shape; speedup = wide / gemm.  Those kernels run up
                       to rank 1024 only (null above)
  gl_us_per_iter       one Griffin-Lim iteration (ISTFT frames + overlap-add, STFT, phase update), summed kernel time / iters
  job_ms_median        the whole client call (fluhip_bufnmfcross_f32, default parameters: 50 NMF + 50 Griffin-Lim
                       iterations), wall clock, median of 3 unprofiled calls; includes the host-side draws (T K values for H,
                       T F phases) and the copies
  kernels              per-kernel totals (us per iteration) of the loop run"""
from __future__ import annotations

import argparse
import csv
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flucoma-core_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

PEAK_FP64_MATRIX = 78.6e12  # bench.py
SR, WIN, FFT, HOP = 44100, 1024, 1024, 512
LIB_AB = os.path.join(ROOT, "flucoma-core_amd", "lib_ab", "libflucoma_hip_ab.so")


def _audio(src_s, tgt_s):
    import oracle_np
    return (oracle_np.synth_audio(int(src_s * SR), 11).astype(np.float32),
            oracle_np.synth_audio(int(tgt_s * SR), 12).astype(np.float32))


def _mags(ctx, src, tgt):
    _, W0 = ctx.stft(src, WIN, FFT, HOP, want_spec=False)
    tspec, X = ctx.stft(tgt, WIN, FFT, HOP)
    return W0, X, tspec[..., 0] + 1j * tspec[..., 1]


def child(shape, what, iters):
    import fluhip
    src_s, tgt_s = (float(v) for v in shape.split("x"))
    ctx = fluhip.Context(0)
    src, tgt = _audio(src_s, tgt_s)
    if what in ("loop", "wide"):
        W0, X, _ = _mags(ctx, src, tgt)
        ctx.nmfcross_process(X, W0, 7, 11, 7, iters, seed=1)
    else:
        import oracle_np  # (the spectrum on the host: no STFT launch of the set-up in the profile)
        ctx.griffinlim(oracle_np.stft(tgt, WIN, FFT, HOP)[0], len(tgt), WIN, FFT, HOP, iters=iters, seed=1)
    ctx.close()


def profiled(shape, what, iters):
    d = tempfile.mkdtemp()
    env = dict(os.environ)
    if what == "wide":
        env["FLUHIP_LIB"] = LIB_AB
        env["FLUHIP_CROSS_WIDE"] = "1"
    cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "b",
           "--", sys.executable, os.path.abspath(__file__), "--child", shape, what, str(iters)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"profiled run failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    path = None
    for root, _dirs, files in os.walk(d):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                path = os.path.join(root, f)
    rows = {row["Name"]: float(row["TotalDurationNs"]) for row in csv.DictReader(open(path))}
    shutil.rmtree(d, ignore_errors=True)
    return rows


def _sum(rows, keys, iters):
    return sum(v for n, v in rows.items() if any(k in n for k in keys)) / iters / 1e3


def run_shape(shape, iters):
    import fluhip
    loop = profiled(shape, "loop", iters)
    # the any-rank path's kernels run up to rank 1024 (its column-sum launch is one workgroup row of Kp threads; the ABI
    # entry that reaches them, fluhip_nmf_process_f64, rejects larger ranks for that reason): no baseline above that
    k_src = (int(float(shape.split("x")[0]) * SR) + HOP) // HOP
    wide = profiled(shape, "wide", iters) if k_src <= 1024 else None
    gl = profiled(shape, "gl", iters)
    ctx = fluhip.Context(0)
    src_s, tgt_s = (float(v) for v in shape.split("x"))
    src, tgt = _audio(src_s, tgt_s)
    W0, X, _ = _mags(ctx, src, tgt)
    K, F = W0.shape
    T = X.shape[0]
    jobs = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.bufnmfcross(src, tgt, WIN, FFT, HOP, seed=1)
        jobs.append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    flop = 4.0 * F * K * T
    gemm = _sum(loop, ("cross_gemm_kernel", "cross_reduce_kernel"), iters)
    loop_all = _sum(loop, ("cross_gemm_kernel", "cross_reduce_kernel", "cross_continuity", "cross_sparsity", "cross_polyphony"),
                    iters)
    wide_update = _sum(wide, ("dgemm_tile_kernel", "ratio_inplace_kernel", "wide_apply_kernel", "colsum"), iters) if wide else None
    return {"shape": f"{shape} s", "K": K, "T": T, "F": F, "iters": iters, "gflop_per_iter": flop / 1e9,
            "loop_us_per_iter": loop_all, "gemm_us_per_iter": gemm, "tflops": flop / (gemm * 1e-6) / 1e12,
            "peak_frac": flop / (gemm * 1e-6) / PEAK_FP64_MATRIX, "wide_us_per_iter": wide_update,
            "speedup_vs_wide": wide_update / gemm if wide else None,
            "gl_us_per_iter": _sum(gl, ("resynth", "stft", "gl_update"), iters), "job_ms_median": statistics.median(jobs),
            "kernels": {n.split("(")[0][-60:]: round(v / iters / 1e3, 2) for n, v in sorted(loop.items(), key=lambda kv: -kv[1])[:8]}}


def main():
    if "--child" in sys.argv:
        i = sys.argv.index("--child")
        child(sys.argv[i + 1], sys.argv[i + 2], int(sys.argv[i + 3]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="3x3,11x30,30x30,120x60")
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    for s in args.shapes.split(","):
        print(json.dumps(run_shape(s, args.iters)), flush=True)


if __name__ == "__main__":
    main()
