#!/usr/bin/env python
"""bench.py -- BufNMF hot path (STFT -> magnitude -> KL-NMF -> write-back) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the headline line (plus the sanity checksum of the
last step's floats).  --full adds everything measured beside the headline: the roofline of the dominant kernels
(one extra event-profiled step, the single-layout STFT), the job with host buffers in and out, the CPU baseline
and the other BASELINE configs.  --dump-outputs DIR writes the bases and activations of the last timed step as
DIR/bases.npy and DIR/activations.npy (float32; a fixed, seeded sample of whole buffers when the job's outputs
exceed 64 MB, the chosen global buffer indices then in DIR/buffer_index.npy).

Workload (BASELINE.json metric "rank-32 fft2048", config 4's per-GPU shard): every rank holds
128 independent 10 s mono 44.1 kHz synthetic buffers (441 000 samples each), STFT win/fft 2048,
hop 512 (T = 862 frames, F = 1025 bins), NMF rank 32, 200 iterations, NMF seed 42.  One "step" =
one full pass of the hot path over the rank's 128 buffers with the audio already resident in
HBM: batched STFT+magnitude, 200 multiplicative-update iterations, float write-back of bases
and activations, and (N > 1) the RCCL all-gather of the dictionaries/activations.  Weak scaling:
per-GPU work is fixed, buffers shard across ranks with no data-path collective.

value = NMF buffer-iterations per second over the whole job
      = ranks * 128 buffers * 200 iterations / (max-over-ranks time of one step).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "flucoma-core_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402

# MI355X peaks used for the roofline fractions.  HBM: /opt/skills/guides/MI355X_MICROARCH.md
# (8.0 TB/s spec).  FP64 matrix: AMD datasheet 78.6 TFLOP/s (the guide has no f64 row) = one
# v_mfma_f64_4x4x4_4b per 16 cycles and SIMD at 2.4 GHz; tools/mfma_f64_probe measures 73.5 at the
# 2.24 GHz the part runs it at (profiles/r01/mfma_f64_probe.txt).
PEAK_HBM_GBS = 8000.0
PEAK_FP64_MFMA_TFLOPS = 78.6
PEAK_MHZ = 2400.0   # the clock the datasheet peak is quoted at (MI355X_MICROARCH.md "Max clock")

WORKLOAD = dict(buffers_per_gpu=128, seconds=10.0, sr=44100, win=2048, fft=2048, hop=512, rank=32,
                iters=200, seed=42)
DUMP_MAX_BYTES = 64_000_000


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--buffers", type=int, default=WORKLOAD["buffers_per_gpu"],
                    help="buffers per GPU (default: the BASELINE config-4 shard, 128)")
    ap.add_argument("--iters", type=int, default=WORKLOAD["iters"])
    ap.add_argument("--rank", type=int, default=WORKLOAD["rank"])
    ap.add_argument("--full", action="store_true",
                    help="also measure what lies beside the headline: roofline, host-buffer job, CPU baseline, other configs")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's bases / activations as DIR/<name>.npy (float32, at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--cpu-seconds", type=float, default=20.0, help="(--full) CPU baseline budget")
    ap.add_argument("--configs", default="auto",
                    help="(--full) BASELINE configs timed behind the headline and reported under `configs`: 'auto' = c2,c3,c5 "
                         "when the headline workload is the default one on one GPU, 'none', or a comma list of c1,c2,c3,c4x1,c5")
    ap.add_argument("--prof-in-timed-region", action="store_true",
                    help="(--full) bracket every update launch by HIP events inside the timed steps (the round-1/2 behaviour) "
                         "instead of in one extra step right behind them")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.prof_in_timed_region and not args.full:
        ap.error("--prof-in-timed-region needs --full")
    return args


def dump_outputs(out_dir, bases, acts):
    """Write the float outputs of every buffer (host arrays, global buffer order) as out_dir/<name>.npy.  When they exceed
    DUMP_MAX_BYTES, a fixed sample of whole buffers (seed 0, ascending global index) is written instead, with its indices."""
    os.makedirs(out_dir, exist_ok=True)
    total = bases.shape[0]
    per_buffer = bases[0].nbytes + acts[0].nbytes
    keep = max(1, min(total, (DUMP_MAX_BYTES - 8 * total) // per_buffer))
    if keep < total:
        idx = np.sort(np.random.default_rng(0).choice(total, size=keep, replace=False))
        np.save(os.path.join(out_dir, "buffer_index.npy"), idx.astype(np.float64))
        bases, acts = bases[idx], acts[idx]
    np.save(os.path.join(out_dir, "bases.npy"), bases)
    np.save(os.path.join(out_dir, "activations.npy"), acts)


def _cpu_worker(job):
    """one host core, one buffer: the reference's deployment unit (a std::thread per BufNMF job,
    clients/common/FluidNRTClientWrapper.hpp:1048)"""
    mag, rank, iters, seed = job
    import oracle_c
    o = oracle_c.get("native")
    t0 = time.perf_counter()
    o.nmf_process(mag, rank, iters, True, True, seed, faithful=True)
    return time.perf_counter() - t0


def cpu_all_cores(mag, wl, procs, iters):
    """Best-case host: `procs` independent jobs at once, one per process.  Returns aggregate
    buffer-iterations/s, or None when the pool cannot be started."""
    try:
        import multiprocessing as mp
        ctx = mp.get_context("spawn")  # the parent holds a live HIP runtime: do not fork it
        with ctx.Pool(procs) as pool:
            pool.map(_cpu_worker, [(mag, wl["rank"], 1, wl["seed"])] * procs)   # load the library, warm up
            t0 = time.perf_counter()
            pool.map(_cpu_worker, [(mag, wl["rank"], iters, wl["seed"])] * procs)
            wall = time.perf_counter() - t0
        return procs * iters / wall
    except Exception:
        return None


def cpu_baseline(audio_one, wl, budget_s, gpu_bases0=None, gpu_acts0=None):
    """The oracle's faithful mode (all seven GEMMs of alg/NMF.hpp:158-173 per iteration) on ONE
    buffer of the same workload, one core -- what one BufNMF job costs the reference."""
    import oracle_c
    o = oracle_c.get("native")
    n = audio_one.shape[0]
    t0 = time.perf_counter()
    _, mag = o.stft_f32(audio_one, wl["win"], wl["fft"], wl["hop"])
    t_stft = time.perf_counter() - t0
    T, F = mag.shape
    # probe 3 iterations, then size the sample to the budget
    t0 = time.perf_counter()
    o.nmf_process(mag, wl["rank"], 3, True, True, wl["seed"], faithful=True)
    per_iter = (time.perf_counter() - t0) / 3
    iters = int(max(3, min(wl["iters"], budget_s / max(per_iter, 1e-9))))
    t0 = time.perf_counter()
    oW, oH, _, _ = o.nmf_process(mag, wl["rank"], iters, True, True, wl["seed"], faithful=True)
    t_nmf = time.perf_counter() - t0
    # when the sample is the whole job of buffer 0, the timed oracle run doubles as a parity check of the very
    # result the GPU just produced for that buffer (float outputs, nrt/NMFClient.hpp:277-300)
    parity = None
    if iters == wl["iters"] and gpu_bases0 is not None and gpu_acts0 is not None:
        rb, ra = o.bufnmf_writeback(oW, oH)
        parity = {"buffer": 0, "iterations": iters,
                  "bases_max_rel_err": float(np.abs(gpu_bases0 - rb).max() / np.abs(rb).max()),
                  "activations_max_rel_err": float(np.abs(gpu_acts0 - ra).max() / np.abs(ra).max())}
    # the reference's shipped Linux default is -msse4 (script/flucoma_simdcmd.cmake:20-22): short probe
    sse4_rate = None
    try:
        o4 = oracle_c.get("sse4")
        t0 = time.perf_counter()
        o4.nmf_process(mag, wl["rank"], 3, True, True, wl["seed"], faithful=True)
        sse4_rate = 3 / (time.perf_counter() - t0)
    except Exception:
        pass
    # best-case host (reported beside the per-job figure, never as `value`): one job per core on a quarter of
    # the host's hardware threads, a few seconds
    procs = max(1, min(64, (os.cpu_count() or 1) // 4))
    all_rate = cpu_all_cores(mag, wl, procs, max(3, int(4.0 / max(per_iter, 1e-9)))) if procs > 1 else None
    executed_flop = 14.0 * F * T * wl["rank"] * iters
    try:
        core_peak = o.fma_peak_gflops()
    except Exception:
        core_peak = None
    cpu_model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {
        "value": iters / t_nmf, "unit": "iterations/s", "cores": 1, "kind": "port",
        "sample": f"1 buffer ({n} samples, T={T}, F={F}), rank {wl['rank']}, {iters} of {wl['iters']} "
                  f"iterations, oracle faithful mode (7 GEMMs/iter like alg/NMF.hpp), gcc -O3 -march=native "
                  f"(AVX-512 micro-kernels where the host has them)",
        "stft_frames_per_s": T / t_stft,
        "value_sse4_build": sse4_rate,
        "executed_gflops": executed_flop / t_nmf / 1e9,
        # the same core's FMA rate measured with nothing but register FMAs in the loop (oracle/fluid_oracle.c fo_fma_burst):
        # how much of the core the restatement's GEMMs use -- Eigen's would sit somewhere above it, the GPU / CPU ratio
        # is only as meaningful as this fraction is high
        "core_fma_peak_gflops": core_peak,
        "frac_of_core_peak": executed_flop / t_nmf / 1e9 / core_peak if core_peak else None,
        "bufnmf_wall_s_200iter_est": t_stft + t_nmf / iters * wl["iters"],
        "value_many_jobs": all_rate, "many_jobs_processes": procs, "parity_vs_gpu": parity,
        "cpu_model": cpu_model, "host_cores_available": os.cpu_count(),
    }


def main():
    args = parse()
    wl = dict(WORKLOAD)
    wl["buffers_per_gpu"], wl["iters"], wl["rank"] = args.buffers, args.iters, args.rank
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: start the launcher as a child -- one rank per GPU through
        # torch.distributed.run, rendezvous on the loopback address (the container hostname may not resolve)
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        sys.exit(subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                                  f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
                                  "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]))
    if args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    # The contract is ONE JSON line on stdout.  Libraries write there too (RCCL prints a version banner through C stdio,
    # flushed when the process exits), so file descriptor 1 is pointed at stderr for the whole run and the line goes to
    # the saved original at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    # torch first: it owns the HIP runtime the process shares; our library is loaded afterwards
    import torch
    import torch.distributed as dist
    assert torch.cuda.is_available(), "bench.py needs a GPU"
    # FLUHIP_BENCH_BACKEND=gloo is a debugging aid: it lets the N > 1 control flow run on a box with
    # fewer GPUs than ranks (ranks share devices, the gather goes through host memory).  The driver's
    # runs use the default: one rank per GPU, RCCL.
    ndev = torch.cuda.device_count()
    # fewer GPUs than ranks (a rehearsal of the N > 1 control flow on a small box): ranks share devices and the
    # gather goes through host memory; RCCL refuses two ranks on one device
    backend = os.environ.get("FLUHIP_BENCH_BACKEND", "nccl" if ndev >= world else "gloo")
    if backend == "gloo":
        local = local % ndev
    assert local < ndev, f"rank {rank}: LOCAL_RANK {local} but only {ndev} GPUs visible"
    torch.cuda.set_device(local)
    # FLUHIP_BENCH_BACKEND set explicitly at N = 1: a ONE-rank process group, so that the collective code of the N > 1
    # job (RCCL all-gather of the device-resident results, MAX all-reduce of the step time) executes on a 1-GPU box
    # exactly as written -- there is no `world > 1` short cut on that path
    use_dist = world > 1 or "FLUHIP_BENCH_BACKEND" in os.environ
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(sk.getsockname()[1]))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    import fluhip
    import sharding
    import synth
    ctx = fluhip.Context(local)
    name, arch, cus = ctx.device_info()

    B, n = wl["buffers_per_gpu"], int(wl["seconds"] * wl["sr"])
    K, iters = wl["rank"], wl["iters"]
    # synthetic corpus of world*B buffers, contiguous-block sharded; global buffer g uses audio
    # seed 1000 + g
    g_begin, g_end = sharding.shard_range(world * B, world, rank)
    # one seeded generator per buffer, so a few host threads (numpy releases the GIL) give the same audio in less set-up time
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, 8 // world)) as pool:
        audio = np.stack(list(pool.map(lambda g: synth.synth_audio(n, 1000 + g), range(g_begin, g_end))))
    corpus = fluhip.Corpus(ctx, B, n, wl["win"], wl["fft"], wl["hop"], K)
    T, F = corpus.T, corpus.F
    audio_dev = torch.from_numpy(audio).cuda()           # resident in HBM before the timed region
    corpus.set_audio_dev(audio_dev.data_ptr())
    bases = torch.empty((B, K, F), dtype=torch.float32, device="cuda")
    acts = torch.empty((B, K, T), dtype=torch.float32, device="cuda")
    gathered = {}
    # receive (and, on the gloo rehearsal path, host staging) buffers of the gather: allocated once, outside the timed steps
    host_b = host_a = None
    if use_dist:
        if backend != "nccl":
            host_b = torch.empty(bases.shape, dtype=bases.dtype).pin_memory()
            host_a = torch.empty(acts.shape, dtype=acts.dtype).pin_memory()
        gathered["bases"] = sharding.gather_buffer(bases if backend == "nccl" else host_b, world)
        gathered["acts"] = sharding.gather_buffer(acts if backend == "nccl" else host_a, world)

    loop_ms = []   # device time of every step's iteration loop (two HIP events per step, recorded by the library on its stream)

    def step():
        corpus.stft()
        corpus.nmf(iters, seed=wl["seed"])
        corpus.writeback_dev(bases.data_ptr(), acts.data_ptr())
        ctx.synchronize()
        try:
            loop_ms.append(corpus.last_loop_ms())
        except Exception:      # (never seen; the line then falls back to the per-launch event pairs)
            pass
        if use_dist:  # the one collective of the path: final dictionary/activation gather (RCCL)
            if backend == "nccl":
                src_b, src_a = bases, acts
            else:
                host_b.copy_(bases); host_a.copy_(acts)
                src_b, src_a = host_b, host_a
            sharding.gather_results(src_b, dist, world, out=gathered["bases"])
            sharding.gather_results(src_a, dist, world, out=gathered["acts"])

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        ctx.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    # The timed steps run as a user's job would: no HIP events between the launches.  The per-kernel durations of the
    # roofline (--full) come from ONE more step of the same loop right behind them, every launch of the dominant kernel
    # classes bracketed by events on the stream it is launched on (--prof-in-timed-region puts the events back into the
    # timed steps).  The shader-cycle stamps of the update kernel cost nothing measurable and cover both.
    if args.prof_in_timed_region:
        ctx.prof_enable(True)
        ctx.prof_reset()
    if args.full:
        corpus.update_clocks(reset=True)
    del loop_ms[:]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    timed_loop_ms = list(loop_ms)
    # what a caller of the timed path receives, from its last step, in global buffer order (rank 0 holds the gather)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, (gathered["bases"] if use_dist else bases).cpu().numpy(),
                     (gathered["acts"] if use_dist else acts).cpu().numpy())
    if args.full:
        if not args.prof_in_timed_region:
            ctx.prof_enable(True)
            ctx.prof_reset()
            t1 = time.perf_counter()
            step()
            fence()
            profiled_step_ms = (time.perf_counter() - t1) * 1e3
        else:
            profiled_step_ms = None
        n_upd, ms_upd = ctx.prof_read(1)
        n_stft, ms_stft = ctx.prof_read(0)
        n_mid, ms_mid = ctx.prof_read(3)
        clocks = corpus.update_clocks()
        # the STFT phase as a spectrogram-only caller runs it (fluhip_stft_*, BufSTFT: STFT::process + magnitude, the frame-major
        # magnitudes alone -- the bin-major copy is written for the H update only), outside the timed region, HIP events on the stream
        ctx.prof_reset()
        for _ in range(3):
            corpus.stft_mag_only()
        ctx.synchronize()
        n_stft1, ms_stft1 = ctx.prof_read(0)
        ctx.prof_enable(False)

    tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
    # which global buffers every rank held (rank r must hold shard_range(world * B, world, r): the rehearsal test checks it)
    rng = torch.tensor([[g_begin, g_end]], dtype=torch.int64, device=tmax.device)
    ranges = torch.empty((world, 2), dtype=torch.int64, device=tmax.device)
    if use_dist:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_gather_into_tensor(ranges, rng)
    else:
        ranges.copy_(rng)
    elapsed_max = float(tmax.item())
    shard_ranges = [[int(a), int(b)] for a, b in ranges.cpu().tolist()]

    if args.full:
        # the same job with host buffers in and out (pageable memory over PCIe), once, outside the timed region:
        # SURVEY 8(d) "end-to-end BufNMF wall-clock (H2D -> W/H D2H)"
        fence()
        t0 = time.perf_counter()
        corpus.set_audio(audio)
        corpus.stft()
        corpus.nmf(iters, seed=wl["seed"])
        bases_h, acts_h = corpus.writeback()
        host_io_ms = (time.perf_counter() - t0) * 1e3

    # sanity on the result of the last step (not timed); the checksum weights buffer g's float outputs by g + 1, over the whole
    # corpus in global buffer order, as every rank holds them after the gather -- equal for any rank count with the same
    # total number of buffers (tests/test_gpu_parity.py compares --gpus 2 against --gpus 1)
    a_host = acts.cpu().numpy()
    finite = bool(np.isfinite(a_host).all())
    all_b = gathered["bases"] if use_dist else bases
    all_a = gathered["acts"] if use_dist else acts
    wts = torch.arange(1, all_b.shape[0] + 1, dtype=torch.float64, device=all_b.device)
    checksum = float((wts * (all_b.double().sum(dim=(1, 2)) + all_a.double().sum(dim=(1, 2)))).sum().item())

    if rank == 0:
        ms_per_step = elapsed_max / args.steps * 1e3
        value = world * B * iters * args.steps / elapsed_max
        out = {
            "metric": f"NMF iterations/sec (buffer-iterations over the whole BufNMF job: STFT + {iters}-iter "
                      f"KL-NMF + write-back), rank-{K} fft{wl['fft']}",
            "value": value, "unit": "iterations/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"BASELINE config 4 shard: {B} x 10 s mono 44.1 kHz buffers per GPU, "
                                   f"fft 2048 / hop 512, rank {K}, {iters} iterations, seed 42",
                       "buffers_per_gpu": B, "samples": n, "frames": T, "bins": F, "rank": K,
                       "iterations": iters, "parallelism": f"shard{world}" if world > 1 else "single"},
            "schedule": corpus.plan(),
            "device": {"name": name, "arch": arch, "compute_units": cus,
                       "corpus_device_bytes": corpus.device_bytes()},
            "result_finite": finite, "result_checksum": checksum, "total_buffers": world * B,
            "shard_ranges": shard_ranges,
            "backend": ("single process" if not use_dist else
                        ("rccl" if backend == "nccl" else backend + " (ranks share devices)") +
                        (" (one-rank group: the collectives of the N > 1 job executed on one GPU)" if world == 1 else "")),
        }
        if args.full:
            # dominant kernel: nmf_update (one launch = one factor update of all B buffers; when the Nyquist bin is a
            # side column 1/F of the W update's flops run in the slice kernel between the updates -- not subtracted)
            # (corpora of several rounds of wavefronts run round by round: a launch then covers one round's buffers, not all B)
            prof_steps = args.steps if args.prof_in_timed_region else 1
            buffers_per_launch = B * (2.0 * iters * prof_steps) / max(n_upd, 1)
            flop_per_launch = 4.0 * F * T * K * buffers_per_launch
            bytes_per_launch = (F * T * 8.0 + 2.0 * (F * K + K * T) * 8.0) * buffers_per_launch
            stft_ms = ms_stft / max(n_stft, 1)
            stft_bytes = (wl["hop"] * 4.0 + F * 8.0) * T * B
            # The dominant kernel's average launch duration, over the TIMED steps: the iteration loop of a
            # step is 2 x iters launches of nmf_update5_kernel back to back and nothing else in the stream (the side column and
            # the norm combine ride inside them; the helper launches of a call's first iteration are in the figure too), and the
            # library brackets that loop with two HIP events on the stream it launches on -- behind the host-side initialisation,
            # behind the last launch.  loop time / launches is the launch duration with its boundary to the next launch, and by
            # construction launches x avg_launch_ms + STFT <= ms_per_step.  The per-launch event pairs of one extra step (which
            # perturb the stream they measure: a pair per launch) are kept beside it as `avg_launch_ms_event_pairs`.
            avg_ms_pairs = ms_upd / max(n_upd, 1)
            launches_per_step = n_upd / prof_steps
            avg_ms = (sum(timed_loop_ms) / len(timed_loop_ms)) / max(launches_per_step, 1) if timed_loop_ms else avg_ms_pairs
            ach_tflops = flop_per_launch / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
            ach_gbs = bytes_per_launch / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            # HBM bytes per launch from the PMC passes committed under profiles/ (FETCH_SIZE doubled per the
            # gfx950 rocprofv3 correction + WRITE_SIZE); only quoted for the workload they were taken on
            # ... and only while the kernel source still hashes to what the counters were taken on (a kernel change must not
            # keep quoting the old kernel's traffic: null until tools/pmc_bench.sh + tools/pmc_summary.py are re-run)
            traffic, traffic_src = None, None
            import hashlib
            try:
                ksha = hashlib.sha256(open(os.path.join(ROOT, "flucoma-core_amd", "csrc", "kernels_nmf5.hip"), "rb").read()).hexdigest()
            except OSError:
                ksha = None
            for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
                try:
                    path = os.path.join("profiles", rnd, "pmc_update_kernel.json")
                    pmc = json.load(open(os.path.join(ROOT, path)))
                    if (B, K, T, F) != (128, 32, 862, 1025):
                        break
                    if pmc.get("kernel_source_sha256") == ksha:
                        traffic = pmc["hbm_bytes_per_launch"]
                        traffic_src = (f"{path}: separate rocprofv3 --pmc passes of this command, not measured in this run; taken on "
                                       f"kernels_nmf5.hip sha256 {ksha[:16]} = the source of this build")
                    else:
                        traffic_src = (f"{path} was taken on another state of kernels_nmf5.hip "
                                       f"({str(pmc.get('kernel_source_sha256'))[:16]} against {str(ksha)[:16]}): traffic withheld")
                    break
                except (OSError, KeyError, ValueError):
                    pass
            # shader cycles per launch and the clock the part sustained while it ran them (s_memtime / s_memrealtime stamps of
            # one wavefront per launch, fluhip_corpus_update_clocks): a kernel change moves cycles_per_launch whatever the box;
            # frac_at_sustained_clock prices the same achieved rate against the peak at THAT clock instead of 2.4 GHz
            cyc = [c["cycles_per_launch"] for c in clocks.values() if c["cycles_per_launch"]]
            mhz = [c["sustained_mhz"] for c in clocks.values() if c["sustained_mhz"]]
            cycles_per_launch = sum(cyc) / len(cyc) if cyc else None
            sustained_mhz = sum(mhz) / len(mhz) if mhz else None
            out.update({
                "job_wall_ms_host_buffers_in_and_out": host_io_ms,
                "stft_frames_per_s": (T * B) / (stft_ms * 1e-3) if stft_ms > 0 else None,
                "nmf_iterations_per_s_kernel_only": buffers_per_launch / (2.0 * avg_ms * 1e-3) if avg_ms > 0 else None,
                "roofline": {"bound": "mfma", "kernel": "nmf_update5_kernel (v_mfma_f64_4x4x4_4b + LDS-DMA)", "achieved": ach_tflops,
                             "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach_tflops / PEAK_FP64_MFMA_TFLOPS,
                             "traffic": traffic, "traffic_from_profile": traffic_src,
                             "launches": int(launches_per_step), "launches_per": "step", "avg_launch_ms": avg_ms,
                             "buffers_per_launch": buffers_per_launch,
                             "events": "two HIP events per TIMED step around its iteration loop, on the library's stream "
                                       "(fluhip_corpus_last_loop_ms): loop time / launches",
                             "timed_loop_ms_per_step": {"mean": sum(timed_loop_ms) / max(len(timed_loop_ms), 1),
                                                        "min": min(timed_loop_ms) if timed_loop_ms else None,
                                                        "max": max(timed_loop_ms) if timed_loop_ms else None},
                             "closes": {"launches_x_avg_launch_ms_plus_stft": launches_per_step * avg_ms + stft_ms,
                                        "ms_per_step": ms_per_step},
                             "avg_launch_ms_event_pairs": avg_ms_pairs,
                             "event_pairs": "in the timed steps" if args.prof_in_timed_region else "one extra step right behind the timed ones",
                             "profiled_step_ms": profiled_step_ms,
                             "shader_cycles_per_launch": cycles_per_launch, "sustained_mhz": sustained_mhz,
                             "datasheet_mhz": PEAK_MHZ,
                             "frac_at_sustained_clock": (ach_tflops / (PEAK_FP64_MFMA_TFLOPS * sustained_mhz / PEAK_MHZ)
                                                         if sustained_mhz else None),
                             # The event pair of a launch that sits right behind another launch also holds the boundary between the
                             # two (drain of the slowest wavefronts, end-of-kernel release, dispatch): with two launches per iteration
                             # and nothing else in the stream, avg_launch_ms is the iteration's whole period / 2.  The stamped
                             # wavefront's own life (shader_cycles_per_launch at sustained_mhz) is the launch without that boundary:
                             "stamped_wavefront_ms": (cycles_per_launch / (sustained_mhz * 1e3)
                                                      if cycles_per_launch and sustained_mhz else None),
                             "frac_of_stamped_wavefront": (flop_per_launch / (cycles_per_launch / (sustained_mhz * 1e6)) / 1e12
                                                           / PEAK_FP64_MFMA_TFLOPS if cycles_per_launch and sustained_mhz else None),
                             "clock_stamps": clocks,
                             "flop_per_launch": flop_per_launch, "bytes_per_launch": bytes_per_launch,
                             "hbm_view": {"achieved": ach_gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                          "frac": ach_gbs / PEAK_HBM_GBS}},
                # algorithmic bytes per frame: hop 4 in + F 8 out; the kernel writes V in BOTH layouts the factor
                # updates stream (frame-major and bin-major), i.e. 2 F 8 bytes per frame really leave the chip
                "roofline_stft": {"bound": "hbm", "kernel": "stft_block_kernel (both magnitude layouts in one pass; no transposing copy)",
                                  "avg_launch_ms": stft_ms,
                                  "written_gbs": ((wl["hop"] * 4.0 + 2 * F * 8.0) * T * B) / (stft_ms * 1e-3) / 1e9 if stft_ms > 0 else None,
                                  "achieved": stft_bytes / (stft_ms * 1e-3) / 1e9 if stft_ms > 0 else None,
                                  "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                  "frac": (stft_bytes / (stft_ms * 1e-3) / 1e9 / PEAK_HBM_GBS) if stft_ms > 0 else None},
                # what the transform costs a caller that wants the spectrogram and nothing else -- ONE layout
                # (fluhip_corpus_stft_mag_only = the path of fluhip_stft_* / BufSTFT as a corpus-sized batch); algorithmic bytes = bytes moved
                "roofline_stft_single_layout": {"bound": "hbm", "kernel": "stft_block_kernel, frame-major magnitudes only",
                                                "avg_launch_ms": ms_stft1 / max(n_stft1, 1),
                                                "frames_per_s": (T * B) / (ms_stft1 / max(n_stft1, 1) * 1e-3) if ms_stft1 > 0 else None,
                                                "achieved": stft_bytes / (ms_stft1 / max(n_stft1, 1) * 1e-3) / 1e9 if ms_stft1 > 0 else None,
                                                "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                                "frac": (stft_bytes / (ms_stft1 / max(n_stft1, 1) * 1e-3) / 1e9 / PEAK_HBM_GBS) if ms_stft1 > 0 else None},
            })
            # (launches between the two factor updates, summed over the profiled step and divided by its ITERATIONS: in the
            #  two-launch steady state only the first iteration of a call has any)
            out["schedule"].update(between_updates_ms_per_iteration=(ms_mid / max(args.iters * (args.steps if args.prof_in_timed_region else 1), 1)),
                                   between_updates_launch_groups_per_step=n_mid)
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(audio[0], wl, args.cpu_seconds, bases[0].cpu().numpy(), a_host[0])
                gpu_job_s = elapsed_max / args.steps / B   # per-buffer share of one step
                out["cpu_baseline"]["gpu_speedup_per_buffer_job"] = (
                    out["cpu_baseline"]["bufnmf_wall_s_200iter_est"] * (iters / WORKLOAD["iters"]) / gpu_job_s)
            # the other BASELINE configs, timed by this process right behind the headline (outside its timed region): c2 and
            # c3 are the shapes SURVEY 8(d) names beside c4, c5 is the feature pipeline.  One GPU, default workload only.
            names = []
            if args.configs == "auto":
                headline = (B, K, iters) == (WORKLOAD["buffers_per_gpu"], WORKLOAD["rank"], WORKLOAD["iters"])
                names = ["c2", "c3", "c5"] if (world == 1 and headline) else []
            elif args.configs != "none":
                names = [c for c in args.configs.split(",") if c]
            if names and world == 1:
                corpus.close()
                corpus = None
                del audio_dev, bases, acts
                torch.cuda.empty_cache()
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                import bench_configs
                out["configs"] = bench_configs.bench_line_configs(ctx, names)
            # the cross-check the line must pass on its own figures: the dominant kernel's launches fit into the step they were timed in
            # (by construction: the loop's events lie inside the step's wall-clock bracket).  With the STFT launch -- event-timed in the
            # extra step behind the timed ones -- added, the sum stays below ms_per_step as well; that second sum is reported, not
            # asserted (a slow STFT sample of another step must not cost the driver its bench line).
            cl = out["roofline"]["closes"]
            cl["launches_x_avg_launch_ms"] = launches_per_step * avg_ms
            cl["with_stft_ok"] = bool(cl["launches_x_avg_launch_ms_plus_stft"] <= cl["ms_per_step"])
            assert not timed_loop_ms or cl["launches_x_avg_launch_ms"] <= cl["ms_per_step"] * 1.0005, \
                f"the roofline's launch time does not fit into the step it was taken from: {cl}"
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if corpus is not None:
        corpus.close()
    ctx.close()


if __name__ == "__main__":
    main()
