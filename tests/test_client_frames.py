"""csrc/client_frames.h on the host (no GPU): the one definition of the clients' frame bookkeeping -- how many frames a
control client analyses and keeps (control_frames), how many a slicer fires (slice_frames), where its detections land
(detections_to_indices) -- against the numpy restatements of the clients: pitch_ref.client_frames for latency = win,
the lengths onset_ref / novelty_ref return on zero signals for latency = hop and the novelty latencies, and
spikes_to_times fed as those two feed it.  tests/cpp/client_frames_host.cpp includes only that header."""
import os
import subprocess

import numpy as np
import pytest

import novelty_ref
import onset_ref
import pitch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "client_frames_host.cpp")

NS = (1, 63, 64, 65, 1000, 4097)
WIN_HOP = ((64, 16), (64, 64), (100, 30), (64, 96), (1024, 512))   # hop | win, hop == win, hop not dividing win, hop > win, the defaults
MODES = (0, 1, 2)
NOVELTY = ((3, 1), (31, 5))                                        # (kernelSize, filterSize)


def fft_of(win):
    return max(4, 1 << (win - 1).bit_length())


def latencies(win, hop):
    """name -> latency of every client family"""
    return {"win": win, "hop": hop, **{kf: novelty_ref.latency(hop, *kf) for kf in NOVELTY}}


def build(tmp_path, *flags):
    exe = str(tmp_path / ("client_frames_host" + ("_san" if flags else "")))
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def ask(exe, queries):
    """one line of integers back per query line"""
    r = subprocess.run([exe], input="".join(q + "\n" for q in queries), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == len(queries) and all(row[0] == q[0] for row, q in zip(rows, queries))
    return [[int(v) for v in row[1:]] for row in rows]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("client_frames"))


def control_queries():
    keys = [(n, win, hop, mode, name) for n in NS for win, hop in WIN_HOP for mode in MODES for name in latencies(win, hop)]
    return keys, [f"c {n} {win} {hop} {mode} {latencies(win, hop)[name]}" for n, win, hop, mode, name in keys]


def slice_queries():
    keys = [(n, win, hop, name) for n in NS for win, hop in WIN_HOP for name in latencies(win, hop) if name != "win"]
    return keys, [f"s {n} {hop} {latencies(win, hop)[name]}" for n, win, hop, name in keys]


def feed_spikes(det, hop, latency, n, start_frame):
    """bufonsetslice / bufnoveltyslice behind their detections: the spike train of the padded signal, spikes inside the
    latency moved to its end, the n samples behind the latency through spikes_to_times"""
    padded = -(-(n + latency) // 64) * 64
    onsets = np.zeros(padded + hop, dtype=np.float32)
    onsets[np.flatnonzero(det) * hop] = 1
    onsets = onsets[:padded]
    if (onsets[:latency] > 0).any():
        onsets[latency] = 1
    a = onset_ref.spikes_to_times(onsets[latency:latency + n], start_frame)
    b = novelty_ref.spikes_to_times(onsets[latency:latency + n], start_frame)
    assert np.array_equal(a, b)
    return a


def detection_cases():
    """(name, hop, latency, n, det) for latency = hop and 3 hop: nothing fires, a firing only inside the latency, one exactly
    at the latency, one past n (alone, and behind a kept one), several kept ones; T as slice_frames counts it"""
    out = []
    for hop, mult, n in ((16, 1, 100), (16, 3, 100), (30, 1, 65), (30, 3, 65), (64, 1, 1), (64, 3, 1)):
        latency = mult * hop
        T = -(-(-(-(n + latency) // 64) * 64) // hop)
        at = latency // hop                  # the frame that stands exactly at the latency
        last = (n - 1 + latency) // hop      # the last frame that stands inside the n samples
        assert at <= last < T

        def det(*frames):
            d = np.zeros(T, dtype=np.uint8)
            d[[f for f in frames if 0 <= f < T]] = 1
            return d
        out.append(("nothing", hop, latency, n, det()))
        out.append(("inside the latency", hop, latency, n, det(0)))
        if mult > 1:
            out.append(("inside the latency, late", hop, latency, n, det(at - 1)))
        out.append(("at the latency", hop, latency, n, det(at)))
        out.append(("inside and at the latency", hop, latency, n, det(0, at)))
        if last + 1 < T:
            out.append(("past n alone", hop, latency, n, det(last + 1)))
            out.append(("kept and past n", hop, latency, n, det(last, last + 1, T - 1)))
        out.append(("several", hop, latency, n, det(0, at, at + 1, last)))
        out.append(("all", hop, latency, n, np.ones(T, dtype=np.uint8)))
    return out


def detection_queries():
    keys = [(c, start, cap) for c in detection_cases() for start in (0, 1000) for cap in (0, 1, 2, 64)]
    return keys, [f"d {hop} {latency} {n} {start} {cap} {''.join(map(str, det))}" for (_, hop, latency, n, det), start, cap in keys]


def test_control_frames_latency_win_against_the_pitch_restatement(exe):
    keys, queries = control_queries()
    checked = 0
    for (n, win, hop, mode, name), (user_pad, padded, T, drop, keep) in zip(keys, ask(exe, queries)):
        if name != "win":
            continue
        first, frames = pitch_ref.client_frames(n, win, hop, mode)
        assert user_pad == (0, win >> 1, win - hop)[mode] and drop == win // hop and keep == T - drop
        if frames >= 1:
            assert padded >= win and keep == frames and drop * hop - win - user_pad == first, (n, win, hop, mode)
            checked += 1
        else:   # "not enough frames", as the entry points test it
            assert padded < win or keep < 1, (n, win, hop, mode)
    assert checked > len(NS) * len(WIN_HOP) * len(MODES) // 2   # (the rest of the grid is too short for a frame)


def ref_length(fn):
    """frames a restatement returns on a zero signal; 0 when it has none to give (a negative count is a ValueError there)"""
    try:
        return len(fn())
    except ValueError:
        return 0


def test_control_frames_latency_hop_and_novelty_against_the_lengths_of_the_restatements(exe):
    keys, queries = control_queries()
    checked = {"hop": 0, **{kf: 0 for kf in NOVELTY}}
    for (n, win, hop, mode, name), (user_pad, padded, T, drop, keep) in zip(keys, ask(exe, queries)):
        x = np.zeros(n, dtype=np.float32)
        fft = fft_of(win)
        if name == "hop":
            frames = ref_length(lambda: onset_ref.bufonsetfeature(x, win=win, fft=fft, hop=hop, padding_mode=mode))
        elif name in NOVELTY and win >= 100 and fft >= 128:   # (the restatement's feature rows need fft / 2 + 1 >= 40 bins)
            frames = ref_length(lambda: novelty_ref.bufnoveltyfeature(x, k=name[0], f=name[1], win=win, fft=fft, hop=hop, padding_mode=mode))
        else:
            continue
        assert drop == latencies(win, hop)[name] // hop and keep == T - drop
        if frames >= 1:
            assert padded >= win and keep == frames, (n, win, hop, mode, name)
            checked[name] += 1
        else:
            assert padded < win or keep < 1, (n, win, hop, mode, name)
    grid = len(NS) * len(MODES)   # rows per (win, hop): all five for the onset family, the two with win >= 100 for novelty;
    assert checked["hop"] > 5 * grid // 2 and all(checked[kf] > 2 * grid // 2 for kf in NOVELTY), checked   # more than half have frames


def test_slice_frames_against_the_slicers_restatements(exe):
    keys, queries = slice_queries()
    checked = 0
    for (n, win, hop, name), (padded, T) in zip(keys, ask(exe, queries)):
        latency = latencies(win, hop)[name]
        assert padded == -(-(n + latency) // 64) * 64 and T == -(-padded // hop)   # the `padded` / `T` lines of the two slicers
        x = np.zeros((1, n), dtype=np.float32)
        fft = fft_of(win)
        if name == "hop":      # one curve value per frame
            assert T == len(onset_ref.bufonsetslice(x, win=win, fft=fft, hop=hop, want_filtered=True)[1])
        elif win >= 100 and fft >= 128:
            assert T == len(novelty_ref.bufnoveltyslice(x, k=name[0], f=name[1], win=win, fft=fft, hop=hop, want_curve=True)[1])
        else:
            continue
        checked += 1
    assert checked == len(NS) * (len(WIN_HOP) + 2 * len(NOVELTY))


def test_detections_to_indices_against_spikes_to_times(exe):
    keys, queries = detection_queries()
    seen = set()
    for ((name, hop, latency, n, det), start, cap), (count, *written) in zip(keys, ask(exe, queries)):
        want = feed_spikes(det, hop, latency, n, start)
        assert count == len(want) and written == list(want[:cap]), (name, hop, latency, n, start, cap)
        seen.add(name)
        if name in ("nothing", "past n alone"):
            assert list(want) == [-1]
        if name in ("inside the latency", "inside the latency, late", "at the latency", "inside and at the latency"):
            assert list(want) == [start]
        if name == "all" and cap in (1, 2) and n > 1:
            assert count > cap   # capacity smaller than the count: the count is still whole
    assert {"nothing", "inside the latency", "at the latency", "past n alone", "kept and past n", "several"} <= seen


def test_under_address_and_undefined_behaviour_sanitizers(exe, tmp_path):
    """the same queries through a -fsanitize=address,undefined build (stand-alone; the runtimes linked statically so the
    run does not depend on what else the host loads): clean, and the same answers"""
    san = build(tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                "-static-libasan", "-static-libubsan")
    queries = control_queries()[1] + slice_queries()[1] + detection_queries()[1]
    assert ask(san, queries) == ask(exe, queries)
