"""tests/golden/reference_corpus_mfcc_sample.npz: the reference's pre-analysed corpus, a fixed sample of its slices.

flucoma-core ships `Resources/Data/flucoma_corpus_mfcc.json` -- for every slice of its concatenated demo files
(`flucoma_corpus_slices.wav` holds the slice points, `flucoma_corpus_files.json` the file order) the mean and deviation
over the slice's frames of BufMFCC's coefficients 1..13, computed by a FluCoMa build.  299 slices lie inside the first
three files (16-bit 44.1 kHz and 24-bit 48 kHz material); all of their audio is too large for a test vector, so this
script keeps slice 0, the slices that straddle a file boundary, and 8 slices of at most 6144 samples drawn per file with
seed 0 -- their samples (24-bit scale, int32: a 16-bit sample v is stored as 256 v) and their rows of the JSON.
tests/test_oracle.py recomputes them with both oracles.

    python tools/make_reference_corpus_sample_fixture.py <flucoma-core checkout>
"""
import json
import os
import struct
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_FILE, MAX_LEN, SEED = 8, 6144, 0


def pcm24(path):
    with wave.open(path, "rb") as w:
        ch, sw, raw = w.getnchannels(), w.getsampwidth(), w.readframes(w.getnframes())
    if sw == 2:
        v = np.frombuffer(raw, "<i2").astype(np.int32) * 256
    else:
        assert sw == 3
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3)
        v = b[:, 0].astype(np.int32) | (b[:, 1].astype(np.int32) << 8) | (b[:, 2].astype(np.int8).astype(np.int32) << 16)
    return v.reshape(-1, ch)[:, 0]


def main(checkout):
    res = os.path.join(checkout, "Resources")
    names = json.load(open(os.path.join(res, "Data", "flucoma_corpus_files.json")))["data"]
    files = [names[str(i)][0] for i in range(3)]
    audio = [pcm24(os.path.join(res, "AudioFiles", f)) for f in files]
    cat = np.concatenate(audio)
    ends = np.cumsum([len(a) for a in audio])
    raw = open(os.path.join(res, "Data", "flucoma_corpus_slices.wav"), "rb").read()
    i = raw.find(b"data")
    points = np.frombuffer(raw[i + 8:i + 8 + struct.unpack("<I", raw[i + 4:i + 8])[0]], "<f4").astype(np.int64)
    rows = json.load(open(os.path.join(res, "Data", "flucoma_corpus_mfcc.json")))["data"]
    n = sum(1 for k in range(len(points) - 1) if points[k + 1] <= len(cat))
    assert n == 299, n
    file_of = np.searchsorted(ends, points[:n], side="right")
    pick = {0} | {k for k in range(n) if file_of[k] != np.searchsorted(ends, points[k + 1] - 1, side="right")}
    rng = np.random.default_rng(SEED)
    for f in range(len(files)):
        cand = [k for k in range(n) if file_of[k] == f and k not in pick and points[k + 1] - points[k] <= MAX_LEN]
        pick |= {int(k) for k in rng.choice(cand, size=PER_FILE, replace=False)}
    pick = np.array(sorted(pick))
    segs = [cat[points[k]:points[k + 1]] for k in pick]
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "reference_corpus_mfcc_sample.npz"),
                        pcm24=np.concatenate(segs), offsets=np.concatenate([[0], np.cumsum([len(s) for s in segs])]),
                        slices=pick, source_file=file_of[pick],
                        expected=np.array([rows["%d.000000" % k] for k in pick], dtype=np.float64),
                        source=np.array("flucoma-core Resources/AudioFiles/%s (concatenated, slices of "
                                        "Resources/Data/flucoma_corpus_slices.wav); Resources/Data/flucoma_corpus_mfcc.json "
                                        "rows of the same slices" % ", ".join(files)))
    print("wrote", len(pick), "slices,", sum(len(s) for s in segs), "samples")


if __name__ == "__main__":
    main(sys.argv[1])
