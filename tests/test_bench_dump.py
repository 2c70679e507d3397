"""bench.py --dump-outputs on the host: what it writes for a job whose outputs fit the limit, and the fixed sample of whole
buffers it writes instead when they do not."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_cli", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    bench = _bench()
    rs = np.random.RandomState(0)
    b = rs.rand(10, 3, 5).astype(np.float32)
    a = rs.rand(10, 3, 7).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "all"), b, a)
    assert sorted(os.listdir(tmp_path / "all")) == ["activations.npy", "bases.npy"]
    assert np.array_equal(np.load(tmp_path / "all" / "bases.npy"), b)
    assert np.array_equal(np.load(tmp_path / "all" / "activations.npy"), a)
    # room for four buffers and the index: four whole buffers, ascending, the same four on every run
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * (b[0].nbytes + a[0].nbytes) + 8 * len(b))
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), b, a)
    idx = np.load(tmp_path / "s1" / "buffer_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 4 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "buffer_index.npy"))
    sel = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "s1" / "bases.npy"), b[sel])
    assert np.array_equal(np.load(tmp_path / "s1" / "activations.npy"), a[sel])
    assert sum(np.load(tmp_path / "s1" / f).nbytes for f in os.listdir(tmp_path / "s1")) <= bench.DUMP_MAX_BYTES
