"""bench.py --dump-outputs (CPU side): the arrays land as float32 .npy files, and above the size limit every array is cut
to the same fixed, seeded sample of pixels."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _frame(seed, h=48, w=64):
    rng = np.random.default_rng(seed)
    return rng.random((h, w, 3), dtype=np.float32) * 100, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_dump_outputs_whole_arrays(tmp_path):
    bench = _bench()
    accum, rgb8 = _frame(1)
    bench.dump_outputs(str(tmp_path), {"accum": accum, "rgb8": rgb8})
    assert sorted(os.listdir(tmp_path)) == ["accum.npy", "rgb8.npy"]
    a, b = np.load(tmp_path / "accum.npy"), np.load(tmp_path / "rgb8.npy")
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a, accum) and np.array_equal(b, rgb8.astype(np.float32))


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 16 << 10)
    accum, rgb8 = _frame(2)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"accum": accum, "rgb8": rgb8})
    files = ["accum.npy", "pixel_index.npy", "rgb8.npy"]
    assert sorted(os.listdir(tmp_path / "one")) == files
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in files) <= (16 << 10) + 3 * 128    # (+ the .npy headers)
    idx = np.load(tmp_path / "one" / "pixel_index.npy").astype(np.int64)
    assert 0 < idx.size < 48 * 64 and np.all(np.diff(idx) > 0)
    a, b = np.load(tmp_path / "one" / "accum.npy"), np.load(tmp_path / "one" / "rgb8.npy")
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape == (idx.size, 3)
    assert np.array_equal(a, accum.reshape(-1, 3)[idx]) and np.array_equal(b, rgb8.reshape(-1, 3)[idx].astype(np.float32))
    for f in files:                                         # the sample is fixed: two runs write the same files
        assert np.array_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f))
