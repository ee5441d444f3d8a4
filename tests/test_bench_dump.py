"""bench.py --dump-outputs, on the CPU: `dump_outputs` writes whole arrays while they fit DUMP_LIMIT, and beyond it the same fixed,
seeded sample of pixels from every array with the sample's flat pixel indices (the form an N > 1 run's 1600x1600 frame takes)."""
import os

import numpy as np

import bench


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def _frame(h, w, dtype):
    rng = np.random.default_rng(5)
    return rng.random((h, w, 3)).astype(dtype), rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def test_dump_outputs_writes_the_whole_frame_under_the_limit(tmp_path):
    for dtype in (np.float64, np.float32):
        lin, rgba = _frame(40, 30, dtype)
        out = tmp_path / np.dtype(dtype).name
        bench.dump_outputs(str(out), {"linear": lin, "rgba8": rgba})
        got = _load(out)
        assert sorted(got) == ["linear", "rgba8"]
        assert got["linear"].dtype == dtype and np.array_equal(got["linear"], lin)
        assert got["rgba8"].dtype == np.float32 and np.array_equal(got["rgba8"], rgba.astype(np.float32))


def test_dump_outputs_samples_a_frame_over_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 64 << 10)
    lin, rgba = _frame(200, 150, np.float64)                       # 1.2 MB as float64 + float32: ~19x the limit
    bench.dump_outputs(str(tmp_path / "a"), {"linear": lin, "rgba8": rgba})
    bench.dump_outputs(str(tmp_path / "b"), {"linear": lin, "rgba8": rgba})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["linear", "pixel_index", "rgba8"]
    assert all(np.array_equal(a[k], b[k]) for k in a)              # fixed seed: the same sample every run
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_LIMIT
    idx = a["pixel_index"]
    assert idx.dtype == np.float64 and np.array_equal(idx, np.round(idx))
    idx = idx.astype(np.int64)
    assert len(idx) > 1000 and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < 200 * 150
    assert a["linear"].dtype == np.float64 and a["linear"].shape == (len(idx), 3)
    assert a["rgba8"].dtype == np.float32 and a["rgba8"].shape == (len(idx), 4)
    assert np.array_equal(a["linear"], lin.reshape(-1, 3)[idx])
    assert np.array_equal(a["rgba8"], rgba.reshape(-1, 4)[idx].astype(np.float32))
