"""bench.py --dump-outputs on the host side: what is written, in which dtype, and the 64 MB bound (no GPU needed)."""
import os

import numpy as np

import bench


def _data(B, nx, gathered_rows=None, W=101):
    rng = np.random.default_rng(1)
    info = rng.normal(size=(B, 8)).astype(np.float32)
    return {"X": rng.normal(size=(B, nx)).astype(np.float32), "info": info,
            "gathered": None if gathered_rows is None else rng.normal(size=(gathered_rows, W)).astype(np.float32)}


def test_dump_writes_the_returned_arrays(tmp_path):
    d = _data(256, 915)
    bench.dump_outputs(str(tmp_path), d)
    assert sorted(os.listdir(tmp_path)) == ["info.npy", "x.npy"]
    x, info = np.load(tmp_path / "x.npy"), np.load(tmp_path / "info.npy")
    np.testing.assert_array_equal(x, d["X"])
    np.testing.assert_array_equal(info, np.delete(d["info"], 6, axis=1))    # solve_cycles (a clock count) left out
    assert x.dtype == np.float32 and info.dtype == np.float32


def test_dump_samples_the_same_rows_under_the_bound(tmp_path):
    d = _data(20000, 915, gathered_rows=40000)                                # ~140 MB in all
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), d)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_LIMIT
    for f in os.listdir(a):
        arr = np.load(a / f)
        assert arr.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(arr, np.load(b / f))                     # seeded: the same sample every run
    rows = np.load(a / "x_rows.npy").astype(np.int64)
    np.testing.assert_array_equal(np.load(a / "x.npy"), d["X"][rows])
    np.testing.assert_array_equal(np.load(a / "info_rows.npy"), rows)
    grows = np.load(a / "gathered_rows.npy").astype(np.int64)
    np.testing.assert_array_equal(np.load(a / "gathered.npy"), d["gathered"][grows])
