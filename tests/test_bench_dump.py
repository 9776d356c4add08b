"""bench.py --dump-outputs: the .npy files written from polled rows (CPU only)."""
import os

import numpy as np

import bench


def _parts():
    """Two polls of rows (chunk, type, ts, values, nulls) over columns (string id, double, float)."""
    def part(n, base):
        vals = np.empty((n, 3), np.uint64)
        vals[:, 0] = np.arange(base, base + n, dtype=np.uint64)
        vals[:, 1] = (np.arange(n) * 0.25 + base).astype(np.float64).view(np.uint64)
        vals[:, 2] = (np.arange(n) * 0.5 - base).astype(np.float32).view(np.uint32).astype(np.uint64)
        return (np.arange(n, dtype=np.int64) // 2, np.zeros(n, np.int32),
                1_700_000_000_000 + np.arange(base, base + n, dtype=np.int64), vals,
                (np.arange(n * 3).reshape(n, 3) % 5 == 0).astype(np.uint8))
    return [part(5, 0), part(7, 100)]


def test_dump_rows_writes_decoded_float64_arrays(tmp_path):
    parts = _parts()
    got, kept = bench.dump_rows(str(tmp_path), parts, [0, 4, 3])
    assert (got, kept) == (12, 12)
    a = {f[:-4]: np.load(str(tmp_path / f)) for f in sorted(os.listdir(str(tmp_path)))}
    assert sorted(a) == ["chunk", "nulls", "rows", "ts", "type", "values"]
    assert all(x.dtype == np.float64 for x in a.values())
    np.testing.assert_array_equal(a["rows"], np.arange(12))
    np.testing.assert_array_equal(a["ts"], np.concatenate([p[2] for p in parts]))
    np.testing.assert_array_equal(a["chunk"][:5], parts[0][0])
    np.testing.assert_array_equal(a["chunk"][5:], parts[1][0] + (1 << 32))
    np.testing.assert_array_equal(a["nulls"], np.concatenate([p[4] for p in parts]))
    np.testing.assert_array_equal(a["values"][:, 0], np.r_[np.arange(5), np.arange(100, 107)])
    np.testing.assert_array_equal(a["values"][:, 1], np.r_[np.arange(5) * 0.25, np.arange(7) * 0.25 + 100])
    np.testing.assert_array_equal(a["values"][:, 2], np.r_[np.arange(5) * 0.5, np.arange(7) * 0.5 - 100])


def test_dump_rows_samples_the_same_rows_every_time(tmp_path, monkeypatch):
    parts = _parts()
    monkeypatch.setattr(bench, "DUMP_LIMIT", 8 * (4 + 2 * 3) * 6)   # room for 6 of the 12 rows
    assert bench.dump_rows(str(tmp_path / "a"), parts, [0, 4, 3]) == (12, 6)
    assert bench.dump_rows(str(tmp_path / "b"), parts, [0, 4, 3]) == (12, 6)
    rows = np.load(str(tmp_path / "a" / "rows.npy"))
    assert len(rows) == 6 and np.all(np.diff(rows) > 0)
    ts_all = np.concatenate([p[2] for p in parts])
    np.testing.assert_array_equal(np.load(str(tmp_path / "a" / "ts.npy")), ts_all[rows.astype(np.int64)])
    total = 0
    for f in os.listdir(str(tmp_path / "a")):
        x, y = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= bench.DUMP_LIMIT


def test_dump_rows_of_a_step_without_rows(tmp_path):
    assert bench.dump_rows(str(tmp_path), [], [0, 4, 4]) == (0, 0)
    assert np.load(str(tmp_path / "values.npy")).shape == (0, 3)
