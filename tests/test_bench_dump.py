"""bench.py --dump-outputs, the host part: the arrays of a step land in DIR/{ids,distances,counts}.npy as float64 /
float32, the API's padding past a query's hit count (FVDB_NO_ID / +inf, include/fvdb.h) becomes -1, and the files of
all ranks together stay under the size limit by a sample of the queries that is the same on every call."""
import os

import numpy as np
import pytest

import bench

NO_ID = 2 ** 64 - 1  # FVDB_NO_ID


def _files(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("ids", "distances", "counts")}


def test_dump_outputs_writes_the_step_and_blanks_the_padding(tmp_path):
    # rows as the search calls return them: fewer than k hits leave FVDB_NO_ID / +inf in the tail
    ids = np.array([[5, 7, 2 ** 40], [3, NO_ID, NO_ID], [NO_ID, NO_ID, NO_ID]], np.uint64)
    dist = np.array([[0.0, 0.25, 1.5], [2.0, np.inf, np.inf], [np.inf, np.inf, np.inf]], np.float32)
    counts = np.array([3, 1, 0], np.uint32)
    bench.dump_outputs(str(tmp_path / "out"), ids, dist, counts)
    f = _files(tmp_path / "out")
    assert sorted(os.listdir(tmp_path / "out")) == ["counts.npy", "distances.npy", "ids.npy"]
    assert f["ids"].dtype == np.float64 and f["distances"].dtype == np.float32 and f["counts"].dtype == np.float64
    assert np.array_equal(f["ids"], [[5, 7, 2 ** 40], [3, -1, -1], [-1, -1, -1]])
    assert np.array_equal(f["distances"], np.array([[0.0, 0.25, 1.5], [2.0, -1, -1], [-1, -1, -1]], np.float32))
    assert np.array_equal(f["counts"], [3, 1, 0])


def test_dump_outputs_names_the_rank_when_there_are_several(tmp_path):
    bench.dump_outputs(str(tmp_path), np.zeros((2, 1), np.uint64), np.zeros((2, 1), np.float32), np.ones(2, np.uint32), rank=1, world=2)
    assert sorted(os.listdir(tmp_path)) == ["counts.rank1.npy", "distances.rank1.npy", "ids.rank1.npy"]


def test_dump_outputs_refuses_ids_float64_cannot_hold(tmp_path):
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path), np.array([[2 ** 53 + 1, NO_ID]], np.uint64), np.zeros((1, 2), np.float32), np.array([1], np.uint32))
    assert not os.listdir(tmp_path)


def test_dump_outputs_keeps_a_fixed_sample_under_the_size_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 65536)
    rng = np.random.default_rng(3)
    B, k = 4000, 4
    ids = rng.integers(0, 1 << 30, (B, k)).astype(np.uint64)
    dist = rng.random((B, k), dtype=np.float32)
    counts = np.full(B, k, np.uint32)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), ids, dist, counts)
        assert sum(os.path.getsize(tmp_path / name / f) for f in os.listdir(tmp_path / name)) <= 65536
    a, b = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert 0 < a["ids"].shape[0] < B and a["ids"].shape[0] == a["distances"].shape[0] == a["counts"].shape[0]
    for n in a:
        assert np.array_equal(a[n], b[n])
    # the kept rows are rows of the input, in their order
    rows = [int(np.flatnonzero((ids == r.astype(np.uint64)).all(axis=1))[0]) for r in a["ids"]]
    assert rows == sorted(rows) and np.array_equal(a["distances"], dist[rows])
    # the limit is for all ranks together: each of 4 ranks keeps a quarter of it
    for r in range(4):
        bench.dump_outputs(str(tmp_path / "w4"), ids, dist, counts, rank=r, world=4)
    assert len(os.listdir(tmp_path / "w4")) == 12 and 0 < np.load(tmp_path / "w4" / "ids.rank3.npy").shape[0] < a["ids"].shape[0]
    assert sum(os.path.getsize(tmp_path / "w4" / f) for f in os.listdir(tmp_path / "w4")) <= 65536
