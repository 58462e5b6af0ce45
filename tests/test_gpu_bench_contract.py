"""The driver-facing contract of bench.py, on a small workload: stdout carries exactly ONE JSON line with the agreed
keys; with --full the `roofline` and `cpu_baseline` objects are included, the roofline fraction is a fraction, and the
GPU answers of the sample equal the oracle's, while a plain run measures its steps and leaves those entries null;
--dump-outputs leaves the results of the last timed step, whichever way the steps ran."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_fields(tmp_path):
    shape = [sys.executable, os.path.join(ROOT, "bench.py"), "--n-vectors", "60000", "--nlist", "64", "--steps", "6",
             "--warmup", "1", "--query-batches", "4", "--train-sample", "20000", "--batch", "256"]
    cmd = shape + ["--full", "--select-batches", "2", "--cpu-sample", "64", "--compare-host-walk", "1", "--insert-sample", "256",
                   "--dump-outputs", str(tmp_path / "pipelined")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[:2000]  # libraries' chatter must not reach stdout
    j = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in j, key
    assert j["n_gpus"] == 1 and j["steps"] == 6 and j["warmup"] == 1 and j["higher_is_better"] is True
    assert j["unit"] == "queries/s" and j["value"] > 0 and j["vs_baseline"] is None and j["data"] == "synthetic"
    assert abs(j["value"] - 256 * 6 / (j["ms_per_step"] * 6 / 1e3)) / j["value"] < 0.02  # value = queries / timed seconds
    assert "workload" in j["config"] and "model" not in j["config"]
    r = j["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert 0.0 < r["frac"] <= 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert 0.0 <= r["list_scan"]["frac"] <= 1.0
    c = j["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] == "port" and c["value"] > 0 and c["gpu_matches_oracle_on_sample"] is True
    # addVectors' path: the headline's graph is the reference's sequential build, and further inserts at its full size are
    # timed on the GPU beside the CPU oracle, with identical adjacency lists
    assert j["config"]["hnsw_graph"].startswith("sequential insert")
    ins = j["insert_path"]
    for key in ("value", "unit", "graph_nodes", "sample", "cpu_value", "cpu_cores", "graph_matches_oracle_on_sample", "whole_build"):
        assert key in ins, key
    assert ins["unit"] == "inserts/s" and ins["value"] > 0 and ins["cpu_value"] > 0 and ins["cpu_cores"] == 1
    assert ins["graph_matches_oracle_on_sample"] is True and ins["device_insert"]["host_path_inserts"] == 0
    # --dump-outputs: what search_dev_end returned for the last of the 6 timed steps
    ids, dist, cnt = (np.load(tmp_path / "pipelined" / f"{n}.npy") for n in ("ids", "distances", "counts"))
    assert ids.dtype == np.float64 and dist.dtype == np.float32 and cnt.dtype == np.float64
    assert ids.shape == dist.shape == (256, 10) and cnt.shape == (256,)
    assert cnt.min() >= 1 and cnt.max() <= 10
    live = np.arange(10)[None, :] < cnt[:, None]
    assert (ids[live] >= 0).all() and (ids[live] < 60000).all() and (dist[live] >= 0).all()
    assert (ids[~live] == -1).all() and (dist[~live] == -1).all()
    # ... of THAT step: step 5 of 6 over 4 query batches searched batch 1 (the warm-up ends on batches 0 and 3, step 0
    # searched batch 0), so every returned row lies at the returned distance from its query of batch 1, and the rows are
    # the batch's nearest ones
    gen = bench.Generator()
    x = np.concatenate([gen.rows(10_000, stream=c) for c in range(6)]).astype(np.float64)
    q = gen.rows(256, stream=10_000_000 + 1).astype(np.float64)
    qi, slot = np.nonzero(live)
    assert np.allclose(np.linalg.norm(x[ids[live].astype(np.int64)] - q[qi], axis=1), dist[live], rtol=1e-4)
    d2 = (q * q).sum(1)[:, None] - 2.0 * q @ x.T + (x * x).sum(1)[None, :]
    exact = np.argsort(d2, axis=1)[:, :10]
    assert bench.recall_at_k(ids.astype(np.int64), cnt.astype(np.int64), exact, 10) >= 0.9
    # the same step collected one batch at a time (search_dev instead of search_dev_begin / _end), at the operating
    # point the first run chose, in a plain run: the same arrays
    one = shape + ["--in-flight", "1", "--nprobe", str(j["config"]["nprobe"]), "--ef", str(j["config"]["hnsw_ef"]),
                   "--dump-outputs", str(tmp_path / "one")]
    p = subprocess.run(one, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    for n, a in (("ids", ids), ("distances", dist), ("counts", cnt)):
        assert np.array_equal(np.load(tmp_path / "one" / f"{n}.npy"), a), n
    # and the plain run's line: the headline entries of the first run, and nothing that takes steps or runs of its own
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[:2000]
    plain = json.loads(lines[0])
    for key in ("metric", "unit", "n_gpus", "steps", "warmup", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert plain[key] == j[key], key
    assert plain["value"] > 0 and abs(plain["value"] - 256 * 6 / (plain["ms_per_step"] * 6 / 1e3)) / plain["value"] < 0.02
    assert plain["config"]["recall_at_10"] == j["config"]["recall_at_10"]
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["insert_path"] is None
    assert plain["config"]["other_traversal_mode"] is None and j["config"]["other_traversal_mode"]["steps"] == 1
    assert plain["config"]["host_collect_merge_ms_per_step"] is None
    assert not [w for w in ("cpu baseline", "insert path", "other traversal mode") if w in p.stderr]


def test_dump_outputs_takes_rows_with_fewer_than_k_hits(tmp_path):
    # c2 with ONE probed list (about 100 rows each) and k = 100: many queries get fewer than k hits, the search pads
    # their rows with FVDB_NO_ID / +inf, and the dump writes that padding as -1
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c2", "--nprobe", "1", "--k", "100", "--steps", "3",
           "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    assert len([ln for ln in p.stdout.splitlines() if ln.strip()]) == 1, p.stdout[:2000]
    ids, dist, cnt = (np.load(tmp_path / f"{n}.npy") for n in ("ids", "distances", "counts"))
    assert ids.shape == dist.shape == (256, 100) and cnt.shape == (256,)
    assert cnt.min() < 100 and cnt.max() <= 100
    live = np.arange(100)[None, :] < cnt[:, None]
    assert (ids[live] >= 0).all() and (ids[live] < 100_000).all() and np.isfinite(dist[live]).all() and (dist[live] >= 0).all()
    assert (ids[~live] == -1).all() and (dist[~live] == -1).all()
