#!/usr/bin/env python3
"""Resident maintenance against the host round trip it replaces.  One JSON line.

  (a) vacuum     10 % of the rows soft-deleted: fvdb_ivf_compact against the old path restated through the public ABI
                 (fvdb_ivf_list_export of every list, filter on the host, fvdb_ivf_clear, fvdb_ivf_add_assigned)
  (b) retrain    nlist --nlist -> --new-nlist with the rows in HBM: gather, k-means, assignment, ranks, move
                 (fvdb_ivf_maintenance_info), bytes moved and the move's effective bandwidth
  (c) scratch    what a user had to do before: export every list, create the new index, add everything again
                 (the k-means is the same work either way and is left out of this leg)

    python tools/maint_bench.py --n 1000000 --d 384

  --graph        HNSWIndex.vacuum instead: a graph of --n nodes (bulk_build; --sequential inserts them on the device
                 instead), 10 % soft-deleted.  The resident job (fvdb_graph_vacuum) against set_resident_vacuum(False)
                 followed by the search that pays for its whole-graph re-upload, and the first device batch_insert
                 after each (the host form loses the stored edge distances).  Wall clock around whole calls, the
                 job's own stages by HIP events (vacuum_info).  The line is also written to --out.

    python tools/maint_bench.py --graph --n 1000000 --d 384 --out profiles/graph_vacuum_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fvdb_import  # noqa: E402


def build(fv, ctx, x, ids, cents, dtype):
    ix = fv.DeviceIVF(ctx, x.shape[1], cents.shape[0], dtype=dtype)
    ix.set_centroids(cents)
    ix.reserve(x.shape[0])
    cl, pos = [], []
    for o in range(0, x.shape[0], 100_000):
        c, p = ix.add(x[o:o + 100_000], ids[o:o + 100_000])
        cl.append(c)
        pos.append(p)
    return ix, np.concatenate(cl), np.concatenate(pos)


def export_all(ix):
    rows, ids, live, cl = [], [], [], []
    for c in range(ix.nlist):
        r, i, l = ix.list_export(c)
        rows.append(r)
        ids.append(i)
        live.append(l)
        cl.append(np.full(i.size, c, np.uint32))
    return np.concatenate(rows), np.concatenate(ids), np.concatenate(live).astype(bool), np.concatenate(cl)


def graph_leg(fv, ctx, a, x, ids, dead, extra, resident):
    g = fv.HNSWIndex(ctx, a.M, 2 * a.M, a.efc, seed=3)
    g.set_resident_vacuum(resident)
    if a.sequential:
        g.batch_insert(ids, x)
    else:
        g.bulk_build(ids, x)
    q = x[:256].copy()
    g.search(q, 10, 50)  # installs the device graph; warm-up of the traversal
    g.search(q, 10, 50)
    for i in dead:
        g.mark_deleted(int(ids[i]))
    rows_before = g.store_rows()
    t0 = time.perf_counter()
    removed = g.vacuum()
    t1 = time.perf_counter()
    g.search(q, 10, 50)  # the host form re-uploads the whole graph here
    t2 = time.perf_counter()
    eids = np.arange(extra.shape[0], dtype=np.uint64) + 10 ** 9
    g.batch_insert(eids, extra)  # ... and recomputes every edge distance here
    t3 = time.perf_counter()
    assert removed == len(dead) and g.insert_stats()["host_path_inserts"] == 0
    info = g.vacuum_info()
    return dict(path=info["path"], vacuum_wall_ms=(t1 - t0) * 1e3, next_search_wall_ms=(t2 - t1) * 1e3,
                vacuum_plus_search_wall_ms=(t2 - t0) * 1e3, first_insert_wall_ms=(t3 - t2) * 1e3, rows_before=rows_before,
                rows_after_vacuum=g.store_rows() - extra.shape[0], info=info)


def graph_main(a):
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    rng = np.random.default_rng(1)
    means = rng.standard_normal((256, a.d)).astype(np.float32)
    n = a.n + 512
    x = (means[rng.integers(0, 256, n)] + np.float32(0.35) * rng.standard_normal((n, a.d)).astype(np.float32))
    ids = np.arange(a.n, dtype=np.uint64)
    dead = rng.choice(a.n, a.n // 10, replace=False)
    out = dict(graph=True, n=a.n, d=a.d, M=a.M, M0=2 * a.M, ef_construction=a.efc, built="sequential" if a.sequential else "bulk_build")
    w = min(a.n, 20000)
    graph_leg(fv, ctx, a, x[:w], ids[:w], dead[dead < w], x[a.n:], True)  # warm-up: kernels loaded, allocator primed
    out["resident"] = graph_leg(fv, ctx, a, x[:a.n], ids, dead, x[a.n:], True)
    out["host"] = graph_leg(fv, ctx, a, x[:a.n], ids, dead, x[a.n:], False)
    info = out["resident"]["info"]
    out["move_TBps"] = info["move_bytes"] / max(info["ms_move"], 1e-6) / 1e9
    out["streaming_copy_TBps_guide"] = [6.0, 6.3]
    out["speedup_vacuum_plus_search"] = out["host"]["vacuum_plus_search_wall_ms"] / out["resident"]["vacuum_plus_search_wall_ms"]
    out["speedup_first_insert"] = out["host"]["first_insert_wall_ms"] / out["resident"]["first_insert_wall_ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--new-nlist", type=int, default=4096)
    ap.add_argument("--max-iterations", type=int, default=25)
    ap.add_argument("--dtype", default="f32", choices=("f32", "f16"))
    ap.add_argument("--skip-old-vacuum", action="store_true", help="leave the host round trip of leg (a) out")
    ap.add_argument("--graph", action="store_true", help="HNSW vacuum: the resident job against the host form")
    ap.add_argument("--sequential", action="store_true", help="--graph: insert the nodes on the device instead of bulk_build")
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--out", default="", help="--graph: also write the JSON line to this file")
    a = ap.parse_args()
    if a.graph:
        return graph_main(a)
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    rng = np.random.default_rng(1)
    means = rng.standard_normal((256, a.d)).astype(np.float32)
    x = (means[rng.integers(0, 256, a.n)] + np.float32(0.35) * rng.standard_normal((a.n, a.d)).astype(np.float32))
    ids = np.arange(a.n, dtype=np.uint64)
    cents = x[rng.choice(a.n, a.nlist, replace=False)].copy()
    dead = rng.choice(a.n, a.n // 10, replace=False)
    out = dict(n=a.n, d=a.d, nlist=a.nlist, new_nlist=a.new_nlist, dtype=a.dtype)

    # (a) vacuum
    ix, cl, pos = build(fv, ctx, x, ids, cents, a.dtype)
    ix.set_deleted(cl[dead], pos[dead])
    t0 = time.perf_counter()
    removed, kept = ix.compact()
    out["vacuum_resident_wall_ms"] = (time.perf_counter() - t0) * 1e3
    info = ix.maintenance_info()
    assert removed == dead.size and kept.size == a.n - dead.size
    out["vacuum_resident"] = info
    out["vacuum_move_TBps"] = info["move_bytes"] / max(info["ms_move"], 1e-6) / 1e9
    if not a.skip_old_vacuum:
        old, cl2, pos2 = build(fv, ctx, x, ids, cents, a.dtype)
        old.set_deleted(cl2[dead], pos2[dead])
        t0 = time.perf_counter()
        rows, rid, live, rcl = export_all(old)
        old.clear()
        for o in range(0, int(live.sum()), 100_000):
            old.add_assigned(rows[live][o:o + 100_000], rid[live][o:o + 100_000], rcl[live][o:o + 100_000])
        out["vacuum_host_round_trip_wall_ms"] = (time.perf_counter() - t0) * 1e3
        out["vacuum_speedup"] = out["vacuum_host_round_trip_wall_ms"] / out["vacuum_resident_wall_ms"]
        assert np.array_equal(old.list_sizes(), ix.list_sizes())
        old.close()

    # (b) retrain in HBM
    dst = fv.DeviceIVF(ctx, a.d, a.new_nlist, dtype=a.dtype)
    t0 = time.perf_counter()
    tr = dst.train_from(ix, max_iterations=a.max_iterations, seed=7)
    t1 = time.perf_counter()
    dst.assign_from(ix)
    t2 = time.perf_counter()
    dst.refill_from(ix)
    t3 = time.perf_counter()
    info = dst.maintenance_info()
    out["retrain"] = dict(info, train=tr, wall_train_ms=(t1 - t0) * 1e3, wall_assign_ms=(t2 - t1) * 1e3,
                          wall_refill_ms=(t3 - t2) * 1e3)
    out["retrain_move_TBps"] = info["move_bytes"] / max(info["ms_move"], 1e-6) / 1e9
    out["retrain_data_movement_ms"] = info["ms_gather"] + info["ms_ranks"] + info["ms_move"]

    # (c) the same index from scratch: export, create, add again
    t0 = time.perf_counter()
    rows, rid, live, _ = export_all(ix)
    t1 = time.perf_counter()
    scratch = fv.DeviceIVF(ctx, a.d, a.new_nlist, dtype=a.dtype)
    scratch.set_centroids(dst.get_centroids())
    for o in range(0, rid.size, 100_000):
        scratch.add(rows[o:o + 100_000], rid[o:o + 100_000])
    t2 = time.perf_counter()
    out["scratch"] = dict(export_wall_ms=(t1 - t0) * 1e3, add_wall_ms=(t2 - t1) * 1e3)
    assert np.array_equal(scratch.list_sizes(), dst.list_sizes())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
