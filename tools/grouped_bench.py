"""Grouped search against the path it replaces.

  (a) IVFIndex.search(fetch_k) alone: what both sides start from;
  (b) IVFIndex.search_grouped(k, group_size, fetch_k): the search, the key lookup in the metadata columns in HBM and
      the selection on the device, the groups copied back;
  (c) the replaced path: search(fetch_k), ids and distances on the host, grouped by a Python loop through the metadata
      map (row id -> name -> dict -> field), the first k groups with group_size members each.

Host clocks around calls that return after a synchronising copy; one warm-up call, then RUNS timed calls, median and
range reported per point.  (c)'s groups are compared with (b)'s on every query of the last run.  Writes one JSON line per
point to stdout and everything to --out.

  python tools/grouped_bench.py --out profiles/grouped_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fvdb_import  # noqa: E402

RUNS = 7


def timed(fn):
    fn()  # warm-up
    ts, out = [], None
    for _ in range(RUNS):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}, out


def by_loop(res, rows, md, path, k, group_size):
    """the Python loop a caller writes today: per query the first k groups of up to group_size row ids"""
    out = []
    for b in range(len(res)):
        ids, _ = res[b]
        order, members = [], {}
        for rid in ids.tolist():
            m = md.get(rows.get(rid))
            if m is None or path not in m:
                continue
            key = m[path]
            got = members.get(key)
            if got is None:
                got = members[key] = []
                order.append(key)
            got.append(rid)
        out.append([(key, members[key][:group_size]) for key in order[:k]])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    rng = np.random.default_rng(0)
    n, d, nlist = args.rows, args.dim, 256
    x = rng.standard_normal((n, d)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64) + 1
    ix = fv.IVFIndex(ctx, n_clusters=nlist, n_probe=32)
    ix.set_trained(x[rng.choice(n, nlist, replace=False)])
    ix.batch_insert(ids, x)
    q = x[rng.choice(n, args.queries, replace=False)] + 0.01 * rng.standard_normal((args.queries, d)).astype(np.float32)
    rows = {int(i): f"row{int(i)}" for i in ids}
    points = []
    for cardinality in (16, 1024, 65536):
        md = {rows[int(i)]: {"doc": f"doc{int(i) % cardinality}"} for i in ids}
        cols = fv.metadata_columns.MetadataColumns(ctx, rows, md)
        cols.group_column("doc")
        for fetch_k in (256, 4096):
            k, gs = 10, 3
            a, cand = timed(lambda: ix.search(q, fetch_k))
            b, grouped = timed(lambda: ix.search_grouped(q, k, gs, fetch_k, cols, "doc"))
            c, looped = timed(lambda: by_loop(ix.search(q, fetch_k), rows, md, "doc", k, gs))
            differ = 0
            for i in range(len(grouped)):
                got = [(cols.decode_key(t, w), g.tolist()) for t, w, g, _, _, _ in grouped[i]]
                differ += got != looped[i]
            point = {"rows": n, "dim": d, "queries": args.queries, "keys": cardinality, "fetch_k": fetch_k, "k": k, "group_size": gs,
                     "search_alone": a, "search_grouped_device": b, "search_then_python_loop_host": c,
                     "queries_where_the_two_differ": differ, "median_candidates": float(np.median(cand.counts))}
            print(json.dumps(point), flush=True)
            points.append(point)
        cols.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"runs_per_point": RUNS, "clock": "host perf_counter around synchronising calls", "points": points}, f, indent=1)


if __name__ == "__main__":
    main()
