#!/usr/bin/env python3
"""Filter evaluation on the device (metadata columns in HBM) against the walk over the metadata
map it replaces.

Part "evaluate": a session-shaped metadata map of --n rows ({"n": i, "tag": ..., "tags": [...], "_originalId": ...}), no
index.  For each of three filters
  selective   {"tag": "rare-7"}                          about 0.1 % of the rows
  half        {"n": {"$gte": n / 2}}                     about half
  mixed       $and of a range and an $or of a contains and an $in
it times
  python_loop   np.fromiter(rid for rid in rows if name in metadata and flt.matches(metadata[name])): the code
                "pushdown" runs, unchanged — the baseline (--loop-repeat runs, host clock)
  evaluate      MetadataColumns.evaluate warm, split by its own host clocks into kernel (upload of the program, the
                four launches, the wait for the counts), fetch (the result arrays to the host) and merge (unknown slots
                decided on the host); one warm-up, then the median, min and max of --repeat runs
  build         the one-off cost of each column the filter named first (one pass over the rows, in Python)
and checks that both give the same array.

Part "session": a VectorDbSession of --session-n rows at d = 3; whole session.search calls with "filterMode":
"pushdown" and "resident" for the same three filters, alternating, one warm-up, the median of --repeat.

Every part runs in a child process of its own under a time limit; the first failure stops the run.

    python tools/filter_eval_bench.py --json profiles/filter_eval_bench.json 2> profiles/filter_eval_bench.log
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def metadata_of(i):
    return {"n": i, "tag": f"rare-{i % 1000}", "tags": [f"t{i % 7}", f"u{i % 11}", i % 3], "_originalId": f"doc-{i}"}


def filters(n):
    return {"selective": {"tag": "rare-7"},
            "half": {"n": {"$gte": n // 2}},
            "mixed": {"$and": [{"n": {"$gte": n // 10, "$lt": n - n // 10}},
                               {"$or": [{"tags": "t3"}, {"tag": {"$in": ["rare-1", "rare-20", "rare-300", "rare-999", "none"]}}]}]}}


def stats(v):
    v = sorted(v)
    return dict(ms_median=v[len(v) // 2], ms_min=v[0], ms_max=v[-1], runs=len(v))


def log(row):
    print(json.dumps(row), file=sys.stderr, flush=True)


def part_evaluate(a, fv):
    ctx = fv.Context(0)
    n = a.n
    t0 = time.perf_counter()
    rows = {(i * 0x9E3779B97F4A7C15) & (2 ** 64 - 1): f"vec_{i:08x}" for i in range(n)}
    metadata = {f"vec_{i:08x}": metadata_of(i) for i in range(n)}
    log(dict(step="map built", n=n, seconds=time.perf_counter() - t0))
    t0 = time.perf_counter()
    cols = fv.metadata_columns.MetadataColumns(ctx, rows, metadata)
    table_s = time.perf_counter() - t0
    out = []
    for name, fj in filters(n).items():
        flt = fv.metadata_filter.MetadataFilter.from_json(fj)
        loop = []
        for _ in range(a.loop_repeat):
            t0 = time.perf_counter()
            want = np.fromiter((rid for rid, key in rows.items() if key in metadata and flt.matches(metadata[key])), np.uint64)
            loop.append((time.perf_counter() - t0) * 1e3)
        build = {}
        for p in fv.metadata_columns.filter_paths(flt):  # the one-off cost, column by column
            if p not in cols.columns:
                t0 = time.perf_counter()
                cols.ensure_column(p, metadata)
                ctx.synchronize()
                build[p] = (time.perf_counter() - t0) * 1e3
        got, info = cols.evaluate(flt, metadata)  # warm-up: program buffer, result buffers, first kernel load
        parts = {k: [] for k in ("ms_kernel", "ms_fetch", "ms_merge", "ms_total")}
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            got, info = cols.evaluate(flt, metadata)
            parts["ms_total"].append((time.perf_counter() - t0) * 1e3)
            for k in ("ms_kernel", "ms_fetch", "ms_merge"):
                parts[k].append(info[k])
        row = dict(filter=name, json=fj, rows=n, matches=int(want.size), results_equal=bool(np.array_equal(want, got)),
                   route=info["route"], unknown=info["unknown"], python_loop=stats(loop), evaluate=stats(parts["ms_total"]),
                   kernel=stats(parts["ms_kernel"]), fetch=stats(parts["ms_fetch"]), merge=stats(parts["ms_merge"]),
                   column_build_ms=build)
        row["loop_over_evaluate"] = row["python_loop"]["ms_median"] / row["evaluate"]["ms_median"]
        out.append(row)
        log(row)
    res = dict(part="evaluate", n=n, table_seconds=table_s, table_info=cols.table.info(), filters=out)
    cols.close()
    return res


def part_session(a, fv):
    ctx = fv.Context(0)
    n = a.session_n
    s = fv.VectorDbSession(ctx)
    t0 = time.perf_counter()
    step = 1000
    for o in range(0, n, step):
        s.add_vectors([{"id": f"doc-{i}", "vector": [float(i), 1.0, 0.5], "metadata": {k: v for k, v in metadata_of(i).items() if k != "_originalId"}}
                       for i in range(o, min(n, o + step))])
    log(dict(step="session built", n=n, seconds=time.perf_counter() - t0))
    q = [float(n // 3), 1.0, 0.5]
    out = []
    for name, fj in filters(n).items():
        def run(mode):
            ctx.device_synchronize()
            t0 = time.perf_counter()
            r = s.search(q, a.k, {"filter": fj, "filterMode": mode})
            return r, (time.perf_counter() - t0) * 1e3

        rp, _ = run("pushdown")
        rr, first_ms = run("resident")  # builds the table and the filter's columns
        ms = {"pushdown": [], "resident": []}
        for _ in range(a.repeat):
            ms["pushdown"].append(run("pushdown")[1])
            ms["resident"].append(run("resident")[1])
        row = dict(filter=name, rows=n, k=a.k, results_equal=rp == rr, hits=len(rr), first_resident_ms=first_ms,
                   pushdown=stats(ms["pushdown"]), resident=stats(ms["resident"]), info=s.last_filter_info())
        row["pushdown_over_resident"] = row["pushdown"]["ms_median"] / row["resident"]["ms_median"]
        out.append(row)
        log(row)
    s.destroy()
    return dict(part="session", n=n, d=3, filters=out)


def child(a):
    import fvdb_import
    fv = fvdb_import.load()
    res = part_evaluate(a, fv) if a.part == "evaluate" else part_session(a, fv)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000, help="rows of the metadata map of part evaluate")
    ap.add_argument("--session-n", type=int, default=20_000, help="rows of the session of part session")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=9, help="timed runs after one warm-up")
    ap.add_argument("--loop-repeat", type=int, default=3, help="runs of the Python loop")
    ap.add_argument("--parts", nargs="+", default=["evaluate", "session"], choices=["evaluate", "session"])
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one part may take")
    ap.add_argument("--json", default=None, help="write the parts' result lines here as one JSON document")
    ap.add_argument("--part", default=None, help="(child) run this one part in this process")
    a = ap.parse_args()
    if a.part is not None:
        return child(a)
    results = []
    for part in a.parts:
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part]
        for name in ("n", "session_n", "k", "repeat", "loop_repeat"):
            cmd += ["--" + name.replace("_", "-"), str(getattr(a, name))]
        try:
            p = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"[filter_eval_bench] {part}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 124
        if p.returncode:
            print(f"[filter_eval_bench] {part}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode
        print(p.stdout, end="", flush=True)
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(tool="tools/filter_eval_bench.py", results=results), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
