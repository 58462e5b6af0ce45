#!/usr/bin/env python3
"""What one quality grid costs against the loop of evaluate_search_quality calls it replaces.
One JSON line, also written to --out.

  grid   one HybridIndex.quality_grid call over E ef values x P n_probe values: one exact search, E traversals,
         P list searches, one device job that merges and counts every pair
  loop   HybridIndex.evaluate_search_quality at every pair, one call each: the sweep a user runs today (E x P exact
         searches, E x P traversals, E x P list searches)

Both run in one process on one index, on the same tree, alternating after a warm-up; each pass is timed with the host
clock around the blocking call (every call ends in a device synchronise).  The figure of a variant is the median of
--reps passes, reported with its minimum and maximum.  The grid's entries are compared with the loop's, bit for bit.

    python tools/quality_grid_bench.py --out profiles/quality_grid_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fvdb_import  # noqa: E402

DAY = 86400.0


def note(msg):
    print(f"[quality_grid_bench] {msg}", file=sys.stderr, flush=True)


def ints(text):
    return [int(v) for v in text.split(",") if v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--recent-frac", type=float, default=0.3)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--efs", type=ints, default=[10, 20, 40, 80, 160, 320])
    ap.add_argument("--n-probes", type=ints, default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    fv = fvdb_import.load()
    ctx = fv.Context(0)
    rng = np.random.default_rng(1)
    means = rng.standard_normal((a.nlist, a.d)).astype(np.float32)
    now = 1000 * DAY
    h = fv.HybridIndex(ctx, max_connections=16, max_connections_layer_0=32, ef_construction=100, n_clusters=a.nlist, n_probe=8)
    t0 = time.perf_counter()
    # the bulk loader takes the whole table in one call (307 MB at the default shape)
    x = means[rng.integers(0, a.nlist, a.n)] + np.float32(0.35) * rng.standard_normal((a.n, a.d), dtype=np.float32)
    h.set_ivf_centroids(x[:a.nlist].copy())
    age = np.where(rng.random(a.n) < a.recent_frac, 1 * DAY, 30 * DAY)  # nothing falls due during the run
    h.bulk_insert(np.arange(a.n, dtype=np.uint64), x, now - age, now)
    del x
    q = means[rng.integers(0, a.nlist, a.B)] + np.float32(0.35) * rng.standard_normal((a.B, a.d)).astype(np.float32)
    note(f"index built in {time.perf_counter() - t0:.1f} s: {a.n} x {a.d}, nlist {a.nlist}, recent {h.recent_count()}, "
         f"historical {h.historical_count()}")

    k, efs, n_probes = a.k, a.efs, a.n_probes
    single = h.evaluate_search_quality if k <= 256 else h.evaluate_search_quality_wide

    def grid():
        return h.quality_grid(q, k, efs, n_probes, now=now)

    def loop():
        return [[single(q, k, now=now, hnsw_ef=ef, ivf_n_probe=p) for p in n_probes] for ef in efs]

    variants = [("grid", grid), ("loop", loop)]
    last = {}
    for name, fn in variants:  # warm-up: scratch allocated, code objects loaded
        last[name] = fn()
    note("warmed up")
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):  # alternate, so that drift hits both alike
        for name, fn in variants:
            t = time.perf_counter()
            last[name] = fn()
            times[name].append((time.perf_counter() - t) * 1e3)
    ms = {name: float(np.median(v)) for name, v in times.items()}
    spread = {name: [float(np.min(v)), float(np.max(v))] for name, v in times.items()}
    note(f"timed: {ms}")

    g, rows = last["grid"], last["loop"]
    bits = lambda v: np.float32(v).view(np.uint32)  # noqa: E731
    equal = all(bits(g["avg_recall"][i, j]) == bits(rows[i][j]["avg_recall"]) and
                bits(g["avg_precision"][i, j]) == bits(rows[i][j]["avg_precision"])
                for i in range(len(efs)) for j in range(len(n_probes)))
    points = fv.index.pareto_points(g, 0.95)
    line = dict(bench="quality_grid", n=a.n, d=a.d, nlist=a.nlist, recent=int(h.recent_count()),
                historical=int(h.historical_count()), B=a.B, k=k, efs=efs, n_probes=n_probes, reps=a.reps, call_ms=ms,
                call_ms_min_max=spread, grid_over_loop=ms["grid"] / ms["loop"], grid_equals_loop_bits=bool(equal),
                avg_recall=[[float(v) for v in row] for row in g["avg_recall"]],
                operating_points_0_95=[[p["ef"], p["n_probe"]] for p in points])
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
