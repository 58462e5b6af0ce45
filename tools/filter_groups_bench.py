#!/usr/bin/env python3
"""Batched filtered search, one allow-set per query, against the loop it replaces.

B queries are spread over G distinct allow-sets of --selectivity of the rows each (query b takes set b mod G):
  grouped   ONE search_allowed_groups call for the batch
  loop      G calls of the existing search_allowed, each on the queries of its group — what a host had to do before
for G in --groups, on
  ivf       IVFIndex over --n rows (the wide score stage with one live word per (block, query))
  graph     HNSWIndex over --graph-n nodes with every group scanned exactly (scan_cutoff = always)
HIP events around each whole call (mask builds included on both sides: every call of the loop rebuilds the one cached
mask, the grouped call builds G), both warmed, the two alternating in one process, the median of --repeat.  At G = 1 the
two take different routes at the same k (the wide selection against the register path); that figure is reported as it is.

Every part runs in a child process of its own under a time limit; the first failure stops the run.

    python tools/filter_groups_bench.py --json profiles/filter_groups_bench.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def data(a, n, rng):
    means = rng.standard_normal((a.nlist, a.d)).astype(np.float32)
    x = means[rng.integers(0, a.nlist, n)] + np.float32(0.35) * rng.standard_normal((n, a.d)).astype(np.float32)
    q = means[rng.integers(0, a.nlist, a.batch)] + np.float32(0.35) * rng.standard_normal((a.batch, a.d)).astype(np.float32)
    return means, x, q


def measure(ctx, a, n, grouped, one):
    """grouped(sets, group) and one(queries_idx, allowed) -> per G the two medians and whether the results agree."""
    rng = np.random.default_rng(2)
    ids = np.arange(n, dtype=np.uint64)
    rows = []
    for G in a.groups:
        sets = [np.ascontiguousarray(ids[rng.random(n) < a.selectivity]) for _ in range(G)]
        group = (np.arange(a.batch) % G).astype(np.uint32)
        members = [np.flatnonzero(group == g) for g in range(G)]

        def run_grouped():
            return grouped(sets, group)

        def run_loop():
            return [one(members[g], sets[g]) for g in range(G)]

        def timed(fn):
            ctx.device_synchronize()
            ctx.timer_start()
            r = fn()
            return r, ctx.timer_stop_ms()

        rg, _ = timed(run_grouped)  # warm both: scratch, pinned blocks, first kernel loads
        rl, _ = timed(run_loop)
        equal = all(np.array_equal(rg.ids[members[g]], rl[g].ids) and
                    np.array_equal(rg.distances[members[g]].view(np.uint32), rl[g].distances.view(np.uint32)) and
                    np.array_equal(rg.counts[members[g]], rl[g].counts) for g in range(G))
        ms = {"grouped": [], "loop": []}
        for _ in range(a.repeat):  # alternating
            ms["grouped"].append(timed(run_grouped)[1])
            ms["loop"].append(timed(run_loop)[1])
        row = dict(G=G, allowed_per_set=int(np.mean([s.size for s in sets])), results_equal_bits=bool(equal))
        for name, v in ms.items():
            v.sort()
            row[name] = dict(ms_median=v[len(v) // 2], ms_min=v[0], ms_max=v[-1], runs=len(v))
        row["loop_over_grouped"] = row["loop"]["ms_median"] / row["grouped"]["ms_median"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return rows


def child(a):
    import fvdb_import
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    rng = np.random.default_rng(1)
    if a.part == "ivf":
        n = a.n
        means, x, q = data(a, n, rng)
        ix = fv.IVFIndex(ctx, n_clusters=a.nlist, n_probe=a.nprobe)
        ix.set_trained(means)
        step = 100_000
        for o in range(0, n, step):
            ix.batch_insert(np.arange(o, min(n, o + step), dtype=np.uint64), x[o:o + step])
        rows = measure(ctx, a, n, lambda sets, group: ix.search_allowed_groups(q, a.k, sets, group, a.nprobe),
                       lambda idx, allowed: ix.search_allowed(q[idx], a.k, allowed, a.nprobe))
        out = dict(part="ivf", n=n, d=a.d, nlist=a.nlist, nprobe=a.nprobe, batch=a.batch, k=a.k, selectivity=a.selectivity, rows=rows)
    else:
        n = a.graph_n
        means, x, q = data(a, n, rng)
        g = fv.HNSWIndex(ctx, 16, 32, 100, seed=3)
        g.batch_insert(np.arange(n, dtype=np.uint64), x)
        g.scan_cutoff = fv.HNSWIndex.SCAN_ALWAYS
        rows = measure(ctx, a, n, lambda sets, group: g.search_allowed_groups(q, a.k, a.ef, sets, group),
                       lambda idx, allowed: g.search_allowed(q[idx], a.k, a.ef, allowed))
        out = dict(part="graph", n=n, d=a.d, batch=a.batch, k=a.k, selectivity=a.selectivity, rows=rows)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--graph-n", type=int, default=300_000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--ef", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--selectivity", type=float, default=0.01)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--parts", nargs="+", default=["ivf", "graph"], choices=["ivf", "graph"])
    ap.add_argument("--repeat", type=int, default=5, help="timed runs of each side, after one warm-up")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds one part may take")
    ap.add_argument("--json", default=None, help="write the parts' result lines here as one JSON document")
    ap.add_argument("--part", default=None, help="(child) run this one part in this process")
    a = ap.parse_args()
    if a.part is not None:
        return child(a)
    results = []
    for part in a.parts:
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--graph-n", str(a.graph_n), "--groups", *map(str, a.groups)]
        for name in ("n", "d", "nlist", "nprobe", "ef", "k", "batch", "selectivity", "repeat"):
            cmd += [f"--{name}", str(getattr(a, name))]
        try:
            p = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"[filter_groups_bench] {part}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 124
        if p.returncode:
            print(f"[filter_groups_bench] {part}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode
        print(p.stdout, end="", flush=True)
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(tool="tools/filter_groups_bench.py", results=results), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
