#!/usr/bin/env python3
"""The graph-health job (fvdb_graph_health) against the two other ways to the same answers.

A random well-formed digraph of --n nodes is installed with restore (levels drawn with p = 0.4 and capped at 3, out-degree
uniform in 0..--m0 on layer 0 and 0..--m0/2 above, targets among the nodes of sufficient level, drawn with replacement),
--deleted of the nodes soft-deleted, the entry a live node of the top level.  Timed:

  (1) device   HNSWIndex.graph_health() with the graph already in HBM: the job's own HIP-event time and the wall clock
               around the call (best and median of --reps), plus how it ran (launches, reach steps, scratch)
  (2) host     the mirror's restatement of the same definitions over its own lists (device traversal off)
  (3) export   export_graph() followed by the Python reference of the tests (tests/_graph_health_ref.py): the only way
               to these answers without the job

All three must agree on every integer figure, the histogram, the unreachable ids and the component labels.  One JSON line,
also written to --out.

    python tools/graph_health_bench.py --out profiles/graph_health_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fvdb_import  # noqa: E402
import _graph_health_ref as ref  # noqa: E402


def random_digraph(n, m0, deleted, seed):
    rng = np.random.default_rng(seed)
    levels = np.minimum(rng.geometric(0.6, n) - 1, 3).astype(np.uint32)
    levels[int(rng.integers(n))] = 3
    slots_of = levels.astype(np.int64) + 1
    slot_node = np.repeat(np.arange(n, dtype=np.int64), slots_of)
    first = np.cumsum(slots_of) - slots_of
    slot_layer = np.arange(slot_node.size, dtype=np.int64) - first[slot_node]
    deg = np.where(slot_layer == 0, rng.integers(0, m0 + 1, slot_node.size), rng.integers(0, m0 // 2 + 1, slot_node.size))
    off = np.zeros(slot_node.size + 1, np.uint64)
    off[1:] = np.cumsum(deg)
    edge_layer = np.repeat(slot_layer, deg)
    nbrs = np.empty(edge_layer.size, np.uint64)
    for l in range(4):
        pool = np.flatnonzero(levels >= l)
        at = np.flatnonzero(edge_layer == l)
        nbrs[at] = pool[rng.integers(0, pool.size, at.size)]
    dead = rng.random(n) < deleted
    top = np.flatnonzero((levels == 3) & ~dead)
    entry = int(top[0]) if top.size else int(np.flatnonzero(levels == 3)[0])
    dead[entry] = False
    return levels, off, nbrs, np.flatnonzero(dead), entry


def figures(h):
    return {k: h[k] for k in ref.INT_FIELDS}, h["degree0_hist"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--m0", type=int, default=32)
    ap.add_argument("--deleted", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_health_bench.json"))
    a = ap.parse_args()
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    t = time.perf_counter()
    levels, off, nbrs, dead, entry = random_digraph(a.n, a.m0, a.deleted, a.seed)
    print(f"graph drawn: {a.n} nodes, {nbrs.size} stored links, {dead.size} deleted ({time.perf_counter() - t:.1f} s)", flush=True)
    h = fv.HNSWIndex(ctx, max(a.m0 // 2, 1), a.m0, 50, seed=1)
    ids = np.arange(a.n, dtype=np.uint64)
    rows = np.zeros((a.n, 4), np.float32)
    rows[:, 0] = np.arange(a.n) % 1024
    t = time.perf_counter()
    h.restore(ids, rows, levels, off, nbrs, entry)
    for r in dead:
        h.mark_deleted(int(r))
    h._graph()  # the one whole-graph upload happens here, outside the timed calls
    print(f"installed and uploaded ({time.perf_counter() - t:.1f} s)", flush=True)

    # (1) the device job
    wall, ms, dev = [], [], None
    for _ in range(a.reps):
        t = time.perf_counter()
        dev = h.graph_health()
        wall.append((time.perf_counter() - t) * 1e3)
        ms.append(dev["ms"])
    assert dev["path"] == "device"
    t = time.perf_counter()
    dev_lost = h.unreachable_ids()
    dev_labels = h.component_labels()[1]
    per_node_ms = (time.perf_counter() - t) * 1e3
    print(f"device: {min(ms):.3f} ms by events, {min(wall):.3f} ms wall", flush=True)

    # (2) the mirror's host restatement
    h.set_device_traversal(False)
    t = time.perf_counter()
    host = h.graph_health()
    host_ms = (time.perf_counter() - t) * 1e3
    assert host["path"] == "host"
    host_lost = h.unreachable_ids()
    host_labels = h.component_labels()[1]
    h.set_device_traversal(True)
    print(f"host restatement: {host_ms:.1f} ms", flush=True)

    # (3) export_graph() and the Python reference
    t = time.perf_counter()
    gi, lv, goff, gnb = h.export_graph()
    export_ms = (time.perf_counter() - t) * 1e3
    print(f"export_graph: {export_ms:.1f} ms", flush=True)
    t = time.perf_counter()
    f, reached, label = ref.graph_health(gi, lv, goff, gnb, ids[dead], entry)
    py_ms = (time.perf_counter() - t) * 1e3
    print(f"python reference: {py_ms:.1f} ms", flush=True)
    dead_set = np.zeros(a.n, bool)
    dead_set[dead] = True
    ref_lost = np.array([u for u in range(a.n) if not dead_set[u] and not reached[u]], np.uint64)
    ref_labels = np.array([2 ** 64 - 1 if x == ref.NONE32 else x for x in label], np.uint64)

    agree = (figures(dev) == figures(host) == ({k: f[k] for k in ref.INT_FIELDS}, f["degree0_hist"])
             and np.array_equal(dev_lost, host_lost) and np.array_equal(dev_lost, ref_lost)
             and np.array_equal(dev_labels, host_labels) and np.array_equal(dev_labels, ref_labels))
    out = {"tool": "graph_health_bench", "n": a.n, "m0": a.m0, "deleted": a.deleted, "seed": a.seed, "stored_links": int(nbrs.size),
           "adjacency_bytes": int(a.n) * (a.m0 + 1) * 4,
           "device_ms_events_best": min(ms), "device_ms_events_median": float(np.median(ms)),
           "device_ms_wall_best": min(wall), "device_ms_wall_median": float(np.median(wall)),
           "device_per_node_results_ms": per_node_ms,
           "host_restatement_ms": host_ms, "export_graph_ms": export_ms, "python_reference_ms": py_ms,
           "export_plus_reference_ms": export_ms + py_ms,
           "launches": dev["launches"], "reach_launches": dev["reach_launches"], "host_syncs": dev["host_syncs"],
           "reach_rounds0": dev["reach_rounds0"], "scratch_bytes": dev["scratch_bytes"],
           "figures": {k: dev[k] for k in ref.INT_FIELDS}, "all_three_agree": bool(agree)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    if not agree:
        sys.exit("the device job, the host restatement and the Python reference disagree")


if __name__ == "__main__":
    main()
