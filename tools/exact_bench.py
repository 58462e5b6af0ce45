#!/usr/bin/env python3
"""Exact k-NN over the rows a graph holds: the flat scan against the two routes that existed before it (DESIGN.md
section 9k).

On an HNSWIndex of --n rows x --d, for both row elements ("f32", "f16") and a batch of --batch queries:
  flat      HNSWIndex.search_exact: the tile scan of the row store where it lies; ms per call and rows*queries/s
  copy      the route the project's tools took for ground truth: a second, one-list flat index holding a full copy of
            every row (built as bench.py's exact_ground_truth builds it), then search_all; build and search timed apart
  allowed   HNSWIndex.search_allowed with every id allowed and scan_cutoff at its maximum: the gather scan
and whether the three answers are identical (ids and distance bits).

The scan reads rows and liveness flags, never links, so the graph is installed with restore() as a ring: the rows get
into the store the way a restored index's do, without a million sequential inserts.

With --route (wide | register | copy, repeatable) the tool times just those routes of DESIGN.md section 9q instead, and
--k may then exceed 256 on the wide and copy routes:
  wide      HNSWIndex.search_exact_wide: the same tile scan writing a distance arena, then the wide selection
  register  HNSWIndex.search_exact (k <= 256)
  copy      the one-list copy, searched with search_all at k <= 256 and with search_wide above; its build time apart
The routes named are warmed once each and then timed in turn, route after route within every repeat, so that a drift of
the machine falls on all of them alike.

Every path is warmed with one untimed call (graph upload, scratch, pinned buffers, the allowed route's mask build), then
timed --repeat times; median, minimum and maximum are reported.  Each row element runs in a child process of its own
under a time limit; the first failure stops the run.  A tree without search_exact (the parent commit) reports the two
older routes alone.

    python tools/exact_bench.py --n 200000 --d 384 --batch 1024
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


def child(a):
    import fvdb_import
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    rng = np.random.default_rng(1)
    n, d, k, B, dtype = a.n, a.d, a.k, a.batch, a.dtype
    means = rng.standard_normal((64, d)).astype(np.float32)
    x = means[rng.integers(0, 64, n)] + np.float32(0.35) * rng.standard_normal((n, d)).astype(np.float32)
    q = means[rng.integers(0, 64, B)] + np.float32(0.35) * rng.standard_normal((B, d)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64)

    def timed(fn, repeat):
        ms = []
        for i in range(repeat + 1):  # the first call is the warm-up
            ctx.device_synchronize()
            t0 = time.perf_counter()
            r = fn()
            ctx.device_synchronize()
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        return r, dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], runs=len(ms))

    out = dict(n=n, d=d, batch=B, k=k, row_dtype=dtype)
    g = fv.HNSWIndex(ctx, 4, 8, 16, row_dtype=dtype)
    g.restore(ids, x, np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64), np.roll(ids, -1), 0)
    answers = {}
    if a.route:
        return routes(a, ctx, fv, g, x, ids, q, out)
    if hasattr(g, "search_exact"):
        r, t = timed(lambda: g.search_exact(q, k), a.repeat)
        t["rows_x_queries_per_s"] = n * B / (t["ms_median"] * 1e-3)
        out["flat"] = t
        answers["flat"] = (r.ids, r.distances, r.counts)

    # the copy route, as bench.py's exact_ground_truth: a one-list index with a copy of every row, then search_all
    ctx.device_synchronize()
    t0 = time.perf_counter()
    flat = fv.DeviceIVF(ctx, d, 1, dtype=dtype)
    flat.set_centroids(np.zeros((1, d), np.float32))
    for c in range(0, n, 200_000):
        flat.add_assigned(x[c:c + 200_000], ids[c:c + 200_000], np.zeros(min(200_000, n - c), np.uint32))
    ctx.device_synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    r, t = timed(lambda: flat.search_all(q, k), a.repeat)
    out["copy"] = dict(build_ms=build_ms, copied_bytes=int(n) * d * 4, search=t)
    answers["copy"] = (r[0], r[1], r[2])
    flat.close()

    g.scan_cutoff = fv.HNSWIndex.SCAN_ALWAYS
    r, t = timed(lambda: g.search_allowed(q, k, 50, ids), a.repeat_allowed)
    out["allowed"] = t
    answers["allowed"] = (r.ids, r.distances, r.counts)

    names = list(answers)
    first = answers[names[0]]
    out["identical"] = all(np.array_equal(first[0], answers[m][0]) and np.array_equal(first[2], answers[m][2]) and
                           np.array_equal(np.ascontiguousarray(first[1]).view(np.uint32),
                                          np.ascontiguousarray(answers[m][1]).view(np.uint32)) for m in names[1:])
    out["compared"] = names
    print(json.dumps(out), flush=True)


def routes(a, ctx, fv, g, x, ids, q, out):
    """--route: the named routes of section 9q, timed in turn within every repeat"""
    n, d, k, B = a.n, a.d, a.k, a.batch
    fns, flat = {}, None
    for name in a.route:
        if name == "wide":
            fns[name] = lambda: g.search_exact_wide(q, k)
        elif name == "register":
            fns[name] = lambda: g.search_exact(q, k)
        else:
            ctx.device_synchronize()
            t0 = time.perf_counter()
            flat = fv.DeviceIVF(ctx, d, 1, dtype=a.dtype)
            flat.set_centroids(np.zeros((1, d), np.float32))
            for c in range(0, n, 200_000):
                flat.add_assigned(x[c:c + 200_000], ids[c:c + 200_000], np.zeros(min(200_000, n - c), np.uint32))
            ctx.device_synchronize()
            out["copy_build_ms"] = (time.perf_counter() - t0) * 1e3
            out["copied_bytes"] = int(n) * d * 4
            fns[name] = (lambda: flat.search_all(q, k)) if k <= 256 else (lambda: flat.search_wide(q, k, 1))
    answers, ms = {}, {name: [] for name in fns}
    for i in range(a.repeat + 1):  # the first round is the warm-up
        for name, fn in fns.items():
            ctx.device_synchronize()
            t0 = time.perf_counter()
            r = fn()
            ctx.device_synchronize()
            if i:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            answers[name] = (r.ids, r.distances, r.counts) if hasattr(r, "ids") else (r[0], r[1], r[2])
    out["routes"] = {}
    for name, v in ms.items():
        v.sort()
        out["routes"][name] = dict(ms_median=v[len(v) // 2], ms_min=v[0], ms_max=v[-1], runs=len(v),
                                   rows_x_queries_per_s=n * B / (v[len(v) // 2] * 1e-3))
    names = list(answers)
    first = answers[names[0]]
    out["identical"] = all(np.array_equal(first[0], answers[m][0]) and np.array_equal(first[2], answers[m][2]) and
                           np.array_equal(np.ascontiguousarray(first[1]).view(np.uint32),
                                          np.ascontiguousarray(answers[m][1]).view(np.uint32)) for m in names[1:])
    out["compared"] = names
    if flat is not None:
        flat.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--k", type=int, default=10, help="may exceed 256 with --route wide / copy")
    ap.add_argument("--route", action="append", choices=["wide", "register", "copy"], default=None,
                    help="time only this route (repeatable): the routes of DESIGN.md section 9q")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=9, help="timed runs per path, after one warm-up")
    ap.add_argument("--repeat-allowed", type=int, default=3, help="timed runs of the gather scan (slow), after one warm-up")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one row element may take")
    ap.add_argument("--dtype", default=None, help="(child) run this one row element in this process")
    a = ap.parse_args()
    if a.route and "register" in a.route and a.k > 256:
        ap.error("--route register takes k <= 256")
    if not a.route and a.k > 256:
        ap.error("k > 256 needs --route wide and / or --route copy")
    if a.dtype is not None:
        return child(a)
    for dtype in ("f32", "f16"):
        cmd = [sys.executable, os.path.abspath(__file__), "--dtype", dtype]
        for name in ("n", "d", "k", "batch", "repeat"):
            cmd += [f"--{name}", str(getattr(a, name))]
        cmd += ["--repeat-allowed", str(a.repeat_allowed)]
        for r in a.route or []:
            cmd += ["--route", r]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"[exact_bench] {dtype}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 124
        if rc:
            print(f"[exact_bench] {dtype}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
