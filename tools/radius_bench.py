#!/usr/bin/env python3
"""Radius search against the route that existed before it.

Two indexes, 1024 queries each (sizes are options):
  graph   an HNSWIndex of 200 K x 384 rows (installed with restore() as a ring: the scan reads rows and liveness flags,
          never links), searched by the flat scan
  lists   a DeviceIVF of 1 M x 384 rows in 1024 lists (centroids = sampled rows), --nprobe lists probed
For each, three radii chosen FROM THE DATA, read off one wide search at k = 4096 — the median over the queries of the
10th and of the 1000th nearest distance, and 1.01 x the median 4096th distance — so that the median ball holds about 10
rows, about 1000 rows and more than 4096 (the totals' median, minimum and maximum are reported beside each).
At every radius:
  radius  the radius search at max_results = 4096 (fvdb_graph_search_flat_radius_dev_slot / fvdb_ivf_search_radius_dev_slot)
  wide    the route of the parent commit: the wide search at k = 4096 (device time), then the host cut of its
          [B][4096] result at the radius (download + numpy, wall time, reported apart: it returns no total)
  count   graph only: fvdb_graph_count_within_dev_slot, the totals alone
and whether the radius route's rows equal the wide route's rows cut at the radius, and its totals the count's.

Times are device times between two events on the stream (fvdb_timer_start / fvdb_timer_stop_ms) around calls whose
inputs and outputs stay in HBM; every route is warmed once, then the routes are timed in turn within each of --repeat
rounds so that a drift of the machine falls on all alike; median, minimum and maximum are reported.  The lists' score and
select stages are timed apart by the engine's own stage events (fvdb_ctx_set_profiling; fine_scan = the score stage,
fine_merge = the select stage), in rounds of their own so that the synchronise those need does not sit in the call times.
The graph's entry points record no stage events: its stage times come from a kernel trace of this tool (--part graph
under rocprofv3 --kernel-trace --stats: flat_score_kernel against range_flat_select_kernel / flat_select_kernel).

Each part runs in a child process of its own under a time limit; the first failure stops the run.

    python tools/radius_bench.py --out profiles/radius_bench.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M = 4096


def data(n, d, B, seed):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((64, d)).astype(np.float32)
    x = np.empty((n, d), np.float32)
    for c in range(0, n, 100_000):  # in chunks: a million rows of float64 noise at once would be 3 GB
        m = min(100_000, n - c)
        x[c:c + m] = means[rng.integers(0, 64, m)] + np.float32(0.35) * rng.standard_normal((m, d)).astype(np.float32)
    q = means[rng.integers(0, 64, B)] + np.float32(0.35) * rng.standard_normal((B, d)).astype(np.float32)
    return x, q


def stats(v):
    v = sorted(v)
    return dict(ms_median=v[len(v) // 2], ms_min=v[0], ms_max=v[-1], runs=len(v))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Outputs:
    """one block of device outputs: ids (8 bytes each: the lists write u64, the graph u32 nodes), distances, counts, totals"""

    def __init__(self, ctx, B, id_dtype):
        self.ctx, self.B, self.id_dtype = ctx, B, id_dtype
        self.ids, self.dist, self.cnt, self.tot = ctx.alloc(B * M * 8), ctx.alloc(B * M * 4), ctx.alloc(B * 4), ctx.alloc(B * 4)

    def fetch(self, totals):
        c = self.ctx
        return (c.download(self.ids, (self.B, M), self.id_dtype), c.download(self.dist, (self.B, M), np.float32),
                c.download(self.cnt, (self.B,), np.uint32), c.download(self.tot, (self.B,), np.uint32) if totals else None)


def run_part(a, ctx, calls, out_r, out_w, radii_from):
    """calls: dict name -> fn(radius_dev) enqueuing one device call; returns the part's report"""
    lib, B = ctx.lib, a.batch

    def timed_rounds(fns, repeat):
        ms = {n: [] for n in fns}
        for i in range(repeat + 1):  # the first round is the warm-up
            for n, fn in fns.items():
                ctx.synchronize()
                ctx.timer_start()
                ctx.check(fn())
                t = ctx.timer_stop_ms()
                if i:
                    ms[n].append(t)
        return {n: stats(v) for n, v in ms.items()}

    # the radii, from one wide search at k = 4096 and (for the third) one look at the totals
    ctx.check(calls["wide"](None))
    ctx.synchronize()
    wi, wd, wc, _ = out_w.fetch(False)
    assert np.all(wc == M), "every query must see at least 4096 rows"
    r10, r1000 = np.median(wd[:, 9]), np.median(wd[:, 999])
    report = dict(radii={})
    for name, r in (("ball_10", r10), ("ball_1000", r1000), ("ball_above_4096", radii_from(wd))):
        radius = np.full(B, r, np.float32)
        r_dev = ctx.upload(radius)
        fns = {n: (lambda f=f: f(r_dev)) for n, f in calls.items()}
        t = timed_rounds(fns, a.repeat)
        ctx.check(calls["radius"](r_dev))
        ctx.synchronize()
        ri, rd, rc, rt = out_r.fetch(True)
        # the parent's route ends on the host: download the [B][4096] block, cut it at the radius
        ctx.check(calls["wide"](r_dev))
        ctx.synchronize()
        t0 = time.perf_counter()
        wi, wd2, wc, _ = out_w.fetch(False)
        keep = bits(wd2) <= bits(radius)[:, None]
        keep &= np.arange(M)[None, :] < wc[:, None]
        cut_counts = keep.sum(1)
        host_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(cut_counts, rc))
        for b in range(B):
            c = int(rc[b])
            same = same and np.array_equal(ri[b, :c], wi[b, :c]) and np.array_equal(bits(rd[b, :c]), bits(wd2[b, :c]))
        entry = dict(radius=float(r), median_total=float(np.median(rt)), min_total=int(rt.min()), max_total=int(rt.max()),
                     queries_above_cap=int((rt > M).sum()), device=t, wide_host_cut_ms=host_ms,
                     rows_equal_wide_cut=same)
        if "count" in calls:
            ctx.check(calls["count"](r_dev))
            ctx.synchronize()
            entry["count_equals_totals"] = bool(np.array_equal(ctx.download(out_w.tot, (B,), np.uint32), rt))
        report["radii"][name] = entry
        ctx.free(r_dev)
    return report


def part_graph(a):
    import fvdb_import
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    lib, n, d, B = ctx.lib, a.n_graph, a.d, a.batch
    x, q = data(n, d, B, 1)
    ids = np.arange(n, dtype=np.uint64)
    g = fv.HNSWIndex(ctx, 4, 8, 16)
    g.restore(ids, x, np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64), np.roll(ids, -1), 0)
    gh, q_dev = g._graph(), ctx.upload(q)
    out_r, out_w = Outputs(ctx, B, np.uint32), Outputs(ctx, B, np.uint32)
    calls = {
        "radius": lambda r: lib.fvdb_graph_search_flat_radius_dev_slot(gh, None, 0, None, q_dev, B, r, M, out_r.ids, out_r.dist,
                                                                       out_r.cnt, out_r.tot),
        "wide": lambda r: lib.fvdb_graph_search_flat_wide_dev_slot(gh, None, 0, None, q_dev, B, M, out_w.ids, out_w.dist, out_w.cnt),
        "count": lambda r: lib.fvdb_graph_count_within_dev_slot(gh, None, 0, None, q_dev, B, r, out_w.tot),
    }
    # a ball above the cap: the median 4096th distance and a little more
    report = run_part(a, ctx, calls, out_r, out_w, lambda wd: np.float32(np.median(wd[:, M - 1]) * 1.01))
    report.update(part="graph", n=n, d=d, batch=B, max_results=M)
    print(json.dumps(report), flush=True)


def part_lists(a):
    import fvdb_import
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    lib, n, d, B, nlist, nprobe = ctx.lib, a.n_lists, a.d, a.batch, a.nlist, a.nprobe
    x, q = data(n, d, B, 2)
    ix = fv.DeviceIVF(ctx, d, nlist)
    ix.set_centroids(x[np.random.default_rng(3).choice(n, nlist, replace=False)])
    for c in range(0, n, 200_000):
        ix.add(x[c:c + 200_000], np.arange(c, min(n, c + 200_000), dtype=np.uint64))
    q_dev = ctx.upload(q)
    out_r, out_w = Outputs(ctx, B, np.uint64), Outputs(ctx, B, np.uint64)
    calls = {
        "radius": lambda r: lib.fvdb_ivf_search_radius_dev_slot(ix.h, None, 0, None, q_dev, B, r, M, nprobe, out_r.ids, out_r.dist,
                                                                out_r.cnt, out_r.tot),
        "wide": lambda r: lib.fvdb_ivf_search_wide_dev_slot(ix.h, None, 0, None, q_dev, B, M, nprobe, out_w.ids, out_w.dist,
                                                            out_w.cnt, None),
    }
    report = run_part(a, ctx, calls, out_r, out_w, lambda wd: np.float32(np.median(wd[:, M - 1]) * 1.01))
    # the stages, by the engine's stage events, in rounds of their own
    ctx.set_profiling(True)
    for name, entry in report["radii"].items():
        r_dev = ctx.upload(np.full(B, entry["radius"], np.float32))
        stages = {}
        for route in ("radius", "wide"):
            score, select = [], []
            for i in range(a.repeat + 1):
                ctx.check(calls[route](r_dev))
                ctx.synchronize()
                _, st = ix.stage_times()
                if i:
                    score.append(st["fine_scan"])
                    select.append(st["fine_merge"])
            stages[route] = dict(score_stage=stats(score), select_stage=stats(select))
        entry["stages"] = stages
        ctx.free(r_dev)
    ctx.set_profiling(False)
    report.update(part="lists", n=n, d=d, nlist=nlist, nprobe=nprobe, batch=B, max_results=M)
    print(json.dumps(report), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-graph", type=int, default=200_000)
    ap.add_argument("--n-lists", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=9, help="timed rounds, after one warm-up round")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one part may take")
    ap.add_argument("--out", default=None, help="write the two reports here as one JSON document")
    ap.add_argument("--part", default=None, choices=["graph", "lists"], help="run this one part in this process")
    a = ap.parse_args()
    if a.part:
        return (part_graph if a.part == "graph" else part_lists)(a)
    reports = []
    for part in ("graph", "lists"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part]
        for name in ("n_graph", "n_lists", "nlist", "nprobe", "d", "batch", "repeat"):
            cmd += ["--" + name.replace("_", "-"), str(getattr(a, name))]
        try:
            p = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"[radius_bench] {part}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        if p.returncode:
            print(f"[radius_bench] {part}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode
        reports.append(json.loads(p.stdout.strip().splitlines()[-1]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/radius_bench.py", parts=reports), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
