#!/usr/bin/env python3
"""Diverse search against the route a caller had before it.

Two indexes, 1024 queries each, k = 10, fetch_k in {32, 64, 256} (sizes are options):
  lists   an IVFIndex of 1 M x 384 rows in 1024 lists (centroids = sampled rows), --nprobe lists probed
  graph   an HNSWIndex of 200 K x 384 rows built by its own device insert, walked with ef = max(64, fetch_k)
At every fetch_k three routes:
  a  search(fetch_k) alone: what every route starts with
  b  search_diverse(k, fetch_k, lam = 0.5, distinct): the search, the gather in HBM, the selection kernel
  c  the route of the parent commit: search(fetch_k), the rows of every candidate brought to the host (get_vectors in
     one call for the lists; for the graph, whose Python class returns one row per call, the caller's own copy of the
     rows, which costs the index nothing and favours this route), then a numpy selection vectorised over the batch.
     It computes distances with numpy's own summation order, so it does NOT give the fold's bits; picks that differ
     from route b's are counted, not hidden.
and the selection kernel alone (fvdb_mmr_select_dev on a staged block, device time between two events), whose share of
route b is reported.

Routes a to c are blocking calls with host pointers, so they are timed with the host clock (perf_counter around the
call); one warm-up round, then the routes in turn within each of --repeat rounds so that a drift of the machine falls
on all alike; median, minimum and maximum are reported.

Each part runs in a child process of its own under a time limit; the first failure stops the run.

    python tools/diverse_bench.py --out profiles/diverse_bench.json
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
K, LAM = 10, 0.5


def data(n, d, B, seed):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((64, d)).astype(np.float32)
    x = np.empty((n, d), np.float32)
    for c in range(0, n, 100_000):
        m = min(100_000, n - c)
        x[c:c + m] = means[rng.integers(0, 64, m)] + np.float32(0.35) * rng.standard_normal((m, d)).astype(np.float32)
    q = means[rng.integers(0, 64, B)] + np.float32(0.35) * rng.standard_normal((B, d)).astype(np.float32)
    return x, q


def stats(v):
    v = sorted(v)
    return dict(ms_median=v[len(v) // 2], ms_min=v[0], ms_max=v[-1], runs=len(v))


def numpy_mmr(ids, dq, counts, rows, k, lam):
    """route c's selection, vectorised over the batch: ranks [B, k] (-1 = none).  distinct: later copies of an id closed."""
    B, F = ids.shape
    a, b = np.float32(lam), np.float32(1) - np.float32(lam)
    open_ = np.arange(F)[None, :] < counts[:, None]
    order = np.argsort(ids, axis=1, kind="stable")
    srt = np.take_along_axis(ids, order, 1)
    dup_sorted = np.concatenate([np.zeros((B, 1), bool), srt[:, 1:] == srt[:, :-1]], 1)
    dup = np.zeros_like(dup_sorted)
    np.put_along_axis(dup, order, dup_sorted, 1)
    open_ &= ~dup
    m = np.full((B, F), np.inf, np.float32)
    ranks = np.full((B, k), -1, np.int64)
    rows_i = np.arange(B)
    pick = np.argmax(open_, axis=1)
    for r in range(k):
        has = open_[rows_i, pick]
        ranks[has, r] = pick[has]
        open_[rows_i, pick] = False
        if r + 1 == k:
            break
        t = np.linalg.norm(rows - rows[rows_i, pick][:, None, :], axis=2)
        m = np.minimum(m, t)
        gain = np.where(open_, b * m - a * dq, -np.inf)
        pick = np.argmax(gain, axis=1)
    return ranks


def run_part(a, fv, ctx, search, diverse, rows_of, what):
    lib, report = ctx.lib, dict(fetch_k={})
    for F in a.fetch_k:
        def route_c():
            cand = search(F)
            rows = rows_of(cand)
            return cand, numpy_mmr(cand.ids, cand.distances, cand.counts, rows, K, LAM)
        routes = {"a_search": lambda: search(F), "b_search_diverse": lambda: diverse(F), "c_host_route": route_c}
        ms = {n: [] for n in routes}
        for i in range(a.repeat + 1):  # the first round is the warm-up
            for n, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                if i:
                    ms[n].append((time.perf_counter() - t0) * 1e3)
        res, ranks = diverse(F)
        cand, c_ranks = route_c()
        rows = rows_of(cand)
        B, d = rows.shape[0], rows.shape[2]
        dpad = (d + 3) // 4 * 4
        staged = np.zeros((B, F, dpad), np.float32)
        staged[:, :, :d] = rows
        bufs = [ctx.upload(staged), ctx.upload(cand.ids), ctx.upload(cand.distances), ctx.upload(cand.counts)]
        outs = [ctx.alloc(B * K * 8), ctx.alloc(B * K * 4), ctx.alloc(B * K * 4), ctx.alloc(B * 4)]
        kern = []
        for i in range(a.repeat + 1):
            ctx.synchronize()
            ctx.timer_start()
            ctx.check(lib.fvdb_mmr_select_dev(ctx.h, bufs[0], dpad, bufs[1], bufs[2], bufs[3], B, F, K, LAM, 1, *outs))
            t = ctx.timer_stop_ms()
            if i:
                kern.append(t)
        k_ranks = ctx.download(outs[2], (B, K), np.uint32)
        for p in bufs + outs:
            ctx.free(p)
        entry = {n: stats(v) for n, v in ms.items()}
        entry["selection_kernel_device"] = stats(kern)
        entry["selection_kernel_share_of_b"] = entry["selection_kernel_device"]["ms_median"] / entry["b_search_diverse"]["ms_median"]
        entry["staging_block_mb"] = B * F * dpad * 4 / 1e6
        entry["median_candidates"] = float(np.median(cand.counts))
        entry["kernel_alone_equals_search_diverse"] = bool(np.array_equal(k_ranks, ranks))
        entry["queries_where_numpy_picks_differ"] = int((np.where(ranks == 0xFFFFFFFF, -1, ranks.astype(np.int64)) != c_ranks).any(1).sum())
        report["fetch_k"][str(F)] = entry
    report.update(part=what, k=K, lam=LAM, distinct=True, batch=a.batch, d=a.d)
    print(json.dumps(report), flush=True)


def part_lists(a):
    import fvdb_import
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    n, d, B = a.n_lists, a.d, a.batch
    x, q = data(n, d, B, 2)
    ix = fv.IVFIndex(ctx, n_clusters=a.nlist, n_probe=a.nprobe)
    ix.set_trained(x[np.random.default_rng(3).choice(n, a.nlist, replace=False)])
    for c in range(0, n, 200_000):
        ix.batch_insert(np.arange(c, min(n, c + 200_000), dtype=np.uint64), x[c:c + 200_000])

    def rows_of(cand):
        rows, found = ix.get_vectors(np.where(cand.ids == np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0), cand.ids).reshape(-1))
        return rows.reshape(B, cand.ids.shape[1], d)

    run_part(a, fv, ctx, lambda F: ix.search(q, F, a.nprobe), lambda F: ix.search_diverse(q, K, F, LAM, True, n_probe=a.nprobe),
             rows_of, f"lists n={n} nlist={a.nlist} nprobe={a.nprobe}")


def part_graph(a):
    import fvdb_import
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    n, d, B = a.n_graph, a.d, a.batch
    x, q = data(n, d, B, 1)
    g = fv.HNSWIndex(ctx, 8, 16, 40, seed=1)
    t0 = time.perf_counter()
    ids = np.arange(n, dtype=np.uint64)
    for c in range(0, n, 50_000):
        g.batch_insert(ids[c:c + 50_000], x[c:c + 50_000])
    build_s = time.perf_counter() - t0
    ef = lambda F: max(64, F)  # noqa: E731

    def rows_of(cand):
        safe = np.where(cand.ids == np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0), cand.ids)
        return x[safe.astype(np.int64)]  # the caller's own copy: ids are row numbers here

    run_part(a, fv, ctx, lambda F: g.search(q, F, ef(F)), lambda F: g.search_diverse(q, K, F, ef(F), LAM, True), rows_of,
             f"graph n={n} M=8/16 ef=max(64, fetch_k) build_s={build_s:.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-graph", type=int, default=200_000)
    ap.add_argument("--n-lists", type=int, default=1_000_000)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--fetch-k", type=int, nargs="+", default=[32, 64, 256])
    ap.add_argument("--repeat", type=int, default=9, help="timed rounds, after one warm-up round")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one part may take")
    ap.add_argument("--out", default=None, help="write the reports here as one JSON document")
    ap.add_argument("--part", default=None, choices=["graph", "lists"], help="run this one part in this process")
    a = ap.parse_args()
    if a.part:
        return (part_graph if a.part == "graph" else part_lists)(a)
    reports = []
    for part in ("lists", "graph"):
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--fetch-k"] + [str(f) for f in a.fetch_k]
        for name in ("n_graph", "n_lists", "nlist", "nprobe", "d", "batch", "repeat"):
            cmd += ["--" + name.replace("_", "-"), str(getattr(a, name))]
        try:
            p = subprocess.run(cmd, timeout=a.step_timeout, stdout=subprocess.PIPE, text=True)
        except subprocess.TimeoutExpired:
            print(f"[diverse_bench] {part}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            break
        sys.stdout.write(p.stdout)
        if p.returncode:
            print(f"[diverse_bench] {part}: exit status {p.returncode}; stopping", file=sys.stderr)
            break
        reports.append(json.loads(p.stdout.strip().splitlines()[-1]))
    if a.out and reports:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/diverse_bench.py", parts=reports), f, indent=1)
            f.write("\n")
    return 0 if len(reports) == 2 else 1


if __name__ == "__main__":
    sys.exit(main() or 0)
