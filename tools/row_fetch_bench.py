#!/usr/bin/env python3
"""Rows by id on the device against what they replace.  One JSON line, also written to --out.

  (1) fetch      the hits of --queries searches (k = 10) read back from an --n x --d IVF index: fvdb_ivf_get_rows
                 (one gather; also its device form alone, fvdb_ivf_get_rows_dev) against the only way there was,
                 fvdb_ivf_list_export of every list a hit sits in
  (2) migration  jobs of --migrate rows each from the graph's row store into the lists: resident
                 (HybridIndex.set_resident_migration(True), the default) against the host path of the same build
                 (False).  One index holds 2 * (1 + --repeats) groups of rows, each group due at its own threshold;
                 the groups alternate between the two paths, so both run against the same lists as they grow.

Seeded.  Every variant is warmed up once, the variants alternate in one process, the figure is the median of --repeats.
Times are HIP events on the index's stream (fvdb_timer_start / fvdb_timer_stop_ms) around the whole call, and the wall
clock around the same call (every call ends in a stream synchronise); fvdb_ivf_get_rows runs on a leased stream of its
own, so only its wall clock is given.

    python tools/row_fetch_bench.py --n 1000000 --d 384 --migrate 10000 100000 --out profiles/row_fetch_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fvdb_import  # noqa: E402

DAY = 86400.0
u32p = C.POINTER(C.c_uint32)


def data(n, d, seed):
    rng = np.random.default_rng(seed)
    means = rng.standard_normal((256, d)).astype(np.float32)
    out = np.empty((n, d), np.float32)
    for o in range(0, n, 100_000):
        m = min(100_000, n - o)
        out[o:o + m] = means[rng.integers(0, 256, m)] + np.float32(0.35) * rng.standard_normal((m, d)).astype(np.float32)
    return out


def timed(ctx, fn):
    """(event ms on the context's stream, wall ms) of fn(), which ends synchronised."""
    ms = C.c_float(0)
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.check(ctx.lib.fvdb_timer_start(ctx.h))
    fn()
    ctx.check(ctx.lib.fvdb_timer_stop_ms(ctx.h, C.byref(ms)))
    return float(ms.value), (time.perf_counter() - t0) * 1e3


def med(v):
    return float(np.median(np.asarray(v, np.float64)))


def fetch_leg(fv, ctx, a):
    x = data(a.n, a.d, 1)
    rng = np.random.default_rng(2)
    ix = fv.DeviceIVF(ctx, a.d, a.nlist)
    ix.set_centroids(x[rng.choice(a.n, a.nlist, replace=False)].copy())
    ix.reserve(a.n)
    cl, pos = np.empty(a.n, np.uint32), np.empty(a.n, np.uint32)
    for o in range(0, a.n, 100_000):
        cl[o:o + 100_000], pos[o:o + 100_000] = ix.add(x[o:o + 100_000], np.arange(o, min(o + 100_000, a.n), dtype=np.uint64))
    q = x[rng.choice(a.n, a.queries, replace=False)] + np.float32(0.05) * rng.standard_normal((a.queries, a.d)).astype(np.float32)
    ids, _, cnt = ix.search(q, 10, a.nprobe)
    hit = np.concatenate([ids[b, :cnt[b]] for b in range(a.queries)]).astype(np.int64)
    hc, hp = np.ascontiguousarray(cl[hit]), np.ascontiguousarray(pos[hit])
    lists = np.unique(hc)
    out_host = np.empty((hit.size, a.d), np.float32)
    dev = ctx.alloc(hit.size * a.d * 4)

    def get_rows():
        ix.get_rows(hc, hp, out=out_host)

    def get_rows_dev():
        ctx.check(ctx.lib.fvdb_ivf_get_rows_dev(ix.h, None, hc.ctypes.data_as(u32p), hp.ctypes.data_as(u32p), hit.size, dev))

    exported = {}

    def export():
        for c in lists:
            exported[int(c)] = ix.list_export(int(c))[0]

    variants = dict(get_rows=get_rows, get_rows_dev=get_rows_dev, list_export=export)
    t = {k: [] for k in variants}
    for rep in range(a.repeats + 1):  # the first round is the warm-up
        for name, fn in variants.items():
            r = timed(ctx, fn)
            if rep:
                t[name].append(r)
    assert np.array_equal(out_host.view(np.uint32), x[hit].view(np.uint32))
    assert np.array_equal(ctx.download(dev, (hit.size, a.d), np.float32).view(np.uint32), x[hit].view(np.uint32))
    got = np.stack([exported[int(c)][p] for c, p in zip(hc, hp)])
    assert np.array_equal(got.view(np.uint32), x[hit].view(np.uint32))
    ctx.free(dev)
    sizes = ix.list_sizes()
    res = dict(rows=int(hit.size), lists_exported=int(lists.size), rows_exported=int(sizes[lists].sum()),
               bytes_fetched=int(hit.size) * a.d * 4, bytes_exported=int(sizes[lists].sum()) * a.d * 4,
               get_rows_wall_ms=med([w for _, w in t["get_rows"]]),
               get_rows_dev_event_ms=med([e for e, _ in t["get_rows_dev"]]),
               get_rows_dev_wall_ms=med([w for _, w in t["get_rows_dev"]]),
               list_export_event_ms=med([e for e, _ in t["list_export"]]),
               list_export_wall_ms=med([w for _, w in t["list_export"]]))
    ix.close()
    return res


def migration_leg(fv, ctx, a, rows):
    groups = 2 * (1 + a.repeats)
    n = groups * rows
    x = data(n, a.d, 3 + rows)
    now = 1000 * DAY
    # group g is (groups - g) * 0.1 days old: migrate_with_threshold((groups - g) * 0.1 - 0.05 days) takes groups 0..g
    ages = np.repeat((groups - np.arange(groups)) * 0.1 * DAY, rows)
    h = fv.HybridIndex(ctx, n_clusters=a.nlist, n_probe=a.nprobe, max_connections=a.M, max_connections_layer_0=2 * a.M,
                       ef_construction=a.efc, auto_migrate=False)
    h.set_ivf_centroids(x[np.random.default_rng(4).choice(n, a.nlist, replace=False)].copy())
    t0 = time.perf_counter()
    h.bulk_insert(np.arange(n, dtype=np.uint64), x, now - ages, now)
    build_s = time.perf_counter() - t0
    jobs = {True: [], False: []}
    for g in range(groups):
        resident = g % 2 == 0
        h.set_resident_migration(resident)
        moved = []
        ev, wall = timed(ctx, lambda: moved.append(h.migrate_with_threshold((groups - g) * 0.1 * DAY - 0.05 * DAY, now)))
        assert moved[0] == rows, (g, moved)
        info = h.migration_info()
        assert info["resident"] == resident
        if g >= 2:  # the first job of each path is its warm-up
            jobs[resident].append(dict(event_ms=ev, wall_ms=wall, host_bytes=info["host_bytes"], ms_gather=info["ms_gather"],
                                       ms_assign=info["ms_assign"], ms_move=info["ms_move"]))
    assert h.historical_count() == n

    def summary(js, stages):
        s = dict(event_ms=med([j["event_ms"] for j in js]), wall_ms=med([j["wall_ms"] for j in js]),
                 host_bytes=int(js[0]["host_bytes"]))
        if stages:
            s.update({k: med([j[k] for j in js]) for k in ("ms_gather", "ms_assign", "ms_move")})
        return s

    return dict(rows=rows, d=a.d, graph_nodes=n, graph_build_s=build_s, resident=summary(jobs[True], True),
                host=summary(jobs[False], False), host_bytes_bound_32n=32 * rows, host_path_bytes_2nd4=2 * rows * a.d * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--migrate", type=int, nargs="*", default=[10_000, 100_000], help="rows per migration job")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--M", type=int, default=8)
    ap.add_argument("--efc", type=int, default=40)
    ap.add_argument("--skip-fetch", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    out = dict(n=a.n, d=a.d, nlist=a.nlist, nprobe=a.nprobe, queries=a.queries, repeats=a.repeats, M=a.M, ef_construction=a.efc)
    if not a.skip_fetch:
        out["fetch"] = fetch_leg(fv, ctx, a)
    out["migration"] = [migration_leg(fv, ctx, a, rows) for rows in a.migrate]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
