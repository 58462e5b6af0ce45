#!/usr/bin/env python3
"""Measures cosine k-NN search on the device, in one process: CosineIndex.search in mode "filter"
and in mode "exact", and the only route the engine had before — fvdb_cosine_similarities (a host-array entry point: rows
up, the B x n matrix down) into fvdb_top_k_indices_dev (the matrix up again).  The three are alternated over two passes,
on normal rows at d = 384 and d = 1024.  The old route and mode "exact" run on the first --old-queries queries of the
batch (the matrix of the whole batch is 4 GiB), the filter on all of it; every rate is queries per second by a host clock
around calls that end in a synchronise.  Also recorded: exact_pairs / (B n), fallback_queries, and that the three agree.
Prints one JSON object and, with --out, writes it to a file.

    python tools/cosine_bench.py --out profiles/cosine_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import fvdb_import  # noqa: E402


def old_route(fv, ctx, q, x, k):
    scores = fv.engine.batch_cosine_similarity(ctx, q, x)
    p = ctx.upload(scores)
    oi, oc = ctx.alloc(q.shape[0] * k * 8), ctx.alloc(q.shape[0] * 4)
    ctx.check(ctx.lib.fvdb_top_k_indices_dev(ctx.h, p, q.shape[0], x.shape[0], k, 0, oi, oc))
    idx = ctx.download(oi, (q.shape[0], k), np.uint64)
    for b in (p, oi, oc):
        ctx.free(b)
    return idx


def qps(fn, nq):
    t = time.perf_counter()
    fn()
    return round(nq / (time.perf_counter() - t), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[384, 1024])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--old-queries", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()

    fv = fvdb_import.load()
    ctx = fv.Context(0)
    N, B, k, Bo = a.n, a.batch, a.k, min(a.old_queries, a.batch)
    res = {"n": N, "batch": B, "k": k, "old_route_and_exact_queries": Bo, "reps": a.reps, "shapes": {},
           "timing": "host clock around host-form calls, which synchronise; uploads and downloads inside; no kernel trace"}
    for d in a.dims:
        rng = np.random.default_rng(d)
        x = rng.standard_normal((N, d), np.float32)
        q = rng.standard_normal((B, d), np.float32)
        ids = np.arange(N, dtype=np.uint64)
        ix = fv.CosineIndex(ctx, d)
        t = time.perf_counter()
        for c in range(0, N, 100_000):
            ix.add(ids[c:c + 100_000], x[c:c + 100_000])
        out = {"add_rows_per_s": round(N / (time.perf_counter() - t)), "bytes_per_row": ix.bytes() / N}
        ix.search(q, k)  # warm-up: scratch allocated
        runs = {"filter": [], "exact": [], "cosine_similarities_then_top_k_dev": []}
        for _ in range(2):  # alternated, so a drift of the shared host shows in all of them
            runs["filter"].append(qps(lambda: [ix.search(q, k) for _ in range(a.reps)], a.reps * B))
            runs["exact"].append(qps(lambda: ix.search(q[:Bo], k, mode="exact"), Bo))
            runs["cosine_similarities_then_top_k_dev"].append(qps(lambda: old_route(fv, ctx, q[:Bo], x, k), Bo))
        out["qps"] = runs
        f = ix.search(q, k)
        info = ix.info()
        out["exact_pairs_share"] = info["exact_pairs"] / (B * N)
        out["fallback_queries"] = info["fallback_queries"]
        out["info"] = info
        e = ix.search(q[:Bo], k, mode="exact")
        out["filter_equals_exact"] = bool(np.array_equal(f.ids[:Bo], e.ids) and np.array_equal(f.similarities[:Bo].view(np.uint32), e.similarities.view(np.uint32)))
        out["filter_equals_old_route"] = bool(np.array_equal(f.ids[:Bo], old_route(fv, ctx, q[:Bo], x, k)))
        res["shapes"][f"d{d}"] = out
        ix.close()
        print(json.dumps({f"d{d}": out}), flush=True)

    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
