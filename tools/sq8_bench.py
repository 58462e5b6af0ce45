#!/usr/bin/env python3
"""Measures u8 scalar quantization on the device on bench.py's mixture, in one run: the parent's
exact scan (HNSWIndex.search_exact over the same rows), PQIndex ADC at m = 48, the symmetric SQ8 search, and the refined
SQ8 search at fetch_k 64 and 256 over the decoded rows and over stored f32 rows — q/s, recall@k against search_exact,
bytes per row, encode rows/s.  Every rate is a host clock around calls that end in a synchronise (the host forms do).
Prints one JSON object and, with --out, writes it to a file.

    python tools/sq8_bench.py --n-vectors 1000000 --out profiles/sq8_bench.json
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
from bench import Generator, recall_at_k  # noqa: E402
from pq_bench import rate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--subspaces", type=int, default=48)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()

    fv = fvdb_import.load()
    ctx = fv.Context(0)
    N, d, k = a.n, a.dim, a.k
    gen = Generator(d=d)
    x = gen.chunks(N, 100_000)
    ids = np.arange(N, dtype=np.uint64)
    queries = [gen.rows(a.batch, stream=10_000 + i) for i in range(a.batches)]
    res = {"n": N, "d": d, "batch": a.batch, "k": k, "reps": a.reps, "pq_m": a.subspaces,
           "timing": "host clock around host-form calls, which synchronise; queries uploaded and results downloaded inside"}

    def build(ix):
        t = time.perf_counter()
        for c in range(0, N, 100_000):
            ix.add(ids[c:c + 100_000], x[c:c + 100_000])
        return time.perf_counter() - t

    sq = fv.SQ8Index(ctx, d)
    res["encode_rows_per_s"] = round(N / build(sq))  # host check + upload + encode + append
    res["info"] = sq.info()
    sqr = fv.SQ8Index(ctx, d, refine_rows="f32")
    build(sqr)
    pq = fv.ProductQuantizer(ctx, d, a.subspaces, 256)
    pq.train(x[np.random.default_rng(0).choice(N, min(N, 50_000), replace=False)], 10, seed=1)
    pqi = fv.PQIndex(ctx, pq)
    build(pqi)
    res["bytes_per_row"] = {"sq8_index": sq.bytes() / N, "sq8_plus_f32_refine": sqr.bytes() / N, "pq_index": pqi.bytes() / N, "f32_rows": 4 * d}

    # the yardstick: the parent's exact scan over the same rows (a graph with the fewest links: only its row store is read)
    g = fv.HNSWIndex(ctx, max_connections=2, max_connections_layer_0=2, ef_construction=8)
    g.bulk_build(ids, x, levels=np.zeros(N, np.int64))
    truth = [g.search_exact(q, k) for q in queries]

    runs = {"search_exact": lambda q: g.search_exact(q, k), "pq_adc": lambda q: pqi.search(q, k), "sq8_symmetric": lambda q: sq.search(q, k)}
    for fk in (64, 256):
        runs[f"sq8_decoded_fetch{fk}"] = lambda q, fk=fk: sq.search(q, k, fetch_k=fk)
        runs[f"sq8_f32_fetch{fk}"] = lambda q, fk=fk: sqr.search(q, k, fetch_k=fk, refine="f32")
    # two alternating passes, so a drift of the shared host shows in all of them
    res["qps"] = {n: [] for n in runs}
    for _ in range(2):
        for n, fn in runs.items():
            res["qps"][n].append(round(rate(fn, queries, a.reps), 1))
    res["recall"] = {n: round(float(np.mean([recall_at_k(r.ids, r.counts, t.ids, k) for r, t in ((fn(q), t) for q, t in zip(queries, truth))])), 4)
                     for n, fn in runs.items() if n != "search_exact"}
    # the same call under both clocks: device events on the context's stream against the host clock
    ctx.timer_start()
    t = time.perf_counter()
    sq.search(queries[0], k)
    host_ms = (time.perf_counter() - t) * 1e3
    res["sq8_one_batch_ms"] = {"device_events": round(ctx.timer_stop_ms(), 3), "host_clock": round(host_ms, 3)}

    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
