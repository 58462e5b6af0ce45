#!/usr/bin/env python3
"""Measures binary quantization on the device on bench.py's mixture, in one run: the exact scan
(HNSWIndex.search_exact over the same rows), the symmetric SQ8 search, the Hamming search with the centre at zero and at
the data mean, and the refined search at fetch_k 64 and 256 over f32 and fp16 rows with both centres — q/s, recall@k
against search_exact, bytes per row, build rows/s, pairs/s of the Hamming scan.  Every rate is a host clock around calls
that end in a synchronise (the host forms do).  Prints one JSON object and, with --out, writes it to a file.

    python tools/bq_bench.py --n-vectors 1000000 --out profiles/bq_bench.json
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
    mean = x.mean(axis=0, dtype=np.float64).astype(np.float32)
    res = {"n": N, "d": d, "batch": a.batch, "k": k, "reps": a.reps,
           "timing": "host clock around host-form calls, which synchronise; queries uploaded and results downloaded inside"}

    def build(ix):
        t = time.perf_counter()
        for c in range(0, N, 100_000):
            ix.add(ids[c:c + 100_000], x[c:c + 100_000])
        return time.perf_counter() - t

    bq = fv.BQIndex(ctx, d, center=mean)
    res["build_rows_per_s"] = round(N / build(bq))  # host check + upload + encode + append
    res["info"] = bq.info()
    kept = {(c, r): fv.BQIndex(ctx, d, refine_rows=r, center=cv) for c, cv in (("zero", None), ("mean", mean)) for r in ("f32", "f16")}
    for ix in kept.values():
        build(ix)
    sq = fv.SQ8Index(ctx, d)
    build(sq)
    res["bytes_per_row"] = {"bq_index": bq.bytes() / N, "bq_plus_f32_refine": kept["mean", "f32"].bytes() / N,
                            "bq_plus_f16_refine": kept["mean", "f16"].bytes() / N, "sq8_index": sq.bytes() / N, "f32_rows": 4 * d}

    # the yardstick of recall: the exact scan over the same rows (a graph with the fewest links: only its row store is read)
    g = fv.HNSWIndex(ctx, max_connections=2, max_connections_layer_0=2, ef_construction=8)
    g.bulk_build(ids, x, levels=np.zeros(N, np.int64))
    truth = [g.search_exact(q, k) for q in queries]

    runs = {"search_exact": lambda q: g.search_exact(q, k), "sq8_symmetric": lambda q: sq.search(q, k),
            "bq_hamming_mean": lambda q: bq.search(q, k), "bq_hamming_zero": lambda q: kept["zero", "f32"].search(q, k)}
    for (c, r), ix in kept.items():
        for fk in (64, 256):
            runs[f"bq_{c}_{r}_fetch{fk}"] = lambda q, ix=ix, fk=fk: ix.search(q, k, fetch_k=fk)
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
    bq.search(queries[0], k)
    host_ms = (time.perf_counter() - t) * 1e3
    dev_ms = ctx.timer_stop_ms()
    res["bq_one_batch_ms"] = {"device_events": round(dev_ms, 3), "host_clock": round(host_ms, 3)}
    res["bq_pairs_per_s_device_events"] = round(bq.info()["last_pairs"] / (dev_ms * 1e-3))
    res["last_slices"] = bq.info()["last_slices"]

    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
