#!/usr/bin/env python3
"""Measures product quantization on the device on bench.py's mixture: train seconds, encode rows/s,
ADC search q/s with the plain and the padded table layout, refined search q/s at fetch_k 64 and 256 over f32 and fp16
rows, recall@k of each against HNSWIndex.search_exact over the same rows, that search's own q/s in the same run, and the
bytes per row of each form.  Every rate is a host clock around calls that end in a synchronise (the host forms do).
Prints one JSON object and, with --out, writes it to a file.

    python tools/pq_bench.py --n-vectors 1000000 --out profiles/pq_bench.json
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


def rate(fn, queries, reps):
    """queries per second of fn(batch) over `reps` passes of the batches, after one warm-up pass"""
    for q in queries:
        fn(q)
    t = time.perf_counter()
    for _ in range(reps):
        for q in queries:
            fn(q)
    return reps * sum(len(q) for q in queries) / (time.perf_counter() - t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--subspaces", type=int, default=48)
    ap.add_argument("--centroids", type=int, default=256)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--train-rows", type=int, default=50_000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()

    fv = fvdb_import.load()
    ctx = fv.Context(0)
    N, d, k = a.n, a.dim, a.k
    gen = Generator(d=d)
    x = gen.chunks(N, 100_000)
    ids = np.arange(N, dtype=np.uint64)
    queries = [gen.rows(a.batch, stream=10_000 + i) for i in range(a.batches)]
    res = {"n": N, "d": d, "m": a.subspaces, "ksub": a.centroids, "batch": a.batch, "k": k, "reps": a.reps,
           "timing": "host clock around host-form calls, which synchronise; queries uploaded and results downloaded inside"}

    def quantizer(pad):
        os.environ["FVDB_PQ_TABLE_PAD"] = "1" if pad else "0"  # read when the quantizer is created
        return fv.ProductQuantizer(ctx, d, a.subspaces, a.centroids)

    pq = quantizer(False)
    train = x[np.random.default_rng(0).choice(N, min(N, a.train_rows), replace=False)]
    t = time.perf_counter()
    pq.train(train, a.iterations, seed=1)
    res["train_s"] = round(time.perf_counter() - t, 3)
    res["train_rows"], res["train_iterations"] = len(train), a.iterations
    res["info"] = pq.info()

    def build(q, refine):
        ix = fv.PQIndex(ctx, q, refine_rows=refine)
        t = time.perf_counter()
        for c in range(0, N, 100_000):
            ix.add(ids[c:c + 100_000], x[c:c + 100_000])
        return ix, time.perf_counter() - t

    ix, sec = build(pq, None)
    res["encode_rows_per_s"] = round(N / sec)  # upload + encode + append
    res["bytes_per_row"] = {"codes_index": ix.bytes() / N, "f32_rows": 4 * d, "f16_rows": 2 * d}

    # the yardstick: the parent's exact scan over the same rows (a graph with the fewest links: only its row store is read)
    g = fv.HNSWIndex(ctx, max_connections=2, max_connections_layer_0=2, ef_construction=8)
    t = time.perf_counter()
    g.bulk_build(ids, x, levels=np.zeros(N, np.int64))
    res["exact_graph_build_s"] = round(time.perf_counter() - t, 2)
    truth = [g.search_exact(q, k) for q in queries]

    def recall(fn):
        return round(float(np.mean([recall_at_k(r.ids, r.counts, t.ids, k) for r, t in ((fn(q), t) for q, t in zip(queries, truth))])), 4)

    pq_pad = quantizer(True)
    pq_pad.set_codebooks(pq.codebooks(), pq.info()["ksub_actual"])
    ix_pad, _ = build(pq_pad, None)
    res["info_padded"] = pq_pad.info()
    # the two layouts and the yardstick alternate, so a drift of the shared host shows in all of them
    runs = {"adc_plain": lambda q: ix.search(q, k), "adc_padded": lambda q: ix_pad.search(q, k), "search_exact": lambda q: g.search_exact(q, k)}
    qps = {n: [] for n in runs}
    for _ in range(2):
        for n, fn in runs.items():
            qps[n].append(round(rate(fn, queries, a.reps), 1))
    res["qps"] = qps
    # the same call under both clocks: device events on the context's stream against the host clock
    ctx.timer_start()
    t = time.perf_counter()
    ix.search(queries[0], k)
    host_ms = (time.perf_counter() - t) * 1e3
    res["adc_one_batch_ms"] = {"device_events": round(ctx.timer_stop_ms(), 3), "host_clock": round(host_ms, 3)}
    res["recall"] = {"adc": recall(runs["adc_plain"])}
    same = all(np.array_equal(ix.search(q, k).ids, ix_pad.search(q, k).ids) for q in queries)
    res["layouts_agree"] = bool(same)
    ix_pad.close()

    for rows in ("f32", "f16"):
        ixr, _ = build(pq, rows)
        res["bytes_per_row"][f"codes_plus_{rows}_refine"] = ixr.bytes() / N
        for fk in (64, 256):
            fn = lambda q: ixr.search(q, k, fetch_k=fk)  # noqa: E731
            res["qps"][f"refined_{rows}_fetch{fk}"] = [round(rate(fn, queries, a.reps), 1)]
            res["recall"][f"refined_{rows}_fetch{fk}"] = recall(fn)
        ixr.close()

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
