#!/usr/bin/env python3
"""Measures the inverted file over PQ codes on bench.py's mixture, in one run: IVFPQIndex at each
nprobe, ADC and refined (fetch_k 64, f32 rows), against the flat PQIndex ADC search (the same arithmetic over every row),
IVFSQ8Index and the f32 IVF-flat index (DeviceIVF) at the same nprobe and the same centroids — q/s, recall@k against
HNSWIndex.search_exact, bytes per row, rows scored per query and the slices S of the scan.  Every rate is a host clock
around calls that end in a synchronise; the runs alternate over two rounds, so a drift of a shared host shows in all of
them.  Prints one JSON object and, with --out, writes it to a file.

    python tools/ivfpq_bench.py --n-vectors 1000000 --out profiles/ivfpq_bench.json

--residual measures the residual index instead of the other index kinds: a second quantizer is
trained on ivf_residuals of the same training rows, a residual IVFPQIndex is built over the same centroids and rows, and
at each nprobe the plain and the residual ADC search alternate, again over two rounds.

    python tools/ivfpq_bench.py --n-vectors 1000000 --residual --out profiles/ivfrpq_bench.json
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


def note(msg):
    print(msg, file=sys.stderr, flush=True)  # progress: the result itself is the one JSON line on stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-vectors", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--subspaces", type=int, default=48)
    ap.add_argument("--centroids", type=int, default=256)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 16, 64, 1024])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch-k", dest="fetch_k", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--train-rows", type=int, default=50_000)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--residual", action="store_true", help="plain against residual codes, nothing else")
    ap.add_argument("--out")
    a = ap.parse_args()

    fv = fvdb_import.load()
    ctx = fv.Context(0)
    N, d, k = a.n, a.dim, a.k
    gen = Generator(d=d)
    x = gen.chunks(N, 100_000)
    ids = np.arange(N, dtype=np.uint64)
    queries = [gen.rows(a.batch, stream=10_000 + i) for i in range(a.batches)]
    res = {"n": N, "d": d, "m": a.subspaces, "ksub": a.centroids, "nlist": a.nlist, "batch": a.batch, "k": k, "fetch_k": a.fetch_k,
           "reps": a.reps,
           "timing": "host clock around host-form calls, which synchronise; queries uploaded and results downloaded inside"}

    pq = fv.ProductQuantizer(ctx, d, a.subspaces, a.centroids)
    pq_rows = x[np.random.default_rng(0).choice(N, min(N, a.train_rows), replace=False)]
    pq.train(pq_rows, a.iterations, seed=1)
    ix = fv.IVFPQIndex(ctx, pq, a.nlist, refine_rows="f32")
    res["train"] = ix.train(x[np.random.default_rng(0).choice(N, min(N, 100_000), replace=False)], max_iterations=10, seed=1)
    t = time.perf_counter()
    for c in range(0, N, 100_000):
        ix.add(ids[c:c + 100_000], x[c:c + 100_000])
    res["add_rows_per_s"] = round(N / (time.perf_counter() - t))  # host check, assign, upload, encode, place, refine rows, tables
    note(f"IVFPQIndex built: {res['add_rows_per_s']} rows/s")
    if a.residual:
        return residual_runs(fv, ctx, a, res, ix, pq_rows, x, ids, queries)
    flat = fv.PQIndex(ctx, pq)
    sq8 = fv.IVFSQ8Index(ctx, d, a.nlist)
    sq8.set_centroids(ix.centroids())
    ivf = fv.DeviceIVF(ctx, d, a.nlist)
    ivf.set_centroids(ix.centroids())
    for c in range(0, N, 100_000):
        flat.add(ids[c:c + 100_000], x[c:c + 100_000])
        sq8.add(ids[c:c + 100_000], x[c:c + 100_000])
        ivf.add(x[c:c + 100_000], ids[c:c + 100_000])
    sizes = ix.list_sizes()
    res["lists"] = {"empty": int((sizes == 0).sum()), "longest": int(sizes.max()), "mean": float(sizes.mean())}
    refine_bytes = 4 * d * N
    res["bytes_per_row"] = {"ivfpq_codes_and_tables": (ix.bytes() - refine_bytes) / N, "ivfpq_with_f32_refine_rows": ix.bytes() / N,
                            "pq_flat": flat.bytes() / N, "ivfsq8": sq8.bytes() / N, "ivf_f32_rows_and_ids": 4 * d + 8}

    g = fv.HNSWIndex(ctx, max_connections=2, max_connections_layer_0=2, ef_construction=8)
    g.bulk_build(ids, x, levels=np.zeros(N, np.int64))
    truth = [g.search_exact(q, k) for q in queries]
    note("yardsticks built")

    runs, scan = {"pq_flat_adc": lambda q: flat.search(q, k)}, {}
    for np_ in a.nprobe:
        ix.search(queries[0], k, np_)
        info = ix.info()
        scan[str(np_)] = {"rows_scored_per_query": info["rows_scored"] / a.batch, "lists_per_query": info["pairs"] / a.batch,
                          "slices": info["last_slices"]}
        runs[f"ivfpq_adc_np{np_}"] = lambda q, p=np_: ix.search(q, k, p)
        runs[f"ivfpq_refined_fetch{a.fetch_k}_np{np_}"] = lambda q, p=np_: ix.search(q, k, p, fetch_k=a.fetch_k)
        runs[f"ivf_f32_np{np_}"] = lambda q, p=np_: ivf.search(q, k, p)
        try:
            sq8.search(queries[0], k, np_)
            runs[f"ivfsq8_symmetric_np{np_}"] = lambda q, p=np_: sq8.search(q, k, p)
        except fv.engine.Unsupported as e:  # more than 256 probed lists
            scan[str(np_)]["ivfsq8"] = str(e)
    res["info"], res["scan"] = ix.info(), scan
    res["qps"] = {n: [] for n in runs}
    for _ in range(2):
        for n, fn in runs.items():
            res["qps"][n].append(round(rate(fn, queries, a.reps), 1))
            note(f"{n}: {res['qps'][n][-1]} q/s")

    def hits(r):  # SearchResults, or DeviceIVF's (ids, distances, counts)
        return (r.ids, r.counts) if hasattr(r, "ids") else (r[0], r[2])
    res["recall"] = {n: round(float(np.mean([recall_at_k(*hits(fn(q)), t.ids, k) for q, t in zip(queries, truth)])), 4) for n, fn in runs.items()}
    report(a, res)


def report(a, res):
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def residual_runs(fv, ctx, a, res, ix, pq_rows, x, ids, queries):
    """the plain index `ix` against a residual one over the same centroids and rows: ADC q/s alternating, recall, bytes"""
    N, d, k = a.n, a.dim, a.k
    rpq = fv.ProductQuantizer(ctx, d, a.subspaces, a.centroids)
    rpq.train(fv.ivf_residuals(ctx, ix.centroids(), pq_rows)[0], a.iterations, seed=1)
    rix = fv.IVFPQIndex(ctx, rpq, a.nlist, residual=True)
    rix.set_centroids(ix.centroids())
    t = time.perf_counter()
    for c in range(0, N, 100_000):
        rix.add(ids[c:c + 100_000], x[c:c + 100_000])
    res["residual_add_rows_per_s"] = round(N / (time.perf_counter() - t))
    note(f"residual IVFPQIndex built: {res['residual_add_rows_per_s']} rows/s")
    res["bytes_per_row"] = {"ivfpq_codes_and_tables": (ix.bytes() - 4 * d * N) / N, "ivfrpq_codes_and_tables": rix.bytes() / N}
    g = fv.HNSWIndex(ctx, max_connections=2, max_connections_layer_0=2, ef_construction=8)
    g.bulk_build(ids, x, levels=np.zeros(N, np.int64))
    truth = [g.search_exact(q, k) for q in queries]
    runs = {}
    for np_ in a.nprobe:
        runs[f"ivfpq_adc_np{np_}"] = lambda q, p=np_: ix.search(q, k, p)
        runs[f"ivfrpq_adc_np{np_}"] = lambda q, p=np_: rix.search(q, k, p)
    res["info"], res["qps"] = rix.info(), {n: [] for n in runs}
    for _ in range(2):
        for n, fn in runs.items():
            res["qps"][n].append(round(rate(fn, queries, a.reps), 1))
            note(f"{n}: {res['qps'][n][-1]} q/s")
    res["recall"] = {n: round(float(np.mean([recall_at_k(r.ids, r.counts, t.ids, k) for r, t in zip(map(fn, queries), truth)])), 4)
                     for n, fn in runs.items()}
    report(a, res)


if __name__ == "__main__":
    main()
