#!/usr/bin/env python3
"""The wide selection (fvdb_ivf_search_wide_dev_slot, k up to 4096) against the register path and the CPU restatement.
One JSON line, also written to --out.

  register(256)   fvdb_ivf_search_dev_slot at k = 256 with the exact scan forced: the path k <= 256 keeps
  wide(k)         the wide path at k = 256, 512, 1024, 4096 (score into the arena, select per query)
  oracle(1024)    the oracle's batch_search with 16 threads at k = 1024 on a 64-query sample, per query

All device variants run in one process on one index, alternating, each timed with HIP events after a warm-up; the
per-stage shares come from a separate profiled pass (stage events), so the timed passes carry no synchronisation.

    python tools/wide_k_bench.py --out profiles/wide_k_bench.json
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

WIDE_KS = (256, 512, 1024, 4096)
ARENA_BUDGET = 1 << 30  # kWideArenaBytes (csrc/fvdb_hip.cpp)
ARENA_SOURCE = "restated from kWideArenaBytes, wide_arena_blocks and wide_sub_batch in csrc/fvdb_hip.cpp, not read from the engine"


def note(msg):
    print(f"[wide_k_bench] {msg}", file=sys.stderr, flush=True)


def arena_plan(list_sizes, nprobe, B):
    """The engine's arena sizing restated (wide_arena_blocks / wide_sub_batch): bytes per query, queries per pass.  The
    engine has no call that reports these, so the figures follow the C++ only as long as this function does: the JSON
    says so in `source`."""
    blocks = (np.asarray(list_sizes, np.int64) + 63) // 64
    cap = max(1, min(nprobe * int(blocks.max()), int(blocks.sum())))
    per_q = cap * 256
    step = min(B, min(max(ARENA_BUDGET // per_q, 1), 16384))
    return dict(source=ARENA_SOURCE, arena_bytes_per_query=per_q, queries_per_pass=step, sub_batches=-(-B // step),
                arena_bytes=per_q * step, mean_probed_bytes_per_query=float(256 * nprobe * blocks.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--oracle-queries", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    fv = fvdb_import.load()
    ctx = fv.Context(0)
    lib = ctx.lib
    rng = np.random.default_rng(1)
    means = rng.standard_normal((a.nlist, a.d)).astype(np.float32)
    x = means[rng.integers(0, a.nlist, a.n)] + np.float32(0.35) * rng.standard_normal((a.n, a.d)).astype(np.float32)
    ids = np.arange(a.n, dtype=np.uint64)
    q = means[rng.integers(0, a.nlist, a.B)] + np.float32(0.35) * rng.standard_normal((a.B, a.d)).astype(np.float32)
    cents = x[:a.nlist].copy()
    ix = fv.DeviceIVF(ctx, a.d, a.nlist)
    ix.set_centroids(cents)
    ix.reserve(a.n)
    clusters = []
    for o in range(0, a.n, 100_000):
        clusters.append(ix.add(x[o:o + 100_000], ids[o:o + 100_000])[0])
    clusters = np.concatenate(clusters)
    note(f"index built: {a.n} x {a.d}, nlist {a.nlist}")
    lib.fvdb_ivf_set_scan_mode(ix.h, 1)  # register path: the exact scan, the same arithmetic as the wide path

    kmax = max(WIDE_KS)
    q_dev = ctx.upload(q)
    out = ctx.alloc(a.B * kmax * 12 + a.B * 4)
    at = lambda off: C.c_void_p(out.value + off)  # noqa: E731
    outs = (at(0), at(a.B * kmax * 8), at(a.B * kmax * 12), None)

    def register():
        ctx.check(lib.fvdb_ivf_search_dev_slot(ix.h, None, 0, q_dev, a.B, 256, a.nprobe, *outs))

    def wide(k):
        return lambda: ctx.check(lib.fvdb_ivf_search_wide_dev_slot(ix.h, None, 0, None, q_dev, a.B, k, a.nprobe, *outs))

    variants = [("register_256", register)] + [(f"wide_{k}", wide(k)) for k in WIDE_KS]
    for _, fn in variants:  # warm-up: scratch allocated, code objects loaded
        fn()
    ctx.synchronize()
    note("warmed up")
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):  # alternate, so that drift hits every variant alike
        for name, fn in variants:
            ctx.timer_start()
            fn()
            times[name].append(ctx.timer_stop_ms())
    ms = {name: float(np.median(v)) for name, v in times.items()}
    spread = {name: [float(np.min(v)), float(np.max(v))] for name, v in times.items()}

    note(f"timed: {ms}")
    # stage shares: coarse stage, plan, score ("fine scan") and select ("fine merge"), from stage events
    shares = {}
    ctx.set_profiling(1)
    for name, fn in variants:
        ix.stage_times()
        for _ in range(3):
            fn()
        n, st = ix.stage_times()
        tot = sum(st.values()) - st["mfma_filter_kernel"]
        shares[name] = {s: round(v / tot, 4) for s, v in st.items() if s != "mfma_filter_kernel"} if n and tot > 0 else {}
    ctx.set_profiling(0)
    stats = ix.last_stats()

    # the CPU restatement: 16 threads, k = 1024, a sample of the queries
    import oracle as orc
    orc.build()
    cpu = orc.IVFIndex(n_clusters=a.nlist, n_probe=a.nprobe)
    cpu.set_trained(cents)
    cpu.batch_insert_assigned(ids, x, clusters)
    note("oracle built")
    qs = q[:a.oracle_queries]
    cpu.batch_search(qs[:8], 1024, a.nprobe, threads=16)
    t0 = time.perf_counter()
    oi, od, oc = cpu.batch_search(qs, 1024, a.nprobe, threads=16)
    oracle_ms = (time.perf_counter() - t0) * 1e3
    gi, gd, gc = ix.search_wide(qs, 1024, a.nprobe)
    identical = bool(np.array_equal(gi, oi) and np.array_equal(gd.view(np.uint32), od.view(np.uint32)) and np.array_equal(gc, oc))

    line = dict(bench="wide_k", n=a.n, d=a.d, nlist=a.nlist, nprobe=a.nprobe, B=a.B, reps=a.reps, batch_ms=ms, batch_ms_min_max=spread,
                us_per_query={name: 1e3 * v / a.B for name, v in ms.items()},
                wide_256_over_register_256=ms["wide_256"] / ms["register_256"],
                oracle_k1024=dict(threads=16, queries=int(qs.shape[0]), wall_ms=oracle_ms, us_per_query=1e3 * oracle_ms / qs.shape[0],
                                  wide_identical_to_oracle=identical),
                wide_1024_speedup_over_oracle=(oracle_ms / qs.shape[0]) / (ms["wide_1024"] / a.B),
                arena=arena_plan(ix.list_sizes(), a.nprobe, a.B), rows_scanned_per_batch=stats["rows_scanned"],
                stage_shares=shares)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.free(q_dev)
    ctx.free(out)


if __name__ == "__main__":
    main()
