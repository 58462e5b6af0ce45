#!/usr/bin/env python3
"""The sharded search beyond the register path's limits against what was there before it.
One process, a communicator of one rank over RCCL (the exchanges are then copies), one JSON line, also written to --out.

  sharded_256       fvdb_ivf_search_sharded_begin at k = 256, nprobe = 32: the existing step
  sharded_new_256   fvdb_ivf_search_sharded_wide_begin at the same point (it takes the same route)
  sharded_new_1024  fvdb_ivf_search_sharded_wide_begin at k = 1024: shard-wide search + wide merge
  wide_1024         fvdb_ivf_search_wide_dev_slot at k = 1024 on the unsharded index
  merge_256         fvdb_merge_keys_dev at G = 8, k = 256
  merge_wide_256    fvdb_merge_keys_wide_dev on the same partial lists

All variants alternate in one process, each timed with HIP events: the median of --reps after a warm-up.

    python tools/sharded_wide_bench.py --out profiles/sharded_wide_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fvdb_import  # noqa: E402


def note(msg):
    print(f"[sharded_wide_bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
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

    def index():
        ix = fv.DeviceIVF(ctx, a.d, a.nlist)
        ix.set_centroids(cents)
        ix.reserve(a.n)
        for o in range(0, a.n, 100_000):
            ix.add(x[o:o + 100_000], ids[o:o + 100_000])
        return ix

    plain, shard = index(), index()
    shard.set_global_list_sizes(shard.list_sizes())  # the one rank's shard holds every list
    comm = fv.sharded.Comm.rccl(ctx)
    s = C.c_void_p()
    ctx.check(lib.fvdb_sharded_create(shard.h, comm.h, C.byref(s)))
    note(f"indexes built: {a.n} x {a.d}, nlist {a.nlist}")

    B, G, kmax = a.B, 8, 1024
    q_dev = ctx.upload(q)
    out = ctx.alloc(B * kmax * 12 + B * 4)
    at = lambda off: C.c_void_p(out.value + off)  # noqa: E731
    outs = (at(0), at(B * kmax * 8), at(B * kmax * 12))
    # partial lists for the merges: G ascending lists of 256 unique keys per query
    km = 256
    pool = (rng.integers(0x3F000000, 0x3F800000, (B, G * km), dtype=np.uint64) << np.uint64(32)) | np.arange(G * km, dtype=np.uint64)
    pool = np.take_along_axis(pool, rng.permuted(np.tile(np.arange(G * km), (B, 1)), axis=1), axis=1)
    keys = np.sort(pool.reshape(B, G, km), axis=2).transpose(1, 0, 2).copy()
    k_dev, i_dev = ctx.upload(keys), ctx.upload(keys ^ np.uint64(0x5A5A5A5A))

    def sharded_old():
        ctx.check(lib.fvdb_ivf_search_sharded_begin(s, None, 0, q_dev, B, 256, a.nprobe, 0, *outs))

    def sharded_new(k):
        return lambda: ctx.check(lib.fvdb_ivf_search_sharded_wide_begin(s, None, 0, None, q_dev, B, k, a.nprobe, 0, *outs))

    def wide():
        ctx.check(lib.fvdb_ivf_search_wide_dev_slot(plain.h, None, 0, None, q_dev, B, 1024, a.nprobe, *outs, None))

    variants = [("sharded_256", sharded_old), ("sharded_new_256", sharded_new(256)), ("sharded_new_1024", sharded_new(1024)),
                ("wide_1024", wide),
                ("merge_256", lambda: fv.engine.merge_keys_dev(ctx, k_dev, i_dev, G, B, km, *outs)),
                ("merge_wide_256", lambda: fv.engine.merge_keys_wide_dev(ctx, k_dev, i_dev, G, B, km, *outs))]
    results = {}
    for name, fn in variants:  # warm-up: scratch allocated, code objects loaded; and what each variant returns
        fn()
        fn()
        ctx.synchronize()
        results[name] = (ctx.download(outs[0], (B, kmax), np.uint64).copy(), ctx.download(outs[2], B, np.uint32).copy())
    note("warmed up")
    same = lambda x, y, k: bool(np.array_equal(results[x][1], results[y][1]) and  # noqa: E731
                                np.array_equal(results[x][0].reshape(-1)[:B * k], results[y][0].reshape(-1)[:B * k]))
    identical = dict(sharded_256=same("sharded_256", "sharded_new_256", 256), k1024=same("sharded_new_1024", "wide_1024", 1024),
                     merge=same("merge_256", "merge_wide_256", 256))
    times = {name: [] for name, _ in variants}
    for _ in range(a.reps):  # alternate, so that drift hits every variant alike
        for name, fn in variants:
            ctx.timer_start()
            fn()
            times[name].append(ctx.timer_stop_ms())
    ms = {name: float(np.median(v)) for name, v in times.items()}
    spread = {name: [float(np.min(v)), float(np.max(v))] for name, v in times.items()}
    line = dict(bench="sharded_wide", n=a.n, d=a.d, nlist=a.nlist, nprobe=a.nprobe, B=B, reps=a.reps, world=1, transport="rccl",
                batch_ms=ms, batch_ms_min_max=spread, identical_results=identical,
                sharded_new_256_over_sharded_256=ms["sharded_new_256"] / ms["sharded_256"],
                sharded_new_1024_over_wide_1024=ms["sharded_new_1024"] / ms["wide_1024"],
                merge_wide_256_over_merge_256=ms["merge_wide_256"] / ms["merge_256"], merge_G=G)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    lib.fvdb_sharded_destroy(s)
    comm.close()


if __name__ == "__main__":
    main()
