#!/usr/bin/env python3
"""What a probed search costs on either side of 256 probed lists, and at nprobe = nlist against fvdb_ivf_search_all.
One JSON line, also written to --out.

  register_256   fvdb_ivf_search_dev_slot at nprobe = 256 with the exact scan forced: the register path's last shape
  wide_256       fvdb_ivf_search_wide_dev_slot at nprobe = 256: the wide selection over the same lists
  probed_N       fvdb_ivf_search_dev_slot at nprobe = 257, 512 and nlist: the full centroid ranking and the wide selection
  search_all     fvdb_ivf_search_all_dev: every list in list-index order through the register path

All variants run in one process on one index at k = 10, alternating, each timed with HIP events after a warm-up; the
figure of a variant is the median of --reps passes.

    python tools/nprobe_bench.py --out profiles/any_nprobe_bench.json
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
    print(f"[nprobe_bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=384)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    fv = fvdb_import.load()
    ctx = fv.Context(0)
    lib = ctx.lib
    rng = np.random.default_rng(1)
    means = rng.standard_normal((a.nlist, a.d)).astype(np.float32)
    ix = fv.DeviceIVF(ctx, a.d, a.nlist)
    cents = None
    ix_ready = False
    for o in range(0, a.n, 100_000):  # rows are drawn chunk by chunk: the host never holds the whole table
        m = min(100_000, a.n - o)
        x = means[rng.integers(0, a.nlist, m)] + np.float32(0.35) * rng.standard_normal((m, a.d)).astype(np.float32)
        if not ix_ready:
            cents = x[:a.nlist].copy()
            ix.set_centroids(cents)
            ix.reserve(a.n)
            ix_ready = True
        ix.add(x, np.arange(o, o + m, dtype=np.uint64))
    q = means[rng.integers(0, a.nlist, a.B)] + np.float32(0.35) * rng.standard_normal((a.B, a.d)).astype(np.float32)
    note(f"index built: {a.n} x {a.d}, nlist {a.nlist}")
    lib.fvdb_ivf_set_scan_mode(ix.h, 1)  # the exact scan on the register path: the same arithmetic as the wide path

    k, B = a.k, a.B
    q_dev = ctx.upload(q)
    out = ctx.alloc(B * k * 12 + B * 4)
    at = lambda off: C.c_void_p(out.value + off)  # noqa: E731
    outs = (at(0), at(B * k * 8), at(B * k * 12))

    def probed(nprobe):
        return lambda: ctx.check(lib.fvdb_ivf_search_dev_slot(ix.h, None, 0, q_dev, B, k, nprobe, *outs, None))

    def wide(nprobe):
        return lambda: ctx.check(lib.fvdb_ivf_search_wide_dev_slot(ix.h, None, 0, None, q_dev, B, k, nprobe, *outs, None))

    def search_all():
        ctx.check(lib.fvdb_ivf_search_all_dev(ix.h, q_dev, B, k, *outs))

    above = [n for n in (257, 512) if n < a.nlist] + [a.nlist]
    variants = [("register_256", probed(256)), ("wide_256", wide(256))]
    variants += [(f"probed_{n}", probed(n)) for n in above]
    variants += [("search_all", search_all)]
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

    # nprobe = nlist and search_all answer the same question: equal up to the order among equal distances
    gi, gd, gc = ix.search(q[:64], k, a.nlist)
    ai, ad, ac = ix.search_all(q[:64], k)
    same = bool(np.array_equal(gd.view(np.uint32), ad.view(np.uint32)) and np.array_equal(gc, ac))

    line = dict(bench="any_nprobe", n=a.n, d=a.d, nlist=a.nlist, B=B, k=k, reps=a.reps, batch_ms=ms, batch_ms_min_max=spread,
                probed_257_over_wide_256=ms["probed_257"] / ms["wide_256"] if "probed_257" in ms else None,
                wide_256_over_register_256=ms["wide_256"] / ms["register_256"],
                probed_nlist_over_search_all=ms[f"probed_{a.nlist}"] / ms["search_all"],
                probed_nlist_distances_equal_search_all=same)
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
