#!/usr/bin/env python3
"""What the whole n_probe curve costs against the repeated searches it replaces.
One JSON line, also written to --out.

  curve        one fvdb_ivf_quality_curve_dev call: recall and precision sums at every n_probe = 1 .. nlist
  loop         fvdb_ivf_search_quality_dev at n_probe = 1, 2, 4, ..., nlist, one call each: the sweep a user runs today
  single       fvdb_ivf_search_quality_dev at n_probe = nlist alone

All variants run in one process on one index, alternating, each timed with HIP events after a warm-up; the figure of a
variant is the median of --reps passes, reported with its minimum and maximum.  The curve's sums at the loop's n_probe
values are compared with the loop's own per-query values summed in query order (they must be equal bit for bit).

    python tools/nprobe_curve_bench.py --out profiles/nprobe_curve_bench.json
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
    print(f"[nprobe_curve_bench] {msg}", file=sys.stderr, flush=True)


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
    ix_ready = False
    for o in range(0, a.n, 100_000):  # rows are drawn chunk by chunk: the host never holds the whole table
        m = min(100_000, a.n - o)
        x = means[rng.integers(0, a.nlist, m)] + np.float32(0.35) * rng.standard_normal((m, a.d)).astype(np.float32)
        if not ix_ready:
            ix.set_centroids(x[:a.nlist].copy())
            ix.reserve(a.n)
            ix_ready = True
        ix.add(x, np.arange(o, o + m, dtype=np.uint64))
    q = means[rng.integers(0, a.nlist, a.B)] + np.float32(0.35) * rng.standard_normal((a.B, a.d)).astype(np.float32)
    note(f"index built: {a.n} x {a.d}, nlist {a.nlist}")

    k, B, nlist = a.k, a.B, a.nlist
    q_dev = ctx.upload(q)
    per_q = ctx.alloc(B * 8)          # recall[B], precision[B] of one fvdb_ivf_search_quality_dev call
    sums = ctx.alloc(nlist * 8)       # recall sums [nlist], precision sums [nlist] of the curve
    at = lambda p, off: C.c_void_p(p.value + off)  # noqa: E731
    sweep = []
    p = 1
    while p < nlist:
        sweep.append(p)
        p *= 2
    sweep.append(nlist)

    def quality(nprobe):
        ctx.check(lib.fvdb_ivf_search_quality_dev(ix.h, None, 0, q_dev, B, k, nprobe, per_q, at(per_q, B * 4)))

    def curve():
        ctx.check(lib.fvdb_ivf_quality_curve_dev(ix.h, None, 0, None, q_dev, B, k, 0, sums, at(sums, nlist * 4)))

    def loop():
        for nprobe in sweep:
            quality(nprobe)

    variants = [("curve", curve), ("loop", loop), ("single", lambda: quality(nlist))]
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

    # the curve against the sweep it replaces
    curve()
    ctx.synchronize()
    both = ctx.download(sums, 2 * nlist, np.float32)
    equal, recall_at = True, {}
    for nprobe in sweep:
        quality(nprobe)
        ctx.synchronize()
        v = ctx.download(per_q, 2 * B, np.float32)
        tr, tp = np.float32(0), np.float32(0)
        for b in range(B):
            tr, tp = np.float32(tr + v[b]), np.float32(tp + v[B + b])
        equal = equal and tr.view(np.uint32) == both[nprobe - 1].view(np.uint32) \
            and tp.view(np.uint32) == both[nlist + nprobe - 1].view(np.uint32)
        recall_at[str(nprobe)] = float(both[nprobe - 1] / np.float32(B))
    reach = np.flatnonzero(both[:nlist] / np.float32(B) >= np.float32(0.95))

    line = dict(bench="nprobe_curve", n=a.n, d=a.d, nlist=nlist, B=B, k=k, reps=a.reps, sweep=sweep, call_ms=ms,
                call_ms_min_max=spread, curve_over_loop=ms["curve"] / ms["loop"], curve_over_single=ms["curve"] / ms["single"],
                curve_equals_loop_bits=bool(equal), avg_recall_at=recall_at,
                smallest_n_probe_for_0_95=int(reach[0]) + 1 if reach.size else None)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for p in (q_dev, per_q, sums):
        ctx.free(p)


if __name__ == "__main__":
    main()
