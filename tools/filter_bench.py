#!/usr/bin/env python3
"""Filtered search: the reference's oversampling path against the allow-set applied on the device.

On a synthetic hybrid index, for filters matching 1/2, 1/10 and 1/100 of the rows: results returned per query and
recall@k against a brute force over the allowed rows, for
  oversample   HybridIndex.search_with_filter (3 k candidates, host callback per id)
  traversal    HybridIndex.search_allowed with the exact scan off (scan_cutoff 0): masked traversal + masked list scan
  scan         HybridIndex.search_allowed with the recent part always scanned exactly
Every path is warmed the same way (one untimed call: graph upload, scratch and pinned buffers, first kernel loads) and
then timed --repeat times; the median and the spread are printed.  For the two search_allowed paths the time of a call
that has to build its masks (the allow-set changed in between) is timed --repeat times as well.

Every selectivity runs in a child process of its own under a time limit; the first failure stops the run.

    python tools/filter_bench.py --n 200000 --d 128 --batch 256
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DAY = 86400.0


def child(a):
    import fvdb_import
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    rng = np.random.default_rng(1)
    n, d, k, B = a.n, a.d, a.k, a.batch
    means = rng.standard_normal((a.nlist, d)).astype(np.float32)
    x = means[rng.integers(0, a.nlist, n)] + np.float32(0.35) * rng.standard_normal((n, d)).astype(np.float32)
    q = means[rng.integers(0, a.nlist, B)] + np.float32(0.35) * rng.standard_normal((B, d)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64)
    now = 1000 * DAY
    ts = now - np.where(rng.random(n) < a.recent_frac, 1 * DAY, 30 * DAY)
    ix = fv.HybridIndex(ctx, n_clusters=a.nlist, n_probe=a.nprobe, auto_migrate=False)
    ix.set_ivf_centroids(means)
    ix.bulk_insert(ids, x, ts, now)
    allowed = ids[rng.random(n) < a.selectivity]
    keep = np.zeros(n, bool)
    keep[allowed] = True
    # ground truth: exact k-NN among the allowed rows (f64 on the host: a yardstick, not the product's arithmetic)
    xa = x[allowed].astype(np.float64)
    d2 = (q.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * q.astype(np.float64) @ xa.T + (xa ** 2).sum(1)[None, :]
    kk = min(k, allowed.size)
    truth = allowed[np.argsort(d2, axis=1)[:, :kk]] if kk else np.zeros((B, 0), np.uint64)

    def score(res):
        hits = sum(np.intersect1d(res.ids[b, :int(res.counts[b])], truth[b]).size for b in range(B))
        return dict(returned_per_query=float(res.counts.mean()), recall=hits / max(1, truth.size))

    def timed(fn, before=None):
        """one warm-up call, then a.repeat timed ones (`before` runs untimed ahead of each): last result, ms statistics"""
        ms = []
        for i in range(a.repeat + 1):
            if before:
                before()
            ctx.device_synchronize()
            t0 = time.perf_counter()
            r = fn()
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        return r, dict(ms_median=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1], runs=len(ms))

    out = dict(selectivity=a.selectivity, n=n, d=d, batch=B, k=k, allowed=int(allowed.size), recent=int(ix.recent_count()))
    r, t = timed(lambda: ix.search_with_filter(q, k, lambda i: bool(keep[i]), now=now))
    out["oversample"] = dict(score(r), **t)
    pushed = lambda: ix.search_allowed(q, k, allowed, now=now, hnsw_ef=a.ef, ivf_n_probe=a.nprobe)  # noqa: E731
    # a different allow-set in between makes the next call build its masks again
    other = lambda: ix.search_allowed(q[:1], k, ids[:1], now=now, hnsw_ef=a.ef, ivf_n_probe=a.nprobe)  # noqa: E731
    for name, cutoff in (("traversal", 0), ("scan", fv.HNSWIndex.SCAN_ALWAYS)):
        ix.hnsw().scan_cutoff = cutoff
        r, cached = timed(pushed)
        _, build = timed(pushed, before=other)
        out[name] = dict(score(r), cached_masks=cached, with_mask_build=build)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--ef", type=int, default=50)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--recent-frac", type=float, default=0.1)
    ap.add_argument("--repeat", type=int, default=9, help="timed runs per path, after one warm-up")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one selectivity may take")
    ap.add_argument("--selectivity", type=float, default=None, help="(child) run this one selectivity in this process")
    a = ap.parse_args()
    if a.selectivity is not None:
        return child(a)
    for sel in (0.5, 0.1, 0.01):
        cmd = [sys.executable, os.path.abspath(__file__), "--selectivity", str(sel)]
        for name in ("n", "d", "nlist", "nprobe", "ef", "k", "batch", "repeat"):
            cmd += [f"--{name}", str(getattr(a, name))]
        cmd += ["--recent-frac", str(a.recent_frac)]
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print(f"[filter_bench] selectivity {sel}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 124
        if rc:
            print(f"[filter_bench] selectivity {sel}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
