"""Shared by tests/test_gpu_paired_batches.py and its child process: the small hybrid index, the query batches, and one
pipelined loop in the shape of bench.py's pipelined().  Run as a program it does the loop in THIS process (whose
environment decides FVDB_HYBRID_PAIR, read once by the library) and writes the results to the .npz named on the
command line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from _data import mixture  # noqa: E402

DAY = 86400.0
NOW = 1000 * DAY
N, D, NLIST, NPROBE, K, EF = 24000, 128, 64, 8, 10, 50
KW = dict(now=NOW, hnsw_ef=EF, ivf_n_probe=NPROBE, dim=D)


def build_index(fv, ctx):
    """24000 x 128 rows, 30 % recent (sequential graph), 64 lists.  d = 128 keeps the workgroup filter's shape."""
    x = mixture(N, D, n_comp=48, seed=311)
    recent = np.random.default_rng(312).random(N) < 0.3
    ts = np.where(recent, NOW - 1 * DAY, NOW - 30 * DAY)
    g = fv.HybridIndex(ctx, max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=NLIST,
                       n_probe=NPROBE, hnsw_seed=11)
    g.set_ivf_centroids(x[:NLIST].copy())
    g.set_sequential_graph(True)
    g.bulk_insert(np.arange(N, dtype=np.uint64), x, ts, NOW)
    return g, x


def batch(x, B, seed):
    """B queries near rows of the index, so that both parts have close neighbours."""
    rng = np.random.default_rng(seed)
    return (x[rng.integers(0, N, B)] + np.float32(0.05) * rng.standard_normal((B, D)).astype(np.float32)).astype(np.float32)


def pipelined(g, qdev, sizes, nsteps, depth, k=K, **kw):
    """bench.py's pipelined(): step i begins in slot i % depth before step i - depth + 1 is collected."""
    kw = dict(KW, **kw)
    nb = len(qdev)
    out = [None] * nsteps
    for i in range(nsteps):
        g.search_dev_begin(i % depth, qdev[i % nb], sizes[i % nb], k, **kw)
        if i >= depth - 1:
            out[i - depth + 1] = g.search_dev_end((i - depth + 1) % depth)
    for i in range(max(nsteps - depth + 1, 0), nsteps):
        out[i] = g.search_dev_end(i % depth)
    return out


LOOP_SIZES = (64, 33, 47, 64)


def child_run(path):
    import fvdb_import
    fv = fvdb_import.load()
    ctx = fv.Context(0)
    g, x = build_index(fv, ctx)
    qs = [batch(x, B, 700 + j) for j, B in enumerate(LOOP_SIZES)]
    qdev = [ctx.upload(q) for q in qs]
    res = pipelined(g, qdev, LOOP_SIZES, 8, 3)
    # two batches begun back to back: the rows the LAST IVF chain scanned tell whether it served one batch or both
    g.search_dev_begin(0, qdev[0], LOOP_SIZES[0], K, **KW)
    g.search_dev_begin(1, qdev[1], LOOP_SIZES[1], K, **KW)
    a, b = g.search_dev_end(0), g.search_dev_end(1)
    rows_last = g.ivf().last_stats()["rows_scanned"]
    out = {"rows_last": np.array([rows_last], np.uint64), "a_ids": a.ids, "b_ids": b.ids}
    for i, r in enumerate(res):
        out[f"ids{i}"], out[f"dist{i}"], out[f"counts{i}"] = r.ids, r.distances.view(np.uint32), r.counts
    np.savez(path, **out)


if __name__ == "__main__":
    child_run(sys.argv[1])
