"""One rank of tests/test_00_gpu_sharded_wide_ranks.py (two of these through torch.distributed.run; both share the box's
one GPU, the collectives travel over gloo through the hosted transport).  Every rank runs ShardedHybrid where the sharded
step goes through fvdb_ivf_search_sharded_wide_begin — k above 256, more than 256 lists probed, an allow-set — and compares
ITS OWN results bit for bit with the CPU oracle's search of the unsharded index.  Writes `rank<r>.json` into argv[1]."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out_dir = sys.argv[1]
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import fvdb_import
    import oracle as orc
    from _data import bits, mixture
    fv = fvdb_import.load()
    sh = fv.sharded
    report = {"rank": rank, "world": world, "checks": []}

    DAY = 86400.0
    # 300 lists of ~14 historical rows: one partly filled block each; B not a multiple of world: ragged last slice
    n, d, nlist, ef, B = 6000, 16, 300, 40, 9
    x = mixture(n, d, n_comp=40, sigma=0.6, seed=270)
    ids = np.arange(n, dtype=np.uint64) * 3 + 11
    cents = x[:nlist].copy()
    now = 1000 * DAY
    is_recent = np.random.default_rng(270).random(n) < 0.3
    ts = np.where(is_recent, now - 1 * DAY, now - 30 * DAY)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=nlist, n_probe=8)

    ctx = fv.Context(0)
    hyb = fv.HybridIndex(ctx, hnsw_seed=19, **kw)
    hyb.set_ivf_centroids(cents)
    comm, used = sh.bring_up(ctx, dist, torch, "hosted", allow_hosted=True)
    assert used == "hosted"
    S = sh.ShardedHybrid(hyb, comm)
    S.bulk_insert(ids, x, ts, now)
    hyb.hnsw().scan_cutoff = 0  # the recent part by the masked traversal, as the oracle walks it after the deletes
    report["lists_owned"] = int((S.owner == rank).sum())

    pos = {int(v): i for i, v in enumerate(ids)}

    def oracle(allowed=None):
        # the WHOLE index on the CPU (same centroids, same graph); under an allow-set the complement is deleted
        o = orc.HybridIndex(**kw)
        o.set_ivf_centroids(cents)
        o.ivf().batch_insert(ids[~is_recent], x[~is_recent])
        gi, lv, off, nb_ = hyb.hnsw().export_graph()
        o.hnsw().restore(gi, x[[pos[int(g)] for g in gi]], lv, off, nb_, hyb.hnsw().entry_point())
        if allowed is not None:
            keep = set(int(i) for i in allowed)
            for i, rec in zip(ids, is_recent):
                if int(i) not in keep:
                    (o.hnsw() if rec else o.ivf()).mark_deleted(int(i))
        return o

    o = oracle()

    def same(res, q_rows, k, nprobe, orc_index=None):
        oi, od, oc = (orc_index or o).batch_search(q_rows, k, now=now, hnsw_ef=ef, ivf_n_probe=nprobe)
        if not (res.counts.shape[0] == q_rows.shape[0] and np.array_equal(res.counts, oc)):
            return False
        return all(np.array_equal(res.ids[b, : oc[b]], oi[b, : oc[b]]) and
                   np.array_equal(bits(res.distances[b, : oc[b]]), bits(od[b, : oc[b]])) for b in range(q_rows.shape[0]))

    own = [mixture(B, d, n_comp=40, sigma=0.6, seed=2900 + 10 * rank + j) for j in range(2)]
    own_dev = [ctx.upload(q) for q in own]
    glob = mixture(B, d, n_comp=40, sigma=0.6, seed=2990)
    gdev = ctx.upload(glob)
    per = -(-B // world)
    lo, hi = min(B, rank * per), min(B, (rank + 1) * per)

    # WEAK at k = 300: every rank brings its own batch
    res = S.search_dev(own_dev[0], B, 300, ef, 64, sh.WEAK)
    report["checks"].append(["weak_k300", bool(same(res, own[0], 300, 64) and np.all(res.counts > 256))])
    # STRONG at 257 probes: the ranking of the whole centroid table, split between the ranks and all-gathered
    res = S.search_dev(gdev, B, 10, ef, 257, sh.STRONG)
    report["checks"].append(["strong_nprobe257", bool(S.rows(B, sh.STRONG) == hi - lo and same(res, glob[lo:hi], 10, 257))])
    # WEAK under an allow-set: the same ids on every rank, each masking its own shard
    allowed = ids[np.random.default_rng(271).random(n) < 0.5]
    oa = oracle(allowed)
    ok = True
    for k, nprobe in ((300, 64), (10, 6)):
        res = S.search_dev(own_dev[1], B, k, ef, nprobe, sh.WEAK, allowed=allowed)
        ok = ok and same(res, own[1], k, nprobe, oa) and bool(np.isin(res.ids[res.ids != sh.NO_ID], allowed).all())
    report["checks"].append(["weak_allowed", bool(ok)])
    # a batch smaller than the world: rank 1's slice is empty, it still takes part in the exchanges
    res = S.search_dev(gdev, 1, 300, ef, 300, sh.STRONG)
    report["checks"].append(["strong_tiny", bool(res.counts.shape[0] == (1 if rank == 0 else 0) and
                                                 (rank != 0 or same(res, glob[:1], 300, 300)))])
    # two slots in flight, one through the existing route and one through the new
    S.search_dev_begin(0, own_dev[0], B, 10, ef, 6, sh.WEAK)
    S.search_dev_begin(1, own_dev[1], B, 300, ef, 64, sh.WEAK)
    ok = same(S.search_dev_end(0), own[0], 10, 6)
    ok = same(S.search_dev_end(1), own[1], 300, 64) and ok
    report["checks"].append(["in_flight", bool(ok)])

    report["ok"] = all(c[1] for c in report["checks"])
    json.dump(report, open(os.path.join(out_dir, f"rank{rank}.json"), "w"))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
