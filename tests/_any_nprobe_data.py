"""Data of the any-nprobe tests (test_any_nprobe_symbols.py checks the generators' conditions through the oracle alone,
test_gpu_any_nprobe.py runs them on the device).  Every index here has 300 lists: five centroid blocks, the last partial."""
import numpy as np

import oracle as orc
from _data import mixture

NLIST = 300
QUALITY_SEED = 4100
TIE_SEED = 4200


def f16_rounded(x):
    return x.astype(np.float16).astype(np.float32)


def main_case(d, seed):
    """3000 mixture rows, the first 300 of them the centroids."""
    x = mixture(3000, d, n_comp=40, seed=seed)
    ids = np.arange(x.shape[0], dtype=np.uint64) * 3 + 7
    return x, ids, x[:NLIST].copy()


def quality_case(seed=QUALITY_SEED, B=33):
    """main_case at d = 20 whose last 20 centroids repeat the first 20: a repeated centroid never wins an assignment (the
    lower index takes the tie), so lists 280..299 are empty, yet each ranks right behind its twin.  The first queries sit
    on those twins: their two nearest lists are a short list and an empty one."""
    x, ids, cents = main_case(20, seed)
    cents[280:] = cents[:20]
    q = mixture(B, 20, n_comp=40, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    m = min(8, B)
    q[:m] = cents[:m] + (rng.standard_normal((m, 20)) * 0.01).astype(np.float32)
    return x, ids, cents, q


def tie_case(seed=TIE_SEED, B=9):
    """Centroids, rows and queries on a coarse grid ({0, 0.5, 1}^8): equal distances everywhere.  Two pairs of identical
    centroids; every row stored twice, in two different lists (under two ids, so that the copies can be told apart):
    which copy comes first depends on the probe rank of its list, not on the list's index."""
    rng = np.random.default_rng(seed)
    d = 8
    grid = lambda n: (rng.integers(0, 3, (n, d)).astype(np.float32) * np.float32(0.5))  # noqa: E731
    cents = grid(NLIST)
    cents[200] = cents[10]
    cents[150] = cents[37]
    base = grid(1500)
    la = rng.integers(0, NLIST, 1500)
    lb = (la + 1 + rng.integers(0, NLIST - 1, 1500)) % NLIST
    assert np.all(la != lb)
    x = np.concatenate([base, base])
    cl = np.concatenate([la, lb]).astype(np.uint32)
    ids = np.arange(3000, dtype=np.uint64) + 1000
    order = rng.permutation(3000)
    x, cl, ids = np.ascontiguousarray(x[order]), np.ascontiguousarray(cl[order]), np.ascontiguousarray(ids[order])
    q = grid(B)
    q[0] = cents[10]
    q[1] = cents[37]
    return x, ids, cents, cl, q


def oracle_index(x, ids, cents, clusters=None, n_probe=4):
    """The oracle over these rows, and the list of every row (the oracle's own assignment unless given)."""
    cpu = orc.IVFIndex(n_clusters=cents.shape[0], n_probe=n_probe)
    cpu.set_trained(cents)
    cl = cpu.assign(x) if clusters is None else np.ascontiguousarray(clusters, np.uint32)
    cpu.batch_insert_assigned(ids, x, cl)
    return cpu, cl


def list_order_answer(x, ids, cl, q, k):
    """What a scan in list-index order keeps (fvdb_ivf_search_all): rows by (list, position), a stable sort by distance,
    the k first."""
    order = np.argsort(cl, kind="stable")
    out = np.empty((q.shape[0], k), np.uint64)
    for b in range(q.shape[0]):
        dist = orc.l2_batch(q[b], x[order])
        out[b] = ids[order][np.argsort(dist, kind="stable")[:k]]
    return out


def per_query_quality(res, truth, k):
    """recall and precision per query from two (ids, distances, counts) results, as src/ivf/operations.rs:357-377."""
    (ri, _, rc), (ti, _, tc) = res, truth
    f32 = np.float32
    recall, precision = np.empty(ri.shape[0], f32), np.empty(ri.shape[0], f32)
    for b in range(ri.shape[0]):
        result_ids = ri[b, : int(rc[b])].tolist()
        truth_ids = ti[b, : int(tc[b])].tolist()
        matches = 0
        for i in result_ids:
            if i in truth_ids:
                matches += 1
        recall[b] = f32(1.0) if len(truth_ids) == 0 else f32(matches) / f32(min(len(truth_ids), k))
        precision[b] = f32(0.0) if len(result_ids) == 0 else f32(matches) / f32(len(result_ids))
    return recall, precision


def averaged(values):
    """total += value in query order, then total / B, all in f32 (:379-387)."""
    total = np.float32(0.0)
    for v in values:
        total = np.float32(total + np.float32(v))
    return np.float32(total / np.float32(len(values)))


def expected_quality(cpu, q, k, n_probe):
    res = cpu.batch_search(q, k, n_probe)
    truth = cpu.batch_search(q, k, NLIST)
    recall, precision = per_query_quality(res, truth, k)
    return recall, precision, averaged(recall), averaged(precision)
