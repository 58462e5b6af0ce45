"""The numpy restatement of the reference's distance and of the exact-search result rule, shared by
test_exact_search_symbols.py (which proves it against the oracle, on the CPU) and test_gpu_exact_search.py (which
leans on it).  Distance: a loop over i of acc = acc + t * t on float32 arrays, t = q_i - x_i, then np.sqrt in f32 — one
rounding per operation, no fused multiply-add.  Order: np.lexsort((node, distance_bits))."""
import numpy as np

NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)


def fold_distances(q, x):
    """[B, n] f32 distances of the f32 queries q [B, d] to the f32 rows x [n, d]."""
    q = np.ascontiguousarray(q, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    acc = np.zeros((q.shape[0], x.shape[0]), np.float32)
    xt = np.ascontiguousarray(x.T)
    for i in range(q.shape[1]):
        t = q[:, i:i + 1] - xt[i][None, :]
        acc = acc + t * t
    assert acc.dtype == np.float32
    return np.sqrt(acc)


def exact_topk(dist, k, live=None, ids=None):
    """(ids [B, k] u64, distances [B, k] f32, counts [B] u32): the k best live nodes of every query by distance bits,
    then node index; the unused tail is NO_ID / +inf.  live: bool [n] (None = all); ids: node -> id (None = the index)."""
    B, n = dist.shape
    nodes = np.arange(n) if live is None else np.flatnonzero(live)
    out_i = np.full((B, k), NO_ID, np.uint64)
    out_d = np.full((B, k), np.inf, np.float32)
    cnt = np.full(B, min(k, nodes.size), np.uint32)
    for b in range(B):
        db = np.ascontiguousarray(dist[b, nodes]).view(np.uint32)
        order = np.lexsort((nodes, db))[:k]
        pick = nodes[order]
        out_i[b, :pick.size] = pick if ids is None else ids[pick]
        out_d[b, :pick.size] = dist[b, pick]
    return out_i, out_d, cnt


def rounded(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def with_duplicates(x, pairs):
    """x with row dst overwritten by row src for every (src, dst) in pairs"""
    x = x.copy()
    for src, dst in pairs:
        x[dst] = x[src]
    return x


def merge_parts(parts, k):
    """The hybrid merge of one query (src/hybrid/core.rs:476-485): concatenate the (ids, distances) parts in order, stable
    sort by distance, truncate to k.  No de-duplication."""
    ids = np.concatenate([p[0] for p in parts])
    d = np.concatenate([p[1] for p in parts])
    order = np.argsort(d, kind="stable")[:k]
    return ids[order], d[order]


def host_quality(res, truth, k):
    """avg_recall, avg_precision as f32, from two SearchResults, by the reference's loop (src/ivf/operations.rs:357-377):
    per-query f32 values summed in query order in f32."""
    tr = tp = np.float32(0)
    B = len(res.counts)
    for b in range(B):
        r = res.ids[b, :int(res.counts[b])]
        t = set(int(v) for v in truth.ids[b, :int(truth.counts[b])])
        matches = sum(1 for v in r if int(v) in t)
        recall = np.float32(1) if not t else np.float32(matches) / np.float32(min(int(truth.counts[b]), k))
        precision = np.float32(0) if r.size == 0 else np.float32(matches) / np.float32(r.size)
        tr = np.float32(tr + recall)
        tp = np.float32(tp + precision)
    return np.float32(tr / np.float32(B)), np.float32(tp / np.float32(B))
