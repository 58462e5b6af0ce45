"""The counting rule of the quality grid, twice: as the device kernels compute it — split by
binary search, prefix counts — and by brute force — the stable merge of the two parts, then the reference's loop.

One query: G = (ids, distances) of the recent part, ascending; H = the historical part, ascending; T = the ids of the
exact result.  The hybrid result is the first L = min(k, |G| + |H|) entries of the stable merge, recent first on equal
distances (src/hybrid/core.rs:476-485)."""
import numpy as np


def split(gd, hd, L):
    """a = recent entries among the first L of the stable merge: entry a of G is inside iff
    a + #{h in H : d_h < d_G[a]} < L, which is monotone in a."""
    lo, hi = max(0, L - len(hd)), min(L, len(gd))
    while lo < hi:
        a = (lo + hi) // 2
        if a + int(np.searchsorted(hd, gd[a], side="left")) < L:
            lo = a + 1
        else:
            hi = a
    return lo


def prefix_hits(ids, truth):
    """f[x] = entries among the first x of `ids` whose id is in `truth` (x = 0 .. len(ids))"""
    t = np.sort(np.asarray(truth, np.uint64))
    ids = np.asarray(ids, np.uint64)
    at = np.searchsorted(t, ids)
    hit = (at < t.size) & (t[np.minimum(at, max(t.size - 1, 0))] == ids) if t.size else np.zeros(ids.size, bool)
    return np.concatenate([[0], np.cumsum(hit)]).astype(np.int64)


def figures(matches, n_truth, L, k):
    """recall, precision as f32: the divisions of search_quality_kernel"""
    f = np.float32
    recall = f(1) if n_truth == 0 else f(matches) / f(min(n_truth, k))
    precision = f(0) if L == 0 else f(matches) / f(L)
    return recall, precision


def rule(gi, gd, hi, hd, truth, k):
    """(recall, precision) f32 by the rule: one split, two prefix reads"""
    L = min(k, len(gi) + len(hi))
    a = split(np.asarray(gd, np.float32), np.asarray(hd, np.float32), L)
    matches = int(prefix_hits(gi, truth)[a] + prefix_hits(hi, truth)[L - a])
    return figures(matches, len(truth), L, k)


def brute(gi, gd, hi, hd, truth, k):
    """(recall, precision) f32 by the merge itself, and the merged ids"""
    ids = np.concatenate([np.asarray(gi, np.uint64), np.asarray(hi, np.uint64)])
    d = np.concatenate([np.asarray(gd, np.float32), np.asarray(hd, np.float32)])
    res = ids[np.argsort(d, kind="stable")[:k]]
    t = set(int(v) for v in truth)
    matches = sum(1 for v in res if int(v) in t)
    return figures(matches, len(truth), len(res), k), res


def grid_brute(truth, recent, hist, k):
    """Per-query figures of a whole grid by brute force.  truth = (ids [B][k], counts [B]); recent = (ids [E][B][rk], dist,
    counts [E][B]) or None; hist likewise with [P].  Returns recall, precision [max(E, 1)][max(P, 1)][B] f32."""
    t_ids, t_cnt = truth
    B = len(t_cnt)
    E = 0 if recent is None else recent[0].shape[0]
    P = 0 if hist is None else hist[0].shape[0]
    recall = np.zeros((max(E, 1), max(P, 1), B), np.float32)
    precision = np.zeros_like(recall)
    none = (np.zeros(0, np.uint64), np.zeros(0, np.float32))
    for i in range(max(E, 1)):
        for j in range(max(P, 1)):
            for b in range(B):
                g = (recent[0][i, b, :recent[2][i, b]], recent[1][i, b, :recent[2][i, b]]) if E else none
                h = (hist[0][j, b, :hist[2][j, b]], hist[1][j, b, :hist[2][j, b]]) if P else none
                (recall[i, j, b], precision[i, j, b]), _ = brute(g[0], g[1], h[0], h[1], t_ids[b, :min(int(t_cnt[b]), k)], k)
    return recall, precision


def summed(values):
    """the f32 sum in query order of per-query values [..., B], as the host mirror adds them"""
    out = np.zeros(values.shape[:-1], np.float32)
    for b in range(values.shape[-1]):
        out = (out + values[..., b]).astype(np.float32)
    return out
