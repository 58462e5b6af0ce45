"""The numpy restatement of the diverse selection, shared by test_mmr_ref.py (which proves the
hand-built cases' properties, on the CPU) and the GPU tests (which lean on it).  Distances between rows come from
_exact_ref.fold_distances — acc = acc + t * t over ascending dimensions in f32, then sqrt — and the gain is
b * m - a * dq with every operation on np.float32 values: two multiplies and one subtract, each rounded once."""
import numpy as np

import _exact_ref as R

NO_ID = R.NO_ID
NO_ROW = np.uint32(0xFFFFFFFF)
INF = np.float32(np.inf)


def kept_mask(ids, n, distinct):
    """kept[c] for c < n: with distinct, False where an earlier candidate has the same id"""
    kept = np.zeros(len(ids), bool)
    seen = set()
    for c in range(n):
        if distinct and int(ids[c]) in seen:
            continue
        seen.add(int(ids[c]))
        kept[c] = True
    return kept


def mmr_one(ids, dq, rows, n, k, lam, distinct, ties=None, pair=None):
    """The picks of one query, in pick order: a list of candidate positions.  ties: a list that receives, per round
    after the first, how many open candidates share the maximal gain.  pair: fold_distances(rows, rows) where the
    caller already holds it (the same bits: (x - y)^2 = (y - x)^2), so that many settings share one fold."""
    a = np.float32(lam)
    b = np.float32(np.float32(1) - a)
    kept = kept_mask(ids, n, distinct)
    open_ = np.flatnonzero(kept).tolist()
    if not open_:
        return []
    picks = [open_.pop(0)]
    m = np.full(len(ids), INF, np.float32)
    dq = np.asarray(dq, np.float32)
    while open_ and len(picks) < k:
        s = picks[-1]
        c = np.asarray(open_)
        t = R.fold_distances(rows[s][None, :], rows[c])[0] if pair is None else pair[s, c]
        m[c] = np.minimum(m[c], t)
        gain = (b * m[c]).astype(np.float32) - (a * dq[c]).astype(np.float32)
        assert gain.dtype == np.float32
        best = int(np.flatnonzero(gain == gain.max())[0])  # the smallest c among equal gains: c ascends
        if ties is not None:
            ties.append(int((gain == gain.max()).sum()))
        picks.append(open_.pop(best))
    return picks


def mmr_brute(ids, dq, rows, n, k, lam, distinct):
    """The same definition written a second time, on its own: every round recomputes each m from scratch as the
    minimum over ALL picks so far, from a distance matrix folded once, with scalar f32 arithmetic."""
    one, a = np.float32(1), np.float32(lam)
    b = np.float32(one - a)
    dq = np.asarray(dq, np.float32)
    kept = [c for c in range(n) if not distinct or all(int(ids[e]) != int(ids[c]) for e in range(c))]
    if not kept:
        return []
    pair = R.fold_distances(rows[:n], rows[:n])  # pair[s, c] = dist(x_c, x_s): (x - y)^2 = (y - x)^2 bit for bit
    picks = [kept[0]]
    while len(picks) < min(k, len(kept)):
        best, best_gain = None, None
        for c in kept:
            if c in picks:
                continue
            m = min(np.float32(pair[s, c]) for s in picks)
            gain = np.float32(np.float32(b * m) - np.float32(a * dq[c]))
            if best is None or gain > best_gain:
                best, best_gain = c, gain
        picks.append(best)
    return picks


def mmr_answer(ids, dq, rows, counts, k, lam, distinct, pairs=None):
    """(ids [B, k] u64, distances [B, k] f32, ranks [B, k] u32, counts [B] u32) for ids / dq [B, fetch_k],
    rows [B, fetch_k, d] and counts [B]; tails NO_ID / +inf / NO_ROW.  pairs: per query, mmr_one's `pair`."""
    B, fetch_k = ids.shape
    out_i = np.full((B, k), NO_ID, np.uint64)
    out_d = np.full((B, k), INF, np.float32)
    out_r = np.full((B, k), NO_ROW, np.uint32)
    out_c = np.zeros(B, np.uint32)
    for b in range(B):
        n = min(int(counts[b]), fetch_k)
        picks = mmr_one(ids[b], dq[b], rows[b], n, k, lam, distinct, pair=None if pairs is None else pairs[b])
        out_c[b] = len(picks)
        out_i[b, :len(picks)] = ids[b, picks]
        out_d[b, :len(picks)] = dq[b, picks]
        out_r[b, :len(picks)] = picks
    return out_i, out_d, out_r, out_c


# ---- hand-built inputs (one query each): (ids [n] u64, dq [n] f32, rows [n, d] f32) ----------------------------------
def nearest_first(q, rows, ids):
    """the candidates as a search returns them: by (distance bits, position)"""
    dq = R.fold_distances(q[None, :], rows)[0]
    order = np.lexsort((np.arange(len(ids)), dq.view(np.uint32)))
    return np.ascontiguousarray(ids[order]), np.ascontiguousarray(dq[order]), np.ascontiguousarray(rows[order])


def random_case(n, d, seed, f16=False):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal(d).astype(np.float32)
    if f16:
        rows = R.rounded(rows)
    return nearest_first(q, rows, np.arange(1000, 1000 + n, dtype=np.uint64))


def lattice_case(n, d, seed):
    """small-integer rows and query: many equal distances, so gains tie at lam 0 and 1"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-1, 2, (n, d)).astype(np.float32)
    q = np.zeros(d, np.float32)
    return nearest_first(q, rows, np.arange(n, dtype=np.uint64))


def twins_case(n, d, seed):
    """the same row stored under different ids, in pairs: equal dq, and equal m against every pick — gains tie at any lam"""
    rng = np.random.default_rng(seed)
    half = rng.standard_normal(((n + 1) // 2, d)).astype(np.float32)
    rows = np.repeat(half, 2, axis=0)[:n]
    q = rng.standard_normal(d).astype(np.float32)
    return nearest_first(q, rows, np.arange(500, 500 + n, dtype=np.uint64))


def identical_case(n, d):
    """all rows identical under different ids: every distance between rows is 0"""
    rows = np.tile(np.linspace(-1, 1, d, dtype=np.float32), (n, 1))
    q = np.zeros(d, np.float32)
    return nearest_first(q, rows, np.arange(n, dtype=np.uint64))


def with_repeats(case, where):
    """ids with copies: for (src, dst) in where, candidate dst becomes a copy (id, dq, row) of candidate src, as the hybrid
    index returns a migrated row twice; the list is re-sorted as a search would return it"""
    ids, dq, rows = (a.copy() for a in case)
    for src, dst in where:
        ids[dst], dq[dst], rows[dst] = ids[src], dq[src], rows[src]
    order = np.lexsort((np.arange(len(ids)), dq.view(np.uint32)))
    return ids[order], dq[order], rows[order]


def tie_rounds(case, k, lam, distinct):
    ties = []
    ids, dq, rows = case
    mmr_one(ids, dq, rows, len(ids), k, lam, distinct, ties)
    return sum(1 for t in ties if t > 1)
