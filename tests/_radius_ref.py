"""The numpy restatement of the radius search's result, on _exact_ref's distance and order: the
ball of a query is the live rows whose distance word is <= the radius word (non-negative f32 bits are monotone as
u32; the boundary is inclusive; a NaN distance is in no ball), total its size, and the results its first min(total, m)
rows by (distance bits, node index) — exact_topk(k = m) over the ball.  test_radius_ref.py proves on the CPU the
properties of the hand-built cases that the GPU tests lean on."""
import numpy as np

import _exact_ref as R

NO_ID = R.NO_ID


def word(r):
    """the bit pattern of an f32 value"""
    return int(np.array(r, np.float32).view(np.uint32))


def below(r):
    """the f32 value just below r > 0"""
    return np.nextafter(np.float32(r), np.float32(-np.inf))


def in_ball(dist, radius):
    """bool [B, n]: bits(dist) <= bits(radius[b]); radius: a scalar or [B], every entry >= 0 (+inf allowed)"""
    dist = np.ascontiguousarray(dist, np.float32)
    r = np.broadcast_to(np.asarray(radius, np.float32).reshape(-1, 1), (dist.shape[0], 1))
    assert np.all(r >= 0), "a radius is >= 0"
    cut = np.ascontiguousarray(r + np.float32(0)).view(np.uint32)  # -0.0 + 0.0 = +0.0
    return dist.view(np.uint32) <= cut


def radius_answer(dist, radius, m, live=None, ids=None):
    """(ids [B, m] u64, distances [B, m] f32, counts [B] u32, totals [B] u32) for the distances dist [B, n]"""
    B, n = dist.shape
    ball = in_ball(dist, radius)
    if live is not None:
        ball = ball & np.asarray(live, bool)[None, :]
    out_i = np.full((B, m), NO_ID, np.uint64)
    out_d = np.full((B, m), np.inf, np.float32)
    cnt = np.zeros(B, np.uint32)
    for b in range(B):
        i, d, c = R.exact_topk(dist[b:b + 1], m, live=ball[b], ids=ids)
        out_i[b], out_d[b], cnt[b] = i[0], d[0], c[0]
    return out_i, out_d, cnt, ball.sum(1).astype(np.uint32)


def kth_distance(dist, k):
    """[B] f32: the k-th nearest distance of every query (k counted from 1)"""
    return np.sort(np.ascontiguousarray(dist, np.float32), axis=1)[:, k - 1].copy()
