"""GPU: fvdb_quality_grid_dev on caller-built blocks.  Every per-query recall and precision must
equal, as f32 bits, the brute-force restatement in _grid_ref.py: the stable merge of the two parts, recent first on equal
distances, then the reference's loop — itself checked against _exact_ref.host_quality in test_grid_ref.py.

Entries at or beyond a count hold poison (an id of the truth, a distance below every real one): a kernel that read them
would count a match or move the cut.  Shapes are the smallest at which the kernels can go wrong: k at both ends and on
both sides of 256, part widths that differ from k and from each other, lists shorter than their width, 64 x 64 points,
one query and more than two waves of them."""
import numpy as np
import pytest

import fvdb_import
from _data import bits
import _grid_ref as G

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = 6, 12
f = np.float32


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def run_grid(ctx, truth, recent, hist, k):
    """truth = (ids [B][k], counts [B]); recent / hist = (ids [n][B][w], dist, counts [n][B]) or None.  Returns the
    per-query recall and precision [max(E, 1)][max(P, 1)][B]."""
    B = len(truth[1])
    E = 0 if recent is None else recent[0].shape[0]
    P = 0 if hist is None else hist[0].shape[0]
    rk = recent[0].shape[2] if E else 0
    hk = hist[0].shape[2] if P else 0
    held = []

    def dev(a, dtype):
        held.append(ctx.upload(np.ascontiguousarray(a, dtype)))
        return held[-1]

    def part(p):
        return (None, None, None) if p is None else (dev(p[0], np.uint64), dev(p[1], np.float32), dev(p[2], np.uint32))

    n = max(E, 1) * max(P, 1) * B
    out = (ctx.alloc(n * 4), ctx.alloc(n * 4))
    try:
        ctx.check(ctx.lib.fvdb_quality_grid_dev(ctx.h, dev(truth[0], np.uint64), dev(truth[1], np.uint32), *part(recent), *part(hist),
                                                B, k, rk, hk, E, P, *out))
        ctx.synchronize()
        shape = (max(E, 1), max(P, 1), B)
        return ctx.download(out[0], shape, np.float32), ctx.download(out[1], shape, np.float32)
    finally:
        for p in held + list(out):
            ctx.free(p)


def same(got, want, what):
    for name, g, w in (("recall", got[0], want[0]), ("precision", got[1], want[1])):
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, f"{what}: {name} differs at (i, j, query) {bad[:4].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"


# ---- hand-built cases, one query each (B = 1) --------------------------------------------------------------------------
def one(gi, gd, hi, hd, truth, k, rk=None, hk=None):
    """blocks of one query from plain lists; the parts are padded to rk / hk with poison"""
    def block(ids, dist, width):
        if width is None:
            return None
        i = np.full((1, 1, width), truth[0] if len(truth) else 0, np.uint64)
        d = np.full((1, 1, width), -1.0, np.float32)
        i[0, 0, :len(ids)], d[0, 0, :len(ids)] = ids, dist
        return i, d, np.array([[len(ids)]], np.uint32)
    t = np.full((1, k), 0xDEAD, np.uint64)
    t[0, :len(truth)] = truth
    return (t, np.array([len(truth)], np.uint32)), block(gi, gd, rk), block(hi, hd, hk)


HAND = {
    # equal distances across the parts exactly at the cut: the recent entry is in, the historical one is out
    "tie_at_cut_truth_recent": (one([1], [2.0], [2], [2.0], [1], 1, 1, 1), 1, (f(1), f(1))),
    "tie_at_cut_truth_hist": (one([1], [2.0], [2], [2.0], [2], 1, 1, 1), 1, (f(0), f(0))),
    "tie_at_cut_longer": (one([1, 3, 5], [1.0, 2.0, 2.0], [2, 4], [2.0, 2.0], [4, 5], 3, 3, 2), 3, (f(1) / f(2), f(1) / f(3))),
    # a migrated row: one id in both parts at the same distance; k = 1 holds it once, k = 2 twice
    "migrated_once": (one([7], [1.0], [7], [1.0], [7], 1, 1, 1), 1, (f(1), f(1))),
    "migrated_twice": (one([7], [1.0], [7], [1.0], [7], 2, 1, 1), 2, (f(2), f(1))),
    # an id twice in the truth
    "truth_twice": (one([7, 8], [1.0, 2.0], [9], [3.0], [7, 7], 2, 2, 1), 2, (f(1) / f(2), f(1) / f(2))),
    # empty truth: recall is 1
    "empty_truth": (one([3], [1.0], [4], [2.0], [], 4, 2, 2), 4, (f(1), f(0))),
    # both parts empty: precision 0, recall 0 unless the truth is empty too
    "empty_parts": (one([], [], [], [], [5], 4, 2, 3), 4, (f(0), f(0))),
    "empty_everything": (one([], [], [], [], [], 4, 2, 3), 4, (f(1), f(0))),
    # counts shorter than rk / hk, rk != hk != k with rk > k
    "short_counts": (one([1, 2, 3], [1.0, 2.0, 3.0], [4], [2.5], [2, 4, 3], 3, 6, 4), 3, (f(2) / f(3), f(2) / f(3))),
    # +inf distances: a recent +inf goes before a historical +inf
    "inf": (one([1, 2], [1.0, np.inf], [3, 4], [np.inf, np.inf], [2, 3], 3, 2, 2), 3, (f(1), f(2) / f(3))),
    "inf_cut": (one([1, 2], [1.0, np.inf], [3, 4], [np.inf, np.inf], [3], 2, 2, 2), 2, (f(0), f(0))),
    # the truth holds more ids than k counts: min(len(truth), k) divides
    "k_below_parts": (one([1, 2, 3, 4], [1.0, 2.0, 3.0, 4.0], [5, 6], [0.5, 9.0], [5, 1, 2], 3, 4, 2), 3, (f(1), f(1))),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_cases(ctx, name):
    (truth, recent, hist), k, want = HAND[name]
    recall, precision = run_grid(ctx, truth, recent, hist, k)
    print(f"{name}: recall={recall.ravel()} precision={precision.ravel()} want={want}")
    same((recall, precision), G.grid_brute(truth, recent, hist, k), name)
    assert (recall[0, 0, 0], precision[0, 0, 0]) == want, name


# ---- seeded blocks at the shapes that matter ---------------------------------------------------------------------------
def random_blocks(seed, B, k, rk, hk, E, P, id_range, levels=6):
    rng = np.random.default_rng(seed)
    t_cnt = rng.integers(0, k + 1, B).astype(np.uint32)
    t_cnt[0] = k
    if B > 2:
        t_cnt[1] = 0
    t_ids = rng.integers(0, id_range, (B, k)).astype(np.uint64)  # repeats inside the truth happen

    def part(n, width):
        if n == 0:
            return None
        d = rng.integers(0, levels, (n, B, width)).astype(np.float32)  # few distinct distances: ties everywhere
        d[d == levels - 1] = np.inf
        d.sort(axis=2)
        ids = rng.integers(0, id_range, (n, B, width)).astype(np.uint64)
        cnt = rng.integers(0, width + 1, (n, B)).astype(np.uint32)
        cnt[0, 0] = width
        cnt[rng.random((n, B)) < 0.1] = 0
        for i in range(n):  # poison beyond the counts: an id of the truth at a distance below every real one
            for b in range(B):
                ids[i, b, cnt[i, b]:] = t_ids[b, 0]
                d[i, b, cnt[i, b]:] = -1.0
        return ids, d, cnt

    return (t_ids, t_cnt), part(E, rk), part(P, hk)


SHAPES = {
    # B, k, rk, hk, E, P, id range
    "k1_one_query": (1, 1, 1, 1, 1, 1, 3),
    "widths_differ_rk_above_k": (130, 5, 7, 3, 2, 3, 12),
    "six_by_six_130_queries": (130, 10, 10, 10, 6, 6, 40),
    "k256": (3, 256, 256, 256, 2, 2, 600),
    "k257": (3, 257, 257, 257, 2, 2, 600),
    "k4096": (2, 4096, 4096, 4096, 2, 2, 9000),
    "k4096_short_truth_wide_parts": (2, 100, 4096, 4095, 1, 2, 400),
    "grid_64_by_64": (5, 3, 3, 3, 64, 64, 8),
    "graph_only": (67, 10, 12, 0, 3, 0, 30),
    "list_only": (67, 10, 0, 12, 0, 3, 30),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_seeded_blocks_equal_the_brute_force_merge(ctx, name):
    B, k, rk, hk, E, P, id_range = SHAPES[name]
    truth, recent, hist = random_blocks(len(name) + B, B, k, rk, hk, E, P, id_range, levels=6 if k < 100 else 40)
    got = run_grid(ctx, truth, recent, hist, k)
    want = G.grid_brute(truth, recent, hist, k)
    print(f"{name}: mean recall {got[0].mean():.4f} precision {got[1].mean():.4f}; "
          f"recall values {np.unique(got[0]).size}, precision values {np.unique(got[1]).size}")
    same(got, want, name)
    assert got[0].shape == (max(E, 1), max(P, 1), B)
    if B > 1 and k > 1:
        assert np.unique(want[0]).size > 2, "the case does not exercise the count"


def test_refusals(ctx):
    truth, recent, hist = random_blocks(3, 4, 5, 5, 5, 2, 2, 10)
    B, k = 4, 5
    bufs = [ctx.upload(a) for a in (*truth, *recent, *hist)]
    out = (ctx.alloc(4 * B * 4), ctx.alloc(4 * B * 4))
    t, r, h = bufs[:2], bufs[2:5], bufs[5:]
    call = ctx.lib.fvdb_quality_grid_dev
    none = (None, None, None)
    try:
        assert call(None, *t, *r, *h, B, k, k, k, 2, 2, *out) == E_INVALID
        assert call(ctx.h, None, t[1], *r, *h, B, k, k, k, 2, 2, *out) == E_INVALID
        assert call(ctx.h, *t, *r, *h, B, k, k, k, 2, 2, None, out[1]) == E_INVALID
        assert call(ctx.h, *t, *none, *none, B, k, k, k, 0, 0, *out) == E_INVALID
        assert call(ctx.h, *t, *none, *h, B, k, k, k, 2, 2, *out) == E_INVALID
        assert call(ctx.h, *t, *r, h[0], None, h[2], B, k, k, k, 2, 2, *out) == E_INVALID
        for bad in (0, 4097):
            assert call(ctx.h, *t, *r, *h, B, bad, k, k, 2, 2, *out) == E_UNSUPPORTED
            assert call(ctx.h, *t, *r, *h, B, k, bad, k, 2, 2, *out) == E_UNSUPPORTED
            assert call(ctx.h, *t, *r, *h, B, k, k, bad, 2, 2, *out) == E_UNSUPPORTED
        assert call(ctx.h, *t, *r, *h, B, k, k, k, 65, 2, *out) == E_UNSUPPORTED
        assert call(ctx.h, *t, *r, *h, B, k, k, k, 2, 65, *out) == E_UNSUPPORTED
        # a part that is absent: its width and its pointers are not looked at
        assert call(ctx.h, *t, *r, *none, B, k, k, 0, 2, 0, *out) == 0
        assert call(ctx.h, *t, *none, *h, B, k, 0, k, 0, 2, *out) == 0
        assert call(ctx.h, *t, *r, *h, 0, k, k, k, 2, 2, *out) == 0  # B = 0 writes nothing
        ctx.synchronize()
    finally:
        for p in bufs + list(out):
            ctx.free(p)
