"""Shared by tests/test_gpu_hybrid_groups.py and its child processes: a small hybrid index whose recent part holds
duplicated rows, the query batches, and the scenarios of grouped begin/end.  Every scenario
compares ids, hit counts and distance bits with the blocking search_dev of the same batch on the same index, and counts
the traversal launches (graph_kernel_times, profiling on) against what the group size in force must give.  Run as a
program it runs every scenario in THIS process, whose environment decides FVDB_HYBRID_GROUP / FVDB_HYBRID_PAIR (read
once by the library); the sizes it must see are on the command line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from _data import bits, mixture  # noqa: E402

DAY = 86400.0
NOW = 1000 * DAY
N, D, NLIST, NPROBE, K, EF = 3000, 32, 16, 4, 5, 8
KW = dict(now=NOW, hnsw_ef=EF, ivf_n_probe=NPROBE, dim=D)
SIZES = (1, 5, 64, 33, 20, 47)


class Env:
    pass


def make_env(fv, gw, gc, d=D, device=True):
    """3000 x d rows, 40 % recent, 16 lists.  Every fourth recent row is a copy of the recent row before it, so that a
    walk meets equal distances and some queries take the tie restart.  gw, gc: the group sizes the library has in force.
    Walks are grouped only where the graph's slots run them as device kernels: not at a d that is no multiple of 4
    (the engine serves padded rows in slot 0 alone) and not under the host walk (device=False); there every batch's
    walk goes alone, from its own query buffer."""
    e = Env()
    e.fv, e.gc, e.device = fv, gc, device
    e.gw = gw if device and d % 4 == 0 else 1
    e.kw = dict(KW, dim=d)
    e.ctx = fv.Context(0)
    x = mixture(N, d, n_comp=12, seed=411)
    recent = np.random.default_rng(412).random(N) < 0.4
    r = np.flatnonzero(recent)
    x[r[3::4]] = x[r[2::4][: len(r[3::4])]]
    ts = np.where(recent, NOW - 1 * DAY, NOW - 30 * DAY)
    e.g = fv.HybridIndex(e.ctx, max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=NLIST,
                         n_probe=NPROBE, hnsw_seed=11)
    e.g.set_ivf_centroids(x[:NLIST].copy())
    e.g.set_sequential_graph(True)
    e.g.bulk_insert(np.arange(N, dtype=np.uint64), x, ts, NOW)
    e.x = x
    rng = np.random.default_rng(413)
    # queries ON rows of the index: a duplicated recent row is then at distance 0 twice
    e.q = [x[rng.integers(0, N, B)].copy() for B in SIZES]
    e.qdev = [e.ctx.upload(q) for q in e.q]
    e.hnsw = e.g.hnsw()
    e.hnsw.set_device_traversal(device)
    e.ctx.set_profiling(2)
    t0 = e.hnsw.tie_restarts()
    e.want = [e.g.search_dev(e.qdev[j], B, K, **e.kw) for j, B in enumerate(SIZES)]  # once, shared, never changed
    t1 = e.hnsw.tie_restarts()
    e.alone = (t1[0] - t0[0], t1[1] - t0[1])  # (queries, restarts) of the six batches searched one by one
    e.rows = []
    for j, B in enumerate(SIZES):
        e.g.search_dev(e.qdev[j], B, K, **e.kw)
        e.rows.append(e.g.ivf().last_stats()["rows_scanned"])
    return e


def same(got, want):
    assert np.array_equal(got.counts, want.counts)
    assert np.array_equal(got.ids, want.ids)
    assert np.array_equal(bits(got.distances), bits(want.distances))


def begin(e, slot, j, **kw):
    e.g.search_dev_begin(slot, e.qdev[j], SIZES[j], kw.pop("k", K), **dict(e.kw, **kw))


def launches(e):
    return e.hnsw.graph_kernel_times()[1]


def expect_launches(e, n):
    """n compatible batches begun back to back, then collected: full groups, and one launch for what is left; the host
    walk launches nothing."""
    g = e.gw
    return 0 if not e.device else n if g == 1 else n // g + (1 if n % g else 0)


def check_launches(e, n):
    """Not at a padded dimension: there a batch begun in slot 0 is walked again when a later slot's end, which has to
    search in slot 0, gets there first (so in this commit's parent too), and the count depends on the order of the ends."""
    got = launches(e)
    if e.x.shape[1] % 4 == 0:
        assert got == expect_launches(e, n)


def s_reference(e):
    assert e.g.recent_count() > 900 and e.g.historical_count() > 1500
    if e.device:
        assert e.alone[0] == sum(SIZES) and e.alone[1] > 0  # the duplicates do bring tie restarts
    assert e.g.hnsw().device_fallbacks() == 0
    assert all(r > 0 for r in e.rows[2:])


def s_groups_of_unequal_batches(e):
    for js in ((0, 1), (2, 3), (0, 1, 2, 3), (3, 2, 1, 0)):
        launches(e)
        t0 = e.hnsw.tie_restarts()
        for slot, j in enumerate(js):
            begin(e, slot, j)
        got = [e.g.search_dev_end(slot) for slot in range(len(js))]
        for r, j in zip(got, js):
            same(r, e.want[j])
        check_launches(e, len(js))
        if len(js) == e.gc:
            assert e.g.ivf().last_stats()["rows_scanned"] == sum(e.rows[j] for j in js)
        t1 = e.hnsw.tie_restarts()
        assert t1[0] - t0[0] == (sum(SIZES[j] for j in js) if e.device else 0)


def s_tie_restarts_add_up(e):
    # all six batches in flight, grouped as the sizes say: the restart counter moves as for the batches one by one
    t0 = e.hnsw.tie_restarts()
    for j in range(len(SIZES)):
        begin(e, j, j)
    for j in reversed(range(len(SIZES))):
        same(e.g.search_dev_end(j), e.want[j])
    t1 = e.hnsw.tie_restarts()
    assert (t1[0] - t0[0], t1[1] - t0[1]) == e.alone
    assert e.g.hnsw().device_fallbacks() == 0


def s_incomplete_groups(e):
    launches(e)
    begin(e, 0, 2)
    same(e.g.search_dev_end(0), e.want[2])
    check_launches(e, 1)
    for slot, j in enumerate((2, 3, 5)):
        begin(e, slot, j)
    for slot, j in reversed(list(enumerate((2, 3, 5)))):
        same(e.g.search_dev_end(slot), e.want[j])
    check_launches(e, 3)


def s_launching_slot_reused(e):
    # the slot that completes a group is collected and begun again with other queries before its partners are collected
    import itertools
    n = max(e.gw, 2)
    for order in itertools.permutations(range(n - 1)):
        js = (2, 3, 4, 5)[:n]
        for slot, j in enumerate(js):
            begin(e, slot, j)
        last = n - 1
        same(e.g.search_dev_end(last), e.want[js[last]])
        begin(e, last, 1)                      # waits, or goes alone: other queries in the launcher's slot
        begin(e, n, 0)                         # a further batch, so that the launcher's walk is in flight again at size 2
        for slot in order:
            same(e.g.search_dev_end(slot), e.want[js[slot]])
        same(e.g.search_dev_end(last), e.want[1])
        same(e.g.search_dev_end(n), e.want[0])


def s_begin_that_cannot_join(e):
    g = e.g
    others = [dict(hnsw_ef=EF + 4), dict(k=3), dict(search_recent=False), dict(search_historical=False)]
    for other in others:
        k2 = other.get("k", K)
        kw = {x: v for x, v in other.items() if x != "k"}
        want_b = g.search_dev(e.qdev[3], SIZES[3], k2, **dict(e.kw, **kw))
        begin(e, 0, 2)
        begin(e, 1, 3, **other)
        ra, rb = g.search_dev_end(0), g.search_dev_end(1)
        same(ra, e.want[2])
        same(rb, want_b)
        begin(e, 0, 2)
        begin(e, 1, 3, **other)
        rb, ra = g.search_dev_end(1), g.search_dev_end(0)
        same(ra, e.want[2])
        same(rb, want_b)
    # an allow-set comes through the blocking search: what waits is enqueued first
    allowed = np.arange(0, N, 3, dtype=np.uint64)
    want_f = g.search_allowed(e.q[3], K, allowed, now=NOW, hnsw_ef=EF, ivf_n_probe=NPROBE)
    begin(e, 0, 2)
    same(g.search_allowed(e.q[3], K, allowed, now=NOW, hnsw_ef=EF, ivf_n_probe=NPROBE), want_f)
    assert np.isin(want_f.ids[want_f.ids != np.uint64(2 ** 64 - 1)], allowed).all()
    same(g.search_dev(e.qdev[5], SIZES[5], K, **e.kw), e.want[5])
    same(g.search_dev_end(0), e.want[2])


def s_mutation_is_refused(e):
    import threading
    g = e.g
    begin(e, 0, 2)  # waits
    try:
        g.insert_with_timestamp(10 ** 9, e.x[0] + 1, NOW, NOW)
        raise AssertionError("insert accepted while a batch waits")
    except e.fv.FvdbError:
        pass
    begin(e, 1, 3)
    begin(e, 2, 4)
    begin(e, 3, 5)  # groups of up to four are running now
    try:
        g.delete(5)
        raise AssertionError("delete accepted while groups run")
    except e.fv.FvdbError:
        pass
    for slot, j in enumerate((2, 3, 4, 5)):
        same(g.search_dev_end(slot), e.want[j])
    # under set_blocking_writers the writer waits for the collection; the row it adds is far from every query
    g.set_blocking_writers(True)
    begin(e, 0, 2)
    begin(e, 1, 3)
    done = []
    far = np.full(e.x.shape[1], 1000.0, np.float32)
    t = threading.Thread(target=lambda: done.append(g.insert_with_timestamp(10 ** 9 + 1, far, NOW - 30 * DAY, NOW)))
    t.start()
    same(g.search_dev_end(1), e.want[3])
    assert not done
    same(g.search_dev_end(0), e.want[2])
    t.join(30)
    assert len(done) == 1
    g.set_blocking_writers(False)
    same(g.search_dev(e.qdev[2], SIZES[2], K, **e.kw), e.want[2])


def s_pipelined(e):
    js = (2, 3, 5, 4, 1)
    for depth in (1, 2, 3, 5, 8):
        out = [None] * 16
        for i in range(16):
            begin(e, i % depth, js[i % 5])
            if i >= depth - 1:
                out[i - depth + 1] = e.g.search_dev_end((i - depth + 1) % depth)
        for i in range(max(16 - depth + 1, 0), 16):
            out[i] = e.g.search_dev_end(i % depth)
        for i, r in enumerate(out):
            same(r, e.want[js[i % 5]])


SCENARIOS = [s_reference, s_groups_of_unequal_batches, s_tie_restarts_add_up, s_incomplete_groups, s_launching_slot_reused,
             s_begin_that_cannot_join, s_pipelined, s_mutation_is_refused]  # the mutation last: it adds a row


if __name__ == "__main__":
    import fvdb_import
    env = make_env(fvdb_import.load(), int(sys.argv[1]), int(sys.argv[2]))
    for s in SCENARIOS:
        s(env)
        print("ok", s.__name__, flush=True)
