"""GPU: what every graph-search entry point of the host mirror answers BEFORE it reaches the device, and the begin/end
protocol.

The expected values are the table of section 9l, read from the code as it stood when the entry points were still eleven
separate functions; they are not whatever the present code returns.  Each raw call goes through the class's own library
handle and error mapping (`_check`, `exc.status`) into buffers that start out holding sentinels, so that "filled empty"
(counts 0, ids NO_ID, distances +inf) and "untouched" can be told apart.

Shape: a graph of 64 rows, d = 8, default config; a second index that stays empty; a third whose entry point was
vacuumed away; a hybrid index of 64 rows.  Nothing here depends on a kernel's tiling — the kernels have their own tests."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture
import _exact_ref as R

pytestmark = pytest.mark.gpu

OK, E_DIM, E_INVALID, E_NOT_FOUND, E_UNSUPPORTED = 0, 3, 6, 7, 12
MAX_K = 256
N, D, EF = 64, 8, 32
DAY = 86400.0
NOW = 1000 * DAY
NO_ID = R.NO_ID
S_ID, S_DIST, S_COUNT = np.uint64(0xABABABABABABABAB), np.float32(-7.0), np.uint32(77)
u64p, f32p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    x = mixture(N, D, n_comp=4, seed=9101)
    ids = np.arange(N, dtype=np.uint64) + 100
    q = mixture(5, D, n_comp=4, seed=9102)
    return x, ids, q


def graph(fv, ctx, x, ids):
    g = fv.HNSWIndex(ctx, seed=3)
    assert g.batch_insert(ids, x) == (len(ids), 0)
    return g


@pytest.fixture(scope="module")
def g(fv, ctx, data):
    return graph(fv, ctx, data[0], data[1])


@pytest.fixture(scope="module")
def empty(fv, ctx):
    return fv.HNSWIndex(ctx, seed=3)


def raw(idx, name, q, B, dim, k, *mid):
    """fvh_<name>(h, q, B, dim, k, *mid, ids, dist, counts) -> (status, "empty" | "untouched" | "results", SearchResults).
    The buffers always hold at least one row, so B = 0 and k = 0 pass valid addresses; the state is judged on the B x k
    block and the B counts (with B = 0 there is nothing to judge: None)."""
    rows, cols = max(B, 1), max(k, 1)
    ids = np.full((rows, cols), S_ID, np.uint64)
    dist = np.full((rows, cols), S_DIST, np.float32)
    cnt = np.full(rows, S_COUNT, np.uint32)
    if not isinstance(q, C.c_void_p):  # host queries; a c_void_p is a batch in HBM (search_dev)
        q = np.ascontiguousarray(q, np.float32).ctypes.data_as(f32p)
    rc = getattr(idx.lib, "fvh_" + name)(idx.h, q, B, dim, k, *mid, ids.ctypes.data_as(u64p),
                                         dist.ctypes.data_as(f32p), cnt.ctypes.data_as(u32p))
    status = OK
    try:
        idx._check(rc)
    except fvdb_import.load().FvdbError as e:
        status = e.status
    assert status == rc
    bi, bd, bc = ids[:B, :k], dist[:B, :k], cnt[:B]
    if B == 0:
        state = None
    elif (bc == S_COUNT).all() and (bi == S_ID).all() and (bd == S_DIST).all():
        state = "untouched"
    elif (bc == 0).all() and (bi == NO_ID).all() and np.isposinf(bd).all():
        state = "empty"
    else:
        assert not (bc == S_COUNT).any(), "a block is either written whole or not at all"
        state = "results"
    return status, state, fv_results(ids[:B, :k], dist[:B, :k], cnt[:B])


def fv_results(ids, dist, cnt):
    return fvdb_import.load().SearchResults(ids, dist, cnt)


def allow(a):
    a = np.ascontiguousarray(a, np.uint64)
    return a.ctypes.data_as(u64p), a.size


NULL_LIST = (None, 3)     # n_allowed != 0 with no list
EMPTY_LIST = (None, 0)


def blocking(idx, q, B, dim, k):
    """status and state of the four blocking entry points for one (B, dim, k)"""
    a = allow([100, 101, 102])
    return {
        "search": raw(idx, "hnsw_search", q, B, dim, k, EF)[:2],
        "search_allowed": raw(idx, "hnsw_search_allowed", q, B, dim, k, EF, *a)[:2],
        "search_exact": raw(idx, "hnsw_search_exact", q, B, dim, k)[:2],
        "search_exact_allowed": raw(idx, "hnsw_search_exact_allowed", q, B, dim, k, *a)[:2],
    }


def same(a, b, what):
    assert np.array_equal(a.counts, b.counts), f"{what}: counts differ: {a.counts} vs {b.counts}"
    assert np.array_equal(a.ids, b.ids), f"{what}: ids differ"
    assert np.array_equal(bits(a.distances), bits(b.distances)), f"{what}: distances are not bit-identical"


# ---- the blocking entry points ------------------------------------------------------------------------------------------
def test_empty_index_answers_nothing(empty, data):
    q = data[2]
    for dim in (D, D + 3):  # an index that has never held a row has no dimension to compare with
        got = blocking(empty, q[:, :1].repeat(dim, 1), 5, dim, 4)
        assert got == {e: (OK, "empty") for e in got}, got
    # the exact entries look at k first, and then write nothing
    for k in (0, MAX_K + 1):
        assert raw(empty, "hnsw_search_exact", q, 5, D, k)[:2] == (E_UNSUPPORTED, "untouched")
        assert raw(empty, "hnsw_search_exact_allowed", q, 5, D, k, *NULL_LIST)[:2] == (E_UNSUPPORTED, "untouched")
    # no entry point comes before the look at the list
    assert raw(empty, "hnsw_search_allowed", q, 5, D, 4, EF, *NULL_LIST)[:2] == (OK, "empty")
    assert raw(empty, "hnsw_search_exact_allowed", q, 5, D, 4, *NULL_LIST)[:2] == (OK, "empty")


def test_wrong_dimension(g, data):
    q5 = np.zeros((5, D + 3), np.float32)
    got = blocking(g, q5, 5, D + 3, 4)
    assert got == {e: (E_DIM, "empty") for e in got}, got
    # the dimension is looked at before the list
    assert raw(g, "hnsw_search_allowed", q5, 5, D + 3, 4, EF, *NULL_LIST)[:2] == (E_DIM, "empty")
    assert raw(g, "hnsw_search_exact_allowed", q5, 5, D + 3, 4, *NULL_LIST)[:2] == (E_DIM, "empty")


def test_k_zero_and_k_above_the_limit(g, data):
    q = data[2]
    got = blocking(g, q, 5, D, 0)
    assert got == {"search": (OK, "empty"), "search_allowed": (OK, "empty"), "search_exact": (E_UNSUPPORTED, "untouched"),
                   "search_exact_allowed": (E_UNSUPPORTED, "untouched")}, got
    # where k = 0 is answered differs: search() has looked at the dimension by then, search_allowed() has not
    q5 = np.zeros((5, D + 3), np.float32)
    assert raw(g, "hnsw_search", q5, 5, D + 3, 0, EF)[:2] == (E_DIM, "empty")
    assert raw(g, "hnsw_search_allowed", q5, 5, D + 3, 0, EF, *allow([100]))[:2] == (OK, "empty")
    assert raw(g, "hnsw_search_allowed", q, 5, D, 0, EF, *NULL_LIST)[:2] == (OK, "empty")
    for name, mid in (("hnsw_search_exact", ()), ("hnsw_search_exact_allowed", allow([100]))):
        assert raw(g, name, q, 5, D, MAX_K + 1, *mid)[:2] == (E_UNSUPPORTED, "untouched")
        assert raw(g, name, q, 5, D, MAX_K, *mid)[0] == OK
        assert raw(g, name, q5, 5, D + 3, MAX_K + 1, *mid)[:2] == (E_UNSUPPORTED, "untouched"), "k before the dimension"


def test_empty_batch(g, data):
    q = data[2]
    got = blocking(g, q, 0, D, 4)
    assert got == {e: (OK, None) for e in got}, got
    # search() and the exact entries have looked at the dimension by then, search_allowed() has not
    got = blocking(g, q, 0, D + 3, 4)
    assert got == {"search": (E_DIM, None), "search_allowed": (OK, None), "search_exact": (E_DIM, None),
                   "search_exact_allowed": (E_DIM, None)}, got
    # ... and an empty batch is answered before the list is looked at
    assert raw(g, "hnsw_search_allowed", q, 0, D, 4, EF, *NULL_LIST)[0] == OK
    assert raw(g, "hnsw_search_exact_allowed", q, 0, D, 4, *NULL_LIST)[0] == OK


def test_null_and_empty_allow_set(g, data):
    q = data[2]
    assert raw(g, "hnsw_search_allowed", q, 5, D, 4, EF, *NULL_LIST)[:2] == (E_INVALID, "empty")
    assert raw(g, "hnsw_search_exact_allowed", q, 5, D, 4, *NULL_LIST)[:2] == (E_INVALID, "empty")
    # nothing is allowed: nothing is found, by the scan (default cutoff) and by the masked traversal alike
    assert raw(g, "hnsw_search_exact_allowed", q, 5, D, 4, *EMPTY_LIST)[:2] == (OK, "empty")
    for cutoff in (g.scan_cutoff, 0):
        keep, g.scan_cutoff = g.scan_cutoff, cutoff
        try:
            assert raw(g, "hnsw_search_allowed", q, 5, D, 4, EF, *EMPTY_LIST)[:2] == (OK, "empty")
        finally:
            g.scan_cutoff = keep


def test_evaluate_search_quality_refusals(g, data):
    q = data[2]

    def quality(B, dim, k):
        out, n = np.zeros(3, np.float32), C.c_uint64(0)
        return g.lib.fvh_hnsw_evaluate_search_quality(g.h, q.ctypes.data_as(f32p), B, dim, k, EF, out.ctypes.data_as(f32p), C.byref(n))

    assert quality(0, D, MAX_K + 1) == E_INVALID, "no queries comes first"
    assert quality(5, D + 3, 0) == quality(5, D + 3, MAX_K + 1) == E_UNSUPPORTED, "k before the dimension"
    assert quality(5, D + 3, 4) == E_DIM
    assert quality(5, D, 4) == OK
    with pytest.raises(fvdb_import.load().InvalidConfig):
        g.evaluate_search_quality(np.zeros((0, D), np.float32), 4, EF)


# ---- the queries in HBM: search_dev and the begin / end pair -------------------------------------------------------------
def started(idx, slot):
    """what the begin reported: HNSWIndex.search_dev_begin (index.py) keeps (q_dev, B, dim, k, ef, started) per slot"""
    return idx._inflight[slot][5]


def end_by_itself(idx, slot, qd, B, dim, k):
    """fvh_hnsw_search_dev_end with the begin's arguments, whatever the begin reported"""
    rows, cols = max(B, 1), max(k, 1)
    ids = np.full((rows, cols), S_ID, np.uint64)
    dist = np.full((rows, cols), S_DIST, np.float32)
    cnt = np.full(rows, S_COUNT, np.uint32)
    rc = idx.lib.fvh_hnsw_search_dev_end(idx.h, slot, qd, B, dim, k, EF, ids.ctypes.data_as(u64p), dist.ctypes.data_as(f32p),
                                         cnt.ctypes.data_as(u32p))
    return rc, fv_results(ids[:B, :k], dist[:B, :k], cnt[:B])


def test_dev_entries_before_the_device(fv, ctx, g, empty, data):
    q = data[2]
    qd = ctx.upload(q)
    try:
        # the empty index: nothing starts, the end answers "nothing"; a slot that does not exist is not even looked at
        assert raw(empty, "hnsw_search_dev", qd, 5, D, 4, EF)[:2] == (OK, "empty")
        assert raw(empty, "hnsw_search_dev", qd, 5, D + 3, 4, EF)[:2] == (OK, "empty")
        for slot in (0, 3, 16):
            empty.search_dev_begin(slot, qd, 5, D, 4, EF)
            assert not started(empty, slot)
            r = empty.search_dev_end(slot)
            assert (r.ids == NO_ID).all() and (r.counts == 0).all() and np.isposinf(r.distances).all()
        # wrong dimension, k = 0, B = 0: not started, status OK at the begin; the end reports
        for B, dim, k, status in ((5, D + 3, 4, E_DIM), (5, D, 0, OK), (0, D, 4, OK), (0, D + 3, 4, E_DIM), (5, D + 3, 0, E_DIM)):
            g.search_dev_begin(1, qd, B, dim, k, EF)
            assert not started(g, 1), (B, dim, k)
            # search_dev into raw buffers: the status, and the outputs filled empty (nothing to judge at B = 0)
            assert raw(g, "hnsw_search_dev", qd, B, dim, k, EF)[:2] == (status, "empty" if B else None), (B, dim, k)
            if status == OK:
                r = g.search_dev_end(1)
                assert (r.counts == 0).all() and (r.ids[:, :k] == NO_ID).all()
                with_k = g.search_dev(qd, B, dim, k, EF)
                assert (with_k.counts == 0).all()
            else:
                with pytest.raises(fv.FvdbError) as e:
                    g.search_dev_end(1)
                assert e.value.status == status
                with pytest.raises(fv.FvdbError) as e:
                    g.search_dev(qd, B, dim, k, EF)
                assert e.value.status == status
        # a search that would start names a slot that does not exist: refused at the begin
        with pytest.raises(fv.FvdbError) as e:
            g.search_dev_begin(16, qd, 5, D, 4, EF)
        assert e.value.status == E_INVALID
    finally:
        ctx.free(qd)


def test_begin_end_with_and_without_device_traversal(fv, ctx, g, data):
    q = data[2]
    qd = ctx.upload(q)
    want = g.search(q, 4, EF)
    assert (want.counts == 4).all()
    try:
        for on in (True, False):
            g.set_device_traversal(on)
            same(g.search(q, 4, EF), want, f"search, device traversal {on}")
            same(g.search_dev(qd, 5, D, 4, EF), want, f"search_dev, device traversal {on}")
            for slot in (0, 2):
                g.search_dev_begin(slot, qd, 5, D, 4, EF)
                assert started(g, slot) == on
                same(g.search_dev_end(slot), want, f"begin / end in slot {slot}, device traversal {on}")
                # the end knows by itself what its begin did
                g.search_dev_begin(slot, qd, 5, D, 4, EF)
                rc, r = end_by_itself(g, slot, qd, 5, D, 4)
                assert rc == OK
                same(r, want, f"begin / end by itself in slot {slot}, device traversal {on}")
    finally:
        g.set_device_traversal(True)
        ctx.free(qd)


# ---- the entry point vacuumed away --------------------------------------------------------------------------------------
def test_lost_entry_point(fv, ctx, data):
    x, ids, q = data
    lost = graph(fv, ctx, x, ids)
    entry = lost.entry_point()
    lost.mark_deleted(entry)
    lost.mark_deleted(int(ids[5]) if int(ids[5]) != entry else int(ids[6]))
    assert lost.vacuum() == 2
    for name, mid in (("hnsw_search", (EF,)), ("hnsw_search_allowed", (EF, *allow(ids[:20])))):
        assert raw(lost, name, q, 5, D, 4, *mid)[:2] == (E_NOT_FOUND, "empty"), name
    with pytest.raises(fv.VectorNotFound) as e:
        lost.search(q, 4, EF)
    assert e.value.status == E_NOT_FOUND
    with pytest.raises(fv.VectorNotFound):
        lost.search_allowed(q, 4, EF, ids[:20])
    # the order of search(): dimension, then the lost entry point, then the empty batch
    assert raw(lost, "hnsw_search", q, 0, D, 4, EF)[0] == E_NOT_FOUND
    assert raw(lost, "hnsw_search", q, 0, D + 3, 4, EF)[0] == E_DIM
    # of search_allowed(): the empty batch, the dimension, the list, then the lost entry point
    assert raw(lost, "hnsw_search_allowed", q, 0, D, 4, EF, *allow(ids[:20]))[0] == OK
    assert raw(lost, "hnsw_search_allowed", q, 5, D, 4, EF, *NULL_LIST)[:2] == (E_INVALID, "empty")
    # the exact search does not start from the entry point: it still answers, over the rows that survive
    gone = np.isin(ids, [entry, int(ids[5]) if int(ids[5]) != entry else int(ids[6])])
    wi, wd, wc = R.exact_topk(R.fold_distances(q, x), 4, live=~gone, ids=ids)
    status, state, r = raw(lost, "hnsw_search_exact", q, 5, D, 4)
    assert (status, state) == (OK, "results")
    same(r, fv_results(wi, wd, wc), "search_exact after the entry point was vacuumed away")
    status, state, r = raw(lost, "hnsw_search_exact_allowed", q, 5, D, 4, *allow(ids))
    assert (status, state) == (OK, "results")
    same(r, fv_results(wi, wd, wc), "search_exact_allowed after the entry point was vacuumed away")
    # the pair: nothing starts, and the end reports why
    qd = ctx.upload(q)
    try:
        assert raw(lost, "hnsw_search_dev", qd, 5, D, 4, EF)[:2] == (E_NOT_FOUND, "empty")
        lost.search_dev_begin(2, qd, 5, D, 4, EF)
        assert not started(lost, 2)
        with pytest.raises(fv.VectorNotFound):
            lost.search_dev_end(2)
        lost.search_dev_begin(2, qd, 5, D, 4, EF)
        assert end_by_itself(lost, 2, qd, 5, D, 4)[0] == E_NOT_FOUND
    finally:
        ctx.free(qd)


# ---- the hybrid index: every way its end can get the recent part ----------------------------------------------------------
@pytest.fixture(scope="module")
def hybrid(fv, ctx, data):
    x, ids, _ = data
    h = fv.HybridIndex(ctx, hnsw_seed=5)
    h.set_ivf_centroids(x[:3].copy())
    ts = np.where(np.arange(N) % 3 == 0, NOW - 30 * DAY, NOW - 1 * DAY)  # a third historical, the rest recent
    h.bulk_insert(ids, x, ts, NOW)
    assert h.recent_count() > 32 and h.historical_count() > 16
    return h


def test_hybrid_begin_end_in_two_slots_three_ways(fv, ctx, hybrid, data):
    """What the hybrid end used to choose among: collect the traversal its begin enqueued; run the blocking search because
    nothing was enqueued; run the blocking search under the allow-set because nothing was enqueued.  The explicit pair of
    the Python class takes no allow-set, so the third is reached through search_allowed(), which is a begin and an end in
    a leased slot — the highest free one, so holding slot 15 with an explicit batch moves it to slot 14."""
    x, ids, q = data
    h, hn = hybrid, hybrid.hnsw()
    kw = dict(now=NOW, hnsw_ef=EF, ivf_n_probe=3)
    qd = ctx.upload(q)
    allowed = ids[::2]
    try:
        want = h.search(q, 6, **kw)
        assert (want.counts == 6).all()
        hn.scan_cutoff = 0  # 32 allowed ids are "above the cutoff": the masked traversal, not the scan
        want_allowed = h.search_allowed(q, 6, allowed, **kw)
        assert (want_allowed.counts == 6).all() and np.isin(want_allowed.ids, allowed).all()
        assert not np.array_equal(want_allowed.ids, want.ids)
        for on in (True, False):
            hn.set_device_traversal(on)
            walked = hn.hops()
            for slot in (0, 1):
                h.search_dev_begin(slot, qd, 5, 6, dim=D, **kw)
            for slot in (0, 1):
                same(h.search_dev_end(slot), want, f"begin / end in slot {slot}, device traversal {on}")
            same(h.search(q, 6, **kw), want, f"search, device traversal {on}")
            assert (hn.hops() > walked) == (not on), "the host walk served the recent part exactly when nothing was enqueued"
        # under the allow-set with the traversal off, in slot 15 and then in slot 14
        walked = hn.hops()
        same(h.search_allowed(q, 6, allowed, **kw), want_allowed, "search_allowed by the host walk, slot 15")
        h.search_dev_begin(15, qd, 5, 6, dim=D, **kw)
        same(h.search_allowed(q, 6, allowed, **kw), want_allowed, "search_allowed by the host walk, slot 14")
        same(h.search_dev_end(15), want, "the batch that held slot 15")
        assert hn.hops() > walked
        # a small allow-set scans, and the scan is a device kernel: it starts with the traversal off
        hn.scan_cutoff = 8192
        walked = hn.hops()
        scanned = h.search_allowed(q, 6, allowed, **kw)
        assert hn.hops() == walked, "no host walk: the scan was enqueued"
        hn.set_device_traversal(True)
        same(scanned, h.search_allowed(q, 6, allowed, **kw), "search_allowed by the scan, device traversal off and on")
    finally:
        hn.set_device_traversal(True)
        hn.scan_cutoff = 8192
        ctx.free(qd)
