"""Rows by id on the device: fvdb_ivf_get_rows (f32 and fp16 lists), IVFIndex / HybridIndex get_vectors, the session's
includeVectors, and the migration that takes its rows from the graph's row store in HBM.

Everything that is a copy is checked bit for bit; the searches of the migrated indexes are checked against the host
path of the same build and against the oracle taken through the same steps.  Shapes: 300 rows in 4 lists put more
than 64 rows (a second block) in some list; d = 3, 100 and 20 leave a tail in the last 16-byte chunk, d = 384 / 768
give a lane a second chunk; d = 3 and 100 have no row-major copy (blocked f32 read), d = 384 has one; 345 fetched rows
leave the gather's last workgroup partly filled."""
import ctypes as C
import threading

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu
DAY = 86400.0
NOT_FOUND = 7  # FVDB_E_NOT_FOUND


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def filled(fv, ctx, d, dtype, seed, n=300, nlist=4):
    x = mixture(n, d, n_comp=nlist, seed=seed)
    ivf = fv.DeviceIVF(ctx, d, nlist, dtype)
    ivf.set_centroids(x[:nlist])
    cl, pos = ivf.add(x, np.arange(n, dtype=np.uint64) + 1000)
    assert ivf.list_sizes().max() >= 75  # pigeonhole: a second block is in play
    rng = np.random.default_rng(seed)
    order = np.concatenate([rng.permutation(n), rng.integers(0, n, 45)])  # shuffled, with repeats; 345 % 4 != 0
    return x, ivf, cl, pos, order


def same_as_export(ivf, cl, pos, got):
    for c in range(ivf.nlist):
        rows, _, _ = ivf.list_export(c)
        sel = cl == c
        assert np.array_equal(bits(got[sel]), bits(rows[pos[sel]])), f"list {c}"


# ---- 1. f32 rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 100, 384])
def test_f32_rows_by_location(fv, ctx, d):
    x, ivf, cl, pos, order = filled(fv, ctx, d, "f32", 900 + d)
    got = ivf.get_rows(cl[order], pos[order])
    assert np.array_equal(bits(got), bits(x[order]))
    same_as_export(ivf, cl[order], pos[order], got)
    # the device form, on the index's own stream
    dev = ctx.alloc(order.size * d * 4)
    c32, p32 = np.ascontiguousarray(cl[order], np.uint32), np.ascontiguousarray(pos[order], np.uint32)
    u32p = C.POINTER(C.c_uint32)
    ctx.check(ctx.lib.fvdb_ivf_get_rows_dev(ivf.h, None, c32.ctypes.data_as(u32p), p32.ctypes.data_as(u32p), order.size, dev))
    ctx.synchronize()
    assert np.array_equal(bits(ctx.download(dev, (order.size, d), np.float32)), bits(x[order]))
    ctx.free(dev)
    # n = 0
    assert ivf.get_rows(np.zeros(0, np.uint32), np.zeros(0, np.uint32)).shape == (0, d)
    # a position equal to the list length is not a row: FVDB_E_NOT_FOUND, nothing written
    sizes = ivf.list_sizes()
    out = np.full((2, d), 7.0, np.float32)
    with pytest.raises(fv.engine.VectorNotFound) as e:
        ivf.get_rows([cl[0], 1], [pos[0], int(sizes[1])], out=out)
    assert e.value.status == NOT_FOUND
    assert np.all(out == 7.0)
    with pytest.raises(fv.engine.VectorNotFound):
        ivf.get_rows([ivf.nlist], [0], out=out)
    assert np.all(out == 7.0)
    ivf.close()


# ---- 2. fp16 rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [20, 768])
def test_f16_rows_by_location(fv, ctx, d):
    x, ivf, cl, pos, order = filled(fv, ctx, d, "f16", 940 + d)
    got = ivf.get_rows(cl[order], pos[order])
    assert np.array_equal(bits(got), bits(x[order].astype(np.float16).astype(np.float32)))
    same_as_export(ivf, cl[order], pos[order], got)
    ivf.close()


# ---- 3. after mutations, through the mirror ----------------------------------------------------------------------
def test_get_vectors_after_delete_vacuum_retrain(fv, ctx):
    n, d = 300, 100
    x = mixture(n, d, n_comp=4, seed=960)
    ids = np.arange(n, dtype=np.uint64) * 3 + 5
    ix = fv.IVFIndex(ctx, n_clusters=4, n_probe=2)
    ix.set_trained(x[:4])
    assert ix.batch_insert(ids, x) == (n, 0)
    unknown = np.uint64(2)
    rows, found = ix.get_vectors(np.concatenate([ids[::-1], [unknown]]))
    assert found[:-1].all() and not found[-1]
    assert np.array_equal(bits(rows[:-1]), bits(x[::-1]))
    assert np.all(rows[-1] == 0)  # a miss leaves its row untouched
    assert np.array_equal(bits(ix.get_vector_by_id(int(ids[7]))), bits(x[7])) and ix.get_vector_by_id(2) is None
    dead = np.arange(0, n, 7)
    for i in dead:
        ix.mark_deleted(int(ids[i]))
    rows, found = ix.get_vectors(ids[dead])  # soft-deleted ids still return their rows
    assert found.all() and np.array_equal(bits(rows), bits(x[dead]))
    assert ix.vacuum() == dead.size
    rows, found = ix.get_vectors(ids)
    gone = np.zeros(n, bool)
    gone[dead] = True
    assert np.array_equal(found, ~gone)
    assert np.array_equal(bits(rows[~gone]), bits(x[~gone])) and np.all(rows[gone] == 0)
    ix.retrain(7, n_probe=2, seed=3)
    rows, found = ix.get_vectors(ids[~gone])
    assert found.all() and np.array_equal(bits(rows), bits(x[~gone]))
    assert not ix.get_vectors([unknown])[1][0]


# ---- 4. beside searches ------------------------------------------------------------------------------------------
def test_fetches_beside_searches(fv, ctx):
    x, ivf, cl, pos, order = filled(fv, ctx, 100, "f32", 970)
    q = mixture(16, 100, n_comp=4, seed=971)
    want = ivf.search(q, 10, 2)
    errors = []

    def fetch(t):
        try:
            o = np.roll(order, 31 * t)
            for _ in range(20):
                if not np.array_equal(bits(ivf.get_rows(cl[o], pos[o])), bits(x[o])):
                    errors.append(f"fetch thread {t}: rows differ")
        except Exception as e:  # noqa: BLE001
            errors.append(f"fetch thread {t}: {e!r}")

    def search(t):
        try:
            for _ in range(20):
                got = ivf.search(q, 10, 2)
                if not all(np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)
                           for a, b in zip(got, want)):
                    errors.append(f"search thread {t}: results differ")
        except Exception as e:  # noqa: BLE001
            errors.append(f"search thread {t}: {e!r}")

    threads = [threading.Thread(target=f, args=(t,)) for t in range(4) for f in (fetch, search)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == []
    ivf.close()


# ---- hybrid fixtures ----------------------------------------------------------------------------------------------
KW = dict(max_connections=6, max_connections_layer_0=12, ef_construction=30, n_probe=3, auto_migrate=False)


def hybrids(fv, ctx, d, seed, n=600, nlist=8, with_oracle=True):
    """Two mirrors (resident migration on / off) and the oracle over the same seeded data: half of the rows old (they go
    straight to the lists), half recent (graph nodes, pending).  Among the recent ones: id DUP is already in its list,
    id GONE is a soft-deleted graph node."""
    x = mixture(n, d, n_comp=nlist, seed=seed)
    now = 1000 * DAY
    rng = np.random.default_rng(seed)
    ages = np.where(rng.random(n) < 0.5, 1 * DAY, 30 * DAY)
    levels = orc.rng_levels(seed, n)
    res, host = fv.HybridIndex(ctx, n_clusters=nlist, **KW), fv.HybridIndex(ctx, n_clusters=nlist, **KW)
    host.set_resident_migration(False)
    all3 = [res, host] + ([orc.HybridIndex(n_clusters=nlist, **KW)] if with_oracle else [])
    recent = np.flatnonzero(ages < 7 * DAY)
    dup, gone = int(recent[5]), int(recent[11])
    for h in all3:
        h.set_ivf_centroids(x[:nlist])
        for i in range(n):
            h.insert_with_timestamp(i, x[i], now - ages[i], now, int(levels[i]))
        h.ivf().insert(dup, x[dup])  # the copy the migration will meet: dropped as a duplicate
        h.delete(gone, now)          # still recent: the graph node is soft-deleted, and stays due
    return x, now, recent, dup, gone, all3


# ---- 5. HybridIndex.get_vectors -----------------------------------------------------------------------------------
def test_hybrid_get_vectors(fv, ctx):
    d = 100
    x, now, recent, dup, gone, (res, host) = hybrids(fv, ctx, d, 980, n=240, nlist=4, with_oracle=False)
    old = np.setdiff1d(np.arange(x.shape[0]), recent)
    ask = np.array([recent[0], old[0], 10**9, old[1], recent[1], dup, gone], np.uint64)

    def check(h):
        rows, found = h.get_vectors(ask)
        assert found.tolist() == [True, True, False, True, True, True, True]
        assert np.array_equal(bits(rows[found]), bits(x[ask[found].astype(np.int64)]))
        assert np.all(rows[2] == 0)

    check(res)  # graph only, lists only, unknown
    migrated = res.migrate_with_threshold(0.5 * DAY, now)
    assert migrated == host.migrate_with_threshold(0.5 * DAY, now) > 0
    check(res)  # now in both: the recent part answers first
    check(host)
    rows, found = res.get_vectors(np.arange(x.shape[0], dtype=np.uint64))
    assert found.all() and np.array_equal(bits(rows), bits(x))
    # the lists alone hold every row now (the graph's copies aside): read them all from HBM
    rows, found = res.ivf().get_vectors(np.arange(x.shape[0], dtype=np.uint64))
    assert found.all() and np.array_equal(bits(rows), bits(x))


# ---- 6. session ---------------------------------------------------------------------------------------------------
def test_session_include_vectors(fv, ctx):
    rng = np.random.default_rng(990)
    vecs = rng.standard_normal((60, 12))  # doubles, like a JS caller's numbers
    s = fv.VectorDbSession(ctx)
    s.add_vectors([{"id": f"doc-{i}", "vector": vecs[i].tolist(), "metadata": {"n": i, "even": i % 2 == 0}}
                   for i in range(60)])
    want = {f"doc-{i}": [float(v) for v in np.float32(vecs[i])] for i in range(60)}
    q = vecs[3].tolist()
    for opts in ({}, {"filter": {"even": True}}, {"filter": {"even": True}, "filterMode": "oversample"},
                 {"filter": {"even": True}, "filterMode": "pushdown"}):
        plain = s.search(q, 5, dict(opts))
        assert plain and all("vector" not in r for r in plain)
        assert plain == s.search(q, 5, dict(opts, includeVectors=False))
        got = s.search(q, 5, dict(opts, includeVectors=True))
        assert [{k: v for k, v in r.items() if k != "vector"} for r in got] == plain
        for r in got:
            assert isinstance(r["vector"], list) and all(type(v) is float for v in r["vector"])
            assert r["vector"] == want[r["id"]]
    # later the rows have aged: the search migrates them, and the hits still carry their vectors
    s.now += 30 * DAY
    got = s.search(q, 5, {"includeVectors": True})
    assert got and all(r["vector"] == want[r["id"]] for r in got)


# ---- 7. resident migration ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 384])
def test_resident_migration_matches_host_path_and_oracle(fv, ctx, d):
    nlist = 8
    x, now, recent, dup, gone, (res, host, o) = hybrids(fv, ctx, d, 1000 + d, nlist=nlist)
    want = o.migrate_with_threshold(0.5 * DAY, now)
    assert res.migrate_with_threshold(0.5 * DAY, now) == want
    assert host.migrate_with_threshold(0.5 * DAY, now) == want
    assert want == recent.size - 1  # every due row but the duplicate; the soft-deleted node is copied like the rest
    assert (res.recent_count(), res.historical_count()) == (o.recent_count(), o.historical_count())
    ri, hi = res.ivf(), host.ivf()
    for c in range(nlist):
        a, b = ri.export_list(c), hi.export_list(c)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), f"list {c}"
    q = mixture(32, d, n_comp=nlist, seed=7)
    for kws in (dict(now=now), dict(now=now, search_recent=False, ivf_n_probe=nlist)):
        a, b = res.search(q, 10, **kws), host.search(q, 10, **kws)
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.ids, b.ids)
        assert np.array_equal(bits(a.distances), bits(b.distances))
        for qi in range(q.shape[0]):
            r = o.search(q[qi], 10, **kws)
            m = int(a.counts[qi])
            assert m == len(r) and np.array_equal(a.ids[qi, :m], r.ids)
            assert np.array_equal(bits(a.distances[qi, :m]), bits(r.distances))
    info = res.migration_info()
    assert info["resident"] and info["path"] == "resident"
    assert info["rows_in"] == info["rows_out"] == want
    assert 0 < info["host_bytes"] <= 32 * want
    hinfo = host.migration_info()
    assert hinfo["path"] == "host" and hinfo["host_bytes"] >= 2 * want * d * 4


def test_from_store_matches_host_form_with_fp16_lists(fv, ctx):
    """The same pair of calls one level down, where the lists can be fp16: fvdb_ivf_assign_from_store +
    fvdb_ivf_add_assigned_from_store against fvdb_ivf_assign + fvdb_ivf_add_assigned of the rows fvdb_store_get returns.
    d = 100: dpad != d in the store."""
    n, d, nlist = 300, 100, 8
    x = mixture(n, d, n_comp=nlist, seed=1100)
    store = fv.RowStore(ctx, d)
    store.append(x)
    rows = np.random.default_rng(5).permutation(n)[:250].astype(np.uint32)
    ids = rows.astype(np.uint64) + 77
    for dtype in ("f16", "f32"):
        a, b = fv.DeviceIVF(ctx, d, nlist, dtype), fv.DeviceIVF(ctx, d, nlist, dtype)
        for ix in (a, b):
            ix.set_centroids(x[:nlist])
            ix.add(x[250:], np.arange(50, dtype=np.uint64))  # lists that are not empty, last blocks partly filled
        host_rows = np.stack([store.get(int(r)) for r in rows])
        assert np.array_equal(bits(host_rows), bits(x[rows]))
        ca, cb = a.assign_from_store(store, rows), b.assign(host_rows)
        assert np.array_equal(ca, cb)
        pa, pb = a.add_assigned_from_store(store, rows, ids, ca), b.add_assigned(host_rows, ids, cb)
        assert np.array_equal(pa, pb)
        for c in range(nlist):
            ea, eb = a.list_export(c), b.list_export(c)
            assert np.array_equal(bits(ea[0]), bits(eb[0])) and np.array_equal(ea[1], eb[1]) and np.array_equal(ea[2], eb[2])
        q = mixture(32, d, n_comp=nlist, seed=8)
        for mode in (0, 1):  # matrix-core filter (fp16 mirror, norms, largest norm) and the exact scan
            a.set_scan_mode(mode)
            b.set_scan_mode(mode)
            ra, rb = a.search(q, 10, nlist), b.search(q, 10, nlist)
            assert all(np.array_equal(bits(u), bits(v)) if u.dtype == np.float32 else np.array_equal(u, v) for u, v in zip(ra, rb))
        m = fv._capi.MaintenanceInfo()
        ctx.check(ctx.lib.fvdb_ivf_maintenance_info(a.h, C.byref(m)))
        assert m.rows_in == m.rows_out == rows.size and 0 < m.host_bytes <= 32 * rows.size
        # checks of the pair: a row index past the store changes nothing; another dimension is refused
        before = a.total_rows()
        with pytest.raises(fv.engine.VectorNotFound):
            a.assign_from_store(store, [0, n])
        with pytest.raises(fv.engine.VectorNotFound):
            a.add_assigned_from_store(store, [0, n], [1, 2], [0, 0])
        assert a.total_rows() == before
        other = fv.RowStore(ctx, d + 1)
        with pytest.raises(fv.engine.DimensionMismatch):
            a.assign_from_store(other, [0])
        other.close()
        a.close()
        b.close()
    store.close()
