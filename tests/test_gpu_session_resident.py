"""VectorDbSession.search / search_many with "filterMode": "resident": the allow-set comes from the metadata columns in HBM
(metadata_columns.py) and must be, element for element, the array "pushdown" computes with MetadataFilter.matches; the
unknown slots the device leaves to the host must be exactly those the rules (tests/_meta_cases.py) define."""
import numpy as np
import pytest

import fvdb_import
import _meta_cases as K

fv = fvdb_import.load()
pytestmark = pytest.mark.gpu
Q = [0.0, 1.0, 0.5]


@pytest.fixture(scope="module")
def ctx():
    c = fv.Context(0)
    yield c
    c.close()


def make_session(ctx, mds, **kw):
    s = fv.VectorDbSession(ctx, **kw)
    s.add_vectors([{"id": f"doc-{i}", "vector": [float(i), 1.0, 0.5], "metadata": md} for i, md in enumerate(mds)])
    return s


class Recorder:
    """Wraps index.search_allowed: keeps the allow-set it was handed; calls through, or answers nothing when told to."""

    def __init__(self, index, call_through=True):
        self.index, self.inner, self.call_through, self.allowed = index, index.search_allowed, call_through, []
        index.search_allowed = self

    def __call__(self, q, k, allowed, now=0.0):
        self.allowed.append(np.array(allowed, copy=True))
        if self.call_through:
            return self.inner(q, k, allowed, now=now)
        return fv.index.SearchResults(np.zeros((1, k), np.uint64), np.zeros((1, k), np.float32), np.zeros(1, np.uint32))

    def restore(self):
        self.index.search_allowed = self.inner


def both_modes(s, flt_json, k=6):
    """(pushdown results, resident results, pushdown allow-set, resident allow-set) of one filter."""
    rec = Recorder(s.index)
    try:
        a = s.search(Q, k, {"filter": flt_json, "filterMode": "pushdown"})
        b = s.search(Q, k, {"filter": flt_json, "filterMode": "resident"})
    finally:
        rec.restore()
    return a, b, rec.allowed[0], rec.allowed[1]


def assert_same(s, flt_json, k=6):
    a, b, pa, ra = both_modes(s, flt_json, k)
    assert ra.dtype == np.uint64 and np.array_equal(pa, ra), flt_json
    assert a == b, flt_json
    return a, ra


def shaped_metadata(n):
    return [{"n": i, "w": i * 0.5, "tag": "even" if i % 2 == 0 else "odd", "tags": ["x", f"t{i % 7}", i % 3], "rare": i % 50 == 7,
             "nested": {"level": i % 4, "deep": {"name": f"g{i % 5}"}}, **({"maybe": None} if i % 9 == 0 else {})} for i in range(n)]


def test_every_filter_shape_agrees_with_pushdown(ctx):
    s = make_session(ctx, shaped_metadata(600))
    shapes = [{"tag": "even"},                                              # equality
              {"tags": "t3"}, {"tags": 2},                                  # an array CONTAINS the value
              {"n": {"$in": [3, 5, 8, 599, 600]}}, {"tag": {"$in": ["odd", "none"]}},
              {"n": {"$gte": 100}}, {"n": {"$gt": 100}}, {"w": {"$lte": 10.5}}, {"n": {"$lt": 7}}, {"n": {"$gte": 10, "$lt": 20}},
              {"$and": [{"tag": "even"}, {"n": {"$lt": 50}}]}, {"$or": [{"rare": True}, {"n": 3}]},
              {"tag": "odd", "rare": True, "n": {"$gt": 50}},               # several fields: implicit AND
              {"nested.level": 2}, {"nested.deep.name": "g4"},              # dotted paths
              {"n": 1.0}, {"rare": 1}, {"maybe": None}, {"n": "1"},         # 1 != 1.0, booleans are not numbers, null, "1"
              {"$and": [{"n": {"$gte": 100, "$lte": 400}}, {"$or": [{"tags": "t1"}, {"n": {"$in": [150, 151, 152]}}]}]},
              {"$and": []}, {"$or": []}, {"nope": 1}]
    nonempty = 0
    for fj in shapes:
        res, allowed = assert_same(s, fj)
        info = s.last_filter_info()
        assert info["route"] == "device" and info["unknown"] == 0 and info["slots"] == 600 and info["matches"] == allowed.size, fj
        nonempty += bool(res)
    assert nonempty >= len(shapes) - 5
    assert s.last_filter_info()["columns_created"] == ["nope"]
    assert_same(s, {"tag": "even"})
    assert s.last_filter_info()["columns_created"] == []                    # a column is built once
    res, allowed = assert_same(s, {"nested": {"level": 1, "deep": {"name": "g1"}}})  # an object compared whole: the host decides it
    info = s.last_filter_info()
    assert info["route"] == "device" and info["unknown"] == 600 and allowed.size == 30 and res
    s.destroy()


def sweep(ctx, complex_too, seed):
    mds, flts = K.population(seed, 400, 300, complex_too)
    s = make_session(ctx, mds)
    rec = Recorder(s.index, call_through=False)  # the allow-set handed to the index is the whole contract here
    unknown_total = 0
    try:
        for fj in flts:
            s.search(Q, 5, {"filter": fj, "filterMode": "pushdown"})
            s.search(Q, 5, {"filter": fj, "filterMode": "resident"})
            want, got = rec.allowed[-2], rec.allowed[-1]
            assert np.array_equal(want, got), fj
            info = s.last_filter_info()
            _, _, unknown = K.interpreter_counts(mds, fj)
            assert info["route"] == "device" and info["unknown"] == unknown and info["matches"] == want.size, fj
            unknown_total += unknown
    finally:
        rec.restore()
    matched = sum(a.size for a in rec.allowed[1::2])
    s.destroy()
    return unknown_total, matched


def test_randomized_sweep_plain_population_is_decided_on_the_device(ctx):
    unknown, matched = sweep(ctx, False, 20240521)  # the population test_metadata_columns_host.py proves free of unknowns
    assert unknown == 0 and matched > 1000


def test_randomized_sweep_full_population(ctx):
    unknown, matched = sweep(ctx, True, 20240522)
    assert unknown > 0 and matched > 1000


def test_mutations_keep_the_columns_in_step(ctx):
    st = fv.chunked.MemoryStorage()
    s = make_session(ctx, shaped_metadata(400), storage=st, session_id="resident-1")
    filters = [{"tag": "even"}, {"tags": "t3"}, {"n": {"$gte": 100, "$lt": 300}}, {"nested.level": 2}, {"rare": True},
               {"$or": [{"fresh": "yes"}, {"n": {"$in": [7, 8, 9, 401]}}]}]

    def all_agree():
        return [assert_same(s, fj, 100)[1].size for fj in filters]

    base = all_agree()
    s.delete_vector("doc-8")
    s.delete_vector("doc-107")
    after_delete = all_agree()
    assert after_delete[0] == base[0] - 1 and after_delete[4] == base[4] - 1
    # the same id again with other metadata.  The hybrid index never forgets an id (src/hybrid/core.rs: a deleted id is
    # still a duplicate), so the call fails before anything of it is stored, and both modes still agree ...
    again_doc = {"id": "doc-8", "vector": [8.0, 1.0, 0.5], "metadata": {"n": 7, "tag": "odd", "tags": ["t3"], "rare": True}}
    with pytest.raises(fv.session.SessionError, match="Failed to add vector"):
        s.add_vectors([again_doc])
    assert all_agree() == after_delete
    # ... and where the index does take it (its insert stood in for, for this one call), the session stores the new
    # metadata under the id's first position among the rows, and the table rewrites that slot
    real_insert = s.index.insert
    s.index.insert = lambda rid, vec, now=0.0: None
    try:
        s.add_vectors([again_doc])
    finally:
        s.index.insert = real_insert
    assert list(s._rows).index(fv.VectorId("doc-8").row_id()) == 8 and s.last_filter_info()["slots"] == 400
    again = all_agree()
    assert again[4] == after_delete[4] + 1 and again[0] == after_delete[0]
    real_delete = s.index.delete  # and out again the same way, so that what is saved below is what the index holds
    s.index.delete = lambda rid, now: None
    try:
        s.delete_vector("doc-8")
    finally:
        s.index.delete = real_delete
    assert all_agree() == after_delete
    s.update_metadata("doc-9", {"n": 250, "tag": "even", "tags": [], "nested": {"level": 2}})
    s.update_metadata("doc-10", {"tags": ["t3", "t3", "t3", "t3"]})
    all_agree()
    s.add_vectors([{"id": f"new-{i}", "vector": [400.0 + i, 1.0, 0.5], "metadata": {"n": 401 + i, "fresh": "yes" if i % 2 else "no"}}
                   for i in range(40)])  # rows that bring a new field, after its column exists
    grown = all_agree()
    assert grown[5] >= 20 + 2
    assert s.last_filter_info()["slots"] == 440
    # delete_by_metadata drops entries from the map: their slots must stop being present
    out = s.delete_by_metadata({"rare": True})
    assert out["deleted_count"] == grown[4] > 0 and len(out["deleted_ids"]) == grown[4]
    grown = all_agree()
    assert grown[4] == 0 and s.last_filter_info()["slots"] == 440
    # save and load: the table is dropped and rebuilt from the loaded rows
    s.save_to_s5()
    t = fv.VectorDbSession(ctx, storage=st, session_id="resident-2")
    t.add_vectors([{"id": "old", "vector": [0.0, 0.0, 0.0], "metadata": {"tag": "even"}}])
    assert [r["id"] for r in t.search(Q, 3, {"filter": {"tag": "even"}, "filterMode": "resident"})] == ["old"]
    t.load_user_vectors("resident-1")
    for fj in filters:
        a, b, pa, ra = both_modes(t, fj, 100)
        assert np.array_equal(pa, ra) and a == b and sorted(ra.tolist()) == sorted(assert_same(s, fj, 100)[1].tolist())
    assert t.last_filter_info()["slots"] == len(t._rows) and t.last_filter_info()["columns_created"]
    # a direct edit of session.metadata is seen once refresh_metadata_columns() has run
    key = s._rows[fv.VectorId("doc-20").row_id()]
    s.metadata[key]["tag"] = "odd"
    s.metadata[key]["rare"] = True
    s.refresh_metadata_columns()
    edited = all_agree()
    assert edited[0] == grown[0] - 1 and edited[4] == grown[4] + 1
    s.destroy()
    t.destroy()


def test_search_many_mixes_modes(ctx):
    s = make_session(ctx, shaped_metadata(500))
    f1, f2 = {"tag": "even"}, {"$and": [{"n": {"$gte": 100}}, {"tags": "t2"}]}
    opts = [{"filter": f1, "filterMode": "resident"}, {"filter": f1, "filterMode": "pushdown"}, {}, {"filter": f2, "filterMode": "resident"},
            {"filter": f1, "filterMode": "resident", "threshold": 0.01}, None, {"filter": f2, "filterMode": "pushdown"},
            {"filter": f2, "filterMode": "resident", "includeVectors": True}]
    qs = [[float(7 * i), 1.0, 0.5] for i in range(len(opts))]
    calls = []
    inner = s._resident_allowed
    s._resident_allowed = lambda flt: (calls.append(1), inner(flt))[1]
    many = s.search_many(qs, 5, opts)
    del s._resident_allowed
    assert len(calls) == 2  # one evaluation per distinct resident filter
    for q, o, got in zip(qs, opts, many):
        assert got == s.search(q, 5, o) and (got or not o)
    assert many[0] == s.search(qs[0], 5, opts[1]) and many[3] == s.search(qs[3], 5, opts[6])
    with pytest.raises(fv.session.SessionError, match="search_many"):
        s.search_many([Q], 5, [{"filter": f1}])
    s.destroy()


def test_filter_over_the_program_limits_takes_the_host_route(ctx):
    s = make_session(ctx, shaped_metadata(400))
    big = {"$or": [{"n": i} for i in range(0, 3000, 3)]}  # 1000 leaves: beyond the program limit
    res, allowed = assert_same(s, big, 10)
    info = s.last_filter_info()
    assert info["route"] == "host" and info["matches"] == allowed.size == 134 and len(res) == 10
    deep = {"n": 5}
    for i in range(20):
        deep = {"$or": [{"n": 1000 + i}, deep]}  # 21 results on the stack at once
    res, allowed = assert_same(s, deep)
    assert s.last_filter_info()["route"] == "host" and [r["id"] for r in res] == ["doc-5"]
    assert_same(s, {"tag": "odd"})
    assert s.last_filter_info()["route"] == "device"
    s.destroy()
