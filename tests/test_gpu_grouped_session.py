"""GPU: the session's grouped-search options "groupBy", "groupSize", "fetchK", "groupMissing" and "fill" (DESIGN.md
section 9v), against the path they replace: the session's own search of fetchK, grouped by a Python loop over the hits'
metadata.  test_gpu_grouped_index.py holds HybridIndex.search_grouped to the reference.

The session holds 300 chunks: chunk i is [i // 3, 0.01 * (i % 3), 0.5] and the query is the origin, so the nearest chunks
run through the passages in order.  "source" has five values (every eleventh chunk has none), "passage" is an int,
"a.b" a nested int.  All rows are recent: the walk returns at most its ef = 50 rows, so a fetchK up to 50 gives a
candidate list that was cut, and a larger one a list that was not."""
import numpy as np
import pytest

import fvdb_import

fv = fvdb_import.load()
pytestmark = pytest.mark.gpu
Q = [0.0, 0.0, 0.0]
N = 300
SessionError = fv.session.SessionError
NONE = object()  # "the hit has no such field"


def vec(i):
    return [float(i // 3), 0.01 * (i % 3), 0.5]


def meta(i):
    m = {"n": i, "passage": i // 3, "source": f"src{i % 5}", "a": {"b": i % 4}, "tag": "even" if i % 2 == 0 else "odd"}
    if i % 11 == 0:
        del m["source"]
    return m


@pytest.fixture(scope="module")
def ctx():
    c = fv.Context(0)
    yield c
    c.close()


def new_session(ctx):
    s = fv.VectorDbSession(ctx)
    s.add_vectors([{"id": f"chunk-{i}", "vector": vec(i), "metadata": meta(i)} for i in range(N)])
    return s


@pytest.fixture(scope="module")
def session(ctx):
    return new_session(ctx)  # shared by the tests that only read


def field(md, path):
    cur = md
    for part in path.split("."):
        if not isinstance(cur, dict) or part not in cur:
            return NONE
        cur = cur[part]
    return cur


def by_loop(session, q, k, path, group_size, fetch_k, missing="drop", options=None):
    """the replaced path: search(fetch_k), then a loop over the hits; (groups as (key, [hit], total), was the list cut)"""
    hits = session.search(q, fetch_k, dict(options or {}))
    order, members = [], {}
    for j, h in enumerate(hits):
        v = field(h["metadata"], path)
        key = (type(v).__name__, v) if v is not NONE else (("own", j) if missing == "own" else None)
        if key is None:
            continue
        if key not in members:
            members[key] = []
            order.append(key)
        members[key].append(h)
    return [(key, members[key][:group_size], len(members[key])) for key in order[:k]], len(hits) == fetch_k


def same_groups(got, want, cut, k, group_size):
    groups = got["groups"]
    assert len(groups) == len(want)
    for g, (key, hits, total) in zip(groups, want):
        if key[0] == "own":
            assert g["key"] is None and g.get("missing") is True and g["complete"] is True
        else:
            assert (type(g["key"]).__name__, g["key"]) == key and "missing" not in g
            assert g["complete"] == (len(hits) == group_size or not cut)
        assert [h["id"] for h in g["hits"]] == [h["id"] for h in hits]
        assert [h["score"] for h in g["hits"]] == [h["score"] for h in hits]
        assert [h["metadata"] for h in g["hits"]] == [h["metadata"] for h in hits]
        assert g["total"] == total
    assert got["groupsComplete"] == (len(want) == k or not cut)


@pytest.mark.parametrize("path", ["source", "passage", "a.b"])
def test_group_by_a_string_an_int_and_a_nested_path(session, path):
    for k, group_size, fetch_k in ((3, 2, 30), (4, 1, 12), (10, 3, 200)):
        options = {"groupBy": path, "groupSize": group_size, "fetchK": fetch_k}
        got = session.search(Q, k, options)
        want, cut = by_loop(session, Q, k, path, group_size, fetch_k)
        assert cut == (fetch_k <= 50) and want
        same_groups(got, want, cut, k, group_size)
    # the defaults: groupSize 1, fetchK min(4096, 4 k groupSize)
    got = session.search(Q, 3, {"groupBy": path})
    want, cut = by_loop(session, Q, 3, path, 1, 12)
    same_groups(got, want, cut, 3, 1)


def test_group_missing(session):
    for missing in ("drop", "own"):
        got = session.search(Q, 8, {"groupBy": "source", "groupSize": 2, "fetchK": 30, "groupMissing": missing})
        want, cut = by_loop(session, Q, 8, "source", 2, 30, missing)
        same_groups(got, want, cut, 8, 2)
        assert any(key[0] == "own" for key, _, _ in want) == (missing == "own")  # chunk 0 has no source and is the nearest


def test_search_many_and_include_vectors(session):
    qs = [Q, vec(40), vec(150), [3.0, 0.2, 0.1]]
    options = {"groupBy": "source", "groupSize": 2, "fetchK": 20, "includeVectors": True}
    many = session.search_many(qs, 3, [dict(options) for _ in qs])
    for q, got in zip(qs, many):
        assert got == session.search(q, 3, options)
        want, cut = by_loop(session, q, 3, "source", 2, 20, options={"includeVectors": True})
        same_groups(got, want, cut, 3, 2)
        for g, (_, hits, _) in zip(got["groups"], want):
            assert [h["vector"] for h in g["hits"]] == [h["vector"] for h in hits] and g["hits"][0]["vector"] is not None
    # each request keeps its own filter; the grouping is shared
    flt = {"tag": "even"}
    mixed = session.search_many(qs[:3], 3, [dict(options), dict(options, filter=flt, filterMode="pushdown"),
                                            dict(options, filter=flt, filterMode="resident")])
    assert mixed[0] == many[0]
    assert mixed[1] == session.search(qs[1], 3, dict(options, filter=flt, filterMode="pushdown"))
    assert mixed[2] == session.search(qs[2], 3, dict(options, filter=flt, filterMode="resident"))
    with pytest.raises(SessionError):
        session.search_many(qs[:2], 3, [dict(options), dict(options, groupSize=3)])
    with pytest.raises(SessionError):
        session.search_many(qs[:2], 3, [dict(options), {}])


def test_a_filter_by_either_route_gives_equal_results(session):
    flt = {"$and": [{"tag": "even"}, {"n": {"$gte": 6}}]}
    options = {"groupBy": "source", "groupSize": 3, "fetchK": 40, "filter": flt}
    a = session.search(Q, 4, dict(options, filterMode="pushdown"))
    b = session.search(Q, 4, dict(options, filterMode="resident"))
    assert a == b and a["groups"]
    want, cut = by_loop(session, Q, 4, "source", 3, 40, options={"filter": flt, "filterMode": "pushdown"})
    same_groups(a, want, cut, 4, 3)
    assert all(h["metadata"]["tag"] == "even" and h["metadata"]["n"] >= 6 for g in a["groups"] for h in g["hits"])


@pytest.mark.parametrize("mode", [None, "pushdown", "resident"])
def test_fill_completes_the_groups_a_cut_list_left_short(session, mode):
    extra = {} if mode is None else {"filter": {"tag": "even"}, "filterMode": mode}
    options = dict({"groupBy": "source", "groupSize": 4, "fetchK": 12}, **extra)
    before = session.search(Q, 5, options)
    short = [g for g in before["groups"] if not g["complete"]]
    assert short, "the precondition: at least one group is incomplete before the fill"
    assert all(len(g["hits"]) < 4 for g in short)
    after = session.search(Q, 5, dict(options, fill=True))
    assert [g["key"] for g in after["groups"]] == [g["key"] for g in before["groups"]]  # the set of groups is not searched again
    assert after["groupsComplete"] == before["groupsComplete"]
    for g0, g1 in zip(before["groups"], after["groups"]):
        assert g1["complete"] is True and g1["total"] == g0["total"]
        if g0["complete"]:
            assert g1["hits"] == g0["hits"]
            continue
        leaf = {"source": g0["key"]}
        combined = {"$and": [extra["filter"], leaf]} if mode else leaf
        want = session.search(Q, 4, {"filter": combined, "filterMode": mode or "resident"})
        assert g1["hits"] == want and len(want) == 4
    # through search_many as well
    assert session.search_many([Q], 5, [dict(options, fill=True)])[0] == after


def test_groups_complete_both_ways(session):
    assert session.search(Q, 3, {"groupBy": "source", "fetchK": 12})["groupsComplete"] is True     # three groups found
    cut = session.search(Q, 10, {"groupBy": "source", "fetchK": 12})
    assert len(cut["groups"]) == 5 and cut["groupsComplete"] is False                              # five sources, a cut list
    whole = session.search(Q, 10, {"groupBy": "source", "fetchK": 200})
    assert len(whole["groups"]) == 5 and whole["groupsComplete"] is True                           # the list was not cut
    assert all(g["complete"] for g in whole["groups"])


def test_each_refused_combination_says_so(session):
    for options, word in (({"groupBy": "source", "mmrLambda": 0.5}, "mmrLambda"), ({"groupBy": "source", "exact": True}, "exact"),
                          ({"groupBy": "source", "threshold": 0.5}, "threshold"),
                          ({"groupBy": "source", "filter": {"tag": "even"}}, "filterMode"),
                          ({"groupBy": "source", "filter": {"tag": "even"}, "filterMode": "oversample"}, "oversample"),
                          ({"groupBy": "source", "groupSize": 0}, "groupSize"), ({"groupBy": "source", "fetchK": 5000}, "fetchK"),
                          ({"groupBy": "source", "groupMissing": "keep"}, "groupMissing"), ({"groupBy": 7}, "groupBy")):
        with pytest.raises(SessionError) as e:
            session.search(Q, 3, options)
        assert word in str(e.value), options
        with pytest.raises(SessionError):
            session.search_many([Q], 3, [options])
    with pytest.raises(SessionError):
        session.search(Q, 3000, {"groupBy": "source", "groupSize": 2})  # k * groupSize > 4096


def test_the_next_search_sees_a_delete_and_an_update(ctx):
    session = new_session(ctx)
    options = {"groupBy": "source", "groupSize": 2, "fetchK": 30}
    first = session.search(Q, 3, options)
    assert first["groups"][0]["key"] == "src1" and first["groups"][0]["hits"][0]["id"] == "chunk-1"  # chunk 0 has no source
    session.delete_vector("chunk-1")
    second = session.search(Q, 3, options)
    assert second["groups"][0]["key"] == "src2" and "chunk-1" not in [h["id"] for g in second["groups"] for h in g["hits"]]
    same_groups(second, *by_loop(session, Q, 3, "source", 2, 30), 3, 2)
    session.update_metadata("chunk-2", dict(meta(2), source="moved"))
    session.update_metadata("chunk-0", dict(meta(0), source=1.5))   # chunk 0 gains a key, a float one
    third = session.search(Q, 3, options)
    assert [g["key"] for g in third["groups"]][:2] == [1.5, "moved"]
    same_groups(third, *by_loop(session, Q, 3, "source", 2, 30), 3, 2)
    session.add_vectors([{"id": "late", "vector": [0.0, 0.0, 0.4], "metadata": {"source": "moved", "n": -1}}])
    fourth = session.search(Q, 3, options)
    assert [h["id"] for h in fourth["groups"][0]["hits"]] == ["late", "chunk-2"] and fourth["groups"][0]["key"] == "moved"
