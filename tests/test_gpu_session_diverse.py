"""GPU: the session's diverse-search options "mmrLambda", "fetchK" and "distinct" (DESIGN.md section 9u), against
HybridIndex.search_diverse, which test_gpu_diverse_search.py holds to the numpy reference.

The session holds 300 chunks in 100 passages of three near-copies: chunk i is [i // 3, 0.01 * (i % 3), 0.5] and the
query is the origin, so the nearest chunks are paraphrases of one passage and a diverse search has something to do.  (The
query is deliberately no stored row: from a query that IS the first pick every other candidate has m = dq, and at
lam = 0.5 every gain is exactly 0.)"""
import numpy as np
import pytest

import fvdb_import

fv = fvdb_import.load()
pytestmark = pytest.mark.gpu
Q = [0.0, 0.0, 0.0]
N = 300
SessionError = fv.session.SessionError


def vec(i):
    return [float(i // 3), 0.01 * (i % 3), 0.5]


@pytest.fixture(scope="module")
def ctx():
    c = fv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def session(ctx):
    s = fv.VectorDbSession(ctx)
    s.add_vectors([{"id": f"chunk-{i}", "vector": vec(i), "metadata": {"n": i, "passage": i // 3, "tag": "even" if i % 2 == 0 else "odd"}}
                   for i in range(N)])
    return s


def original_id(session, rid):
    """the caller's id of row `rid`, as _results_of reports it"""
    key = session._rows[rid]
    md = session.metadata.get(key, {})
    return md["_originalId"] if isinstance(md.get("_originalId"), str) else key


def index_level(session, q, k, fetch_k, lam, distinct, allowed=None):
    """what HybridIndex.search_diverse returns for one query, as (names, f32 scores) in pick order"""
    res, ranks = session.index.search_diverse(np.asarray(q, np.float32).reshape(1, -1), k, fetch_k, lam, distinct, now=session.now,
                                              allowed=allowed)
    n = int(res.counts[0])
    names = [original_id(session, int(i)) for i in res.ids[0, :n]]
    scores = [float(np.float32(1.0) / (np.float32(1.0) + d)) for d in res.distances[0, :n]]
    return names, scores


def ids_of(results):
    return [r["id"] for r in results]


def test_the_three_options_are_the_index_level_call(session):
    for options, (fetch_k, lam, distinct) in (({"mmrLambda": 0.5, "fetchK": 20}, (20, 0.5, True)),
                                              ({"mmrLambda": 0.25}, (20, 0.25, True)),  # fetchK defaults to min(256, 4 k)
                                              ({"mmrLambda": 0.0, "fetchK": 7, "distinct": False}, (7, 0.0, False)),
                                              ({"fetchK": 12}, (12, 1.0, True)),        # no mmrLambda: no re-ranking
                                              ({"distinct": True}, (20, 1.0, True))):
        got = session.search(Q, 5, options)
        names, scores = index_level(session, Q, 5, fetch_k, lam, distinct)
        assert ids_of(got) == names and [r["score"] for r in got] == scores, options
        assert [r["metadata"]["n"] for r in got] == [int(n.split("-")[1]) for n in names]
    # the plain search returns the paraphrases of the first two passages; the diverse one spreads over passages
    plain = session.search(Q, 5)
    assert sorted(r["metadata"]["passage"] for r in plain) == [0, 0, 0, 1, 1]
    diverse = session.search(Q, 5, {"mmrLambda": 0.5, "fetchK": 20})
    assert len({r["metadata"]["passage"] for r in diverse}) >= 4 and diverse[0]["id"] == "chunk-0"
    # "distinct" alone is lam = 1: the first k of the search of fetchK (no id repeats in this session), in search order
    assert ids_of(session.search(Q, 5, {"distinct": True})) == ids_of(session.search(Q, 20))[:5]
    assert ids_of(session.search(Q, 5, {"distinct": False})) == ids_of(session.search(Q, 20))[:5]


def test_results_come_in_pick_order_and_the_threshold_applies_afterwards(session):
    options = {"mmrLambda": 0.5, "fetchK": 20}
    picks = session.search(Q, 6, options)
    scores = [r["score"] for r in picks]
    assert scores != sorted(scores, reverse=True)  # pick order, not nearest first
    t = sorted(scores)[2]
    kept = session.search(Q, 6, dict(options, threshold=t))
    assert kept == [r for r in picks if np.float32(r["score"]) >= np.float32(t)] and 0 < len(kept) < len(picks)


def test_include_vectors(session):
    got = session.search(Q, 4, {"mmrLambda": 0.5, "fetchK": 16, "includeVectors": True})
    for r in got:
        assert r["vector"] == [float(np.float32(v)) for v in vec(r["metadata"]["n"])]


def test_filters_pushdown_and_resident(session):
    flt = {"tag": "even"}
    allowed = np.array([rid for rid in session._rows if int(original_id(session, rid).split("-")[1]) % 2 == 0], np.uint64)
    a = session.search(Q, 5, {"mmrLambda": 0.5, "fetchK": 20, "filter": flt, "filterMode": "pushdown"})
    b = session.search(Q, 5, {"mmrLambda": 0.5, "fetchK": 20, "filter": flt, "filterMode": "resident"})
    assert a == b and len(a) == 5 and all(r["metadata"]["tag"] == "even" for r in a)
    names, scores = index_level(session, Q, 5, 20, 0.5, True, allowed=allowed)
    assert ids_of(a) == names and [r["score"] for r in a] == scores
    for options in ({"filter": flt}, {"filter": flt, "filterMode": "oversample"}):
        with pytest.raises(SessionError, match="filterMode"):
            session.search(Q, 5, dict(options, mmrLambda=0.5))
    with pytest.raises(SessionError, match="Invalid filter"):
        session.search(Q, 5, {"distinct": True, "filter": {"$nope": 1}, "filterMode": "pushdown"})


def test_refusals(session):
    with pytest.raises(SessionError, match="exact"):
        session.search(Q, 5, {"mmrLambda": 0.5, "exact": True})
    for bad in (1.5, -0.1, float("nan"), "x"):
        with pytest.raises(SessionError, match="mmrLambda"):
            session.search(Q, 5, {"mmrLambda": bad})
    for bad in (4, 257, 0):
        with pytest.raises(SessionError, match="fetchK"):
            session.search(Q, 5, {"fetchK": bad})
    with pytest.raises(SessionError, match="fetchK"):
        session.search(Q, 0, {"distinct": True})
    with pytest.raises(SessionError, match="dimension mismatch"):
        session.search([0.0, 1.0], 5, {"distinct": True})
    assert 0 < len(session.search(Q, 256, {"mmrLambda": 0.5})) <= 256  # fetchK defaults to min(256, 4 k); the walk yields <= ef rows


def test_search_many_uniform_and_mixed(session):
    qs = [Q, [3.0, 0.0, 0.5], [50.0, 0.02, 0.5], [99.0, 0.0, 0.5]]
    options = {"mmrLambda": 0.5, "fetchK": 20}
    many = session.search_many(qs, 5, [dict(options) for _ in qs])
    assert many == [session.search(q, 5, options) for q in qs]
    # per-request threshold, includeVectors and filter are allowed to differ; the three options are not
    per = [dict(options), dict(options, threshold=0.2), dict(options, includeVectors=True),
           dict(options, filter={"tag": "odd"}, filterMode="pushdown")]
    many = session.search_many(qs, 5, per)
    assert many == [session.search(q, 5, o) for q, o in zip(qs, per)]
    assert all(r["metadata"]["tag"] == "odd" for r in many[3]) and "vector" in many[2][0]
    two = [dict(options, filter={"tag": "odd"}, filterMode="resident"), dict(options, filter={"tag": "even"}, filterMode="resident")]
    assert session.search_many(qs[:2], 5, two) == [session.search(q, 5, o) for q, o in zip(qs, two)]
    for mixed in ([dict(options), {}], [dict(options), dict(options, mmrLambda=0.25)], [dict(options), dict(options, fetchK=21)],
                  [dict(options), dict(options, distinct=False)], [{}, {"distinct": True}]):
        with pytest.raises(SessionError, match="same values"):
            session.search_many(qs[:2], 5, mixed)
    with pytest.raises(SessionError, match="filterMode"):
        session.search_many(qs[:2], 5, [dict(options, filter={"tag": "odd"}), dict(options)])
