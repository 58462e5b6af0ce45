"""GPU: the session's "exact" search option and evaluate_search_quality.

The data make the plain search miss by construction, whatever walks or scans it: 16 inverted lists whose centroids are
+-e_i in 8 dimensions, each holding ONE row close to the origin (at t * centroid, t = 0.100 .. 0.175) and 30 rows around
its centroid (distance ~1 from the origin).  A query at the origin has those 16 rows as its 16 nearest, one per list; the
session's search probes the default 10 lists, so it cannot return more than 10 of them, while the exact search scores
every resident row.  All of these rows are historical from the start (the graph does not hold them); 40 further rows
added through add_vectors are recent, so the exact search's two parts both contribute."""
import inspect

import numpy as np
import pytest

import fvdb_import
from _data import bits
import _exact_ref as R

pytestmark = pytest.mark.gpu

DAY = 86400.0
D, NLIST, PER_LIST = 8, 16, 30


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def lists_data():
    rng = np.random.default_rng(4242)
    cent = np.concatenate([np.eye(D, dtype=np.float32), -np.eye(D, dtype=np.float32)])
    near = np.stack([np.float32(0.100 + 0.005 * m) * cent[m] for m in range(NLIST)])
    bulk = np.concatenate([cent[m] + np.float32(0.05) * rng.standard_normal((PER_LIST, D)).astype(np.float32)
                           for m in range(NLIST)])
    x = np.concatenate([near, bulk]).astype(np.float32)
    docs = (np.float32(5.0) * cent[0] + np.float32(0.05) * rng.standard_normal((40, D)).astype(np.float32)).astype(np.float32)
    q_origin = (np.float32(0.001) * rng.standard_normal(D)).astype(np.float32)
    q_docs = (np.float32(5.0) * cent[0]).astype(np.float32)
    return cent, x, docs, q_origin, q_docs


@pytest.fixture(scope="module")
def session(fv, ctx):
    cent, x, docs, q_origin, q_docs = lists_data()
    now = 100 * DAY
    s = fv.VectorDbSession(ctx, now=now, max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=NLIST)
    s.index.set_ivf_centroids(cent)
    ids = np.arange(x.shape[0], dtype=np.uint64) + 1
    s.index.bulk_insert(ids, x, np.full(ids.size, now - 30 * DAY), now)  # older than the threshold: straight to the lists
    assert s.index.historical_count() == ids.size and s.index.recent_count() == 0
    s.add_vectors([{"id": f"doc-{i}", "vector": docs[i].tolist(), "metadata": {"i": i}} for i in range(docs.shape[0])])
    assert s.index.recent_count() == docs.shape[0]
    names = [f"row_{int(i)}" for i in ids] + [f"doc-{i}" for i in range(docs.shape[0])]
    yield s, np.concatenate([x, docs]), names, q_origin, q_docs
    s.destroy()


def numpy_top(q, rows, names, k):
    """[(id, score)] of the k nearest rows: the reference fold, score = 1 / (1 + distance) in f32 as the session computes it"""
    d = R.fold_distances(q[None], rows)[0]
    order = np.lexsort((np.arange(d.size), bits(d)))[:k]
    return [(names[i], float(np.float32(1.0) / (np.float32(1.0) + d[i]))) for i in order]


def test_exact_option_returns_the_numpy_top_20_and_the_plain_search_does_not(session):
    s, rows, names, q_origin, q_docs = session
    default_n_probe = inspect.signature(s.index.search).parameters["ivf_n_probe"].default
    assert default_n_probe < NLIST, "the session's searches probe every list: the plain search would be exact too"
    want = numpy_top(q_origin, rows, names, 20)
    assert [n for n, _ in want[:16]] == [f"row_{i}" for i in range(1, 17)], "the 16 nearest rows are the near rows, one per list"
    got = s.search(q_origin.tolist(), 20, {"exact": True})
    assert [(r["id"], r["score"]) for r in got] == want
    plain = s.search(q_origin.tolist(), 20)
    missed = set(n for n, _ in want) - set(r["id"] for r in plain)
    print(f"plain search misses {len(missed)} of the exact top 20")
    assert len(missed) >= 1, "the plain search found the whole exact top 20: the test shows nothing"
    assert s.search(q_origin.tolist(), 20, {"exact": False}) == plain
    # the recent part: rows added through add_vectors come back under their own ids, with their metadata
    got = s.search(q_docs.tolist(), 20, {"exact": True})
    want = numpy_top(q_docs, rows, names, 20)
    assert [(r["id"], r["score"]) for r in got] == want and all(r["id"].startswith("doc-") for r in got)
    assert all(r["metadata"] == {"i": int(r["id"][4:])} for r in got)


def test_exact_option_at_k_300_threshold_and_vectors(session):
    s, rows, names, q_origin, _ = session
    got = s.search(q_origin.tolist(), 300, {"exact": True})
    assert [(r["id"], r["score"]) for r in got] == numpy_top(q_origin, rows, names, 300)
    # threshold and includeVectors are applied as ever
    want = numpy_top(q_origin, rows, names, 300)
    thr = want[15][1]  # the score of the 16th: the 16 near rows pass
    got = s.search(q_origin.tolist(), 300, {"exact": True, "threshold": thr, "includeVectors": True})
    assert [r["id"] for r in got] == [n for n, sc in want if sc >= np.float32(thr)] and len(got) == 16
    for r in got:
        assert np.array_equal(np.asarray(r["vector"], np.float32), rows[names.index(r["id"])])


def test_exact_with_filter_is_refused(fv, session):
    s, _, _, q_origin, _ = session
    with pytest.raises(fv.session.SessionError) as e:
        s.search(q_origin.tolist(), 20, {"exact": True, "filter": {"i": 1}})
    assert '"exact"' in str(e.value) and '"filter"' in str(e.value)


def test_evaluate_search_quality_agrees_with_the_index_call(fv, session):
    s, rows, _, q_origin, q_docs = session
    qs = np.stack([q_origin, q_docs, rows[20], rows[400]])
    for k, index_call in ((20, s.index.evaluate_search_quality), (300, s.index.evaluate_search_quality_wide)):
        a = s.evaluate_search_quality([q.tolist() for q in qs], k)
        b = index_call(qs, k, now=s.now)
        print(f"k={k}: session {a['avg_recall']}, {a['avg_precision']}; index {b['avg_recall']}, {b['avg_precision']}")
        assert bits(a["avg_recall"]) == bits(b["avg_recall"]) and bits(a["avg_precision"]) == bits(b["avg_precision"])
        assert a["queries_evaluated"] == 4
    assert s.evaluate_search_quality([q_origin.tolist()], 20)["avg_recall"] < 1.0
    c = s.evaluate_search_quality([q_origin.tolist()], 20, {"ivfNProbe": NLIST})
    assert c["avg_recall"] == np.float32(1.0)
    with pytest.raises(fv.session.SessionError):
        s.evaluate_search_quality([], 20)
