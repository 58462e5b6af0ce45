"""GPU: VectorDbSession.search_within — every row whose f32 score 1/(1+distance) clears the
threshold, with the exact total, where search(k, {"threshold": t}) returns at most k of them.

The session holds 600 rows [i, 1, 0.5] and the query is [0, 1, 0.5]: the distance of row i is exactly i in f32, so the
rows that clear a threshold are known on the CPU from the f32 score alone."""
import numpy as np
import pytest

import fvdb_import

fv = fvdb_import.load()
pytestmark = pytest.mark.gpu
Q = [0.0, 1.0, 0.5]
N = 600


@pytest.fixture(scope="module")
def ctx():
    c = fv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def session(ctx):
    s = fv.VectorDbSession(ctx)
    s.add_vectors([{"id": f"doc-{i}", "vector": [float(i), 1.0, 0.5], "metadata": {"n": i, "tag": "even" if i % 2 == 0 else "odd"}}
                   for i in range(N)])
    return s


def clearing(threshold, keep=lambda i: True):
    """the rows whose f32 score clears the threshold, nearest first, by the session's own arithmetic"""
    t = np.float32(threshold)
    return [i for i in range(N) if keep(i) and np.float32(1.0) / (np.float32(1.0) + np.float32(i)) >= t]


@pytest.mark.parametrize("threshold", [0.02, 1 / 3, 0.5, 1.0, 0.0101, 1 / 601])
def test_every_row_that_clears_the_threshold_comes_back(session, threshold):
    want = clearing(threshold)
    got = session.search_within(Q, threshold)
    assert [r["id"] for r in got["results"]] == [f"doc-{i}" for i in want]
    assert got["total"] == len(want) and got["truncated"] is False
    assert all(np.float32(r["score"]) >= np.float32(threshold) for r in got["results"])
    assert [r["metadata"]["n"] for r in got["results"]] == want
    # search() with the same threshold: at most k of them, and no total
    by_count = session.search(Q, 10, {"threshold": threshold})
    assert len(by_count) == min(10, len(want))
    if len(want) > 10:
        assert len(got["results"]) > len(by_count)


def test_the_total_is_not_capped_and_truncated_says_so(session):
    want = clearing(0.02)
    assert len(want) == 50
    got = session.search_within(Q, 0.02, {"maxResults": 20})
    assert [r["id"] for r in got["results"]] == [f"doc-{i}" for i in want[:20]]
    assert got["total"] == 50 and got["truncated"] is True
    got = session.search_within(Q, 0.02, {"maxResults": 50})
    assert len(got["results"]) == 50 and got["total"] == 50 and got["truncated"] is False
    got = session.search_within(Q, 0.0)  # every score is >= 0
    assert got["total"] == N and len(got["results"]) == N and got["truncated"] is False
    got = session.search_within(Q, -1.0, {"maxResults": 1})
    assert got["total"] == N and [r["id"] for r in got["results"]] == ["doc-0"] and got["truncated"] is True


def test_pushdown_and_resident_filters_agree_and_oversample_is_refused(session):
    flt = {"tag": "even"}
    want = clearing(0.02, keep=lambda i: i % 2 == 0)
    a = session.search_within(Q, 0.02, {"filter": flt, "filterMode": "pushdown"})
    b = session.search_within(Q, 0.02, {"filter": flt, "filterMode": "resident"})
    assert a == b
    assert [r["id"] for r in a["results"]] == [f"doc-{i}" for i in want] and a["total"] == len(want) == 25 and a["truncated"] is False
    assert session.last_filter_info()["route"] == "device"
    c = session.search_within(Q, 0.02, {"filter": {"n": {"$gte": 40}}, "filterMode": "resident", "maxResults": 4})
    assert [r["id"] for r in c["results"]] == ["doc-40", "doc-41", "doc-42", "doc-43"] and c["total"] == 10 and c["truncated"] is True
    none = session.search_within(Q, 0.02, {"filter": {"n": {"$gte": 100}}, "filterMode": "pushdown"})
    assert none == {"results": [], "total": 0, "truncated": False}
    for options in ({"filter": flt, "filterMode": "oversample"}, {"filterMode": "oversample"}, {"filter": flt, "filterMode": "nope"}):
        with pytest.raises(fv.session.SessionError, match="filterMode"):
            session.search_within(Q, 0.02, options)
    with pytest.raises(fv.session.SessionError, match="Invalid filter"):
        session.search_within(Q, 0.02, {"filter": {"$nope": 1}, "filterMode": "pushdown"})


def test_thresholds_that_need_no_device_call_and_the_errors(session, monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("a threshold above 1 needs no device call")

    monkeypatch.setattr(session.index, "search_radius", no_call)
    for t in (1.5, np.nextafter(np.float32(1), np.float32(2)), np.inf):
        assert session.search_within(Q, t) == {"results": [], "total": 0, "truncated": False}
    monkeypatch.undo()
    with pytest.raises(fv.session.SessionError, match="NaN"):
        session.search_within(Q, np.nan)
    with pytest.raises(fv.session.SessionError, match="dimension mismatch"):
        session.search_within([0.0, 1.0], 0.5)
    for m in (0, 4097):
        with pytest.raises(fv.session.SessionError, match="Search failed"):
            session.search_within(Q, 0.5, {"maxResults": m})


def test_include_vectors(session):
    got = session.search_within(Q, 0.3, {"includeVectors": True})
    assert [r["id"] for r in got["results"]] == ["doc-0", "doc-1", "doc-2"]
    assert [r["vector"] for r in got["results"]] == [[float(i), 1.0, 0.5] for i in range(3)]
