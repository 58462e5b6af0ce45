"""VectorDbSession.search_many(queries, k, options_list): one option set per query, one HybridIndex.search_allowed_groups
call for the batch.  Equal filters share a group and are evaluated once; requests without a filter take the None group."""
import numpy as np
import pytest

import fvdb_import

fv = fvdb_import.load()


class FakeIndex:
    """Records the grouped call, answers query b with rows b, b + 1, ... at distances 0, 1, 3."""

    def __init__(self):
        self.calls = []

    def search_allowed_groups(self, q, k, allow_sets, group_of_query, now=0.0):
        self.calls.append((np.array(q), k, allow_sets, np.array(group_of_query), now))
        B = len(q)
        ids = (np.arange(B)[:, None] + np.arange(k)[None, :]).astype(np.uint64)
        dist = np.tile(np.array([0.0, 1.0, 3.0], np.float32)[:k], (B, 1))
        return fv.index.SearchResults(ids, dist, np.full(B, k, np.uint32))

    def search_allowed(self, *a, **kw):
        raise AssertionError("search_many makes one grouped call")

    search_with_filter = search_allowed


def session_without_gpu(monkeypatch=None):
    s = object.__new__(fv.VectorDbSession)
    s.destroyed = False
    s.vector_dimension = 3
    s.now = 5.0
    s.index = FakeIndex()
    s._rows = {i: f"vec_{i:08x}" for i in range(10)}
    s.metadata = {f"vec_{i:08x}": {"n": i, "tag": "even" if i % 2 == 0 else "odd"} for i in range(9)}  # row 9: no metadata
    return s


PUSH = "pushdown"
Q = [[0.0, 1.0, 0.5], [1.0, 1.0, 0.5], [2.0, 1.0, 0.5], [3.0, 1.0, 0.5], [4.0, 1.0, 0.5]]


def test_equal_filters_share_a_group_and_are_evaluated_once(monkeypatch):
    s = session_without_gpu()
    built = []
    real = fv.session.MetadataFilter.from_json
    monkeypatch.setattr(fv.session.MetadataFilter, "from_json", staticmethod(lambda j: (built.append(j), real(j))[1]))
    opts = [{"filter": {"tag": "even"}, "filterMode": PUSH}, None, {"filter": {"tag": "odd"}, "filterMode": PUSH},
            {"filterMode": PUSH, "filter": {"tag": "even"}}, {}]
    out = s.search_many(Q, 3, opts)
    (q, k, allow_sets, group, now), = s.index.calls
    assert q.shape == (5, 3) and q.dtype == np.float32 and np.array_equal(q[:, 0], [0, 1, 2, 3, 4])
    assert k == 3 and now == 5.0
    assert len(allow_sets) == 3, "even, no filter, odd"
    assert group.tolist() == [0, 1, 2, 0, 1], "one entry per query, in order"
    assert allow_sets[1] is None, "requests without a filter take the None group"
    assert allow_sets[0].dtype == np.uint64 and sorted(allow_sets[0].tolist()) == [0, 2, 4, 6, 8]
    assert sorted(allow_sets[2].tolist()) == [1, 3, 5, 7]
    assert built == [{"tag": "even"}, {"tag": "odd"}], "each distinct filter is built and evaluated once"
    assert len(out) == 5 and all(len(r) == 3 for r in out)
    assert [r["id"] for r in out[2]] == ["vec_00000002", "vec_00000003", "vec_00000004"]


def test_key_order_does_not_split_a_group():
    s = session_without_gpu()
    s.search_many(Q[:2], 1, [{"filter": {"tag": "even", "n": 2}, "filterMode": PUSH},
                             {"filter": {"n": 2, "tag": "even"}, "filterMode": PUSH}])
    (_, _, allow_sets, group, _), = s.index.calls
    assert len(allow_sets) == 1 and group.tolist() == [0, 0] and allow_sets[0].tolist() == [2]


def test_no_filter_anywhere_is_one_none_group():
    s = session_without_gpu()
    s.search_many(Q[:3], 2)
    (_, _, allow_sets, group, _), = s.index.calls
    assert allow_sets == [None] and group.tolist() == [0, 0, 0]


def test_a_filter_without_pushdown_raises():
    s = session_without_gpu()
    for opt in ({"filter": {"tag": "even"}}, {"filter": {"tag": "even"}, "filterMode": "oversample"}):
        with pytest.raises(fv.session.SessionError, match="filterMode"):
            s.search_many(Q[:2], 3, [{}, opt])
    with pytest.raises(fv.session.SessionError, match="Invalid filter"):
        s.search_many(Q[:1], 3, [{"filter": {"$bogus": 1}, "filterMode": PUSH}])
    with pytest.raises(fv.session.SessionError, match="dimension mismatch"):
        s.search_many([[0.0, 1.0]], 3, [{}])
    with pytest.raises(fv.session.SessionError, match="option sets"):
        s.search_many(Q[:2], 3, [{}])
    assert s.index.calls == []


def test_threshold_applies_per_request():
    s = session_without_gpu()
    # distances 0, 1, 3 -> scores 1, 0.5, 0.25
    out = s.search_many(Q[:3], 3, [{"threshold": 0.5}, {}, {"threshold": 0.9}])
    assert [len(r) for r in out] == [2, 3, 1]
    assert [r["score"] for r in out[1]] == [1.0, 0.5, 0.25]
    assert out[0][0]["metadata"] == {"n": 0, "tag": "even"}


def test_empty_batch_and_destroyed_session():
    s = session_without_gpu()
    assert s.search_many([], 3, []) == [] and s.index.calls == []
    s.destroyed = True
    with pytest.raises(fv.session.SessionError, match="destroyed"):
        s.search_many(Q[:1], 3)
