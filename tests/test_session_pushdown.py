"""VectorDbSession.search(..., {"filter": f, "filterMode": "pushdown"}): the filter is evaluated over the metadata map once
and goes down as an allow-set (HybridIndex.search_allowed); absent or "oversample" is the reference's path
(HybridIndex.search_with_filter), untouched."""
import numpy as np
import pytest

import fvdb_import

fv = fvdb_import.load()


class FakeIndex:
    """Records which search the session called, and with what."""

    def __init__(self):
        self.calls = []

    def _empty(self, k):
        return fv.index.SearchResults(np.zeros((1, k), np.uint64), np.zeros((1, k), np.float32), np.zeros(1, np.uint32))

    def search_with_filter(self, q, k, matches, now=0.0):
        self.calls.append(("search_with_filter", matches))
        return self._empty(k)

    def search_allowed(self, q, k, allowed, now=0.0):
        self.calls.append(("search_allowed", np.array(allowed)))
        return self._empty(k)


def session_without_gpu():
    s = object.__new__(fv.VectorDbSession)
    s.destroyed = False
    s.vector_dimension = 3
    s.now = 0.0
    s.index = FakeIndex()
    s._rows = {i: f"vec_{i:08x}" for i in range(10)}
    s.metadata = {f"vec_{i:08x}": {"n": i, "tag": "even" if i % 2 == 0 else "odd"} for i in range(9)}  # row 9: no metadata
    return s


def test_filter_mode_is_validated():
    s = session_without_gpu()
    for bad in ("device", "", None, 3):
        with pytest.raises(fv.session.SessionError, match="Invalid filterMode"):
            s.search([0.0, 1.0, 0.5], 3, {"filter": {"tag": "even"}, "filterMode": bad})
    assert s.index.calls == []


def test_default_and_oversample_take_the_reference_path():
    s = session_without_gpu()
    s.search([0.0, 1.0, 0.5], 3)
    s.search([0.0, 1.0, 0.5], 3, {"filter": {"tag": "even"}})
    s.search([0.0, 1.0, 0.5], 3, {"filter": {"tag": "even"}, "filterMode": "oversample"})
    s.search([0.0, 1.0, 0.5], 3, {"filterMode": "pushdown"})  # no filter: nothing to push down
    assert [c[0] for c in s.index.calls] == ["search_with_filter"] * 4
    assert s.index.calls[0][1] is None and s.index.calls[3][1] is None
    assert s.index.calls[1][1](2) and not s.index.calls[1][1](3) and not s.index.calls[1][1](9)


def test_pushdown_hands_the_matching_ids_down():
    s = session_without_gpu()
    s.search([0.0, 1.0, 0.5], 3, {"filter": {"tag": "even"}, "filterMode": "pushdown"})
    (name, allowed), = s.index.calls
    assert name == "search_allowed" and allowed.dtype == np.uint64
    assert sorted(allowed.tolist()) == [0, 2, 4, 6, 8]
    s.search([0.0, 1.0, 0.5], 3, {"filter": {"tag": "none"}, "filterMode": "pushdown"})
    assert s.index.calls[1][1].size == 0
    with pytest.raises(fv.session.SessionError, match="Invalid filter"):
        s.search([0.0, 1.0, 0.5], 3, {"filter": {"$bogus": 1}, "filterMode": "pushdown"})


@pytest.mark.gpu
def test_session_pushdown_end_to_end():
    ctx = fv.Context(0)
    s = fv.VectorDbSession(ctx)
    n = 400
    s.add_vectors([{"id": f"doc-{i}", "vector": [float(i), 1.0, 0.5], "metadata": {"n": i, "rare": i % 50 == 7}}
                   for i in range(n)])
    flt = {"rare": True}
    want = [f"doc-{i}" for i in range(n) if i % 50 == 7]  # 8 rows, nearest first from the origin
    pushed = s.search([0.0, 1.0, 0.5], 5, {"filter": flt, "filterMode": "pushdown"})
    assert [r["id"] for r in pushed] == want[:5]
    assert all(r["metadata"]["rare"] is True for r in pushed)
    assert pushed[0]["score"] == float(np.float32(1.0) / (np.float32(1.0) + np.float32(7.0)))
    over = s.search([0.0, 1.0, 0.5], 5, {"filter": flt})  # 15 candidates hold one match
    assert [r["id"] for r in over] == want[:1]
    assert [r["id"] for r in s.search([0.0, 1.0, 0.5], 100, {"filter": flt, "filterMode": "pushdown"})] == want
    assert s.search([0.0, 1.0, 0.5], 5, {"filter": {"n": -1}, "filterMode": "pushdown"}) == []
    s.delete_vector("doc-7")  # the cached masks are stale now: rebuilt, and the deleted row is gone
    assert [r["id"] for r in s.search([0.0, 1.0, 0.5], 5, {"filter": flt, "filterMode": "pushdown"})] == want[1:6]
    s.destroy()
    ctx.close()
