"""The Python statement of grouped selection (tests/_group_cases.py) against hand-built cases
whose answers are written out literally.  No GPU: this is what the GPU tests are measured with."""
import numpy as np

import _group_cases as G
from _group_cases import BOOL, DROP, FLOAT, INT, MISSING, NO_ID, NO_ROW, NULL, OWN, STRING

INF = float("inf")


def run(tags, vals, k, gs, ids=None, count=None, fetch_k=None, distinct=True, missing=DROP, dist=None):
    n = len(tags)
    fetch_k = n if fetch_k is None else fetch_k
    ids = list(range(100, 100 + n)) if ids is None else ids
    dist = [float(c) for c in range(n)] if dist is None else dist
    pad = fetch_k - n
    out = G.select_one(np.asarray(ids + [0] * pad, np.uint64), np.asarray(dist + [0.0] * pad, np.float32), n if count is None else count,
                       np.asarray(tags + [0] * pad, np.uint8), np.asarray(vals + [0] * pad, np.uint64), fetch_k, k, gs, distinct, missing)
    return dict(zip(G.NAMES, (o.tolist() if isinstance(o, np.ndarray) else o for o in out)))


def test_every_candidate_one_key():
    r = run([STRING] * 4, [9] * 4, k=2, gs=3)
    assert r["ids"] == [[100, 101, 102], [NO_ID] * 3]
    assert r["dist"] == [[0.0, 1.0, 2.0], [INF] * 3]
    assert r["rank"] == [[0, 1, 2], [NO_ROW] * 3]
    assert r["members"] == [3, 0] and r["total"] == [4, 0]
    assert r["key_tag"] == [STRING, 0] and r["key_val"] == [9, 0]
    assert r["groups"] == 1 and r["flags"] == 1


def test_every_candidate_its_own_key():
    r = run([INT] * 4, [5, 6, 7, 8], k=3, gs=2)
    assert r["ids"] == [[100, NO_ID], [101, NO_ID], [102, NO_ID]]
    assert r["rank"] == [[0, NO_ROW], [1, NO_ROW], [2, NO_ROW]]
    assert r["members"] == [1, 1, 1] and r["total"] == [1, 1, 1]
    assert r["key_val"] == [5, 6, 7] and r["groups"] == 3


def test_three_interleaved_keys():
    r = run([STRING] * 7, [2, 0, 1, 0, 2, 2, 1], k=3, gs=2)
    assert r["rank"] == [[0, 4], [1, 3], [2, 6]]      # groups by their first member; members in position order
    assert r["ids"] == [[100, 104], [101, 103], [102, 106]]
    assert r["total"] == [3, 2, 2] and r["members"] == [2, 2, 2]
    assert r["key_val"] == [2, 0, 1] and r["groups"] == 3
    r = run([STRING] * 7, [2, 0, 1, 0, 2, 2, 1], k=2, gs=1)
    assert r["rank"] == [[0], [1]] and r["total"] == [3, 2] and r["groups"] == 2


def test_the_four_one_like_values_are_four_groups():
    one = G.f64_bits(1.0)
    r = run([INT, FLOAT, STRING, BOOL, INT, FLOAT], [1, one, 1, 1, 1, one], k=6, gs=2)
    assert r["groups"] == 4
    assert r["rank"][:4] == [[0, 4], [1, 5], [2, NO_ROW], [3, NO_ROW]]
    assert r["key_tag"][:4] == [INT, FLOAT, STRING, BOOL] and r["key_val"][:4] == [1, one, 1, 1]


def test_plus_and_minus_zero_are_one_group_and_a_nan_is_none():
    pz, nz, nan = G.f64_bits(0.0), G.f64_bits(-0.0), G.f64_bits(float("nan"))
    assert G.cell_key(FLOAT, nz) == (FLOAT, pz) == G.cell_key(FLOAT, pz)
    assert G.cell_key(FLOAT, nan) is None and G.cell_key(FLOAT, nan | (1 << 63)) is None
    assert G.cell_key(FLOAT, G.f64_bits(float("inf"))) == (FLOAT, 0x7FF0000000000000)
    assert G.cell_key(NULL, 12345) == (NULL, 0)
    assert G.cell_key(MISSING, 0) is None and G.cell_key(G.ARRAY, 3) is None and G.cell_key(G.COMPLEX, 0) is None
    # through the lookup: slots 0..3 hold +0.0, -0.0, NaN and 2.5; id 13 is in no slot; slot 4 is not present
    slot_ids = [10, 11, 12, 14, 15]
    tags, keys = G.keys_of_ids([10, 11, 12, 13, 14, 15, NO_ID], slot_ids, [1, 1, 1, 1, 0], [FLOAT] * 5,
                               [pz, nz, nan, G.f64_bits(2.5), pz])
    assert tags.tolist() == [FLOAT, FLOAT, MISSING, MISSING, FLOAT, MISSING, MISSING]
    assert keys.tolist() == [pz, pz, 0, 0, G.f64_bits(2.5), 0, 0]
    r = run(tags.tolist()[:3], keys.tolist()[:3], k=2, gs=2)
    assert r["rank"] == [[0, 1], [NO_ROW, NO_ROW]] and r["groups"] == 1 and r["total"] == [2, 0]


def test_a_duplicated_id_answers_from_its_lowest_slot():
    tags, keys = G.keys_of_ids([7, 0], [7, 0, 7], [1, 1, 1], [INT, STRING, INT], [1, 2, 3])
    assert tags.tolist() == [INT, STRING] and keys.tolist() == [1, 2]
    tags, keys = G.keys_of_ids([7], [7, 7], [0, 1], [INT, INT], [1, 3])  # the lowest slot is absent: none, not the next copy
    assert tags.tolist() == [MISSING] and keys.tolist() == [0]


def test_distinct_on_and_off_with_a_repeated_id():
    ids = [100, 101, 100, 102, 100]
    on = run([STRING] * 5, [1, 1, 1, 2, 1], k=2, gs=4, ids=ids, distinct=True)
    assert on["rank"] == [[0, 1, NO_ROW, NO_ROW], [3, NO_ROW, NO_ROW, NO_ROW]]
    assert on["total"] == [2, 1] and on["members"] == [2, 1]
    off = run([STRING] * 5, [1, 1, 1, 2, 1], k=2, gs=4, ids=ids, distinct=False)
    assert off["rank"] == [[0, 1, 2, 4], [3, NO_ROW, NO_ROW, NO_ROW]]
    assert off["ids"][0] == [100, 101, 100, 100] and off["total"] == [4, 1]
    # a later copy is dropped before its key is looked at: it opens no group even under another key
    moved = run([STRING] * 3, [1, 2, 3], k=3, gs=1, ids=[100, 100, 101], distinct=True)
    assert moved["rank"] == [[0], [2], [NO_ROW]] and moved["key_val"] == [1, 3, 0] and moved["groups"] == 2


def test_missing_drop_and_own():
    tags, vals = [MISSING, STRING, MISSING, STRING, STRING], [0, 4, 0, 4, 5]
    drop = run(tags, vals, k=4, gs=2, missing=DROP)
    assert drop["rank"] == [[1, 3], [4, NO_ROW], [NO_ROW] * 2, [NO_ROW] * 2]
    assert drop["groups"] == 2 and drop["key_tag"] == [STRING, STRING, 0, 0]
    own = run(tags, vals, k=4, gs=2, missing=OWN)
    assert own["rank"] == [[0, NO_ROW], [1, 3], [2, NO_ROW], [4, NO_ROW]]
    assert own["groups"] == 4 and own["total"] == [1, 2, 1, 1]
    assert own["key_tag"] == [MISSING, STRING, MISSING, STRING] and own["key_val"] == [0, 4, 0, 5]
    # FVDB_NO_ID has no key whatever its key arrays say
    r = run([STRING, STRING], [4, 4], k=2, gs=2, ids=[NO_ID, 100], missing=DROP)
    assert r["rank"] == [[1, NO_ROW], [NO_ROW, NO_ROW]] and r["total"] == [1, 0]
    # a tag beyond STRING is none as well
    r = run([G.ARRAY, G.COMPLEX, 9, INT], [1, 1, 1, 1], k=2, gs=1, missing=DROP)
    assert r["rank"] == [[3], [NO_ROW]] and r["groups"] == 1


def test_counts_and_the_flags_they_give():
    tags, vals = [STRING] * 4, [1, 2, 1, 3]
    zero = run(tags, vals, k=2, gs=2, count=0)
    assert zero["groups"] == 0 and zero["flags"] == 0 and zero["members"] == [0, 0] and zero["ids"] == [[NO_ID] * 2] * 2
    less = run(tags, vals, k=2, gs=2, count=3)
    assert less["flags"] == 0 and less["rank"] == [[0, 2], [1, NO_ROW]] and less["groups"] == 2
    full = run(tags, vals, k=2, gs=2, count=4)
    assert full["flags"] == 1 and full["rank"] == [[0, 2], [1, NO_ROW]]
    over = run(tags, vals, k=3, gs=1, count=9)  # a count beyond fetch_k is fetch_k
    assert over["flags"] == 1 and over["rank"] == [[0], [1], [3]] and over["total"] == [2, 1, 1]


def test_position_order_only():
    r = run([STRING] * 4, [1, 2, 1, 2], k=2, gs=2, dist=[9.0, 1.0, 0.5, 7.0])
    assert r["rank"] == [[0, 2], [1, 3]] and r["dist"] == [[9.0, 0.5], [1.0, 7.0]]


def test_the_population_builders_do_what_their_names_say():
    n = 300
    for kind in G.POPULATIONS:
        tag, val = G.population(kind, n, 3)
        assert tag.shape == val.shape == (n,) and tag.dtype == np.uint8 and val.dtype == np.uint64
    words = G.colliding_words(STRING, n, 9, 5)
    assert len(set(words)) == 9 and len({G.table_cell(w, STRING, n) for w in words}) == 1
    tag, val = G.population("low_bits", n, 1)
    assert len(set((val & np.uint64(0xFFFFFFFF)).tolist())) == 1 and len(set(val.tolist())) == 5
    tag, val = G.population("tags", n, 1)
    assert len(set(zip(tag.tolist(), val.tolist()))) == 5
    assert G.population("none_every_second", n, 1)[0][::2].max() == MISSING
