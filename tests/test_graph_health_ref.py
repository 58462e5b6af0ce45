"""No GPU needed: the Python statement of the graph-health definitions (tests/_graph_health_ref.py) against answers worked
out by hand.  The GPU tests compare the device job and the host mirror with this reference, so it is pinned here first."""
import pytest

import _graph_health_ref as ref

CASES = ref.hand_built_cases()
REQUIRED = ("one_node", "two_mutual", "island_points_in", "island_one_way_in", "deleted_bridge", "deleted_entry",
            "inbound_on_layer_1_only", "dangling_entries", "no_live_node", "entry_lost")


def test_the_table_holds_every_case():
    assert sorted(CASES) == sorted(REQUIRED)


@pytest.mark.parametrize("name", REQUIRED)
def test_reference_gives_the_hand_computed_answer(name):
    levels, lists, deleted, entry, expect = CASES[name]
    ids = [100 + i for i in range(len(levels))]
    off, nb = ref.csr(levels, lists)
    f, reached, label = ref.graph_health(ids, levels, off, [100 + x for x in nb], [100 + x for x in deleted],
                                         None if entry is None else 100 + entry)
    for k in ref.INT_FIELDS:
        assert f[k] == expect[k], (name, k, f[k], expect[k])
    hist = [0] * 65
    for b, c in expect["hist"].items():
        hist[b] = c
    assert f["degree0_hist"] == hist
    assert reached == expect["reached"]
    assert label == expect["label"]


def test_unreachable_is_n_live_minus_reachable_and_histogram_sums_to_n_live():
    for name, (levels, lists, deleted, entry, expect) in CASES.items():
        assert expect["unreachable_live"] == expect["n_live"] - expect["reachable_live"], name
        assert sum(expect["hist"].values()) == expect["n_live"], name


def test_the_last_histogram_bin_is_64_or_more():
    levels = [0] * 71
    lists = [[list(range(1, 71))]] + [[[0]] for _ in range(70)]  # node 0 names 70 nodes
    off, nb = ref.csr(levels, lists)
    f, reached, label = ref.graph_health(list(range(71)), levels, off, nb, [], 0)
    assert f["degree0_hist"][64] == 1 and f["degree0_hist"][1] == 70 and sum(f["degree0_hist"]) == 71
    assert f["reachable_live"] == 71 and f["components0"] == 1 and f["reach_rounds0"] == 2
