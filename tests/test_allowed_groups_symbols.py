"""Batched filtered search, one allow-set per query: the grouped entry points are declared,
exported and bound, and the index classes and the session have their methods.  No GPU needed."""
import inspect
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = {"fvdb_ivf_search_groups_dev_slot": 14, "fvdb_graph_scan_allowed_groups_dev_slot": 12}
HOST = ("fvh_ivf_search_allowed_groups", "fvh_hnsw_search_allowed_groups", "fvh_hybrid_search_allowed_groups")


def test_engine_symbols_are_declared_exported_and_bound():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    lib = fv._capi.load()
    for name, nargs in ENGINE.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in include/fvdb.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in fv._capi.SIGNATURES and len(fv._capi.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported by the engine"
    # the single-mask entry points keep the arguments they had
    assert len(fv._capi.SIGNATURES["fvdb_ivf_search_wide_dev_slot"][1]) == 12
    assert len(fv._capi.SIGNATURES["fvdb_graph_scan_allowed_dev_slot"][1]) == 10


def test_header_points_from_the_single_mask_rule_to_the_grouped_calls():
    text = open(os.path.join(ROOT, "include", "fvdb.h")).read()
    rule = text[text.index("One mask serves a whole batch call"):][:400]
    for name in ENGINE:
        assert name in rule, f"the single-mask rule does not point at {name}"


def test_host_mirror_wrappers_are_present():
    fv = fvdb_import.load()
    host = fv.load_host()
    for name in HOST:
        assert name in fv.index.HOST_SIGNATURES, name
        assert hasattr(host, name), f"{name} is not exported by the host mirror"
    assert len(fv.index.HOST_SIGNATURES["fvh_ivf_search_allowed_groups"][1]) == 14
    assert len(fv.index.HOST_SIGNATURES["fvh_hnsw_search_allowed_groups"][1]) == 14
    assert len(fv.index.HOST_SIGNATURES["fvh_hybrid_search_allowed_groups"][1]) == 18


def test_python_surface():
    fv = fvdb_import.load()
    want = {
        fv.IVFIndex: ["queries", "k", "allow_sets", "group_of_query", "n_probe"],
        fv.HNSWIndex: ["queries", "k", "ef", "allow_sets", "group_of_query"],
        fv.HybridIndex: ["queries", "k", "allow_sets", "group_of_query", "now", "hnsw_ef", "ivf_n_probe", "search_recent",
                         "search_historical"],
    }
    for cls, names in want.items():
        p = list(inspect.signature(cls.search_allowed_groups).parameters)
        assert p == ["self"] + names, cls.__name__
    p = list(inspect.signature(fv.VectorDbSession.search_many).parameters)
    assert p[:3] == ["self", "query_vectors", "k"] and p[3] == "options_list"
