"""Grouped search: the new C entry points are declared, exported and bound with the stated
arguments, the host mirror's wrappers are in HOST_SIGNATURES and exported, the Python methods and the session options
exist.  No GPU.

The key lookup is fvdb_group_keys_of_ids_dev: it takes the metadata table, but its name carries the feature's prefix,
because the set of fvdb_meta_ entry points is pinned by test_metadata_columns_symbols.py."""
import ctypes as C
import inspect
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SYMBOLS = {"fvdb_group_keys_of_ids_dev": 6, "fvdb_group_select_dev": 21, "fvdb_group_keys_ctx": 1}
HOST_SYMBOLS = {"fvh_ivf_search_grouped": 24, "fvh_hnsw_search_grouped": 24, "fvh_hybrid_search_grouped": 28}


def test_the_c_entry_points_are_declared_exported_and_bound():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    lib = fv._capi.load()
    for name, arity in C_SYMBOLS.items():
        m = re.search(r"\b(?:int|fvdb_ctx\s*\*)\s*%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == arity, f"{name}: declared with another number of arguments"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(fv._capi.SIGNATURES[name][1]) == arity, f"{name}: bound with another number of arguments"
    sig = fv._capi.SIGNATURES["fvdb_group_select_dev"][1]
    assert sig[10] is C.c_int and sig[11] is C.c_int  # distinct, missing
    assert sig[6:10] == [C.c_uint32] * 4              # B, fetch_k, k, group_size
    defs = dict(re.findall(r"#define (FVDB_GROUP_MISSING_[A-Z]+) (\d+)", header))
    assert defs == {"FVDB_GROUP_MISSING_DROP": "0", "FVDB_GROUP_MISSING_OWN": "1"}
    assert fv.index.GROUP_MISSING == {"drop": 0, "own": 1}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in C_SYMBOLS:
        assert name in doc, f"{name} is missing from INTEGRATION.md"


def test_the_host_mirror_exports_the_grouped_wrappers():
    fv = fvdb_import.load()
    host = fv.load_host()
    sig = fv.index.HOST_SIGNATURES
    for name, arity in HOST_SYMBOLS.items():
        assert name in sig, name
        assert hasattr(host, name), name
        assert len(sig[name][1]) == arity, name
        assert sig[name][1][-9:] == sig["fvh_ivf_search_grouped"][1][-9:], name  # the nine output arrays


def test_the_python_methods_exist():
    fv = fvdb_import.load()
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(fv.IVFIndex.search_grouped) == ["self", "queries", "k", "group_size", "fetch_k", "columns", "path", "distinct",
                                                  "missing", "n_probe", "allowed", "metadata"]
    assert params(fv.HNSWIndex.search_grouped) == ["self", "queries", "k", "group_size", "fetch_k", "ef", "columns", "path",
                                                   "distinct", "missing", "allowed", "metadata"]
    assert params(fv.HybridIndex.search_grouped) == ["self", "queries", "k", "group_size", "fetch_k", "columns", "path", "distinct",
                                                     "missing", "now", "hnsw_ef", "ivf_n_probe", "search_recent", "search_historical",
                                                     "allowed", "metadata"]
    for f in (fv.IVFIndex.search_grouped, fv.HNSWIndex.search_grouped, fv.HybridIndex.search_grouped):
        p = inspect.signature(f).parameters
        assert p["distinct"].default is True and p["missing"].default == "drop"
    mc = fv.metadata_columns
    assert callable(mc.MetaTable.keys_of_ids) and callable(mc.MetadataColumns.decode_key) and callable(mc.MetadataColumns.group_column)


def test_a_key_decodes_to_its_python_value():
    fv = fvdb_import.load()
    mc = fv.metadata_columns
    cols = object.__new__(mc.MetadataColumns)  # no table: decoding needs the dictionary alone
    cols.strings = {"red": 0, "green": 1}
    assert cols.decode_key(mc.STRING, 1) == "green" and cols.decode_key(mc.STRING, 0) == "red"
    cols.strings["blue"] = 2  # a code handed out after the first decode
    assert cols.decode_key(mc.STRING, 2) == "blue"
    assert cols.decode_key(mc.INT, 7) == 7 and cols.decode_key(mc.INT, (1 << 64) - 3) == -3
    assert cols.decode_key(mc.FLOAT, mc.f64_bits(2.5)) == 2.5 and cols.decode_key(mc.FLOAT, 0) == 0.0
    assert cols.decode_key(mc.BOOL, 1) is True and cols.decode_key(mc.BOOL, 0) is False
    assert cols.decode_key(mc.NULL, 0) is None
    for tag, value in ((mc.INT, -3), (mc.INT, 1 << 62), (mc.FLOAT, -1.5), (mc.STRING, "red"), (mc.BOOL, True), (mc.NULL, None)):
        t, payload = mc.encode_scalar(value, cols.strings, False)
        assert t == tag and cols.decode_key(t, payload) == value  # the encoder's inverse


def test_the_results_object_reports_the_two_completeness_facts():
    import numpy as np
    fv = fvdb_import.load()
    z = lambda *s: np.zeros(s, np.uint32)  # noqa: E731
    members = np.asarray([[2, 1], [2, 2], [1, 0]], np.uint32)
    r = fv.index.GroupedResults(np.zeros((3, 2, 2), np.uint64), np.zeros((3, 2, 2), np.float32), z(3, 2, 2), members, members.copy(),
                                np.full((3, 2), 5, np.uint8), np.zeros((3, 2), np.uint64), np.asarray([2, 2, 1], np.uint32),
                                np.asarray([1, 0, 1], np.uint32), 2, 2)
    assert [r.cut(b) for b in range(3)] == [True, False, True]
    assert [r.groups_complete(b) for b in range(3)] == [True, True, False]      # k groups, or a list that was not cut
    assert r.group_complete(0, 0) and not r.group_complete(0, 1) and r.group_complete(1, 1)
    assert len(r[2]) == 1 and r[2][0][0] == 5 and r[2][0][5] == 1 and len(r[0][1][2]) == 1


def test_the_session_options_parse_without_a_device():
    fv = fvdb_import.load()
    opt, err = fv.session.grouped_options, fv.session.SessionError
    assert opt({}, 10) is None and opt({"fetchK": 64}, 10) is None
    assert opt({"groupBy": "doc"}, 10) == ("doc", 1, 40, "drop", False, True)
    assert opt({"groupBy": "a.b", "groupSize": 3, "groupMissing": "own", "fill": True}, 5) == ("a.b", 3, 60, "own", True, True)
    assert opt({"groupBy": "doc", "groupSize": 4}, 1000)[2] == 4096           # min(4096, 4 k groupSize)
    assert opt({"groupBy": "doc", "fetchK": 4096, "distinct": False}, 2) == ("doc", 1, 4096, "drop", False, False)
    assert opt({"groupBy": "doc", "filter": {"x": 1}, "filterMode": "resident"}, 2) is not None
    for bad in ({"groupBy": ""}, {"groupBy": 3}, {"groupBy": "d", "groupSize": 0}, {"groupBy": "d", "groupSize": 2049},
                {"groupBy": "d", "fetchK": 0}, {"groupBy": "d", "fetchK": 4097}, {"groupBy": "d", "groupMissing": "keep"},
                {"groupBy": "d", "mmrLambda": 0.5}, {"groupBy": "d", "exact": True}, {"groupBy": "d", "threshold": 0.5},
                {"groupBy": "d", "filter": {"x": 1}}, {"groupBy": "d", "filter": {"x": 1}, "filterMode": "oversample"}):
        try:
            opt(bad, 2)
        except err:
            continue
        raise AssertionError(f"{bad} was accepted")
