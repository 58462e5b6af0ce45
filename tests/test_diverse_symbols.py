"""Diverse search: the new C entry points are declared, exported and bound with the stated
arguments, the host mirror's wrappers are in HOST_SIGNATURES and exported, and the Python methods exist.  No GPU."""
import ctypes as C
import inspect
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> number of arguments, as include/fvdb.h declares them
C_SYMBOLS = {"fvdb_mmr_select_dev": 15, "fvdb_ivf_get_rows_dev_strided": 7, "fvdb_store_get_rows_dev": 6}
HOST_SYMBOLS = {"fvh_ivf_search_diverse": 15, "fvh_hnsw_search_diverse": 15, "fvh_hybrid_search_diverse": 19,
                "fvh_hybrid_search_diverse_groups": 22, "fvh_set_diverse_stage_bytes": 1, "fvh_diverse_stage_bytes": 0}


def test_the_c_entry_points_are_declared_exported_and_bound():
    fv = fvdb_import.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvdb.h")).read(), flags=re.S)
    lib = fv._capi.load()
    for name, arity in C_SYMBOLS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == arity, f"{name}: declared with another number of arguments"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(fv._capi.SIGNATURES[name][1]) == arity, f"{name}: bound with another number of arguments"
    sig = fv._capi.SIGNATURES
    # lam travels as a C float (a = f32(lam) is the definition's constant), distinct as an int
    assert sig["fvdb_mmr_select_dev"][1][9] is C.c_float and sig["fvdb_mmr_select_dev"][1][10] is C.c_int
    # the strided gather is the plain one with the stride appended
    assert sig["fvdb_ivf_get_rows_dev_strided"][1][:-1] == sig["fvdb_ivf_get_rows_dev"][1]
    assert sig["fvdb_ivf_get_rows_dev_strided"][1][-1] is C.c_uint32
    # the extern "C" block of INTEGRATION.md names them too
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in C_SYMBOLS:
        assert name in doc, f"{name} is missing from INTEGRATION.md"


def test_the_host_mirror_exports_the_diverse_wrappers():
    fv = fvdb_import.load()
    host = fv.load_host()
    sig = fv.index.HOST_SIGNATURES
    for name, arity in HOST_SYMBOLS.items():
        assert name in sig, name
        assert hasattr(host, name), name
        assert len(sig[name][1]) == arity, name
    for name in ("fvh_ivf_search_diverse", "fvh_hnsw_search_diverse", "fvh_hybrid_search_diverse"):
        assert sig[name][1][6] is C.c_float, name  # lam


def test_the_staging_cap_has_a_default_and_a_setter():
    fv = fvdb_import.load()
    if "FVDB_DIVERSE_STAGE_BYTES" not in os.environ:
        assert fv.index.set_diverse_stage_bytes(0) == 256 << 20
    assert fv.index.set_diverse_stage_bytes(12345) == 12345
    fv.index.set_diverse_stage_bytes(0)


def test_the_python_methods_exist():
    fv = fvdb_import.load()
    params = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert params(fv.IVFIndex.search_diverse) == ["self", "queries", "k", "fetch_k", "lam", "distinct", "n_probe", "allowed"]
    assert params(fv.HNSWIndex.search_diverse) == ["self", "queries", "k", "fetch_k", "ef", "lam", "distinct", "allowed"]
    assert params(fv.HybridIndex.search_diverse) == ["self", "queries", "k", "fetch_k", "lam", "distinct", "now", "hnsw_ef",
                                                     "ivf_n_probe", "search_recent", "search_historical", "allowed"]
    for f in (fv.IVFIndex.search_diverse, fv.HNSWIndex.search_diverse, fv.HybridIndex.search_diverse):
        p = inspect.signature(f).parameters
        assert p["lam"].default == 0.5 and p["distinct"].default is True
    assert callable(fv.HybridIndex.search_diverse_groups) and callable(fv.session.diverse_options)


def test_the_session_options_parse_without_a_device():
    fv = fvdb_import.load()
    opt, err = fv.session.diverse_options, fv.session.SessionError
    assert opt({}, 10) is None and opt({"threshold": 0.5, "includeVectors": True}, 10) is None
    assert opt({"distinct": True}, 10) == (40, 1.0, True)          # "distinct" alone: lam = 1, fetchK = min(256, 4 k)
    assert opt({"mmrLambda": 0.5}, 100) == (256, 0.5, True)
    assert opt({"fetchK": 64, "distinct": False}, 10) == (64, 1.0, False)
    assert opt({"mmrLambda": 0.1}, 1)[1] == float(__import__("numpy").float32(0.1))  # lam as the f32 the kernel sees
    for bad in ({"mmrLambda": 1.5}, {"mmrLambda": float("nan")}, {"mmrLambda": -1}, {"fetchK": 9}, {"fetchK": 257}, {"mmrLambda": None}):
        try:
            opt(bad, 10)
        except err:
            continue
        raise AssertionError(f"{bad} was accepted")
