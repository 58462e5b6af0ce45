"""fvdb_graph_search_info (the traversal's plan, read-only): declared in the header, exported, in the ctypes table with
the struct laid out as the header lays it out, and reachable as HNSWIndex.search_info.  No GPU needed."""
import ctypes as C
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "fvdb.h")).read()


def test_the_entry_is_declared_exported_and_bound():
    fv = fvdb_import.load()
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+fvdb_graph_search_info\s*\(\s*fvdb_graph\s*\*\s*g\s*,\s*uint32_t\s+B\s*,\s*uint32_t\s+ef\s*,"
                     r"\s*fvdb_graph_search_info_t\s*\*\s*out\s*\)\s*;", text)
    lib = fv._capi.load()
    assert hasattr(lib, "fvdb_graph_search_info")
    res, args = fv._capi.SIGNATURES["fvdb_graph_search_info"]
    assert res is C.c_int and args == [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(fv._capi.GraphSearchInfo)]
    assert callable(fv.HNSWIndex.search_info)


def test_the_struct_is_laid_out_as_the_header_says():
    fv = fvdb_import.load()
    body = re.search(r"typedef struct fvdb_graph_search_info_t \{(.*?)\} fvdb_graph_search_info_t;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for ctype, names in re.findall(r"\b(uint32_t|uint64_t)\s+([^;]+);", body):
        declared += [(n.strip(), {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64}[ctype]) for n in names.split(",")]
    info = fv._capi.GraphSearchInfo
    assert [(n, t) for n, t in info._fields_] == declared
    assert [n for n, _ in declared] == ["visited", "kernel", "nb128", "rows_per_round", "nearest_in_registers", "tcap",
                                        "cand_cap", "spill_cap", "lds_bytes", "reserved", "visited_bytes"]
    assert C.sizeof(info) == 48 and info.visited_bytes.offset == 40 and info.lds_bytes.offset == 32
    # the values of the two enumerations the Python surface names
    for name, value in (("FVDB_GRAPH_VISITED_BYTES", 1), ("FVDB_GRAPH_VISITED_BITS", 2), ("FVDB_GRAPH_KERNEL_SORTED", 1),
                        ("FVDB_GRAPH_KERNEL_HEAPS", 2)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), header()), name


def test_the_thresholds_stand_in_one_place():
    """one decision function: the launch path and the report read the same 2^30, ef <= 63 and rows-per-round table"""
    src = open(os.path.join(ROOT, "fabstir-vectordb_amd", "csrc", "fvdb_graph.cpp")).read()
    assert src.count("1ull << 30") == 1 and src.count("ef <= 63 &&") == 1
    assert len(re.findall(r"\? 12 : \(", src)) == 1  # the R table
    assert len(re.findall(r"\bsearch_plan\(g, ctx, B, ef, &sp\)", src)) == 2  # graph_search_slot and fvdb_graph_search_info
