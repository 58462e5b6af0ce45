"""The metadata-column entry points (include/fvdb.h, "metadata columns"): declared in the header, exported by the library,
listed in the ctypes table, and the header's constants equal the Python module's.  No GPU, no compute calls."""
import ctypes as C
import os
import re

import fvdb_import

fv = fvdb_import.load()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fvdb_meta_add_column", "fvdb_meta_create", "fvdb_meta_destroy", "fvdb_meta_eval", "fvdb_meta_eval_dev", "fvdb_meta_eval_fetch",
         "fvdb_meta_info", "fvdb_meta_set_cells", "fvdb_meta_set_present", "fvdb_meta_set_rows"]


def header():
    return open(os.path.join(ROOT, "include", "fvdb.h")).read()


def test_header_library_and_ctypes_table_agree():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fvdb_meta_[a-z0-9_]+)\s*\(", code)))
    assert declared == NAMES
    assert sorted(n for n in fv._capi.SIGNATURES if n.startswith("fvdb_meta_")) == NAMES
    lib = fv._capi.load()
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported by libfvdb_hip.so"
    # argument counts of the table against the declarations
    for n in NAMES:
        args = re.search(r"\b" + n + r"\s*\(([^)]*)\)", code).group(1)
        assert len(fv._capi.SIGNATURES[n][1]) == len([a for a in args.split(",") if a.strip()]), n


def test_constants_match_the_header():
    mc = fv.metadata_columns
    defs = {k: int(v) for k, v in re.findall(r"#define (FVDB_META_[A-Z_]+) (\d+)u", header())}
    want = {"MISSING": mc.MISSING, "NULL": mc.NULL, "BOOL": mc.BOOL, "INT": mc.INT, "FLOAT": mc.FLOAT, "STRING": mc.STRING,
            "ARRAY": mc.ARRAY, "COMPLEX": mc.COMPLEX, "NEVER": mc.NEVER, "OP_EQUALS": mc.OP_EQUALS, "OP_IN": mc.OP_IN,
            "OP_RANGE": mc.OP_RANGE, "OP_AND": mc.OP_AND, "OP_OR": mc.OP_OR, "IN_HAS_COMPLEX": mc.IN_HAS_COMPLEX,
            "IN_HAS_ANY": mc.IN_HAS_ANY, "RANGE_HAS_MIN": mc.RANGE_HAS_MIN, "RANGE_MIN_INCLUSIVE": mc.RANGE_MIN_INCLUSIVE,
            "RANGE_HAS_MAX": mc.RANGE_HAS_MAX, "RANGE_MAX_INCLUSIVE": mc.RANGE_MAX_INCLUSIVE, "MAX_PROGRAM": mc.MAX_PROGRAM,
            "MAX_STACK": mc.MAX_STACK, "MAX_CONSTS": mc.MAX_CONSTS}
    assert defs == {"FVDB_META_" + k: v for k, v in want.items()}
    assert C.sizeof(fv._capi.MetaInfo) == 48  # six uint64: fvdb_meta_info_t


def test_session_validates_the_new_mode_without_a_gpu():
    s = object.__new__(fv.VectorDbSession)  # made without __init__: the other modes must not need the new attributes
    s.destroyed, s.vector_dimension, s.now = False, 3, 0.0
    assert s.last_filter_info() is None
    s.refresh_metadata_columns()
    try:
        s.search([0.0, 1.0, 0.5], 3, {"filter": {"tag": "even"}, "filterMode": "device"})
    except fv.session.SessionError as e:
        assert "Invalid filterMode" in str(e) and "resident" in str(e)
    else:
        raise AssertionError('"device" must stay invalid')


def test_a_table_that_cannot_follow_the_map_is_dropped():
    class Broken:
        closed = False

        def set_absent_many(self, rids):
            raise RuntimeError("engine error")

        def close(self):
            self.closed = True

    class Index:
        def delete(self, rid, now):
            pass

    s = object.__new__(fv.VectorDbSession)
    s.destroyed, s.now, s.index = False, 0.0, Index()
    s.metadata = {"vec_a": {"_originalId": "a", "tag": "x"}, "vec_b": {"_originalId": "b", "tag": "y"}}
    s._rows = {}
    cols = s._meta_columns = Broken()
    assert s.delete_by_metadata({"tag": "x"}) == {"deleted_count": 1, "deleted_ids": ["a"]}  # the call's own outcome stands
    assert s._meta_columns is None and cols.closed and list(s.metadata) == ["vec_b"]         # rebuilt by the next resident filter
