"""The wide search (k up to FVDB_MAX_K_WIDE) is declared, exported and bound: header, library and ctypes table agree."""
import os
import re

import fvdb_import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = ("fvdb_ivf_search_wide_dev_slot", "fvdb_ivf_search_wide")


def header():
    return open(os.path.join(ROOT, "include", "fvdb.h")).read()


def test_header_declares_the_wide_entries_and_their_limit():
    text = header()
    assert re.search(r"^#define\s+FVDB_MAX_K_WIDE\s+4096u\s*$", text, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in WIDE:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/fvdb.h"
    assert re.search(r"^#define\s+FVDB_MAX_K\s+256u\s*$", text, flags=re.M), "the register path keeps its limit"


def test_ctypes_table_lists_them():
    fv = fvdb_import.load()
    for name in WIDE:
        assert name in fv._capi.SIGNATURES
    slot_form = fv._capi.SIGNATURES["fvdb_ivf_search_wide_dev_slot"][1]
    assert len(slot_form) == 12, "ivf, ctx, slot, mask, q, B, k, nprobe and four outputs"


def test_built_library_exports_them():
    fv = fvdb_import.load()
    lib = fv._capi.load()
    for name in WIDE:
        assert hasattr(lib, name), f"{name} is not exported by libfvdb_hip.so"
