"""Shared by the GPU tests of the graph-health job: an index's figures, unreachable ids, labels and raw per-node arrays
against the Python reference (tests/_graph_health_ref.py) on that index's own export."""
import ctypes as C

import numpy as np

import _graph_health_ref as ref

NO_LABEL = 2 ** 64 - 1


def reference_of(h):
    """-> (exported ids, (figures, reached, label)) from export_graph(), the deleted flags and the entry point"""
    gi, lv, off, nb = h.export_graph()
    deleted = [int(i) for i in gi if h.is_deleted(int(i))]
    entry = h.entry_point()
    if entry is not None and entry not in set(gi.tolist()):
        entry = None  # lost to a vacuum
    return gi, ref.graph_health(gi, lv, off, nb, deleted, entry)


def raw_nodes(fv, h, n, want_reached=True, want_label=True):
    """fvdb_graph_health_nodes of the last job -> (status, reached, label)"""
    lib = fv._capi.load()
    reached, label = np.full(max(n, 1), 7, np.uint8), np.full(max(n, 1), 7, np.uint32)
    rc = lib.fvdb_graph_health_nodes(h._graph(), reached.ctypes.data_as(C.POINTER(C.c_uint8)) if want_reached else None,
                                     label.ctypes.data_as(C.POINTER(C.c_uint32)) if want_label else None)
    return rc, reached[:n], label[:n]


def agrees(fv, h, path, known=None):
    """every integer figure, the unreachable ids, the labels (and, on the device, the raw per-node arrays) against the
    Python reference on the index's own export (known: that reference, computed before for an index that exports the
    same graph); returns (figures of the job, figures of the reference)"""
    gi, (f, reached, label) = known or reference_of(h)
    got = h.graph_health()
    assert got["path"] == path
    for k in ref.INT_FIELDS:
        assert got[k] == f[k], (k, got[k], f[k])
    assert got["degree0_hist"] == f["degree0_hist"]
    if path == "device":
        assert got["launches"] >= got["reach_launches"] and got["host_syncs"] == got["reach_launches"] + 1
        if got["n_nodes"] == len(gi) == h.store_rows():  # node index = export index: the raw arrays line up
            rc, r, l = raw_nodes(fv, h, len(gi))
            assert rc == 0
            assert r.tolist() == reached and l.tolist() == label
    live = [not h.is_deleted(int(i)) for i in gi]
    assert h.unreachable_ids().tolist() == [int(gi[u]) for u in range(len(gi)) if live[u] and not reached[u]]
    ids, labels = h.component_labels()
    assert ids.tolist() == gi.tolist()
    assert labels.tolist() == [NO_LABEL if x == ref.NONE32 else int(gi[x]) for x in label]
    return got, f
