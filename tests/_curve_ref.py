"""The rule of the n_probe curve, restated in numpy over the oracle's own outputs.

Per query, with the lists ranked by a stable argsort of the centroid distances and for p = 1 .. nlist:
  matches(p)    = truth entries (top k of the search of every list) whose list has rank < p
  len_result(p) = min(k, live rows of the first p ranked lists)
  recall(p)     = 1 if the truth is empty, else matches(p) / min(len(truth), k)
  precision(p)  = 0 if len_result(p) == 0, else matches(p) / len_result(p)          (f32 divisions)
It holds for an index in which no id is stored in two lists.  test_nprobe_curve_symbols.py pins it against the oracle's
p-probe searches; test_gpu_nprobe_curve.py takes its expected values from here."""
import numpy as np

import oracle as orc
from _any_nprobe_data import averaged


def live_sizes(ids, cl, nlist, live_ids=None):
    """Live rows per list: rows of `ids` (row i in list cl[i]) whose id is in live_ids (all when None)."""
    cl = np.asarray(cl, np.int64)
    if live_ids is not None:
        cl = cl[np.isin(ids, np.asarray(list(live_ids), np.uint64))]
    return np.bincount(cl, minlength=nlist).astype(np.int64)


def curve_per_query(cpu, q, k, cents, ids, cl, live):
    """(recall [B][nlist], precision [B][nlist], result_len [B][nlist]) by the rule, from ONE search of every list by the
    oracle `cpu`.  ids / cl: every stored row's id and list; live: live rows per list (live_sizes)."""
    nlist = cents.shape[0]
    q = np.ascontiguousarray(q, np.float32)
    B = q.shape[0]
    ti, _, tc = cpu.batch_search(q, k, nlist)
    list_of = dict(zip((int(i) for i in ids), (int(c) for c in cl)))
    assert len(list_of) == len(ids), "the rule needs every id in one list only"
    f32 = np.float32
    recall, precision = np.empty((B, nlist), f32), np.empty((B, nlist), f32)
    length = np.empty((B, nlist), np.int64)
    for b in range(B):
        order = np.argsort(orc.l2_batch(q[b], cents), kind="stable")
        rank_of = np.empty(nlist, np.int64)
        rank_of[order] = np.arange(nlist)
        nt = int(tc[b])
        hist = np.zeros(nlist, np.int64)
        for i in ti[b, :nt]:
            hist[rank_of[list_of[int(i)]]] += 1
        matches = np.cumsum(hist)
        length[b] = np.minimum(k, np.cumsum(live[order]))
        m32 = matches.astype(f32)
        recall[b] = f32(1.0) if nt == 0 else m32 / f32(min(nt, k))
        with np.errstate(divide="ignore", invalid="ignore"):
            precision[b] = np.where(length[b] == 0, f32(0.0), m32 / length[b].astype(f32))
    return recall, precision, length


def curve_sums(values):
    """[nlist] total += value in query order in f32 (src/ivf/operations.rs:379-380), per n_probe."""
    total = np.zeros(values.shape[1], np.float32)
    for row in values:
        total = (total + row.astype(np.float32)).astype(np.float32)
    return total


def curve_averages(values):
    """The sums over B as f32 (:386-387); equal to _any_nprobe_data.averaged of each column."""
    return (curve_sums(values) / np.float32(values.shape[0])).astype(np.float32)


def expected_curve(cpu, q, k, cents, ids, cl, live):
    """avg_recall [nlist], avg_precision [nlist] as IVFIndex.recall_by_nprobe must return them, and the per-query values."""
    recall, precision, _ = curve_per_query(cpu, q, k, cents, ids, cl, live)
    return curve_averages(recall), curve_averages(precision), recall, precision


__all__ = ["live_sizes", "curve_per_query", "curve_sums", "curve_averages", "expected_curve", "averaged"]
