"""The hand-built cases of test_gpu_exact_wide.py, kept apart from it so that
test_exact_wide_data.py can prove on the CPU, with _exact_ref.fold_distances, that they have the properties the GPU
tests lean on: a GPU failure is then never a data accident.

  cut_case(d, dtype)   4500 rows (71 tiles of 64, the last part-filled) with duplicated rows, 33 queries of which four
                       sit ON duplicated rows, and their reference distances
  tie_case(dtype)      the d = 10 graph of cut_case with rows 100..699 overwritten by ONE vector `v` (representable in
                       fp16, so an fp16 index stores it unchanged); q_on = v itself: 600 distance words of bits 0;
                       q_50: a query with exactly 50 rows strictly nearer than the group, found by search below
  same_rows_case()     300 identical rows: every distance word of a query is the same word
"""
import functools

import numpy as np

from _data import mixture
import _exact_ref as R

N = 4500
DUPS = [(3, 4), (10, 11), (10, 12), (255, 256), (700, 2100)]  # test_gpu_exact_search.py's
GROUP = slice(100, 700)  # the tie group: 600 nodes
NEARER = 50


def stored(x, dtype):
    return R.rounded(x) if dtype == "f16" else np.asarray(x, np.float32)


@functools.lru_cache(maxsize=None)
def cut_case(d, dtype):
    x = R.with_duplicates(mixture(N, d, n_comp=8, seed=d), DUPS)
    ids = np.arange(N, dtype=np.uint64) + 1000
    # 29 free queries, then four ON duplicated rows (x, not the stored rows: see test_gpu_exact_search.big_case)
    q = np.concatenate([mixture(29, d, n_comp=8, seed=d + 1), x[[10, 255, 700, 3]]])
    return x, ids, q, R.fold_distances(q, stored(x, dtype))


def strictly_nearer(dist_row, group_word):
    """rows of one query whose distance word is below the group's"""
    return int((np.ascontiguousarray(dist_row, np.float32).view(np.uint32) < group_word).sum())


@functools.lru_cache(maxsize=None)
def tie_case(dtype):
    """(x, ids, v, q_on, q_50): x[GROUP] == v; dist(q_on, v) has bits 0; exactly NEARER rows outside the group are
    strictly nearer to q_50 than the group is.  q_50 and v are found by search: q_50 is a row of the data rounded to
    fp16, v = q_50 moved along one axis by a step between q_50's 50th and 51st nearest other rows, rounded to fp16; the
    first (query, axis, sign) for which the property holds on the STORED rows of both row types is taken."""
    d = 10
    x0 = cut_case(d, "f32")[0]
    ids = np.arange(N, dtype=np.uint64) + 1000
    outside = np.ones(N, bool)
    outside[GROUP] = False
    for cand in range(1000, 1200):
        q = R.rounded(x0[cand])
        per_type = [np.sort(R.fold_distances(q[None], stored(x0[outside], t))[0]) for t in ("f32", "f16")]
        lo = max(p[NEARER - 1] for p in per_type)
        hi = min(p[NEARER] for p in per_type)
        if not lo < hi:
            continue
        step = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        for axis in range(d):
            for sign in (1, -1):
                v = q.copy()
                v[axis] = q[axis] + np.float32(sign) * step
                v = R.rounded(v)
                g = R.fold_distances(q[None], v[None])[0, 0]
                if lo < g < hi:
                    x = x0.copy()
                    x[GROUP] = v
                    return x, ids, v, v.copy(), q
    raise AssertionError("no query with exactly %d rows strictly nearer than the tie group" % NEARER)


def tie_dist(dtype):
    """reference distances of (q_on, q_50) to the stored rows of tie_case(dtype)"""
    x, _, _, q_on, q_50 = tie_case(dtype)
    return R.fold_distances(np.stack([q_on, q_50]), stored(x, dtype))


@functools.lru_cache(maxsize=None)
def same_rows_case():
    d, n = 10, 300
    row = mixture(1, d, n_comp=1, seed=77)[0]
    x = np.tile(row, (n, 1)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64) * 7 + 3
    q = mixture(3, d, n_comp=1, seed=78)
    return x, ids, q, R.fold_distances(q, x)
