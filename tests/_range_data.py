"""Data of test_gpu_range_edges.py: rows at the ends of the f32 and fp16 ranges, and the conditions a case states about
the oracle's answer before it looks at the device (so that no case can pass while testing nothing).

Every row set is `default_rng(seed).standard_normal((n, d))` as f32 times an exact power of two (or 1e-40: rows that are
subnormal themselves); the first lists' worth of rows are the centroids and query b is x[b] + 0.25 x[B + b]."""
import numpy as np

import oracle as orc
from _data import mixture

F32 = np.float32
TINY, TINIER, HUGE, OVER = F32(2.0 ** -70), F32(2.0 ** -74), F32(2.0 ** 62), F32(2.0 ** 64)
SUBNORMAL = F32(1e-40)

# kind -> (scale at d = 20, scale at d = 128, what the oracle's 10 nearest look like).  At d = 128 a squared sum has six
# times as many terms: 2^61 is the scale at which a query's own row is still at a finite distance and the others are not.
KINDS = {
    "tiny": (TINY, TINY, "distinct_subnormal_sums"),
    "tinier": (TINIER, TINIER, "ties"),
    "subnormal_rows": (SUBNORMAL, SUBNORMAL, "all_zero"),
    "huge": (HUGE, F32(2.0 ** 61), "inf_and_finite"),
    "over": (OVER, OVER, "mostly_inf"),
    "thirds": (None, None, "inf_zero_and_finite"),
}


def base(n=600, d=20, seed=1):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(F32)


def rows(kind, n=600, d=20, seed=1):
    """The rows of `kind`, finite f32 all of them."""
    x = base(n, d, seed)
    scale = KINDS[kind][0 if d <= 20 else 1]
    if scale is None:  # thirds: x 2^64 / x 2^-70 / x 1
        x[::3] *= OVER
        x[1::3] *= TINY
    else:
        x = (x * scale).astype(F32)
    assert np.isfinite(x).all()
    return x


def queries(x, B=16):
    q = (x[:B] + x[B:2 * B] * F32(0.25)).astype(F32)
    assert np.isfinite(q).all()
    return q


def f16_rounded(x):
    with np.errstate(over="ignore"):  # a finite f32 beyond the fp16 range becomes +-Inf: that is the case, not an accident
        return x.astype(np.float16).astype(F32)


def live(res):
    """The entries of (ids, distances, counts) that are results, as a flat array of distances."""
    _, dist, cnt = res
    return dist[np.arange(dist.shape[1])[None, :] < cnt[:, None]]


def distinct_per_query(res):
    _, dist, cnt = res
    return np.array([np.unique(dist[b, :int(cnt[b])].view(np.uint32)).size for b in range(dist.shape[0])])


def assert_oracle(res, what, k=10):
    """The precondition of a case, on the oracle's answer alone.  Every kind: each query has its k results, none NaN."""
    _, dist, cnt = res
    v = live(res)
    assert np.all(cnt == k), f"not every query has {k} results: not this case"
    assert not np.isnan(v).any(), "the oracle returned NaN"
    per_q = dist[:, :k]
    if what == "distinct_subnormal_sums":
        # every distance the root of a subnormal sum (below 2^-63) and none zero; k distinct ones in at least three
        # queries of four and never fewer than k - 1 (at d = 128 the sums are coarse enough for a stray equal pair)
        n_distinct = distinct_per_query(res)
        assert np.all(v > 0) and np.all(v < F32(2.0 ** -63))
        assert np.all(n_distinct >= k - 1) and 4 * int((n_distinct == k).sum()) >= 3 * n_distinct.size
    elif what == "distinct":
        assert np.all(distinct_per_query(res) == k) and np.all(v > 0) and np.isfinite(v).all()
    elif what == "ties":
        # underflow makes distances equal: some query holds fewer than k distinct values
        assert np.any(distinct_per_query(res) < k) and np.isfinite(v).all()
    elif what == "all_zero":
        assert np.all(v.view(np.uint32) == 0)
    elif what == "inf_and_finite":
        # +Inf as a real distance beside finite ones, in at least half the queries
        both = np.isposinf(per_q).any(axis=1) & np.isfinite(per_q).any(axis=1)
        assert 2 * int(both.sum()) >= per_q.shape[0], f"only {int(both.sum())} queries hold +Inf and finite results"
    elif what == "mostly_inf":
        assert np.isposinf(v).mean() > 0.9
    elif what == "inf_zero_and_finite":
        # a third of the queries is huge (everything at +Inf), a third tiny, a third ordinary
        assert np.isposinf(v).any() and np.any(v == 0) and np.any((v > 0) & np.isfinite(v))
    else:
        raise KeyError(what)


def oracle_ivf(x, ids, cents, nprobe=4, clusters=None, stored=None):
    """The oracle over `stored` (default x: what the engine stores) in the lists its own assignment of x gives, or in
    `clusters`; returns it and the list of every row."""
    cpu = orc.IVFIndex(n_clusters=cents.shape[0], n_probe=nprobe)
    cpu.set_trained(cents)
    cl = cpu.assign(x) if clusters is None else np.ascontiguousarray(clusters, np.uint32)
    cpu.batch_insert_assigned(ids, x if stored is None else stored, cl)
    return cpu, cl


def list_order_search(x, ids, cl, q, k, dead=()):
    """What a scan in list-index order keeps (fvdb_ivf_search_all): rows by (list, position), a stable sort by distance,
    the k first — (ids, distances, counts) like a search."""
    keep = np.ones(x.shape[0], bool)
    keep[list(dead)] = False
    order = np.argsort(cl, kind="stable")
    order = order[keep[order]]
    B = q.shape[0]
    oi = np.full((B, k), 2 ** 64 - 1, np.uint64)
    od = np.full((B, k), np.inf, F32)
    m = min(k, order.size)
    for b in range(B):
        dist = orc.l2_batch(q[b], x[order])
        best = np.argsort(dist, kind="stable")[:m]
        oi[b, :m], od[b, :m] = ids[order][best], dist[best]
    return oi, od, np.full(B, m, np.uint32)


def mixed_huge_case(n, d, nlist, B, seed=1):
    """Unit-scale mixture rows, six of them (rows B .. B+5) times 2^64: |x|^2 overflows and the fp16 mirror is +-Inf.  Their own
    nearest centroid is a tie of +Inf distances (list 0), so the lists are given: the oracle's assignment, but the six in
    lists 0, 1, 2, 0, 1, 2.  Query b sits near row b; the last query IS huge row B, which those three lists hold: under
    the reference's fold its distance to that row is 0.0 and to every other row +Inf, while the matrix cores say NaN."""
    x = mixture(n, d, seed=seed)  # clustered, so that the filter has something to discard
    huge = np.arange(B, B + 6)
    x[huge] *= OVER
    assert np.isfinite(x).all() and np.isinf(f16_rounded(x[huge])).all()
    ids = np.arange(n, dtype=np.uint64) * 3 + 1
    cents = x[n - nlist:].copy()  # unit-scale rows
    cpu0 = orc.IVFIndex(n_clusters=nlist, n_probe=4)
    cpu0.set_trained(cents)
    cl = cpu0.assign(x)
    assert np.all(cl[huge] == 0)  # the tie the docstring speaks of
    cl[huge] = np.arange(6) % 3
    q = (x[:B] + F32(0.05) * base(B, d, seed + 1)).astype(F32)
    q[B - 1] = x[huge[0]]
    return x, ids, cents, cl, q, huge


def assert_mixed_huge_oracle(res, ids, huge, k=10):
    oi, od, oc = res
    B = oi.shape[0]
    assert np.all(oc == k) and not np.isnan(od).any()
    assert np.isfinite(od[:B - 1]).all(), "a query near normal rows has its k finite neighbours"
    assert oi[B - 1, 0] == ids[huge[0]] and od[B - 1, 0] == 0.0 and np.isposinf(od[B - 1, 1:]).all()


# ---- fp16 storage -----------------------------------------------------------------------------------------------------
def f16_case(kind, n=600, d=20, seed=1):
    """Finite f32 rows whose fp16 roundings are subnormal ("f16_subnormal"), the largest finite values ("f16_max") or
    +-Inf ("f16_overflow")."""
    x = base(n, d, seed)
    if kind == "f16_subnormal":
        x = (x * F32(2e-6)).astype(F32)
        r = f16_rounded(x)
        assert np.all(np.abs(r) < F32(2.0 ** -14)) and np.unique(r).size > 100  # subnormal or zero, yet many values
    elif kind == "f16_max":
        x = (x * F32(100)).astype(F32)
        x[40:48, 3], x[48:56, 0], x[56:64, 7] = 65504.0, 65519.0, -65504.0
        x[3, 3], x[5, 0], x[7, 7] = 65504.0, 65519.0, -65504.0  # among the queries' own rows too
        r = f16_rounded(x)
        assert np.isfinite(r).all() and r[48, 0] == 65504.0 and (np.abs(r) == 65504.0).sum() == 27
    elif kind == "f16_overflow":
        x = (x * F32(100)).astype(F32)
        x[40:48, 3], x[48:56, 0], x[56:64, 7] = 65520.0, -65520.0, 70000.0
        x[3, 3], x[5, 0] = 65520.0, -65520.0
        r = f16_rounded(x)
        assert np.isfinite(x).all() and np.isinf(r).sum() == 26 and np.isposinf(r[40, 3]) and np.isneginf(r[48, 0])
    else:
        raise KeyError(kind)
    return x, r


def f16_short_list_case(d=20, B=32, seed=1):
    """The rows of f16_case("f16_overflow") in 8 lists, searched with nprobe = 1.  List 7 lies far from the rest (its
    centroid is 1000 in every dimension) and is given four finite rows near that centroid and 24 rows that hold, mixed in
    sign, values rounding to +-Inf.  The last eight queries sit at that centroid: they probe list 7 alone, so their 10
    nearest are its four finite rows and then six rows at +Inf, in scan order."""
    n, nlist = 600, 8
    x = (base(n, d, seed) * F32(100)).astype(F32)
    over = np.arange(40, 64)
    near = np.arange(64, 68)
    noise = base(n, d, seed + 1)
    x[over, 3] = np.where(over % 2 == 0, 65520.0, -65520.0)
    x[over, 0] = np.where(over % 3 == 0, 70000.0, -70000.0)
    x[over, 7] = 65520.0
    x[near] = F32(1000) + noise[near]
    r = f16_rounded(x)
    assert np.isfinite(x).all() and np.isinf(r[over]).sum() == 3 * over.size and np.isfinite(np.delete(r, over, 0)).all()
    cents = x[:nlist].copy()
    cents[7] = F32(1000)
    ids = np.arange(n, dtype=np.uint64) * 3 + 1
    cpu0 = orc.IVFIndex(n_clusters=nlist, n_probe=1)
    cpu0.set_trained(cents)
    cl = cpu0.assign(x)
    cl[over] = 7
    assert set(np.flatnonzero(cl == 7).tolist()) == set(over.tolist()) | set(near.tolist())  # and nothing else
    q = queries(x, B)
    q[B - 8:] = F32(1000) + noise[100:108]
    return x, r, ids, cents, cl, q


def assert_f16_short_list_oracle(res, k=10):
    _, od, oc = res
    assert np.all(oc[-8:] == k) and np.all(oc > 0) and not np.isnan(live(res)).any()
    assert np.isfinite(od[-8:, :4]).all() and np.isposinf(od[-8:, 4:]).all(), "not four finite rows, then +Inf"


# ---- utilities -----------------------------------------------------------------------------------------------------------
EDGE_SCORES = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4e38], F32)
EDGE_ORDER = [2, 6, 4, 0, 1, 5, 3]  # the oracle's top_k_indices of EDGE_SCORES


def edge_scores(n, seed):
    """n scores drawn from EDGE_SCORES (every one of them, repeated), the first seven being EDGE_SCORES itself."""
    rng = np.random.default_rng(seed)
    s = EDGE_SCORES[rng.integers(0, EDGE_SCORES.size, n)]
    s[:7] = EDGE_SCORES
    return np.ascontiguousarray(s, F32)


def cosine_pairs(size):
    """(name, a, b, what the oracle's cosine is) at `size` dimensions."""
    full = lambda v: np.full(size, v, F32)  # noqa: E731
    return [("subnormal norm product", full(2.0 ** -70), full(2.0 ** -72), "one"),
            ("just above underflow", full(2.0 ** -40), full(2.0 ** -41), "near_one"),
            ("zero norm", full(2.0 ** -80), full(2.0 ** -80), "zero"),
            ("overflow", full(2.0 ** 64), full(2.0 ** 64), "nan")]
