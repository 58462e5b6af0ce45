"""IVF searches of more queries than one sub-batch holds.

Every IVF search entry point cuts its batch into sub-batches of at most 16384 queries and advances its pointers per
sub-batch: queries by d, results by k (counts by 1), probe lists by nprobe.  The contract pinned here: one call with B =
16384 + 300 queries returns, bit for bit, what two calls on q[:16384] and q[16384:] return — ids, distance bits, counts
and selection keys — through every entry point, and the plain search equals the CPU oracle on all B queries.  The index is
as small as a second sub-batch allows: 700 rows in 4 lists, among them copies of other rows (equal distances: the order
of ties is part of the result) and soft-deleted rows (short counts)."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits

pytestmark = pytest.mark.gpu

E_NOT_TRAINED, E_INVALID, E_NONFINITE, E_UNSUPPORTED = 1, 6, 9, 12
MAX_K, MAX_K_WIDE = 256, 4096
SUB = 16384            # the most queries one sub-batch holds
B = SUB + 300            # a multiple of NLIST
N, NLIST, NPROBE, K = 700, 4, 2, 10
K_WIDE = MAX_K + 1
# rows, d: f32 rows; fp16 rows; a d the queries are padded for, once per sub-batch; a d the matrix-core filter serves
CASES = {"f32": ("f32", 8), "f16": ("f16", 8), "padded": ("f32", 6), "filter": ("f32", 16)}


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def other(fv, ctx):
    c = fv.Context(0)  # a second stream of the same device: the `on` of the slot entry points
    yield c
    c.close()


def clustered(n_per_list, d, rng):
    """Rows around four far-apart centres, of which the last two are each other's nearest: a query near either probes
    both of those lists."""
    comp = np.repeat(np.arange(NLIST), n_per_list)
    return (CENTRES[d][comp] + np.float32(0.35) * rng.standard_normal((comp.size, d))).astype(np.float32)


CENTRES = {}
for _d in (6, 8, 16):
    _c = (np.random.default_rng(_d).standard_normal((NLIST, _d)) * 4).astype(np.float32)
    _c[3] = _c[2] + np.float32(0.8)
    CENTRES[_d] = _c


class World:
    """One index, its oracle, B queries, a mask admitting about half of the rows, and (refs) the oracle's answers.
    Lists 0 and 1 hold nearly all rows; lists 2 and 3 together fewer than K, so their queries come back short."""

    def __init__(self, fv, ctx, dtype, d, refs=True):
        self.d = d
        rng = np.random.default_rng(70 + d)
        x = clustered([340, 351, 5, 4], d, rng)
        assert x.shape[0] == N
        x[600:650] = x[100:150]  # copies: equal distances within a list
        ids = np.arange(N, dtype=np.uint64) * 3 + 5
        cents = CENTRES[d]
        self.gpu = fv.DeviceIVF(ctx, d, NLIST, dtype=dtype)
        self.gpu.set_centroids(cents)
        self.cpu = orc.IVFIndex(n_clusters=NLIST, n_probe=NPROBE)
        self.cpu.set_trained(cents)
        cl, pos = self.gpu.add(x, ids)
        rows = x.astype(np.float16).astype(np.float32) if dtype == "f16" else x  # what the reference would be given
        self.cpu.batch_insert_assigned(ids, rows, cl)
        dead = np.concatenate([np.arange(7, N, 29), [100, 101, 602, 693]])  # among them one of two copies
        self.gpu.set_deleted(cl[dead], pos[dead], True)
        for i in dead:
            self.cpu.mark_deleted(int(ids[i]))
        q = clustered([B // NLIST] * NLIST, d, rng)
        q = q[rng.permutation(B)]
        q[5:45] = x[100:140]               # queries that are stored rows, in both sub-batches
        q[SUB + 3:SUB + 13] = x[640:650]
        self.q = np.ascontiguousarray(q)
        allowed = np.ascontiguousarray(ids[rng.random(N) < 0.5])
        self.mask = C.c_void_p()
        ctx.check(ctx.lib.fvdb_mask_create_ivf(self.gpu.h, allowed.ctypes.data_as(C.POINTER(C.c_uint64)), allowed.size,
                                               C.byref(self.mask)))
        if refs:
            self.ref = self.cpu.batch_search(q, K, NPROBE, threads=8)
            self.ref_all = self.cpu.batch_search(q, K, NLIST, threads=8)


_worlds = {}


@pytest.fixture(params=list(CASES))
def world(request, fv, ctx):
    if request.param not in _worlds:
        _worlds[request.param] = World(fv, ctx, *CASES[request.param])
    return _worlds[request.param]


def on_device(ctx, q, k, call):
    """call(q_dev, n, ids, dist, counts, keys) on a batch and outputs in HBM -> (ids, distances, counts, keys)."""
    q = np.ascontiguousarray(q, np.float32)
    n = q.shape[0]
    q_dev, out = ctx.upload(q), ctx.alloc(n * k * 20 + n * 4)
    at = lambda off: C.c_void_p(out.value + off)  # noqa: E731
    ids, keys, dist, cnt = at(0), at(n * k * 8), at(n * k * 16), at(n * k * 20)
    try:
        ctx.check(call(q_dev, n, ids, dist, cnt, keys))
        ctx.device_synchronize()
        return (ctx.download(ids, (n, k), np.uint64), ctx.download(dist, (n, k), np.float32),
                ctx.download(cnt, n, np.uint32), ctx.download(keys, (n, k), np.uint64))
    finally:
        ctx.free(q_dev)
        ctx.free(out)


def same_bits(a, b, what):
    names = ("ids", "distances", "counts", "keys")
    for name, u, v in zip(names, a, b):
        u, v = (bits(u), bits(v)) if u.dtype == np.float32 else (u, v)
        assert u.shape == v.shape, f"{what}: {name}: {u.shape} vs {v.shape}"
        diff = np.flatnonzero((u != v).reshape(u.shape[0], -1).any(axis=1))
        assert diff.size == 0, f"{what}: {name} differ at {diff.size} queries, the first of them query {diff[0]}"


def split_equal(q, run, what):
    """run(q) on all B queries equals run(q[:SUB]) and run(q[SUB:]) put together; returns the former."""
    whole, head, tail = run(q), run(q[:SUB]), run(q[SUB:])
    same_bits(whole, tuple(np.concatenate([h, t]) for h, t in zip(head, tail)), what)
    return whole


def same_as_oracle(got, ref, what):
    gi, gd, gc = got[:3]
    oi, od, oc = ref
    assert np.array_equal(gc, oc), f"{what}: hit counts differ from the oracle's"
    live = np.arange(gi.shape[1])[None, :] < oc[:, None]
    assert np.array_equal(gi[live], oi[live]), f"{what}: ids differ from the oracle's"
    assert np.array_equal(bits(gd)[live], bits(od)[live]), f"{what}: distances not bit-identical to the oracle's"


def slot_search(ctx, w, on, slot, k=K):
    lib, h = ctx.lib, w.gpu.h
    return lambda q: on_device(ctx, q, k, lambda qd, n, *out: lib.fvdb_ivf_search_dev_slot(h, on, slot, qd, n, k, NPROBE, *out))


def test_the_batch_needs_a_second_sub_batch(world):
    assert B > SUB and B - SUB < SUB
    assert world.ref[2].min() < K <= world.ref[2].max(), "short and full results"
    near = world.ref[1][5:45]
    assert (bits(near[:, 0]) == bits(near[:, 1])).any(), "two copies of a row at the same distance"


def test_host_search(ctx, world):
    got = split_equal(world.q, lambda q: world.gpu.search(q, K, NPROBE), "fvdb_ivf_search")
    same_as_oracle(got, world.ref, "fvdb_ivf_search")


def test_host_search_all(ctx, world):
    got = split_equal(world.q, lambda q: world.gpu.search_all(q, K), "fvdb_ivf_search_all")
    same_as_oracle(got, world.ref_all, "fvdb_ivf_search_all")


def test_slot_search_on_another_stream(ctx, other, world):
    got = split_equal(world.q, slot_search(ctx, world, other.h, 3), "fvdb_ivf_search_dev_slot")
    same_as_oracle(got, world.ref, "fvdb_ivf_search_dev_slot")


@pytest.mark.parametrize("mode", [1, 2], ids=["exact", "filter"])
def test_slot_search_in_each_scan_mode(ctx, other, world, mode):
    ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(world.gpu.h, mode))
    try:
        got = split_equal(world.q, slot_search(ctx, world, other.h, 2), f"scan mode {mode}")
    finally:
        ctx.check(ctx.lib.fvdb_ivf_set_scan_mode(world.gpu.h, 0))
    same_as_oracle(got, world.ref, f"scan mode {mode}")


def probes_then_search(ctx, w, on, slot, mask=None):
    """fvdb_ivf_coarse_dev_slot into a probe buffer, then the search that is given those probes."""
    lib, h = ctx.lib, w.gpu.h

    def run(q):
        probes = ctx.alloc(q.shape[0] * NPROBE * 4)

        def call(qd, n, *out):
            rc = lib.fvdb_ivf_coarse_dev_slot(h, on, slot, qd, n, NPROBE, probes)
            if rc:
                return rc
            if mask is None:
                return lib.fvdb_ivf_search_probes_dev_slot(h, on, slot, qd, probes, n, K, NPROBE, *out)
            return lib.fvdb_ivf_search_probes_dev_slot_masked(h, on, slot, mask, qd, probes, n, K, NPROBE, *out)

        try:
            return on_device(ctx, q, K, call)
        finally:
            ctx.free(probes)

    return run


def test_coarse_stage_then_search_with_given_probes(ctx, other, world):
    got = split_equal(world.q, probes_then_search(ctx, world, other.h, 5), "coarse + given probes")
    same_bits(got, slot_search(ctx, world, other.h, 5)(world.q), "given probes vs the plain slot search")


def test_masked_searches(ctx, other, world):
    lib, h, mask = ctx.lib, world.gpu.h, world.mask
    run = lambda q: on_device(ctx, q, K, lambda qd, n, *out: lib.fvdb_ivf_search_dev_slot_masked(  # noqa: E731
        h, other.h, 4, mask, qd, n, K, NPROBE, *out))
    got = split_equal(world.q, run, "fvdb_ivf_search_dev_slot_masked")
    given = split_equal(world.q, probes_then_search(ctx, world, other.h, 4, mask=mask), "fvdb_ivf_search_probes_dev_slot_masked")
    same_bits(given, got, "masked: given probes vs the coarse stage of the call")
    plain = slot_search(ctx, world, other.h, 4)(world.q)
    assert got[2].sum() < plain[2].sum(), "the mask took rows away"


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_wide_search(ctx, other, world, masked):
    lib, h = ctx.lib, world.gpu.h
    mask = world.mask if masked else None
    run = lambda q: on_device(ctx, q, K_WIDE, lambda qd, n, *out: lib.fvdb_ivf_search_wide_dev_slot(  # noqa: E731
        h, other.h, 6, mask, qd, n, K_WIDE, NPROBE, *out))
    got = split_equal(world.q, run, "fvdb_ivf_search_wide_dev_slot")
    if not masked:
        same_as_oracle(got, world.cpu.batch_search(world.q, K_WIDE, NPROBE, threads=8), "fvdb_ivf_search_wide_dev_slot")


def test_refusals_keep_their_codes(fv, ctx, other):
    lib = ctx.lib
    d, n = 8, 8
    w = _worlds.get("f32") or World(fv, ctx, "f32", d)
    _worlds.setdefault("f32", w)
    h, mask = w.gpu.h, w.mask
    q = np.ascontiguousarray(w.q[:n])
    q_dev, probes = ctx.upload(q), ctx.alloc(n * NPROBE * 4)
    out_dev = ctx.alloc(n * MAX_K_WIDE * 20 + n * 4)
    at = lambda off: C.c_void_p(out_dev.value + off)  # noqa: E731
    out = (at(0), at(n * MAX_K_WIDE * 16), at(n * MAX_K_WIDE * 20), at(n * MAX_K_WIDE * 8))
    f32p, u64p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    hi, hd, hc = np.empty((n, MAX_K_WIDE + 1), np.uint64), np.empty((n, MAX_K_WIDE + 1), np.float32), np.empty(n, np.uint32)
    host_out = (hi.ctypes.data_as(u64p), hd.ctypes.data_as(f32p), hc.ctypes.data_as(u32p))
    qp = q.ctypes.data_as(f32p)

    def refused(rc, code, text):
        assert rc == code, f"{text!r}: status {rc}, expected {code}"
        assert text in lib.fvdb_last_error(ctx.h), f"{lib.fvdb_last_error(ctx.h)!r} does not say {text!r}"

    # the explicit-slot forms, each on a foreign stream: the failure text is read from the index's own context
    slot = lambda on, s, k=K, nprobe=NPROBE: lib.fvdb_ivf_search_dev_slot(h, on, s, q_dev, n, k, nprobe, *out)  # noqa: E731
    given = lambda p, k=K, nprobe=NPROBE: lib.fvdb_ivf_search_probes_dev_slot(  # noqa: E731
        h, other.h, 1, q_dev, p, n, k, nprobe, *out)
    masked = lambda m, k=K, nprobe=NPROBE: lib.fvdb_ivf_search_dev_slot_masked(  # noqa: E731
        h, other.h, 1, m, q_dev, n, k, nprobe, *out)
    given_masked = lambda m, p, k=K: lib.fvdb_ivf_search_probes_dev_slot_masked(  # noqa: E731
        h, other.h, 1, m, q_dev, p, n, k, NPROBE, *out)
    wide = lambda m, k=K_WIDE, nprobe=NPROBE, s=1, hh=h: lib.fvdb_ivf_search_wide_dev_slot(  # noqa: E731
        hh, other.h, s, m, q_dev, n, k, nprobe, *out)
    coarse = lambda s, p, nprobe=NPROBE: lib.fvdb_ivf_coarse_dev_slot(h, other.h, s, q_dev, n, nprobe, p)  # noqa: E731
    ctx.check(coarse(1, probes))

    for rc in (slot(other.h, 16), coarse(16, probes), wide(None, s=16), wide(mask, s=16),
               lib.fvdb_ivf_search_dev_slot_masked(h, other.h, 16, mask, q_dev, n, K, NPROBE, *out)):
        refused(rc, E_INVALID, b"slot out of range")
    try:
        far = fv.Context(1)
    except fv.FvdbError:
        far = None  # one device visible: nothing to name another device with
    if far is not None:
        refused(slot(far.h, 1), E_INVALID, b"context of another device")
        refused(lib.fvdb_ivf_search_wide_dev_slot(h, far.h, 1, None, q_dev, n, K_WIDE, NPROBE, *out), E_INVALID,
                b"context of another device")
        far.close()
    refused(given(None), E_INVALID, b"null probes")
    refused(given_masked(mask, None), E_INVALID, b"null probes")
    refused(coarse(1, None), E_INVALID, b"null output")

    # masks: of another index, none where one is required, stale
    w2 = World(fv, ctx, "f32", d, refs=False)
    for call in (masked, lambda m: given_masked(m, probes), wide):
        refused(call(w2.mask), E_INVALID, b"mask of another index")
    refused(masked(None), E_INVALID, b"mask of another index")
    refused(given_masked(None, probes), E_INVALID, b"mask of another index")
    stale = C.c_void_p()
    some = np.arange(5, dtype=np.uint64) * 3 + 5
    ctx.check(lib.fvdb_mask_create_ivf(w2.gpu.h, some.ctypes.data_as(u64p), some.size, C.byref(stale)))
    w2.gpu.add(q[:1], np.array([10 ** 9], np.uint64))  # the index changes
    h2 = w2.gpu.h
    refused(lib.fvdb_ivf_search_dev_slot_masked(h2, other.h, 1, stale, q_dev, n, K, NPROBE, *out), E_INVALID, b"stale mask")
    refused(lib.fvdb_ivf_search_probes_dev_slot_masked(h2, other.h, 1, stale, q_dev, probes, n, K, NPROBE, *out), E_INVALID,
            b"stale mask")
    refused(wide(stale, hh=h2), E_INVALID, b"stale mask")
    lib.fvdb_mask_destroy(stale)

    # k and nprobe, by kind
    for k in (0, MAX_K + 1):
        for rc in (slot(other.h, 1, k=k), given(probes, k=k), masked(mask, k=k), given_masked(mask, probes, k=k),
                   lib.fvdb_ivf_search_dev(h, q_dev, n, k, NPROBE, *out), lib.fvdb_ivf_search_all_dev(h, q_dev, n, k, *out[:3]),
                   lib.fvdb_ivf_search(h, qp, n, k, NPROBE, *host_out), lib.fvdb_ivf_search_all(h, qp, n, k, *host_out)):
            refused(rc, E_UNSUPPORTED, b"k must be in 1..FVDB_MAX_K")
    for k in (0, MAX_K_WIDE + 1):
        for rc in (wide(None, k=k), wide(mask, k=k), lib.fvdb_ivf_search_wide(h, qp, n, k, NPROBE, *host_out)):
            refused(rc, E_UNSUPPORTED, b"k must be in 1..FVDB_MAX_K_WIDE")
    for rc in (slot(other.h, 1, nprobe=0), given(probes, nprobe=0), masked(mask, nprobe=0), wide(None, nprobe=0),
               coarse(1, probes, nprobe=0), lib.fvdb_ivf_search(h, qp, n, K, 0, *host_out),
               lib.fvdb_ivf_search_wide(h, qp, n, K_WIDE, 0, *host_out)):
        refused(rc, E_INVALID, b"nprobe must be > 0")

    # a shard of a larger index: the wide search alone refuses it
    w2.gpu.set_global_list_sizes(w2.gpu.list_sizes())
    refused(wide(None, hh=h2), E_UNSUPPORTED, b"does not serve a shard")
    refused(lib.fvdb_ivf_search_wide(h2, qp, n, K_WIDE, NPROBE, *host_out), E_UNSUPPORTED, b"does not serve a shard")
    ctx.check(lib.fvdb_ivf_search_dev_slot(h2, other.h, 1, q_dev, n, K, NPROBE, *out))
    ctx.device_synchronize()

    # an untrained index, and the order of the host form's answers: not trained, nothing to do, k, non-finite input
    raw = fv.DeviceIVF(ctx, d, NLIST)
    for rc in (lib.fvdb_ivf_search_dev_slot(raw.h, other.h, 1, q_dev, n, K, NPROBE, *out),
               lib.fvdb_ivf_search_wide_dev_slot(raw.h, other.h, 1, None, q_dev, n, K_WIDE, NPROBE, *out),
               lib.fvdb_ivf_coarse_dev_slot(raw.h, other.h, 1, q_dev, n, NPROBE, probes),
               lib.fvdb_ivf_search(raw.h, qp, 0, 0, NPROBE, *host_out), lib.fvdb_ivf_search_all(raw.h, qp, n, K, *host_out),
               lib.fvdb_ivf_search_wide(raw.h, qp, n, K_WIDE, NPROBE, *host_out)):
        refused(rc, E_NOT_TRAINED, b"index not trained")
    bad = q.copy()
    bad[3, 2] = np.inf
    bp = bad.ctypes.data_as(f32p)
    assert lib.fvdb_ivf_search(h, bp, 0, 0, NPROBE, *host_out) == 0, "no queries: nothing is looked at"
    assert lib.fvdb_ivf_search_wide(h, bp, 0, MAX_K_WIDE + 1, NPROBE, *host_out) == 0
    refused(lib.fvdb_ivf_search(h, bp, n, 0, NPROBE, *host_out), E_UNSUPPORTED, b"k must be in 1..FVDB_MAX_K")
    refused(lib.fvdb_ivf_search_wide(h, bp, n, 0, NPROBE, *host_out), E_UNSUPPORTED, b"k must be in 1..FVDB_MAX_K_WIDE")
    for rc in (lib.fvdb_ivf_search(h, bp, n, K, NPROBE, *host_out), lib.fvdb_ivf_search_all(h, bp, n, K, *host_out),
               lib.fvdb_ivf_search_wide(h, bp, n, K_WIDE, NPROBE, *host_out), lib.fvdb_ivf_search(h, bp, n, K, 0, *host_out)):
        refused(rc, E_NONFINITE, b"non-finite input value")

    # and after all of it the index answers as before
    same_as_oracle(on_device(ctx, q, K, lambda qd, m, *o: lib.fvdb_ivf_search_dev_slot(h, other.h, 1, qd, m, K, NPROBE, *o)),
                   tuple(a[:n] for a in w.ref), "after the refusals")
    for p in (q_dev, probes, out_dev):
        ctx.free(p)
