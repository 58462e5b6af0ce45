"""Sharded search at any k and nprobe, and under an allow-set.

The wide selection on a shard (fvdb_ivf_search_shard_wide_dev_slot) writes keys by the LOGICAL index's scan position, the
wide merge (fvdb_merge_keys_wide_dev) places every entry by lower bounds, and fvdb_ivf_search_sharded_wide_begin puts the
two behind the exchanges of the sharded step.  Shards are emulated as in test_gpu_configs.py: G DeviceIVFs on one device,
plan_list_shards, set_global_list_sizes.  Every comparison is bit for bit — ids, distance bits, counts, and keys where
keys are returned — against the unsharded index on the same GPU and against the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
import oracle as orc
from _data import bits, mixture

pytestmark = pytest.mark.gpu

E_INVALID = 6
NO_ID = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
DAY = 86400.0
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    orc.build()
    c = fv.Context(0)
    yield c
    c.close()


def at(p, off):
    return C.c_void_p(p.value + off)


def assert_same(got, ref, what=""):
    gi, gd, gc = got
    ci, cd, cc = ref
    assert np.array_equal(gc, cc), f"{what}: hit counts differ: {gc[:8]} vs {cc[:8]}"
    for q in range(gi.shape[0]):
        n = int(cc[q])
        assert np.array_equal(gi[q, :n], ci[q, :n]), f"{what}: query {q}: ids differ"
        assert np.array_equal(bits(gd[q, :n]), bits(cd[q, :n])), f"{what}: query {q}: distances not bit-identical"
        assert np.all(gi[q, n:] == NO_ID) and np.all(np.isposinf(gd[q, n:])), f"{what}: query {q}: tail not padded"


def assert_equal(got, ref, what=""):
    assert np.array_equal(got[2], ref[2]), f"{what}: counts differ"
    assert np.array_equal(got[0], ref[0]), f"{what}: ids differ"
    assert np.array_equal(bits(got[1]), bits(ref[1])), f"{what}: distances not bit-identical"


def make_mask(ctx, ivf, allowed):
    a = np.ascontiguousarray(allowed, np.uint64)
    m = C.c_void_p()
    ctx.check(ctx.lib.fvdb_mask_create_ivf(ivf.h, a.ctypes.data_as(u64p), a.size, C.byref(m)))
    return m


class Sharded:
    """One logical index three ways: whole on the GPU, in G shards on the same GPU, and in the CPU oracle."""

    def __init__(self, fv, ctx, x, ids, cents, G, dtype="f32", owner=None):
        nlist, d = cents.shape
        self.fv, self.ctx, self.G, self.ids = fv, ctx, G, ids
        self.cpu = orc.IVFIndex(n_clusters=nlist, n_probe=min(4, nlist))
        self.cpu.set_trained(cents)
        self.cl = np.ascontiguousarray(self.cpu.assign(x), np.uint32)
        rows = x.astype(np.float16).astype(np.float32) if dtype == "f16" else x
        self.cpu.batch_insert_assigned(ids, rows, self.cl)
        self.sizes = np.bincount(self.cl, minlength=nlist).astype(np.uint64)
        self.owner = fv.sharded.plan_list_shards(self.sizes, G) if owner is None else owner
        self.whole = fv.DeviceIVF(ctx, d, nlist, dtype=dtype)
        self.whole.set_centroids(cents)
        self.wpos = self.whole.add_assigned(x, ids, self.cl)
        self.shards, self.mine, self.spos = [], [], []
        for g in range(G):
            sh = fv.DeviceIVF(ctx, d, nlist, dtype=dtype)
            sh.set_centroids(cents)
            mine = np.flatnonzero(self.owner[self.cl] == g)
            self.spos.append(sh.add_assigned(x[mine], ids[mine], self.cl[mine]) if mine.size else np.zeros(0, np.uint32))
            sh.set_global_list_sizes(self.sizes)
            self.shards.append(sh)
            self.mine.append(mine)

    def delete(self, rows):
        """Soft-delete rows (indices into x) in all three."""
        rows = np.asarray(rows)
        self.whole.set_deleted(self.cl[rows], self.wpos[rows], True)
        for g in range(self.G):
            sel = np.isin(self.mine[g], rows)
            if sel.any():
                self.shards[g].set_deleted(self.cl[self.mine[g][sel]], self.spos[g][sel], True)
        for i in rows:
            self.cpu.mark_deleted(int(self.ids[i]))

    def partials(self, q, k, nprobe, masks=None, wide=True):
        """Every shard's partial result: keys, ids (G x B x k, still on the device) and the host copies with counts."""
        ctx, G, B = self.ctx, self.G, q.shape[0]
        qd = ctx.upload(q)
        keys_all, ids_all = ctx.alloc(G * B * k * 8), ctx.alloc(G * B * k * 8)
        sd, sc = ctx.alloc(G * B * k * 4), ctx.alloc(G * B * 4)
        for g, sh in enumerate(self.shards):
            o = g * B * k
            if wide:
                sh.search_shard_wide_dev(qd, B, k, nprobe, at(ids_all, o * 8), at(sd, o * 4), at(sc, g * B * 4), at(keys_all, o * 8),
                                         mask=masks[g] if masks else None)
            else:
                sh.search_dev(qd, B, k, nprobe, at(ids_all, o * 8), at(sd, o * 4), at(sc, g * B * 4), at(keys_all, o * 8))
        ctx.synchronize()
        host = (ctx.download(keys_all, (G, B, k), np.uint64), ctx.download(ids_all, (G, B, k), np.uint64),
                ctx.download(sc, (G, B), np.uint32))
        for p in (qd, sd, sc):
            ctx.free(p)
        return keys_all, ids_all, host

    def merged(self, keys_all, ids_all, B, k, wide=True):
        ctx, G = self.ctx, self.G
        oi, od, oc = ctx.alloc(B * k * 8), ctx.alloc(B * k * 4), ctx.alloc(B * 4)
        merge = self.fv.engine.merge_keys_wide_dev if wide else self.fv.engine.merge_keys_dev
        merge(ctx, keys_all, ids_all, G, B, k, oi, od, oc)
        ctx.synchronize()
        res = (ctx.download(oi, (B, k), np.uint64), ctx.download(od, (B, k), np.float32), ctx.download(oc, B, np.uint32))
        for p in (oi, od, oc, keys_all, ids_all):
            ctx.free(p)
        return res

    def whole_wide(self, q, k, nprobe, mask=None):
        """The unsharded index's wide search with its keys."""
        ctx, B = self.ctx, q.shape[0]
        qd, out = ctx.upload(q), ctx.alloc(B * k * 20 + B * 4)
        n = B * k
        self.whole.search_wide_dev(qd, B, k, nprobe, at(out, 0), at(out, n * 16), at(out, n * 20), at(out, n * 8), mask=mask)
        ctx.synchronize()
        res = (ctx.download(at(out, 0), (B, k), np.uint64), ctx.download(at(out, n * 16), (B, k), np.float32),
               ctx.download(at(out, n * 20), B, np.uint32), ctx.download(at(out, n * 8), (B, k), np.uint64))
        ctx.free(qd)
        ctx.free(out)
        return res

    def check(self, q, k, nprobe, what, allowed=None, oracle=None):
        """Shards + wide merge == the whole index (keys included) == the oracle."""
        masks = [make_mask(self.ctx, sh, allowed) for sh in self.shards] if allowed is not None else None
        wmask = make_mask(self.ctx, self.whole, allowed) if allowed is not None else None
        B = q.shape[0]
        keys_all, ids_all, (pk, pi, pc) = self.partials(q, k, nprobe, masks)
        got = self.merged(keys_all, ids_all, B, k)
        wi, wd, wc, wk = self.whole_wide(q, k, nprobe, wmask)
        assert_equal(got, (wi, wd, wc), what + " vs the whole index")
        for b in range(B):  # the shards' keys, merged on the host, are the whole index's keys
            valid = pk[:, b, :][pk[:, b, :] != NO_KEY]
            assert valid.size == int(pc[:, b].sum()) and np.unique(valid).size == valid.size, f"{what}: query {b}: keys"
            assert np.array_equal(np.sort(valid)[:k], wk[b, : wc[b]]), f"{what}: query {b}: keys differ from the whole index's"
        for g in range(self.G):  # each partial list: ascending, "no result" last
            assert np.all(np.sort(pk[g], axis=1) == pk[g])
            assert np.all((pk[g] != NO_KEY).sum(axis=1) == pc[g])
        ref = (oracle or self.cpu).batch_search(q, k, nprobe, threads=8)
        assert_same(got, ref, what + " vs the oracle")
        for m in (masks or []) + ([wmask] if wmask else []):
            self.ctx.lib.fvdb_mask_destroy(m)
        return got

    def close(self):
        for s in self.shards + [self.whole]:
            s.close()


# ---- 1. ties across owners -------------------------------------------------------------------------------------------
def grid_case(seed=4):
    rng = np.random.default_rng(seed)
    n, d, nlist, B = 6000, 8, 40, 37
    x = rng.integers(-1, 2, (n, d)).astype(np.float32)
    q = rng.integers(-1, 2, (B, d)).astype(np.float32)
    uniq = np.unique(x, axis=0)
    cents = uniq[rng.choice(uniq.shape[0], nlist, replace=False)].copy()
    return x, np.arange(n, dtype=np.uint64) * 3 + 11, q, cents


def test_ties_across_owners(fv, request):
    # rows and queries on the grid {-1, 0, 1}^8: squared distances are small integers, so every cut falls inside a tie
    x, ids, q, cents = grid_case()
    G, nprobe, ks = 4, 8, (257, 300, 1024, 4096)
    orc.build()
    cpu = orc.IVFIndex(n_clusters=cents.shape[0], n_probe=nprobe)
    cpu.set_trained(cents)
    cl = cpu.assign(x)
    cpu.batch_insert_assigned(ids, x, cl)
    owner = fv.sharded.plan_list_shards(np.bincount(cl, minlength=cents.shape[0]).astype(np.uint64), G)
    # the case is what it claims, on the oracle's answer alone and before the GPU is touched: for some query and k the
    # k-th and (k+1)-th rows are equally far and lie in lists of different owners
    own_of = {int(i): int(owner[c]) for i, c in zip(ids, cl)}
    split = 0
    for k in ks:
        oi, od, oc = cpu.batch_search(q, k + 1, nprobe, threads=8)
        for b in range(q.shape[0]):
            if oc[b] == k + 1 and bits(od[b, k - 1 : k]) == bits(od[b, k : k + 1]):
                split += own_of[int(oi[b, k - 1])] != own_of[int(oi[b, k])]
    assert split > 0, "no cut falls between equally distant rows of different owners: choose another seed"
    ctx = request.getfixturevalue("ctx")
    S = Sharded(fv, ctx, x, ids, cents, G)
    assert np.array_equal(S.owner, owner)
    for k in ks:
        got = S.check(q, k, nprobe, f"grid k={k}")
        if k == 4096:  # fewer probed rows than k for every query: counts below k, padded tails, ~0 keys in the merge
            assert np.all(got[2] < k) and np.all(got[2] > 256)
    S.close()


# ---- 2. more than 256 probes -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_lists(fv, ctx):
    # 6000 rows in 300 lists: most lists are one partly filled block; d = 20 is no multiple of 16
    n, d, nlist = 6000, 20, 300
    x = mixture(n, d, n_comp=40, sigma=0.6, seed=5100)
    ids = np.arange(n, dtype=np.uint64) * 7 + 3
    S = Sharded(fv, ctx, x, ids, x[:nlist].copy(), G=3)
    yield S, mixture(5, d, n_comp=40, sigma=0.6, seed=5101)
    S.close()


@pytest.mark.parametrize("k", [10, 300])
@pytest.mark.parametrize("nprobe", [257, 300])
def test_more_than_256_probes(many_lists, nprobe, k):
    S, q = many_lists
    S.check(q, k, nprobe, f"nprobe={nprobe} k={k}")


# ---- 3. fp16 rows ----------------------------------------------------------------------------------------------------
def test_fp16_rows(fv, ctx):
    n, d, nlist = 5000, 32, 16
    x = mixture(n, d, n_comp=nlist, seed=5200)
    S = Sharded(fv, ctx, x, np.arange(n, dtype=np.uint64) + 9, x[:nlist].copy(), G=3, dtype="f16")
    S.check(mixture(21, d, n_comp=nlist, seed=5201), 300, 6, "fp16 k=300")
    S.close()


# ---- 4. a shard that owns no list ------------------------------------------------------------------------------------
def test_a_shard_that_owns_no_list(fv, ctx):
    n, d, nlist, B, k = 3000, 16, 12, 7, 300
    x = mixture(n, d, n_comp=nlist, seed=5300)
    owner = (np.arange(nlist) % 2).astype(np.uint32) * 2  # ranks 0 and 2 own everything, rank 1 nothing
    S = Sharded(fv, ctx, x, np.arange(n, dtype=np.uint64), x[:nlist].copy(), G=3, owner=owner)
    q = mixture(B, d, n_comp=nlist, seed=5301)
    keys_all, ids_all, (pk, pi, pc) = S.partials(q, k, 5)
    assert np.all(pk[1] == NO_KEY) and np.all(pi[1] == NO_ID) and np.all(pc[1] == 0)
    ctx.free(keys_all)
    ctx.free(ids_all)
    S.check(q, k, 5, "empty shard")
    S.close()


# ---- 5. deleted rows and a mask --------------------------------------------------------------------------------------
def test_deleted_rows_and_a_mask(fv, ctx):
    n, d, nlist, nprobe, B = 6000, 24, 16, 6, 19
    x = mixture(n, d, n_comp=nlist, seed=5400)
    ids = np.arange(n, dtype=np.uint64) * 3 + 7
    rng = np.random.default_rng(54)
    S = Sharded(fv, ctx, x, ids, x[:nlist].copy(), G=4)
    S.delete(rng.choice(n, 400, replace=False))
    q = mixture(B, d, n_comp=nlist, seed=5401)
    S.check(q, 300, nprobe, "deleted rows")
    allowed = ids[rng.random(n) < 0.5]  # every shard builds its mask from the full list
    keep = set(int(i) for i in allowed)
    for i in ids:  # the oracle after deleting the complement
        if int(i) not in keep:
            S.cpu.mark_deleted(int(i))
    for k in (10, 300, 1024):
        S.check(q, k, nprobe, f"masked k={k}", allowed=allowed)
    S.close()


# ---- 6. k <= 256 through the new calls -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 256])
def test_small_k_through_the_new_calls_equals_the_register_path(fv, ctx, k):
    n, d, nlist, nprobe, B = 6000, 48, 24, 7, 33
    x = mixture(n, d, n_comp=nlist, seed=5500)
    S = Sharded(fv, ctx, x, np.arange(n, dtype=np.uint64) + 100, x[:nlist].copy(), G=4)
    q = mixture(B, d, n_comp=nlist, seed=5501)
    nk, ni, (npk, npi, npc) = S.partials(q, k, nprobe, wide=True)
    ok_, oi_, (opk, opi, opc) = S.partials(q, k, nprobe, wide=False)
    assert np.array_equal(npc, opc)
    valid = (opk >> np.uint64(32)) != 0xFFFFFFFF  # "no result": the distance word of a key is all ones
    assert np.array_equal(valid, npk != NO_KEY) and np.array_equal(valid.sum(axis=2), opc)
    assert np.array_equal(npk[valid], opk[valid]) and np.array_equal(npi[valid], opi[valid])
    new = S.merged(nk, ni, B, k, wide=True)
    old = S.merged(ok_, oi_, B, k, wide=False)
    assert_equal(new, old, f"k={k}")
    assert_same(new, S.cpu.batch_search(q, k, nprobe), f"k={k} vs the oracle")
    S.close()


# ---- 7. the merge alone ----------------------------------------------------------------------------------------------
def hand_partials(rng, G, B, k, counts):
    """G x B x k ascending unique keys with ~0 tails (counts[g][b] valid entries) and ids that name their key."""
    keys = np.full((G, B, k), NO_KEY, np.uint64)
    for b in range(B):
        tot = int(sum(counts[g][b] for g in range(G)))
        # few distinct distance words: ties in the high word, decided by the low one
        pool = (rng.integers(0x3F000000, 0x3F000040, tot, dtype=np.uint64) << np.uint64(32)) | rng.permutation(tot).astype(np.uint64)
        o = 0
        for g in range(G):
            c = int(counts[g][b])
            keys[g, b, :c] = np.sort(pool[o : o + c])
            o += c
    ids = np.where(keys == NO_KEY, NO_ID, keys ^ np.uint64(0x5A5A5A5A))
    return keys, ids


def merge_case(fv, ctx, keys, ids, k):
    G, B, _ = keys.shape
    dk, di = ctx.upload(keys), ctx.upload(ids)
    oi, od, oc = ctx.alloc(B * k * 8), ctx.alloc(B * k * 4), ctx.alloc(B * 4)
    fv.engine.merge_keys_wide_dev(ctx, dk, di, G, B, k, oi, od, oc)
    ctx.synchronize()
    got = (ctx.download(oi, (B, k), np.uint64), ctx.download(od, (B, k), np.float32), ctx.download(oc, B, np.uint32))
    for p in (dk, di, oi, od, oc):
        ctx.free(p)
    for b in range(B):
        flat = keys[:, b, :].reshape(-1)
        order = np.sort(flat[flat != NO_KEY])[:k]
        n = order.size
        assert got[2][b] == n
        assert np.array_equal(got[0][b, :n], order ^ np.uint64(0x5A5A5A5A))
        assert np.array_equal(bits(got[1][b, :n]), (order >> np.uint64(32)).astype(np.uint32))
        assert np.all(got[0][b, n:] == NO_ID) and np.all(np.isposinf(got[1][b, n:]))
    return got


def test_the_merge_alone(fv, ctx):
    rng = np.random.default_rng(56)
    B = 3
    full = lambda G, k: [[k] * B for _ in range(G)]  # noqa: E731
    merge_case(fv, ctx, *hand_partials(rng, 1, B, 300, full(1, 300)), 300)            # G = 1: a copy
    merge_case(fv, ctx, *hand_partials(rng, 8, B, 4096, full(8, 4096)), 4096)         # the largest shape
    merge_case(fv, ctx, *hand_partials(rng, 5, B, 300, full(5, 0)), 300)              # every list empty
    merge_case(fv, ctx, *hand_partials(rng, 4, B, 1000, [[100, 0, 7], [3, 0, 250], [0, 0, 1], [60, 999, 0]]), 1000)  # short
    merge_case(fv, ctx, *hand_partials(rng, 3, B, 7, full(3, 7)), 7)
    # one list holds every winner: its keys lie below all the others'
    keys, ids = hand_partials(rng, 4, B, 500, full(4, 500))
    keys[2] = np.where(keys[2] == NO_KEY, NO_KEY, keys[2] & np.uint64(0x00FFFFFFFFFFFFFF))
    ids = np.where(keys == NO_KEY, NO_ID, keys ^ np.uint64(0x5A5A5A5A))
    got = merge_case(fv, ctx, keys, ids, 500)
    assert np.array_equal(got[0], ids[2])
    with pytest.raises(fv.Unsupported):
        fv.engine.merge_keys_wide_dev(ctx, None, None, 2, 1, 4097, None, None, None)
    with pytest.raises(fv.Unsupported):
        fv.engine.merge_keys_wide_dev(ctx, None, None, 2, 1, 0, None, None, None)


# ---- 8. world 1 over RCCL --------------------------------------------------------------------------------------------
class Step:
    """fvdb_ivf_search_sharded_wide_begin / _end on a world of one rank."""

    def __init__(self, fv, ctx, ivf):
        self.ctx, self.lib = ctx, ctx.lib
        self.comm = fv.sharded.Comm.rccl(ctx)
        self.s = C.c_void_p()
        ctx.check(self.lib.fvdb_sharded_create(ivf.h, self.comm.h, C.byref(self.s)))

    def run(self, q, k, nprobe, mode, mask=None, old=False, rc_only=False):
        ctx, lib, B = self.ctx, self.lib, q.shape[0]
        qd, out = ctx.upload(q), ctx.alloc(B * k * 12 + B * 4)
        n = B * k
        outs = (at(out, 0), at(out, n * 8), at(out, n * 12))
        if old:
            rc = lib.fvdb_ivf_search_sharded_begin(self.s, None, 0, qd, B, k, nprobe, mode, *outs)
        else:
            rc = lib.fvdb_ivf_search_sharded_wide_begin(self.s, None, 0, mask, qd, B, k, nprobe, mode, *outs)
        if not rc_only:
            ctx.check(rc)
        ctx.check(lib.fvdb_ivf_search_sharded_end(self.s, None, 0))
        res = (ctx.download(outs[0], (B, k), np.uint64), ctx.download(outs[1], (B, k), np.float32), ctx.download(outs[2], B, np.uint32))
        ctx.free(qd)
        ctx.free(out)
        return rc if rc_only else res

    def close(self):
        self.lib.fvdb_sharded_destroy(self.s)
        self.comm.close()


def test_sharded_wide_step_on_one_rank_equals_the_single_index(fv, ctx, many_lists):
    S0, q = many_lists
    n, d, nlist = 6000, 20, 300
    x = mixture(n, d, n_comp=40, sigma=0.6, seed=5100)
    ids = S0.ids
    one = Sharded(fv, ctx, x, ids, x[:nlist].copy(), G=1)  # the one shard holds every list, with global sizes set
    step = Step(fv, ctx, one.shards[0])
    allowed = ids[np.random.default_rng(57).random(n) < 0.5]
    smask, wmask = make_mask(ctx, one.shards[0], allowed), make_mask(ctx, one.whole, allowed)
    for mode in (fv.sharded.WEAK, fv.sharded.STRONG):
        for k, nprobe in ((300, 8), (10, 257), (300, 300)):
            assert_equal(step.run(q, k, nprobe, mode), one.whole_wide(q, k, nprobe)[:3], f"mode={mode} k={k} nprobe={nprobe}")
            assert_same(step.run(q, k, nprobe, mode), one.cpu.batch_search(q, k, nprobe), f"oracle mode={mode} k={k} nprobe={nprobe}")
        for k, nprobe in ((300, 8), (10, 6), (10, 257)):  # under a mask: the wide route, and the register path at (10, 6)
            assert_equal(step.run(q, k, nprobe, mode, mask=smask), one.whole_wide(q, k, nprobe, wmask)[:3],
                         f"masked mode={mode} k={k} nprobe={nprobe}")
        # what the existing call serves, the new one serves alike
        assert_equal(step.run(q, 10, 6, mode), step.run(q, 10, 6, mode, old=True), f"mode={mode} small")
    # a mask of another index, and one built before the index last changed
    lib = ctx.lib
    assert step.run(q, 300, 8, 0, mask=wmask, rc_only=True) == E_INVALID and b"mask of another index" in lib.fvdb_last_error(ctx.h)
    one.shards[0].set_deleted(one.cl[:1], one.spos[0][:1], True)
    assert step.run(q, 300, 8, 0, mask=smask, rc_only=True) == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    assert step.run(q, 10, 6, 0, mask=smask, rc_only=True) == E_INVALID and b"stale mask" in lib.fvdb_last_error(ctx.h)
    with pytest.raises(fv.Unsupported):
        step.run(q, 4097, 8, 0)
    lib.fvdb_mask_destroy(smask)
    lib.fvdb_mask_destroy(wmask)
    step.close()
    one.close()


def test_sharded_hybrid_world_1_at_k_300_and_under_an_allow_set(fv, ctx):
    sh = fv.sharded
    n, d, nlist, k, nprobe, ef, B = 4000, 32, 8, 300, 8, 50, 20
    x = mixture(n, d, n_comp=nlist, seed=5800)
    ids = np.arange(n, dtype=np.uint64) + 5
    cents = x[:nlist].copy()
    now = 1000 * DAY
    is_recent = np.random.default_rng(58).random(n) < 0.3
    ts = np.where(is_recent, now - 1 * DAY, now - 30 * DAY)
    kw = dict(max_connections=8, max_connections_layer_0=16, ef_construction=40, n_clusters=nlist, n_probe=nprobe)
    hyb = fv.HybridIndex(ctx, hnsw_seed=29, **kw)
    hyb.set_ivf_centroids(cents)
    comm = sh.Comm.rccl(ctx)
    S = sh.ShardedHybrid(hyb, comm)
    S.bulk_insert(ids, x, ts, now)
    hyb.hnsw().scan_cutoff = 0  # the recent part by the masked traversal, as the oracle walks it after the deletes

    def oracle():
        o = orc.HybridIndex(**kw)
        o.set_ivf_centroids(cents)
        o.ivf().batch_insert(ids[~is_recent], x[~is_recent])
        gi, lv, off, nb_ = hyb.hnsw().export_graph()
        o.hnsw().restore(gi, x[(gi - 5).astype(np.int64)], lv, off, nb_, hyb.hnsw().entry_point())
        return o

    def same(res, ref):
        oi, od, oc = ref
        assert np.array_equal(res.counts, oc), f"hit counts differ: {res.counts[:8]} vs {oc[:8]}"
        for b in range(len(res)):
            m = int(oc[b])
            assert np.array_equal(res.ids[b, :m], oi[b, :m]) and np.array_equal(bits(res.distances[b, :m]), bits(od[b, :m]))

    q = mixture(B, d, n_comp=nlist, seed=5801)
    qd = ctx.upload(q)
    o = oracle()
    for mode in (sh.WEAK, sh.STRONG):
        r = S.search_dev(qd, B, k, ef, nprobe, mode)
        same(r, o.batch_search(q, k, now=now, hnsw_ef=ef, ivf_n_probe=nprobe))
        assert np.all(r.counts > 256), "historical rows are part of the answer"
    # the existing route is what it was
    r10 = S.search_dev(qd, B, 10, ef, 6)
    same(r10, o.batch_search(q, 10, now=now, hnsw_ef=ef, ivf_n_probe=6))
    # under an allow-set: the oracle deletes the complement from both parts
    allowed = ids[np.random.default_rng(59).random(n) < 0.5]
    keep = set(int(i) for i in allowed)
    for i, rec in zip(ids, is_recent):
        if int(i) not in keep:
            (o.hnsw() if rec else o.ivf()).mark_deleted(int(i))
    for mode in (sh.WEAK, sh.STRONG):
        for kk in (300, 10):
            r = S.search_dev(qd, B, kk, ef, nprobe, mode, allowed=allowed)
            same(r, o.batch_search(q, kk, now=now, hnsw_ef=ef, ivf_n_probe=nprobe))
            assert np.isin(r.ids[r.ids != NO_ID], allowed).all()
    # the plain filtered search keeps refusing a sharded index, and the slot holds no mask afterwards
    with pytest.raises(fv.Unsupported):
        hyb.search_allowed(q, 10, allowed, now=now, hnsw_ef=ef, ivf_n_probe=nprobe)
    same(S.search_dev(qd, B, 10, ef, 6), (r10.ids, r10.distances, r10.counts))
    ctx.free(qd)
    comm.close()
