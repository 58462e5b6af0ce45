"""GPU: the grouped selection kernel alone, driven through fvdb_group_select_dev.

Every output array must equal _group_cases.select_batch, the Python statement of the definition, exactly and tails
included; test_group_reference.py checks that statement on the CPU.  Every launch holds B = 37 queries: query b takes key
population b mod 11 (one key, all distinct, three keys, a Zipf-like mix, equal low words under different high words,
multiples of the table size, different keys that start their probe at one cell of the kernel's table, equal words under
different tags, a none key at the first / the last / every second position) and a count from (fetch_k, 0, 1, a few,
fetch_k - 1).  Some queries repeat an id (adjacent, far apart, three copies), one holds FVDB_NO_ID, and one has its
distances shuffled: only positions may order the result.  fetch_k covers the wave edge (64, 65), the edge between the two
instantiations (256, 257), a width that is no power of two (1000) and the limit (4096)."""
import numpy as np
import pytest

import fvdb_import
import _group_cases as G

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = 6, 12
B = 37
FETCH_KS = (1, 5, 64, 65, 256, 257, 1000, 4096)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def batch(fetch_k):
    """ids u64 / dist f32 / key_tag u8 / key_val u64 [B, fetch_k] and counts [B]"""
    rng = np.random.default_rng(fetch_k)
    ids = np.zeros((B, fetch_k), np.uint64)
    dist = np.zeros((B, fetch_k), np.float32)
    tag = np.zeros((B, fetch_k), np.uint8)
    val = np.zeros((B, fetch_k), np.uint64)
    few = min(fetch_k, 7)
    counts = np.array([(fetch_k, 0, 1, few, max(fetch_k - 1, 0))[b % 5] for b in range(B)], np.uint32)
    counts[B - 1] = fetch_k + 3  # a count beyond fetch_k is fetch_k
    for b in range(B):
        # 64-bit ids whose low words repeat: only the whole id tells them apart
        ids[b] = (rng.permutation(fetch_k).astype(np.uint64) % np.uint64(17)) | (np.arange(fetch_k, dtype=np.uint64) << np.uint64(32))
        dist[b] = np.sort(rng.random(fetch_k).astype(np.float32))
        tag[b], val[b] = G.population(G.POPULATIONS[b % len(G.POPULATIONS)], fetch_k, 100 * b + fetch_k)
        n = fetch_k
        if b % 4 == 1 and n > 1:      # a migrated twin next to its copy
            ids[b, 1] = ids[b, 0]
        if b % 4 == 2 and n > 4:      # the same id far apart, and three copies of another
            ids[b, n - 1] = ids[b, 0]
            ids[b, n // 2] = ids[b, 2] = ids[b, 1]
        if b == 7 and n > 2:
            ids[b, 1] = G.NO_ID
        if b == 11 and n > 3:         # two FVDB_NO_ID: `distinct` treats them as copies of one id
            ids[b, 0] = ids[b, 3] = G.NO_ID
        if b == 5:
            dist[b] = rng.permutation(dist[b])
    return ids, dist, counts, tag, val


class Launch:
    """the inputs of one batch in device memory, and two sets of outputs sized for the largest k * group_size"""

    def __init__(self, fv, ctx, ids, dist, counts, tag, val):
        self.ctx, self.lib = ctx, fv._capi.load()
        self.B, self.fetch_k = ids.shape
        self.bufs = [ctx.upload(ids), ctx.upload(dist), ctx.upload(counts), ctx.upload(tag), ctx.upload(val)]
        cells = self.B * 4096
        self.sizes = (8, 4, 4, 4, 4, 1, 8, 4, 4)
        self.outs = [[ctx.alloc(cells * w) for w in self.sizes] for _ in range(2)]

    def enqueue(self, which, k, gs, distinct, missing):
        rc = self.lib.fvdb_group_select_dev(self.ctx.h, *self.bufs, self.B, self.fetch_k, k, gs, int(distinct), missing, *self.outs[which])
        assert rc == 0, rc

    def fetch(self, which, k, gs):
        shapes = [(self.B, k, gs)] * 3 + [(self.B, k)] * 4 + [(self.B,)] * 2
        dtypes = (np.uint64, np.float32, np.uint32, np.uint32, np.uint32, np.uint8, np.uint64, np.uint32, np.uint32)
        return {n: self.ctx.download(p, s, t) for n, p, s, t in zip(G.NAMES, self.outs[which], shapes, dtypes)}

    def close(self):
        for p in self.bufs + self.outs[0] + self.outs[1]:
            self.ctx.free(p)


def same(got, want, what):
    for name in G.NAMES:
        g, w = got[name], want[name]
        assert g.shape == w.shape, (what, name)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {name} differs first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def shapes_of(fetch_k):
    out = []
    for k in sorted({1, 3, fetch_k}):
        for gs in (1, 2, 7):
            if k * gs <= 4096:
                out.append((k, gs))
    return out


@pytest.mark.parametrize("fetch_k", FETCH_KS)
def test_every_output_equals_the_reference(fv, ctx, fetch_k):
    data = batch(fetch_k)
    run = Launch(fv, ctx, *data)
    try:
        modes = ((True, G.DROP), (False, G.OWN), (True, G.OWN), (False, G.DROP))
        for i, (k, gs) in enumerate(shapes_of(fetch_k)):
            distinct, missing = modes[i % 4]
            run.enqueue(0, k, gs, distinct, missing)
            run.enqueue(1, k, gs, distinct, missing)  # the same call again: identical bytes
            got, again = run.fetch(0, k, gs), run.fetch(1, k, gs)
            want = G.select_batch(*data, k, gs, distinct, missing)
            what = f"fetch_k={fetch_k} k={k} group_size={gs} distinct={distinct} missing={missing}"
            same(got, want, what)
            for name in G.NAMES:
                assert got[name].tobytes() == again[name].tobytes(), (what, name, "two runs differ")
    finally:
        run.close()


@pytest.mark.parametrize("fetch_k", (64, 257))
def test_all_four_modes_at_one_shape(fv, ctx, fetch_k):
    data = batch(fetch_k)
    run = Launch(fv, ctx, *data)
    try:
        for distinct in (True, False):
            for missing in (G.DROP, G.OWN):
                run.enqueue(0, 5, 3, distinct, missing)
                same(run.fetch(0, 5, 3), G.select_batch(*data, 5, 3, distinct, missing), f"{fetch_k} {distinct} {missing}")
    finally:
        run.close()


def test_k_beyond_the_candidates(fv, ctx):
    """k may exceed fetch_k: the groups stop at the candidates, the tails are written all the same"""
    data = batch(5)
    run = Launch(fv, ctx, *data)
    try:
        run.enqueue(0, 600, 2, True, G.OWN)
        same(run.fetch(0, 600, 2), G.select_batch(*data, 600, 2, True, G.OWN), "k=600 over fetch_k=5")
    finally:
        run.close()


def test_refusals_just_outside_the_limits(fv, ctx):
    lib = fv._capi.load()
    p = ctx.alloc(64)
    outs = [p] * 9
    ins = [p] * 5

    def call(B_, fetch_k, k, gs, missing=G.DROP, ins_=ins):
        return lib.fvdb_group_select_dev(ctx.h, *ins_, B_, fetch_k, k, gs, 1, missing, *outs)

    try:
        assert call(1, 0, 1, 1) == E_UNSUPPORTED
        assert call(1, 4097, 1, 1) == E_UNSUPPORTED
        assert call(1, 8, 0, 1) == E_INVALID
        assert call(1, 8, 1, 0) == E_INVALID
        assert call(1, 8, 4097, 1) == E_UNSUPPORTED
        assert call(1, 8, 586, 7) == E_UNSUPPORTED      # 4102 cells
        assert call(1, 8, 1, 4097) == E_UNSUPPORTED
        assert call(1, 8, 1, 1, missing=2) == E_INVALID
        assert call(1, 8, 1, 1, ins_=[None] + ins[1:]) == E_INVALID
        assert call(0, 8, 1, 1, ins_=[None] * 5) == 0   # B == 0: nothing enqueued, nothing looked at
        assert call(0, 4096, 4096, 1) == 0 and call(0, 4096, 585, 7) == 0
    finally:
        ctx.free(p)
