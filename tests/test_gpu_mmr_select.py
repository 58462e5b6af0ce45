"""GPU: the diverse selection kernel alone, driven through fvdb_mmr_select_dev.

Ids, distance bits, ranks, counts and tails must equal _mmr_ref.mmr_answer, the numpy restatement of the definition;
test_mmr_ref.py proves on the CPU that the hand-built inputs tie where they are meant to.  Every launch holds B = 33
queries of mixed kinds (random, fp16-rounded, lattice, the same row under different ids, all rows identical, repeated ids
adjacent / far apart / three copies) and mixed counts (0, 1, a few, fetch_k).  d covers a part-filled pair (3), one
part-filled block (20), exactly one block (128), a second block of two dims (130) and three blocks (384); fetch_k the
16-row chunk and 64-lane wave edges."""
import ctypes as C

import numpy as np
import pytest

import fvdb_import
from _data import bits
import _exact_ref as R
import _mmr_ref as M

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = 6, 12
B = 33
LAMS = (0.0, 0.25, 0.5, 1.0)


@pytest.fixture(scope="module")
def fv():
    return fvdb_import.load()


@pytest.fixture(scope="module")
def ctx(fv):
    c = fv.Context(0)
    yield c
    c.close()


def same_id(case, where):
    """candidate dst takes candidate src's ID only (its own row and distance stay): copies of an id that sit far apart"""
    ids, dq, rows = (a.copy() for a in case)
    for src, dst in where:
        if src < dst < len(ids):
            ids[dst] = ids[src]
    return ids, dq, rows


def one_case(kind, n, d, seed):
    if kind == 0:
        return M.random_case(n, d, seed)
    if kind == 1:
        return M.random_case(n, d, seed, f16=True)
    if kind == 2:
        return M.lattice_case(n, min(d, 6), seed) if d <= 6 else widen(M.lattice_case(n, 6, seed), d)
    if kind == 3:
        return M.twins_case(n, d, seed)
    if kind == 4:
        return M.identical_case(n, d)
    if kind == 5:  # a migrated twin: the same id, row and distance, next to its copy
        return M.with_repeats(M.random_case(n, d, seed), [(s, t) for s, t in ((0, 1), (5, 6)) if t < n])
    if kind == 6:  # the same id far apart
        return same_id(M.random_case(n, d, seed), [(0, n - 1), (2, n // 2)])
    return same_id(M.random_case(n, d, seed), [(1, 2), (1, n - 2), (3, 4)])  # three copies of one id


def widen(case, d):
    """lattice rows padded with a constant tail up to d dims: the distances between them do not change"""
    ids, dq, rows = case
    out = np.zeros((rows.shape[0], d), np.float32)
    out[:, :rows.shape[1]] = rows
    return ids, dq, out


def batch(d, fetch_k):
    """ids / dq [B, fetch_k], rows [B, fetch_k, d], counts [B] and the per-query pairwise folds"""
    ids = np.zeros((B, fetch_k), np.uint64)
    dq = np.zeros((B, fetch_k), np.float32)
    rows = np.zeros((B, fetch_k, d), np.float32)
    rng = np.random.default_rng(fetch_k * 1000 + d)
    few = int(rng.integers(2, max(3, min(fetch_k, 9))))
    counts = np.array([(fetch_k, 0, 1, min(few, fetch_k))[b % 4] for b in range(B)], np.uint32)
    counts[B - 1] = fetch_k
    pairs = []
    for b in range(B):
        i, t, x = one_case((b // 4 + b) % 8, fetch_k, d, 100 * b + d)
        ids[b], dq[b], rows[b] = i, t, x
        n = int(counts[b])
        pair = np.zeros((fetch_k, fetch_k), np.float32)
        pair[:n, :n] = R.fold_distances(x[:n], x[:n])
        pairs.append(pair)
    return ids, dq, rows, counts, pairs


class Launch:
    """the inputs of one batch in device memory, and room for the outputs of the largest k"""

    def __init__(self, fv, ctx, ids, dq, rows, counts, stride=None):
        self.ctx, self.lib = ctx, fv._capi.load()
        self.B, self.fetch_k, d = rows.shape
        self.stride = stride or (d + 3) // 4 * 4
        staged = np.zeros((self.B, self.fetch_k, self.stride), np.float32)
        staged[:, :, :d] = rows
        self.bufs = [ctx.upload(staged), ctx.upload(ids), ctx.upload(dq), ctx.upload(counts)]
        n = self.B * self.fetch_k
        self.out = [ctx.alloc(n * 8), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(self.B * 4)]

    def run(self, k, lam, distinct):
        rc = self.lib.fvdb_mmr_select_dev(self.ctx.h, self.bufs[0], self.stride, self.bufs[1], self.bufs[2], self.bufs[3], self.B,
                                          self.fetch_k, k, lam, int(distinct), *self.out)
        assert rc == 0, rc
        return (self.ctx.download(self.out[0], (self.B, k), np.uint64), self.ctx.download(self.out[1], (self.B, k), np.float32),
                self.ctx.download(self.out[2], (self.B, k), np.uint32), self.ctx.download(self.out[3], (self.B,), np.uint32))

    def close(self):
        for p in self.bufs + self.out:
            self.ctx.free(p)


def same(got, want, what):
    gi, gd, gr, gc = got
    wi, wd, wr, wc = want
    assert np.array_equal(gc, wc), f"{what}: counts differ: {gc} vs {wc}"
    bad = np.flatnonzero((gr != wr).any(1))
    assert bad.size == 0, f"{what}: ranks differ in queries {bad[:4]}: {gr[bad[0]][:12]} vs {wr[bad[0]][:12]}"
    assert np.array_equal(gi, wi), f"{what}: ids differ"
    assert np.array_equal(bits(gd), bits(wd)), f"{what}: distances are not bit-identical"


@pytest.mark.parametrize("fetch_k", [1, 5, 16, 17, 64, 65, 255, 256])
@pytest.mark.parametrize("d", [3, 20, 128, 130, 384])
def test_the_kernel_equals_the_reference(fv, ctx, d, fetch_k):
    ids, dq, rows, counts, pairs = batch(d, fetch_k)
    run = Launch(fv, ctx, ids, dq, rows, counts)
    try:
        for k in sorted({1, min(10, fetch_k), fetch_k}):
            for lam in LAMS:
                for distinct in (False, True):
                    got = run.run(k, lam, distinct)
                    want = M.mmr_answer(ids, dq, rows, counts, k, lam, distinct, pairs=pairs)
                    same(got, want, f"d={d} fetch_k={fetch_k} k={k} lam={lam} distinct={distinct}")
                    gi, gd, gr, gc = got
                    for b in range(B):  # tails, whatever the reference says
                        n = int(gc[b])
                        assert np.all(gi[b, n:] == M.NO_ID) and np.all(np.isposinf(gd[b, n:])) and np.all(gr[b, n:] == M.NO_ROW)
                    if lam == 1.0 and not distinct:  # the prefix of the candidates, bit for bit
                        for b in range(B):
                            n = min(k, int(counts[b]))
                            assert gc[b] == n and np.array_equal(gi[b, :n], ids[b, :n]) and np.array_equal(bits(gd[b, :n]), bits(dq[b, :n]))
                    if distinct:
                        for b in range(B):
                            assert len(set(gi[b, :int(gc[b])].tolist())) == int(gc[b])
    finally:
        run.close()


def test_a_wider_stride_with_zero_padding_gives_the_same_picks(fv, ctx):
    ids, dq, rows, counts, pairs = batch(20, 17)
    run = Launch(fv, ctx, ids, dq, rows, counts, stride=32)
    try:
        same(run.run(10, 0.5, True), M.mmr_answer(ids, dq, rows, counts, 10, 0.5, True, pairs=pairs), "stride 32")
    finally:
        run.close()


def test_refusals(fv, ctx):
    ids, dq, rows, counts, _ = batch(3, 5)
    run = Launch(fv, ctx, ids, dq, rows, counts)
    lib = run.lib
    try:
        def call(rows_p=run.bufs[0], stride=run.stride, ids_p=run.bufs[1], dq_p=run.bufs[2], cnt_p=run.bufs[3], nb=B, fetch_k=5, k=2,
                 lam=0.5, out=None):
            out = run.out if out is None else out
            return lib.fvdb_mmr_select_dev(ctx.h, rows_p, stride, ids_p, dq_p, cnt_p, nb, fetch_k, k, lam, 1, *out)
        assert call() == 0
        assert call(fetch_k=0) == E_UNSUPPORTED and call(fetch_k=257, k=2) == E_UNSUPPORTED
        assert call(k=0) == E_INVALID and call(k=6) == E_INVALID
        for lam in (float("nan"), -0.25, 1.5, float("inf")):
            assert call(lam=lam) == E_INVALID, lam
        assert call(lam=0.0) == 0 and call(lam=1.0) == 0
        for stride in (0, 3, 6):
            assert call(stride=stride) == E_INVALID, stride
        null = C.c_void_p(None)
        assert call(rows_p=null) == E_INVALID and call(ids_p=null) == E_INVALID and call(dq_p=null) == E_INVALID
        assert call(cnt_p=null) == E_INVALID
        for i in range(4):
            out = list(run.out)
            out[i] = null
            assert call(out=out) == E_INVALID, i
        # B == 0: nothing is enqueued, null pointers are fine
        assert lib.fvdb_mmr_select_dev(ctx.h, null, 4, null, null, null, 0, 5, 2, 0.5, 1, null, null, null, null) == 0
        ctx.synchronize()
    finally:
        run.close()
