"""Grouped selection as plain Python: the key of a candidate, the selection, and the builders of
the key populations the GPU tests run.  test_group_reference.py checks this file against hand-built cases whose answers
are written out literally; the GPU tests then compare the engine with it exactly, tails included."""
import struct

import numpy as np

MISSING, NULL, BOOL, INT, FLOAT, STRING, ARRAY, COMPLEX = range(8)  # FVDB_META_*
NO_ID, NO_ROW = (1 << 64) - 1, (1 << 32) - 1
DROP, OWN = 0, 1                                                    # FVDB_GROUP_MISSING_*
_M64 = (1 << 64) - 1


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- the key of a candidate -----------------------------------------------------------------------------------------
def cell_key(tag, val):
    """(tag, canon) of a cell, or None: MISSING, ARRAY, COMPLEX and a FLOAT NaN have no key; -0.0 folds onto 0.0; NULL is 0."""
    tag, val = int(tag), int(val)
    if tag < NULL or tag > STRING:
        return None
    if tag == NULL:
        return NULL, 0
    if tag == FLOAT:
        if (val << 1) & _M64 == 0:
            val = 0
        if val & 0x7FFFFFFFFFFFFFFF > 0x7FF0000000000000:
            return None
    return tag, val


def keys_of_ids(ids, slot_ids, present, tags, vals):
    """out_tag u8 [n], out_key u64 [n] of fvdb_group_keys_of_ids_dev: per id the key of the cell at the LOWEST slot that
    carries the id, (MISSING, 0) when the key is none."""
    lowest = {}
    for s, rid in enumerate(np.asarray(slot_ids, np.uint64).tolist()):
        lowest.setdefault(rid, s)
    out_tag, out_key = np.zeros(len(ids), np.uint8), np.zeros(len(ids), np.uint64)
    for i, rid in enumerate(np.asarray(ids, np.uint64).tolist()):
        s = lowest.get(rid)
        if rid == NO_ID or s is None or not present[s]:
            continue
        key = cell_key(tags[s], vals[s])
        if key is not None:
            out_tag[i], out_key[i] = key
    return out_tag, out_key


# ---- the selection --------------------------------------------------------------------------------------------------
def select_one(ids, dist, count, key_tag, key_val, fetch_k, k, group_size, distinct=True, missing=DROP):
    """One query.  Returns (out_ids [k][gs], out_dist, out_rank, out_members [k], out_total [k], out_key_tag [k],
    out_key_val [k], groups, flags)."""
    n = min(int(count), fetch_k)
    seen, order, members = set(), [], {}
    for c in range(n):
        rid = int(ids[c])
        if distinct:
            if rid in seen:
                continue
            seen.add(rid)
        tag = int(key_tag[c])
        key = None if (tag < NULL or tag > STRING or rid == NO_ID) else (tag, int(key_val[c]))
        if key is None:
            if missing == DROP:
                continue
            key = ("own", c)
        if key not in members:
            members[key] = []
            order.append(key)
        members[key].append(c)
    out_ids = np.full((k, group_size), NO_ID, np.uint64)
    out_dist = np.full((k, group_size), np.inf, np.float32)
    out_rank = np.full((k, group_size), NO_ROW, np.uint32)
    out_members, out_total = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
    out_key_tag, out_key_val = np.zeros(k, np.uint8), np.zeros(k, np.uint64)
    for g, key in enumerate(order[:k]):
        cs = members[key]
        out_total[g] = len(cs)
        out_members[g] = min(len(cs), group_size)
        for m, c in enumerate(cs[:group_size]):
            out_ids[g, m], out_dist[g, m], out_rank[g, m] = ids[c], dist[c], c
        if key[0] != "own":
            out_key_tag[g], out_key_val[g] = key
    return out_ids, out_dist, out_rank, out_members, out_total, out_key_tag, out_key_val, min(len(order), k), int(n == fetch_k)


NAMES = ("ids", "dist", "rank", "members", "total", "key_tag", "key_val", "groups", "flags")


def select_batch(ids, dist, counts, key_tag, key_val, k, group_size, distinct=True, missing=DROP):
    """The whole launch: a dict of the nine output arrays of fvdb_group_select_dev, stacked over the B queries."""
    B, fetch_k = ids.shape
    rows = [select_one(ids[b], dist[b], counts[b], key_tag[b], key_val[b], fetch_k, k, group_size, distinct, missing) for b in range(B)]
    out = {}
    for i, name in enumerate(NAMES):
        col = [r[i] for r in rows]
        out[name] = np.stack(col) if isinstance(col[0], np.ndarray) else np.asarray(col, np.uint32)
    return out


# ---- where a key starts its probe in the kernel's LDS table (kernels_group.h: group_hash) ------------------------------
def table_cell(val, tag, n):
    """The cell of the 2 * next_pow2(n)-cell table at which (tag, val) starts its probe among n candidates."""
    p = 1 if n <= 1 else 1 << (n - 1).bit_length()
    shift = 32 - p.bit_length()  # clz(P) for a 32-bit P
    m32 = 0xFFFFFFFF
    x = (val & m32) ^ (((val >> 32) * 0x85EBCA6B) & m32) ^ ((tag * 0xC2B2AE35) & m32)
    return ((x * 0x9E3779B1) & m32) >> shift


def colliding_words(tag, n, want, seed):
    """`want` different words of one tag that all start their probe at the same cell among n candidates."""
    rng = np.random.default_rng(seed)
    p = 1 if n <= 1 else 1 << (n - 1).bit_length()
    m32 = np.uint64(0xFFFFFFFF)
    out = []
    while len(out) < want:
        v = rng.integers(0, 1 << 62, 32 * p + 64).astype(np.uint64)
        x = (v & m32) ^ (((v >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & m32) ^ np.uint64((tag * 0xC2B2AE35) & 0xFFFFFFFF)
        cell = ((x * np.uint64(0x9E3779B1)) & m32) >> np.uint64(32 - p.bit_length())
        target = int(cell[0]) if not out else table_cell(out[0], tag, n)
        out = list(dict.fromkeys(out + v[cell == np.uint64(target)].tolist()))
    assert all(table_cell(w, tag, n) == table_cell(out[0], tag, n) for w in out[:want])  # the array form agrees with the scalar one
    return out[:want]


# ---- key populations: (key_tag u8 [n], key_val u64 [n]) ----------------------------------------------------------------
POPULATIONS = ("one", "distinct", "three", "zipf", "low_bits", "table_multiples", "same_cell", "tags", "none_first", "none_last",
               "none_every_second")


def population(kind, n, seed):
    rng = np.random.default_rng(seed)
    tag = np.full(n, STRING, np.uint8)
    val = np.zeros(n, np.uint64)
    pos = np.arange(n, dtype=np.uint64)
    if kind == "one":
        val[:] = 7
    elif kind == "distinct":
        val[:] = rng.permutation(n).astype(np.uint64) + np.uint64(1000)
    elif kind == "three":
        val[:] = pos % np.uint64(3)
    elif kind == "zipf":
        val[:] = np.minimum(rng.zipf(1.5, n), 50).astype(np.uint64)
    elif kind == "low_bits":  # equal low words, different high words
        tag[:] = INT
        val[:] = (rng.integers(0, 5, n).astype(np.uint64) << np.uint64(32)) | np.uint64(0x1234)
    elif kind == "table_multiples":  # multiples of the table size (and of every smaller power of two)
        tag[:] = INT
        val[:] = rng.integers(0, 6, n).astype(np.uint64) * np.uint64(8192)
    elif kind == "same_cell":  # different keys that start their probe at one cell of the kernel's table
        words = colliding_words(STRING, n, min(n, 9), seed)
        val[:] = np.asarray(words, np.uint64)[rng.integers(0, len(words), n)]
    elif kind == "tags":  # equal words under different tags: NULL / BOOL / INT / FLOAT / STRING are five groups
        tag[:] = rng.integers(NULL, STRING + 1, n).astype(np.uint8)
        val[:] = 1
        val[tag == NULL] = 0
    else:
        val[:] = pos % np.uint64(4)
        if kind == "none_first":
            tag[0] = MISSING
        elif kind == "none_last":
            tag[n - 1] = MISSING
        elif kind == "none_every_second":
            tag[::2] = MISSING
        else:
            raise AssertionError(kind)
        val[tag == MISSING] = 0
    return tag, val
