"""The definitions of include/fvdb.h, "binary quantization" (DESIGN.md section 9zb), in numpy: the f32 subtraction and
compare, packbits, the popcount of the xor and the (ham, row) order; the refined distances are _sq8_ref's f32 fold."""
import numpy as np

from _sq8_ref import fold, top  # noqa: F401  (the refine tests' fold and key order)

f32 = np.float32
POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.uint16)


def encode(x, center=None):
    """[n][ceil(d / 8)] bytes: bit i = (x_i - c_i) > 0 in f32, dim i = bit i & 7 of byte i >> 3"""
    x = np.asarray(x, f32)
    c = np.zeros(x.shape[1], f32) if center is None else np.asarray(center, f32)
    with np.errstate(over="ignore"):
        return np.packbits((x - c[None, :]).astype(f32) > 0, axis=1, bitorder="little")


def hamming(q, x, center=None):
    """[B][n] popcounts of the xor of the codes"""
    a, b = encode(q, center), encode(x, center)
    return np.stack([POP[b ^ a[i]].sum(1) for i in range(a.shape[0])]).astype(np.int64)


def search(ham, live, k):
    """per query the k smallest (ham, row) over the live rows: [(rows, (float)ham)]"""
    rows = np.flatnonzero(live)
    out = []
    for h in ham[:, rows]:
        o = np.lexsort((rows, h))[:k]
        out.append((rows[o], h[o].astype(f32)))
    return out
