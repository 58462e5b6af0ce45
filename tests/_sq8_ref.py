"""The definitions of include/fvdb.h, "scalar quantization to u8" (DESIGN.md section 9x), in numpy: f32 operations for
the codec, int64 sums and f64 for the symmetric score, the reference's f32 fold for the refined distances."""
import numpy as np

f32 = np.float32


def encode(x):
    """(codes u8 [n][d], lo [n], hi [n]); every operation rounds to f32, the division before the multiplication"""
    x = np.asarray(x, f32)
    lo, hi = x.min(axis=1), x.max(axis=1)
    rng = (hi - lo).astype(f32)
    safe = np.where(rng == 0, f32(1), rng)
    t = (((x - lo[:, None]).astype(f32) / safe[:, None]).astype(f32) * f32(255)).astype(f32)
    fl = np.floor(t)
    codes = (fl + ((t - fl) >= f32(0.5))).astype(np.uint8)  # round half away from zero (t >= 0)
    codes[rng == 0] = 0
    return codes, lo, hi


def decode(codes, lo, hi):
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    rng = (hi - lo).astype(f32)
    t = (codes.astype(f32) / f32(255)).astype(f32)
    return (lo[:, None] + (t * rng[:, None]).astype(f32)).astype(f32)


def sym_dist(q, x):
    """[B][n] f32 distances of the encoded queries q to the encoded rows x"""
    a, lq, hq = encode(q)
    c, lr, hr = encode(x)
    a, c = a.astype(np.int64), c.astype(np.int64)
    d = float(q.shape[1])
    A1, A2 = a.sum(1).astype(np.float64)[:, None], (a * a).sum(1).astype(np.float64)[:, None]
    C1, C2 = c.sum(1).astype(np.float64)[None, :], (c * c).sum(1).astype(np.float64)[None, :]
    P = (a @ c.T).astype(np.float64)
    sq = ((hq - lq).astype(f32).astype(np.float64) / 255.0)[:, None]
    sr = ((hr - lr).astype(f32).astype(np.float64) / 255.0)[None, :]
    D = lq.astype(np.float64)[:, None] - lr.astype(np.float64)[None, :]
    S = ((((d * D) * D) + (2.0 * D) * (sq * A1 - sr * C1)) + ((sq * sq) * A2 + (sr * sr) * C2)) - ((2.0 * sq) * sr) * P
    return np.sqrt(np.where(S > 0.0, S, 0.0).astype(f32))


def top(dist, rows, k):
    """the k smallest (bits(dist) << 32) | row of one query: (rows, dist)"""
    keys = np.sort((dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64))[:k]
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), (keys >> np.uint64(32)).astype(np.uint32).view(f32)


def search(q, x, live, k):
    dist, rows = sym_dist(q, x), np.flatnonzero(live)
    return [top(np.ascontiguousarray(dist[b, rows]), rows, k) for b in range(q.shape[0])]


def fold(q, rows):
    """euclidean_distance_scalar: t = a - b; s = s + t * t, ascending, f32; sqrt last"""
    s = np.zeros(rows.shape[0], f32)
    for i in range(q.shape[0]):
        t = (q[i] - rows[:, i]).astype(f32)
        s = (s + (t * t).astype(f32)).astype(f32)
    return np.sqrt(s)


def refine(q, source, cand, k):
    """re-score the candidate rows `cand` of one query against source[cand]"""
    return top(fold(q, source[cand]), cand, k)
