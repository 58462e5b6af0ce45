"""The product-quantization definitions of include/fvdb.h ("product quantization") restated in numpy: the f32 fold
vectorised over rows with a Python loop over dims, first-min argmin after the f32 root, the Lloyd step, SplitMix64 in
Python ints, the ADC table and sum, keys and the sort by (bits, row)."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def geom(d, m):
    """[(offset, dims)] of the m subspaces of d dims: d // m each, the last one runs to d"""
    ds = d // m
    return [(j * ds, ds if j + 1 < m else d - j * ds) for j in range(m)]


def split_books(flat, d, m, ka):
    """the flat [m][ka][dims of j] block as a list of [ka][dims] arrays"""
    out, at = [], 0
    for _, dj in geom(d, m):
        out.append(np.asarray(flat[at:at + ka * dj], np.float32).reshape(ka, dj))
        at += ka * dj
    return out


def join_books(books):
    return np.concatenate([b.reshape(-1) for b in books]).astype(np.float32)


def fold(a, b):
    """[rows of a][rows of b] squared distances: t = a_i - b_i; s = s + t*t, i ascending, all f32"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    s = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for i in range(a.shape[1]):
        t = a[:, i, None] - b[None, :, i]
        s = s + t * t
    return s


def encode(x, books, d, m):
    x = np.asarray(x, np.float32)
    codes = np.empty((x.shape[0], m), np.uint8)
    for j, (o, dj) in enumerate(geom(d, m)):
        codes[:, j] = np.argmin(np.sqrt(fold(x[:, o:o + dj], books[j])), axis=1)  # first minimum
    return codes


def decode(codes, books):
    return np.concatenate([books[j][codes[:, j]] for j in range(len(books))], axis=1)


def sm64(x):
    z = (x + GOLD) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_init(n, m, ka, seed):
    picks, t = np.empty((m, ka), np.uint32), 0
    for j in range(m):
        seen = []
        while len(seen) < ka:
            r = sm64((seed + t * GOLD) & M64) % n
            t += 1
            if r not in seen:
                seen.append(r)
        picks[j] = seen
    return picks


def train(x, d, m, ksub, iterations, init_rows, seed):
    x = np.asarray(x, np.float32)
    n, ka = x.shape[0], min(ksub, x.shape[0])
    init = draw_init(n, m, ka, seed) if init_rows is None else np.asarray(init_rows)
    g = geom(d, m)
    books = [x[init[j], o:o + dj].copy() for j, (o, dj) in enumerate(g)]
    for it in range(iterations):
        codes = encode(x, books, d, m)
        for j, (o, dj) in enumerate(g):
            for c in range(ka):
                members = np.flatnonzero(codes[:, j] == c)
                if members.size == 0:
                    books[j][c] = x[sm64((seed + ((it * m + j) * 256 + c)) & M64) % n, o:o + dj]
                    continue
                acc = np.zeros(dj, np.float32)
                for r in members:
                    acc = acc + x[r, o:o + dj]
                books[j][c] = acc / np.float32(members.size)
    return books


def tables(q, books, d, m):
    """[B][m][ka]: the fold without the root"""
    q = np.asarray(q, np.float32)
    return np.stack([fold(q[:, o:o + dj], books[j]) for j, (o, dj) in enumerate(geom(d, m))], axis=1)


def adc(T, codes):
    """[B][n] ADC distances: the table entries added with j ascending, then the root"""
    s = np.zeros((T.shape[0], codes.shape[0]), np.float32)
    for j in range(T.shape[1]):
        s = s + T[:, j, :][:, codes[:, j]]
    return np.sqrt(s)


def select(dist, rows, k):
    """the k smallest (bits(dist) << 32) | row of one query: rows, distances"""
    key = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    o = np.argsort(key, kind="stable")[:k]
    return rows[o], dist[o]


def search(q, books, codes, live, d, m, k):
    """ADC search: lists of (rows, distances) per query over the rows where `live`"""
    rows = np.flatnonzero(live).astype(np.uint32)
    a = adc(tables(q, books, d, m), codes[rows]) if rows.size else np.zeros((len(q), 0), np.float32)
    return [select(a[b], rows, k) for b in range(len(q))]


def refine(q, x, cand_rows, k):
    """the candidates re-scored against their rows with the full fold, the k best"""
    dist = np.sqrt(fold(q[None, :], x[cand_rows]))[0] if cand_rows.size else np.zeros(0, np.float32)
    return select(dist, cand_rows, k)
