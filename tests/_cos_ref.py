"""The definitions of include/fvdb.h, "cosine search" (DESIGN.md section 9y), in numpy: every operation rounds to f32,
the folds run left to right over d with whole-array operations, a stable argsort gives the order."""
import numpy as np

f32 = np.float32


def sims(q, x):
    """[B][n] cosine_similarity_scalar: dot / (mag_q * mag_x), 0.0 when either magnitude is 0"""
    q, x = np.asarray(q, f32), np.asarray(x, f32)
    dot, sq, sx = np.zeros((q.shape[0], x.shape[0]), f32), np.zeros(q.shape[0], f32), np.zeros(x.shape[0], f32)
    for i in range(q.shape[1]):
        dot = dot + q[:, i, None] * x[None, :, i]
        sq = sq + q[:, i] * q[:, i]
        sx = sx + x[:, i] * x[:, i]
    den = np.sqrt(sq)[:, None] * np.sqrt(sx)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, f32(0), dot / den).astype(f32)


def top(sim, rows, k):
    """the k largest of one query's similarities over the candidate rows, ties to the earlier row: (rows, sims)"""
    order = np.argsort(-sim[rows], kind="stable")[:k]
    return rows[order], sim[rows][order]


def normalize(x):
    """batch_normalize: x / norm, a zero-norm row unchanged"""
    x = np.asarray(x, f32)
    s = np.zeros(x.shape[0], f32)
    for i in range(x.shape[1]):
        s = s + x[:, i] * x[:, i]
    norm = np.sqrt(s)
    return np.where(norm[:, None] == 0, x, x / np.where(norm == 0, f32(1), norm)[:, None]).astype(f32)
