"""The residual-code definitions of include/fvdb.h ("IVF over residual PQ codes") restated in numpy f32 with Python loops
over dims, beside _pq_ref.py whose geom, encode, decode, fold, select and refine they reuse."""
import numpy as np

import _pq_ref as ref


def codes(x, cents, label, books, d, m):
    """the quantizer's encode rule on row - centroid of the row's list"""
    return ref.encode(np.asarray(x, np.float32) - cents[label], books, d, m)


def row_terms(codes_, cents, label, books):
    """[n]: s = s + r^_i * (r^_i + (c_i + c_i)), i ascending, from +0"""
    rh, c = ref.decode(codes_, books), cents[label]
    s = np.zeros(rh.shape[0], np.float32)
    for i in range(rh.shape[1]):
        s = s + rh[:, i] * (rh[:, i] + (c[:, i] + c[:, i]))
    return s


def ip_tables(q, books, d, m):
    """[B][m][ka]: s = s + q_i * cb_i over the dims of each subspace, ascending"""
    q, out = np.asarray(q, np.float32), []
    for j, (o, dj) in enumerate(ref.geom(d, m)):
        s = np.zeros((q.shape[0], books[j].shape[0]), np.float32)
        for i in range(dj):
            s = s + q[:, o + i, None] * books[j][None, :, i]
        out.append(s)
    return np.stack(out, axis=1)


def scores(q, cents, label, books, codes_, d, m):
    """[B][n]: sqrt(max((base + t_row) - (ip + ip), +0)), base the squared fold of the query against the row's centroid"""
    P, base, term = ip_tables(q, books, d, m), ref.fold(q, cents), row_terms(codes_, cents, label, books)
    ip = np.zeros((P.shape[0], codes_.shape[0]), np.float32)
    for j in range(m):
        ip = ip + P[:, j, :][:, codes_[:, j]]
    v = (base[:, label] + term[None, :]) - (ip + ip)
    return np.sqrt(np.where(v > 0, v, np.float32(0.0)))
