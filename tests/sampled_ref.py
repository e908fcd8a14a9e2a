"""Host restatement of spsamd_multiply_sampled (the sampled dense-dense product), the yardstick of its GPU tests.

For each tuple t of M IN STORAGE ORDER, as (i, j, v) -- (j, i, v) with 'T':
    d = +0.0
    for r = 0 .. k-1:  d = d + P[i, r] * Q[j, r]          (serial, ascending r)
    o = alpha * d;  if beta != 0:  o = o + beta * v      (beta == 0: v is never read)
    out[t] = o

Every product and sum takes the x86-64 NaN bits of tests/dense_ref.py (mul / add; the left operand is the one written on
the left above).

sample_loop  tuple by tuple, the loop as written (small cases)
sample_ref   vectorised across tuples, still serial over r: each tuple sees its k terms one at a time in ascending r, so
             the result is the loop's bit for bit; tuples are processed in chunks to bound the gathered temporaries
"""
import numpy as np

from tests import dense_ref as dr


def _as2d(A):
    A = np.asarray(A, dtype=np.float64)
    return A.reshape(-1, 1) if A.ndim == 1 else A


def _finish(d, v, alpha, beta):
    o = dr.mul(np.float64(alpha), d)
    if beta != 0:                                            # a NaN beta reads v as well
        o = dr.add(o, dr.mul(np.float64(beta), np.asarray(v, dtype=np.float64)))
    return o


def sample_loop(i0, i1, v, P, Q, transpose='.', alpha=1.0, beta=0.0):
    P2, Q2 = _as2d(P), _as2d(Q)
    rows, cols = (i1, i0) if transpose == 'T' else (i0, i1)
    out = np.empty(len(rows), dtype=np.float64)
    for t in range(len(rows)):
        i, j = int(rows[t]), int(cols[t])
        d = np.float64(0.0)
        for r in range(P2.shape[1]):
            d = dr.add(d, dr.mul(P2[i, r], Q2[j, r]))
        out[t] = _finish(d, None if beta == 0 else v[t], alpha, beta)
    return out


def sample_ref(i0, i1, v, P, Q, transpose='.', alpha=1.0, beta=0.0, chunk=1 << 20):
    P2, Q2 = _as2d(P), _as2d(Q)
    rows, cols = (np.asarray(i1), np.asarray(i0)) if transpose == 'T' else (np.asarray(i0), np.asarray(i1))
    n, k = len(rows), P2.shape[1]
    out = np.empty(n, dtype=np.float64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        pr, qc = P2[rows[s:e].astype(np.int64)], Q2[cols[s:e].astype(np.int64)]
        d = np.zeros(e - s)
        for r in range(k):
            d = dr.add(d, dr.mul(pr[:, r], qc[:, r]))
        out[s:e] = _finish(d, None if beta == 0 else np.asarray(v)[s:e], alpha, beta)
    return out
