"""Host restatement of spsamd_extract (include/spsparse_amd.h): the yardstick of the device kernels.

S is op(A) as the call takes it (tests/select_ref.operand_S).  For every output row r, every output column c and every tuple
(I[r], J[c], v) of S at position p the result holds one tuple (r, c, v), and no other; the order is (r, c, p) ascending.
I / J None: every index of that dimension, ascending.  Values are copied, never computed.

extract_ref       vectorised: one join of S's tuples with the row list and the column list, one lexsort on (r, c, p)
extract_ref_loop  the same by brute force, straight from the sentence above: what test_extract_host.py pins it to
"""
import numpy as np


def _list(L, dim):
    return np.arange(dim, dtype=np.int64) if L is None else np.asarray(L, np.int64)


def extract_ref(S, I, J, nrows, ncols):
    """(rows, cols, vals) of the submatrix; nrows x ncols is the shape of op(A)."""
    sr, sc, sv = (np.asarray(x) for x in S)
    I, J = _list(I, nrows), _list(J, ncols)
    assert (I.size == 0 or (I.min() >= 0 and I.max() < nrows)) and (J.size == 0 or (J.min() >= 0 and J.max() < ncols))
    # output rows per source row and output columns per source column, ascending (stable sorts of the lists)
    oi, oj = np.argsort(I, kind="stable"), np.argsort(J, kind="stable")
    ip = np.searchsorted(I[oi], np.arange(nrows + 1))
    jp = np.searchsorted(J[oj], np.arange(ncols + 1))
    p = np.arange(len(sv), dtype=np.int64)
    mr = ip[sr.astype(np.int64) + 1] - ip[sr] if len(sv) else np.zeros(0, np.int64)
    mc = jp[sc.astype(np.int64) + 1] - jp[sc] if len(sv) else np.zeros(0, np.int64)
    # every tuple once per output row that names its row ...
    t1 = np.repeat(p, mr)
    r = oi[np.repeat(ip[sr], mr) + (np.arange(t1.size) - np.repeat(np.cumsum(mr) - mr, mr))] if t1.size else np.zeros(0, np.int64)
    # ... and each of those once per output column that names its column
    m2 = mc[t1]
    t2 = np.repeat(t1, m2)
    r2 = np.repeat(r, m2)
    c2 = oj[np.repeat(jp[sc[t1]], m2) + (np.arange(t2.size) - np.repeat(np.cumsum(m2) - m2, m2))] if t2.size else np.zeros(0, np.int64)
    o = np.lexsort((t2, c2, r2))
    return r2[o].astype(np.int32), c2[o].astype(np.int32), sv[t2[o]]


def extract_ref_loop(S, I, J, nrows, ncols):
    sr, sc, sv = (np.asarray(x) for x in S)
    I, J = _list(I, nrows), _list(J, ncols)
    out = []
    for r in range(len(I)):
        for c in range(len(J)):
            for p in range(len(sv)):
                if sr[p] == I[r] and sc[p] == J[c]:
                    out.append((r, c, p))
    rr = np.array([t[0] for t in out], np.int32)
    cc = np.array([t[1] for t in out], np.int32)
    pp = np.array([t[2] for t in out], np.int64)
    return rr, cc, sv[pp]


# ---------------------------------------------------------------- inputs

LIST_KINDS = ("all", "range", "ascending", "permutation", "repeats", "empty")


def index_list(rng, kind, dim):
    """An index list of one of the shapes the tests sweep (None: every index)."""
    if kind == "all":
        return None
    if kind == "empty" or dim == 0:
        return np.zeros(0, np.int32)
    if kind == "range":
        lo = int(rng.integers(0, dim))
        return np.arange(lo, int(rng.integers(lo, dim)) + 1, dtype=np.int32)
    if kind == "ascending":
        return np.flatnonzero(rng.random(dim) < 0.6).astype(np.int32)
    if kind == "permutation":
        return rng.permutation(dim).astype(np.int32)
    return rng.integers(0, dim, int(rng.integers(1, 2 * dim + 2))).astype(np.int32)


def selection_matrix(L, dim):
    """S_L = {(k, L[k], 1.0)}: len(L) x dim, so that S_I * A * S_J^T is the extraction (stored row-major sorted)."""
    L = _list(L, dim)
    return np.arange(len(L), dtype=np.int32), L.astype(np.int32), np.ones(len(L)), (len(L), dim)
