"""Host yardstick of spsamd_multiply_masked (include/spsparse_amd.h): the test oracle's product, then the tuples whose key
is a key of M.

    masked_ref(A, B, (mi, mj), ...)   orc.multiply(A, B, ...) (row-wise checker by default), filtered by np.isin on the
                                      int64 keys i * ncol + j

tests/test_masked_host.py pins the row-wise form to the oracle's inner-product loop (orc_multiply_mm), filtered the same way.
"""
import numpy as np

from oracle import binding as orc
from tests import add_ref as ar


def keys(i, j, ncol):
    return np.asarray(i, np.int64) * np.int64(ncol) + np.asarray(j, np.int64)


def masked_ref(A, B, M, C_=1.0, scalei=None, tA='.', scalej=None, tB='.', scalek=None, duplicate_policy=ar.ADD,
               zero_nan=False, rowwise=True, nthreads=1):
    """(i, j, v) of the reference's product restricted to M's keys, ascending (i, j).  A, B: orc.Mat; M: (rows, cols) of
    its keys in the product's orientation (duplicates allowed)."""
    i, j, v, shape = orc.multiply(A, B, C_, scalei, tA, scalej, tB, scalek, duplicate_policy, zero_nan,
                                  rowwise=rowwise, nthreads=nthreads)
    ncol = max(int(shape[1]), 1)
    keep = np.isin(keys(i, j, ncol), keys(M[0], M[1], ncol))
    i, j, v = i[keep], j[keep], v[keep]
    o = np.lexsort((j, i))
    return i[o].astype(np.int32), j[o].astype(np.int32), v[o].astype(np.float64)


def same_tuples(got, want, payloads=False):
    """Indices equal; values bit-identical (signed zeros and infinities count) except that where both are NaN only the
    NaN counts, unless payloads: the oracle's two loops (orc_multiply_mm, the row-wise checker) are compiled separately
    and already disagree on which payload wins where two NaNs meet in one product or sum."""
    if payloads:
        return ar.same_tuples(got, want)
    gi, gj, gv = (np.asarray(x) for x in got)
    wi, wj, wv = (np.asarray(x) for x in want)
    if gi.shape != wi.shape or not (np.array_equal(gi, wi) and np.array_equal(gj, wj)):
        return False
    gn, wn = np.isnan(gv), np.isnan(wv)
    return np.array_equal(gn, wn) and np.array_equal(gv[~gn].view(np.int64), wv[~wn].view(np.int64))


def sanitize_duplicates(X):
    """X = (idx0, idx1, val) with NaN and +-Inf kept off keys that occur more than once: a merge of duplicates is the
    device consolidation's own sum (the multiply path's), whose NaN bits are the device's, not x86-64's.  Specials on
    keys that occur once, +-0 and duplicates themselves stay."""
    i0, i1, v = (np.asarray(x).copy() for x in X)
    if v.size:
        k = keys(i0, i1, int(max(i1.max(), 0)) + 1)
        _, inv, cnt = np.unique(k, return_inverse=True, return_counts=True)
        bad = (cnt[inv] > 1) & ~np.isfinite(v)
        v[bad] = np.arange(1, int(bad.sum()) + 1) * 0.375
    return i0.astype(np.int32), i1.astype(np.int32), v.astype(np.float64)


def random_scale(rng, dim, present=True):
    """Sorted, unique scale vector over part of [0, dim) with some zero entries, or None."""
    if not present or dim == 0:
        return None
    idx = np.flatnonzero(rng.random(dim) < 0.8).astype(np.int32)
    if idx.size == 0:
        idx = np.array([0], np.int32)
    val = rng.standard_normal(idx.size)
    val[rng.random(idx.size) < 0.15] = 0.0
    return idx, val


def random_mask(rng, shape, n):
    """(rows, cols) of n random keys of `shape` with duplicates."""
    if n == 0 or shape[0] == 0 or shape[1] == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    r = rng.integers(0, shape[0], n).astype(np.int32)
    c = rng.integers(0, shape[1], n).astype(np.int32)
    d = rng.integers(0, n, n // 5)
    return np.concatenate([r, r[d]]), np.concatenate([c, c[d]])
