"""Host restatement of spsamd_add (include/spsparse_amd.h): the yardstick of the device merge.

    VectorCooArray T;
    for (i, j, v) in op(A), in storage order:  T.add({i, j}, alpha * v);
    for (i, j, v) in op(B), in storage order:  T.add({i, j}, beta * v);
    consolidate(ret, T, {0, 1}, duplicate_policy, zero_nan);          (algorithm.hpp:251-319)

Products and sums go through the x86 helpers of tests/dense_ref.py, so a NaN result carries the bits x86-64 gives it.
The consolidate() loop is written out tuple by tuple: the leading run of zeros (and NaNs under zero_nan) is skipped, after
the first kept entry only exact zeros are, and the rest is folded left to right by the policy.

add_ref      the loop as written (small cases)
scaled_cat   op(A)'s and op(B)'s scaled tuples appended, A's first: what the test oracle's consolidate() takes
"""
import numpy as np

from tests import dense_ref as dr

ADD, LEAVE_ALONE, REPLACE = dr.ADD, dr.LEAVE_ALONE, dr.REPLACE


def op(i0, i1, transpose):
    """(rows, cols) of op(X): the indices swap exactly when the flag is 'T'."""
    return (np.asarray(i1), np.asarray(i0)) if transpose == 'T' else (np.asarray(i0), np.asarray(i1))


def scaled_cat(A, B, alpha=1.0, beta=1.0, tA='.', tB='.'):
    """(rows, cols, vals) of the appended operands, every value alpha * v / beta * v (also for 1 and 0)."""
    ra, ca = op(A[0], A[1], tA)
    rb, cb = op(B[0], B[1], tB)
    va = dr.mul(np.float64(alpha), np.asarray(A[2], np.float64))
    vb = dr.mul(np.float64(beta), np.asarray(B[2], np.float64))
    return (np.concatenate([ra, rb]).astype(np.int32), np.concatenate([ca, cb]).astype(np.int32),
            np.concatenate([va, vb]).astype(np.float64))


def consolidate(rows, cols, vals, policy=ADD, zero_nan=False):
    """consolidate() by sort order {0, 1}, tuple by tuple."""
    order = np.lexsort((cols, rows))                 # stable
    out_i, out_j, out_v = [], [], []
    k, n = 0, len(order)
    while k < n and (vals[order[k]] == 0 or (zero_nan and np.isnan(vals[order[k]]))):
        k += 1                                       # the leading run (algorithm.hpp:272-275)
    if k == n:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
    ai, aj, acc = rows[order[k]], cols[order[k]], np.float64(vals[order[k]])
    for t in order[k + 1:]:
        v = np.float64(vals[t])
        if v == 0:                                   # only exact zeros from here on (algorithm.hpp:284-292)
            continue
        if rows[t] != ai or cols[t] != aj:
            out_i.append(ai); out_j.append(aj); out_v.append(acc)
            ai, aj, acc = rows[t], cols[t], v
        elif policy == ADD:
            acc = np.float64(dr.add(acc, v))
        elif policy == REPLACE:
            acc = v
    out_i.append(ai); out_j.append(aj); out_v.append(acc)
    return np.array(out_i, np.int32), np.array(out_j, np.int32), np.array(out_v, np.float64)


def add_ref(A, B, alpha=1.0, beta=1.0, tA='.', tB='.', policy=ADD, zero_nan=False):
    """alpha * op(A) + beta * op(B); A, B: (idx0, idx1, val) in storage order.  Returns (i, j, v) row-major."""
    return consolidate(*scaled_cat(A, B, alpha, beta, tA, tB), policy=policy, zero_nan=zero_nan)


NAN_PAYLOADS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FF80000DEADBEEF, 0xFFF4000000000123)


def _values(rng, n, special=0.3):
    """Standard normal values with ~special of them +-0, NaNs of several payloads (quiet and signalling) or +-Inf."""
    v = rng.standard_normal(n)
    k = rng.random(n)
    pick = rng.integers(0, 6, n)
    for t in np.flatnonzero(k < special):
        if pick[t] == 0:
            v[t] = 0.0
        elif pick[t] == 1:
            v[t] = -0.0
        elif pick[t] == 2:
            v[t] = np.inf
        elif pick[t] == 3:
            v[t] = -np.inf
        else:
            v[t:t + 1].view(np.uint64)[0] = np.uint64(NAN_PAYLOADS[int(rng.integers(len(NAN_PAYLOADS)))])
    return v


def random_operand(rng, shape, nnz, special=0.3, lead_junk=False):
    """(idx0, idx1, val) in storage order, unsorted, with duplicates (few distinct indices).  lead_junk: the tuples at the
    smallest (row, col) keys of either orientation are 0 / NaN, so that zero_nan has a leading run to drop."""
    i0 = rng.integers(0, shape[0], nnz).astype(np.int32)
    i1 = rng.integers(0, shape[1], nnz).astype(np.int32)
    v = _values(rng, nnz, special)
    if lead_junk and nnz:
        low = (i0 <= min(1, shape[0] - 1)) | (i1 <= min(1, shape[1] - 1))
        j = _values(rng, int(low.sum()), 1.0)
        j[np.isinf(j)] = np.nan
        v[low] = j
    return i0, i1, v


def sort_storage(X, lead):
    """X stored sorted by (idx_lead, idx_other), stable: a consolidated-order operand that may still hold duplicates."""
    i0, i1, v = X
    o = np.lexsort((i1, i0)) if lead == 0 else np.lexsort((i0, i1))
    return i0[o], i1[o], v[o]


def same_tuples(got, want):
    """Indices equal and values bit-identical (NaN payloads and signed zeros count)."""
    gi, gj, gv = (np.asarray(x) for x in got)
    wi, wj, wv = (np.asarray(x) for x in want)
    return (gi.shape == wi.shape and np.array_equal(gi, wi) and np.array_equal(gj, wj)
            and dr.same_bits(gv, wv))
