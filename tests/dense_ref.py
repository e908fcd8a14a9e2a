"""Host restatements of the reference's multiply(M, x, y, handle_nan, transpose) (multiply_dense.hpp:11-35) into a
DenseAccum (accum.hpp:110-140), for nrhs right-hand sides: the yardstick of spsamd_multiply_dense.

For each right-hand side r, over M's tuples (i, j, v) in STORAGE order ((j, i) with 'T'):
    p = v * X[j, r];  if handle_nan and not isfinite(p): skip
    Y[i, r]:  ADD  Y += p  |  REPLACE  Y = p  |  LEAVE_ALONE  if not isnan(Y): Y = p

A NaN result carries the bits x86-64 SSE gives it (the reference's build): the left operand's NaN quieted if it is one
(`v` in `v * x`, the entry in `oval += val`), else the right operand's, else the default NaN 0xFFF8000000000000.  numpy's
own loops do not fix which operand wins when both are NaN, so both restatements apply the rule explicitly.

apply_ref  one tuple at a time (the loop as written: small cases)
apply_fast stable sort by the output row, then ROUNDS: round t adds the t-th product of every row, vectorised across
           rows (exact: each entry still sees its products one at a time in storage order; rounds = longest row)
"""
import numpy as np

ADD, LEAVE_ALONE, REPLACE = 1, 0, 2
QUIET = np.uint64(1 << 51)
DEFAULT_NAN = np.uint64(0xFFF8000000000000)


def _x86(r, a, b):
    """r = a (op) b computed by numpy; give its NaNs the x86-64 bits."""
    r = np.array(r, dtype=np.float64, copy=True)
    bad = np.isnan(r)
    if bad.any():
        a = np.broadcast_to(np.asarray(a, dtype=np.float64), r.shape)
        b = np.broadcast_to(np.asarray(b, dtype=np.float64), r.shape)
        ai, bi = a.view(np.uint64), b.view(np.uint64)
        fix = np.where(np.isnan(a), ai | QUIET, np.where(np.isnan(b), bi | QUIET, DEFAULT_NAN))
        r.view(np.uint64)[bad] = fix[bad]
    return r


def mul(v, x):
    with np.errstate(all="ignore"):
        return _x86(np.multiply(v, x), v, x)


def add(y, p):
    with np.errstate(all="ignore"):
        return _x86(np.add(y, p), y, p)


def _step(y, p, policy, handle_nan):
    """One DenseAccum::add (accum.hpp:124-135) per entry of y with the products p (same shape)."""
    ok = np.isfinite(p) if handle_nan else np.ones(p.shape, bool)
    if policy == ADD:
        new = add(y, p)
    elif policy == REPLACE:
        new = p
    else:
        new = p
        ok = ok & ~np.isnan(y)
    out = y.copy()
    out[ok] = new[ok]
    return out


def _as2d(A):
    A = np.asarray(A, dtype=np.float64)
    return A.reshape(-1, 1) if A.ndim == 1 else A


def apply_ref(i0, i1, v, X, Y, transpose='.', policy=ADD, handle_nan=False):
    """The reference loop, tuple by tuple.  Returns a new Y (same shape as Y)."""
    X2, Y2 = _as2d(X), _as2d(Y).copy()
    rows, cols = (i1, i0) if transpose == 'T' else (i0, i1)
    for t in range(len(v)):
        i, j = int(rows[t]), int(cols[t])
        p = mul(np.float64(v[t]), X2[j, :])
        Y2[i, :] = _step(Y2[i, :], p, policy, handle_nan)
    return Y2.reshape(np.shape(Y))


def apply_fast(i0, i1, v, X, Y, transpose='.', policy=ADD, handle_nan=False):
    """The same result by rounds across rows (for large cases)."""
    X2, Y2 = _as2d(X), _as2d(Y).copy()
    rows, cols = (np.asarray(i1), np.asarray(i0)) if transpose == 'T' else (np.asarray(i0), np.asarray(i1))
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    if n == 0 or Y2.shape[1] == 0:
        return Y2.reshape(np.shape(Y))
    order = np.argsort(rows, kind="stable")                  # storage order inside a row
    srow = rows[order].astype(np.int64)
    first = np.searchsorted(srow, srow, side="left")
    rank = np.arange(n) - first                              # position of each tuple inside its row
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2), side="left")
    for t in range(rank.max() + 1):
        sel = order[by_rank[bounds[t]:bounds[t + 1]]]        # the t-th tuple of every row that has one: distinct rows
        r = rows[sel].astype(np.int64)
        p = mul(v[sel][:, None], X2[cols[sel].astype(np.int64), :])
        Y2[r, :] = _step(Y2[r, :], p, policy, handle_nan)
    return Y2.reshape(np.shape(Y))


def same_bits(a, b):
    """Bit-identical float64 arrays (NaN payloads and signed zeros count)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
