"""Host restatement of spsamd_reduce (include/spsparse_amd.h): the yardstick of the device kernels.

S is op(A) as the call takes it (tests/select_ref.operand_S: the intake model spsamd_select uses, not restated here).  For
every row the contributing tuples -- all of them, for DIAG those with col == row -- are folded ONE AT A TIME in S's order:

    SUM      acc = +0.0;  acc = acc + v
    SUM_ABS  acc = +0.0;  acc = acc + |v|       (sign bit cleared)
    SUM_SQ   acc = +0.0;  acc = acc + v * v     (two roundings)
    MAX_ABS  the largest |v| over the non-NaN tuples through mag, +0.0 when there is none
    COUNT    the number of tuples, as a double
    DIAG     SUM over the tuples with col == row

Sums and products go through tests/dense_ref.add / mul, so a NaN result has the bits x86-64 gives it (the accumulator is
the left operand).  post() is numpy's 1.0 / x and sqrt on x86-64 -- the SSE divsd / sqrtsd -- with the NaN rules written
out beside them, so that the restatement does not lean on numpy's choice of NaN.
"""
import numpy as np

from tests import dense_ref as dr
from tests import select_ref as sr

SUM, SUM_ABS, SUM_SQ, MAX_ABS, COUNT, DIAG = 1, 2, 3, 4, 5, 6
OPS = (SUM, SUM_ABS, SUM_SQ, MAX_ABS, COUNT, DIAG)
ORDERED = (SUM, SUM_ABS, SUM_SQ, DIAG)
NONE, RECIP, SQRT, RSQRT = 0, 1, 2, 3
POSTS = (NONE, RECIP, SQRT, RSQRT)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def recip(r):
    """1.0 / r, correctly rounded; a NaN operand comes back quieted."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = np.divide(1.0, r)
    nan = np.isnan(r)
    out.view(np.uint64)[nan] = _bits(r)[nan] | dr.QUIET
    return out


def sqrt(r):
    """sqrt(r), correctly rounded; a NaN operand comes back quieted, r < 0 gives the default NaN, sqrt(-0.0) = -0.0."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = np.sqrt(r)
    nan = np.isnan(r)
    out.view(np.uint64)[nan] = _bits(r)[nan] | dr.QUIET
    out.view(np.uint64)[~nan & (r < 0)] = dr.DEFAULT_NAN
    return out


def post_apply(r, post):
    r = np.ascontiguousarray(r, dtype=np.float64)
    if post == RECIP:
        return recip(r)
    if post == SQRT:
        return sqrt(r)
    if post == RSQRT:
        return recip(sqrt(r))
    return r.copy()


def fold_row(op, row, cols, vals):
    """(has a contributing tuple, r_i) of one row: the loop as the header writes it."""
    if op == COUNT:
        return len(vals) > 0, np.float64(len(vals))
    if op == MAX_ABS:
        g = sr.mag(vals)
        g = g[g <= sr.INF_BITS]
        m = np.array([g.max() if g.size else 0], np.uint64)
        return len(vals) > 0, m.view(np.float64)[0]
    acc, has = np.float64(0.0), False
    for c, v in zip(cols, vals):
        v = np.float64(v)
        if op == DIAG and int(c) != int(row):
            continue
        has = True
        if op == SUM_ABS:
            v = (_bits(np.array([v])) & sr.SIGN).view(np.float64)[0]
        elif op == SUM_SQ:
            v = np.float64(dr.mul(v, v))
        acc = np.float64(dr.add(acc, v))
    return has, acc


def reduce_ref(S, nrow, op, post=NONE):
    """(idx, val) of the sparse form and the dense form's val, for S = (rows, cols, vals) with non-descending rows."""
    rows, cols, vals = (np.asarray(x) for x in S)
    assert np.all(np.diff(rows.astype(np.int64)) >= 0)
    bounds = np.searchsorted(rows, np.arange(nrow + 1), side="left")
    idx, raw = [], []
    for i in range(nrow):
        b, e = bounds[i], bounds[i + 1]
        if b == e:
            continue
        has, r = fold_row(op, i, cols[b:e], vals[b:e])
        if has:
            idx.append(i); raw.append(r)
    idx = np.array(idx, np.int32)
    val = post_apply(np.array(raw, np.float64), post)
    dense = np.zeros(nrow, np.float64)
    dense[idx] = val
    return idx, val, dense


def reduce_fast(S, nrow, op, post=NONE):
    """The same by rounds across rows (round t adds the t-th contributing tuple of every row that has one: each row still
    sees its tuples one at a time in order), for the long rows of the GPU tests."""
    rows, cols, vals = (np.asarray(x) for x in S)
    rows = rows.astype(np.int64)
    lens = np.bincount(rows, minlength=nrow)
    if op == COUNT:
        has, acc = lens > 0, lens.astype(np.float64)
    elif op == MAX_ABS:
        has, acc = lens > 0, sr.row_max(rows, vals, nrow)
    else:
        keep = cols.astype(np.int64) == rows if op == DIAG else np.ones(len(vals), bool)
        r, v = rows[keep], np.asarray(vals, np.float64)[keep]
        if op == SUM_ABS:
            v = (_bits(v) & sr.SIGN).view(np.float64)
        elif op == SUM_SQ:
            v = dr.mul(v, v)
        has = np.bincount(r, minlength=nrow) > 0
        acc = np.zeros(nrow, np.float64)
        if len(v):
            rank = np.arange(len(v)) - np.searchsorted(r, r, side="left")
            by_rank = np.argsort(rank, kind="stable")
            bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2), side="left")
            for t in range(rank.max() + 1):
                sel = by_rank[bounds[t]:bounds[t + 1]]
                acc[r[sel]] = dr.add(acc[r[sel]], v[sel])
    idx = np.flatnonzero(has).astype(np.int32)
    val = post_apply(acc[idx], post)
    dense = np.zeros(nrow, np.float64)
    dense[idx] = val
    return idx, val, dense


def post_probe_values(rng, n=100_000):
    """Doubles for the post-operation check: every exponent, subnormals, +-0, +-Inf, negatives, quiet and signalling NaNs
    with payloads, and the neighbours of powers of two and of perfect squares."""
    bits = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    v = bits.view(np.float64).copy()
    sub = rng.integers(1, 2 ** 52, n // 20, dtype=np.uint64)
    sub[::2] |= np.uint64(1 << 63)
    nan = np.uint64(0x7FF0000000000000) | rng.integers(1, 2 ** 52, n // 20, dtype=np.uint64)
    nan[::3] |= np.uint64(1 << 63)
    k = np.arange(-1070, 1024, 7, dtype=np.float64)
    near = np.concatenate([np.nextafter(2.0 ** k, 0), 2.0 ** k, np.nextafter(2.0 ** k, np.inf)])
    sq = rng.integers(1, 2 ** 26, n // 20).astype(np.float64) ** 2
    edge = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308,
                     4.4501477170144023e-308, 8.98846567431158e307])
    return np.concatenate([v, sub.view(np.float64), nan.view(np.float64), near, -near, sq, np.nextafter(sq, 0), edge])
