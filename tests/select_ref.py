"""Host restatement of spsamd_select (include/spsparse_amd.h): the yardstick of the device kernels.

S is op(A) as the call takes it: a raw operand consolidated by op()'s rows (tests/add_ref.consolidate, pinned to the test
oracle's consolidate() by tests/test_select_host.py), an operand whose sort0 names op()'s row order as stored.  The result
is the subsequence of S a predicate keeps, decided tuple by tuple through

    mag(x) = the bits of x with the sign cleared, as an unsigned integer

    TRIL / TRIU / DIAG / OFFDIAG   j - i  <= / >= / == / !=  d
    ABS_GE                         mag(v) >= mag(theta)
    ROW_REL                        mag(v) >= mag(theta * m_i),  m_i = the largest |v| over the non-NaN entries of the row
    ROW_TOPK                       rank of the tuple in its row by (mag descending, position ascending) < k

select_mask     the decision for every tuple of S (vectorised; top-k by one stable sort)
topk_mask_loop  top-k row by row with sorted(): what test_select_host.py pins select_mask to
"""
import numpy as np

from tests import add_ref as ar

TRIL, TRIU, DIAG, OFFDIAG, ABS_GE, ROW_REL, ROW_TOPK = 1, 2, 3, 4, 5, 6, 7
PREDICATES = (TRIL, TRIU, DIAG, OFFDIAG, ABS_GE, ROW_REL, ROW_TOPK)
SIGN = np.uint64(0x7FFFFFFFFFFFFFFF)
INF_BITS = np.uint64(0x7FF0000000000000)


def mag(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) & SIGN


def operand_S(A, transpose='.', policy=ar.ADD, zero_nan=False, sort0=-1):
    """(rows, cols, vals) of S for the stored tuples A = (idx0, idx1, val)."""
    r, c = ar.op(A[0], A[1], transpose)
    r, c, v = np.asarray(r, np.int32), np.asarray(c, np.int32), np.asarray(A[2], np.float64)
    lead = 1 if transpose == 'T' else 0
    if sort0 == lead:
        return r.copy(), c.copy(), v.copy()
    return ar.consolidate(r, c, v, policy=policy, zero_nan=zero_nan)


def row_max(rows, vals, nrow):
    """m_i as float64: the largest |v| over the non-NaN entries of each row, +0.0 where there are none."""
    m = np.zeros(nrow, np.uint64)
    g = mag(vals)
    ok = g <= INF_BITS
    np.maximum.at(m, np.asarray(rows)[ok], g[ok])
    return m.view(np.float64)


def topk_mask(rows, vals, k):
    """rank < k by one stable sort on (row, mag descending): equal keys stay in position order."""
    n = len(vals)
    inv = np.uint64(0xFFFFFFFFFFFFFFFF) - mag(vals)
    order = np.lexsort((inv, np.asarray(rows)))
    rs = np.asarray(rows)[order]
    start = np.zeros(n, np.int64)
    if n:
        first = np.flatnonzero(np.r_[True, rs[1:] != rs[:-1]])
        start = np.repeat(first, np.diff(np.r_[first, n]))
    keep = np.zeros(n, bool)
    keep[order] = (np.arange(n) - start) < k
    return keep


def topk_mask_loop(rows, vals, k):
    """The same by brute force: every row's tuples through sorted() on (-mag, position)."""
    rows = np.asarray(rows)
    g = mag(vals)
    keep = np.zeros(len(vals), bool)
    for r in np.unique(rows):
        pos = [int(t) for t in np.flatnonzero(rows == r)]
        for t in sorted(pos, key=lambda t: (-int(g[t]), t))[:max(int(k), 0)]:
            keep[t] = True
    return keep


def select_mask(S, nrow, predicate, iparam=0, dparam=0.0, complement=False):
    rows, cols, vals = S
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    if predicate in (TRIL, TRIU, DIAG, OFFDIAG):
        diff, d = cols - rows, int(iparam)
        d = max(min(d, 2 ** 62), -2 ** 62)            # |j - i| <= 2^31: the comparison is the same
        keep = {TRIL: diff <= d, TRIU: diff >= d, DIAG: diff == d, OFFDIAG: diff != d}[predicate]
    elif predicate == ABS_GE:
        keep = mag(vals) >= mag(np.array([dparam]))[0]
    elif predicate == ROW_REL:
        with np.errstate(invalid="ignore", over="ignore"):
            t = np.float64(dparam) * row_max(rows, vals, nrow)
        keep = mag(vals) >= mag(t)[rows] if len(vals) else np.zeros(0, bool)
    elif predicate == ROW_TOPK:
        keep = topk_mask(rows, vals, int(iparam))
    else:
        raise ValueError("unknown predicate")
    keep = np.asarray(keep, bool)
    return ~keep if complement else keep


def select_ref(S, nrow, predicate, iparam=0, dparam=0.0, complement=False):
    keep = select_mask(S, nrow, predicate, iparam, dparam, complement)
    return tuple(np.asarray(x)[keep] for x in S)


# ---------------------------------------------------------------- inputs

TIE_MAGS = (0.5, 1.0, 3.0)


def special_values(rng, n, special=0.3, ties=False):
    """add_ref's value mix (+-0, NaN payloads quiet and signalling, +-Inf); ties: drawn from a handful of magnitudes with
    both signs, so that most decisions at a k-th magnitude are ties."""
    v = ar._values(rng, n, special)
    if ties:
        plain = np.isfinite(v) & (v != 0)
        t = rng.choice(TIE_MAGS, n) * rng.choice((-1.0, 1.0), n)
        v[plain] = t[plain]
    return v


def unique_key_operand(rng, shape, nnz, special=0.3, ties=False):
    """Raw operand with every (i, j) once, in shuffled storage order: NaN and Inf are fair game."""
    total = shape[0] * shape[1]
    nnz = min(nnz, total)
    flat = rng.choice(total, nnz, replace=False)
    i0, i1 = (flat // shape[1]).astype(np.int32), (flat % shape[1]).astype(np.int32)
    return i0, i1, special_values(rng, nnz, special, ties)


def duplicate_key_operand(rng, shape, nnz, ties=False):
    """Raw operand with duplicate keys; NaN and +-Inf only on keys that occur once (a folded NaN's bits are the
    consolidation's business), +-0 anywhere."""
    i0 = rng.integers(0, shape[0], nnz).astype(np.int32)
    i1 = rng.integers(0, shape[1], nnz).astype(np.int32)
    v = special_values(rng, nnz, 0.3, ties)
    key = i0.astype(np.int64) * shape[1] + i1
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    dup = cnt[inv] > 1
    bad = dup & ~np.isfinite(v)
    v[bad] = rng.choice(TIE_MAGS, int(bad.sum())) if ties else rng.standard_normal(int(bad.sum()))
    return i0, i1, v


def rows_of_lengths(rng, lengths, ncol, equal_rows=(), special=0.02):
    """Row-major sorted operand whose row r has exactly lengths[r] tuples (distinct ascending columns); the rows named in
    equal_rows hold one magnitude with both signs (every top-k decision in them is a tie)."""
    rows, cols, vals = [], [], []
    for r, n in enumerate(lengths):
        if n == 0:
            continue
        c = np.sort(rng.choice(ncol, n, replace=False)).astype(np.int32)
        if r in equal_rows:
            v = 2.0 * rng.choice((-1.0, 1.0), n)
        else:
            v = special_values(rng, n, special, ties=bool(r % 2))
        rows.append(np.full(n, r, np.int32)); cols.append(c); vals.append(v)
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
