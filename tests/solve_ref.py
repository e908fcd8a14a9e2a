"""Host restatement of spsamd_solve_tri (include/spsparse_amd.h): the yardstick of the device kernels.

S = (rows, cols, vals) is op(A) as the call takes it (tests/select_ref.operand_S).  T is the `uplo` triangle of S: under LOWER
the tuples with j > i are skipped, under UPPER those with j < i, under UNIT the diagonal too.  For each right-hand side r,
rows ascending (LOWER) or descending (UPPER):

    acc = B[i, r];  d = +0.0
    for each used tuple (i, j, v) of row i, in S's order:
        if j == i:  d = d + v
        else:       acc = acc - v * X[j, r]
    X[i, r] = acc if UNIT else acc / d

Every operation is rounded on its own and a NaN result carries the bits x86-64 gives it (the left operand's NaN quieted, else
the right one's, else 0xFFF8000000000000): numpy does not fix which operand wins, so sub and div apply the rule explicitly,
like dense_ref.add and dense_ref.mul.

solve_ref   the loop as written, tuple by tuple (small cases)
solve_fast  the same by levels: the rows of a level vectorised, one tuple rank of their rows at a time
levels      level(i) = 0 without a used off-diagonal tuple, else 1 + the largest level its used off-diagonal tuples name
zero_pivot  the smallest row whose diagonal fold is +-0.0 (NONUNIT), else -1
"""
import numpy as np

from tests import dense_ref as dr

LOWER, UPPER = 0, 1
NONUNIT, UNIT = 0, 1


def sub(a, b):
    """a - b as subsd gives it (never a + (-b): the negation would flip the sign of a NaN b)."""
    with np.errstate(all="ignore"):
        return dr._x86(np.subtract(a, b), a, b)


def div(a, b):
    """a / b as divsd gives it (0 / 0 and Inf / Inf: the default NaN)."""
    with np.errstate(all="ignore"):
        return dr._x86(np.divide(a, b), a, b)


def _as2d(A):
    A = np.asarray(A, dtype=np.float64)
    return A.reshape(-1, 1) if A.ndim == 1 else A


def classes(S, uplo, diag):
    """Per tuple of S: 0 skipped, 1 used off-diagonal, 2 used diagonal."""
    rows, cols = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64)
    off = (cols > rows) if uplo == UPPER else (cols < rows)
    cl = np.where(off, 1, 0)
    if diag != UNIT:
        cl = np.where(cols == rows, 2, cl)
    return cl


def tuples_used(S, uplo, diag):
    return int(np.count_nonzero(classes(S, uplo, diag)))


def _row_spans(rows, n):
    """S is row-major: [beg[i], beg[i + 1]) are the tuples of row i."""
    return np.searchsorted(np.asarray(rows, np.int64), np.arange(n + 1), side="left")


def diag_fold(S, n, uplo=LOWER, diag=NONUNIT):
    """d_i: +0.0 and then every diagonal tuple of row i added in S's order."""
    d = np.zeros(n, np.float64)
    cl = classes(S, uplo, diag)
    for t in np.flatnonzero(cl == 2):
        i = int(S[0][t])
        d[i] = dr.add(d[i], np.float64(S[2][t]))
    return d


def zero_pivot(S, n, uplo=LOWER, diag=NONUNIT):
    if diag == UNIT:
        return -1
    z = np.flatnonzero(diag_fold(S, n, uplo, diag) == 0)
    return int(z[0]) if z.size else -1


def levels(S, n, uplo=LOWER, diag=NONUNIT):
    """level per row (int64 array of n)."""
    rows, cols = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64)
    cl = classes(S, uplo, diag)
    beg = _row_spans(rows, n)
    lev = np.zeros(n, np.int64)
    order = range(n - 1, -1, -1) if uplo == UPPER else range(n)
    for i in order:
        dep = cols[beg[i]:beg[i + 1]][cl[beg[i]:beg[i + 1]] == 1]
        if dep.size:
            lev[i] = 1 + lev[dep].max()
    return lev


def solve_ref(S, n, B, uplo=LOWER, diag=NONUNIT):
    """The loop as written.  Returns X (the shape of B)."""
    rows, cols, vals = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64), np.asarray(S[2], np.float64)
    B2 = _as2d(B)
    X = np.zeros_like(B2)
    cl = classes(S, uplo, diag)
    beg = _row_spans(rows, n)
    order = range(n - 1, -1, -1) if uplo == UPPER else range(n)
    for i in order:
        acc = B2[i, :].copy()
        d = np.float64(0.0)
        for t in range(beg[i], beg[i + 1]):
            if cl[t] == 2:
                d = np.float64(dr.add(d, vals[t]))
            elif cl[t] == 1:
                acc = sub(acc, dr.mul(vals[t], X[cols[t], :]))
        X[i, :] = acc if diag == UNIT else div(acc, d)
    return X.reshape(np.shape(B))


def solve_fast(S, n, B, uplo=LOWER, diag=NONUNIT, lev=None):
    """The same by levels (for large cases): each (row, rhs) still sees its tuples one at a time in S's order."""
    rows, cols, vals = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64), np.asarray(S[2], np.float64)
    B2 = _as2d(B)
    X = np.zeros_like(B2)
    if n == 0 or B2.shape[1] == 0:
        return X.reshape(np.shape(B))
    cl = classes(S, uplo, diag)
    if lev is None:
        lev = levels(S, n, uplo, diag)
    used = np.flatnonzero(cl)                                   # used tuples, S's order
    urow = rows[used]
    first = np.searchsorted(urow, urow, side="left")
    rank = np.arange(used.size) - first                         # position among the used tuples of its row
    nlev = int(lev.max()) + 1
    row_order = np.argsort(lev, kind="stable")
    rb = np.searchsorted(lev[row_order], np.arange(nlev + 1), side="left")
    tlev = lev[urow]
    t_order = np.lexsort((rank, tlev))                          # by level, then by rank
    tb = np.searchsorted(tlev[t_order], np.arange(nlev + 1), side="left")
    slot = np.zeros(n, np.int64)
    for L in range(nlev):
        r = row_order[rb[L]:rb[L + 1]]
        acc = B2[r, :].copy()
        d = np.zeros(r.size, np.float64)
        slot[r] = np.arange(r.size)
        by_rank = t_order[tb[L]:tb[L + 1]]
        if by_rank.size:
            rk = rank[by_rank]
            bounds = np.searchsorted(rk, np.arange(rk[-1] + 2), side="left")
            for k in range(len(bounds) - 1):
                tt = used[by_rank[bounds[k]:bounds[k + 1]]]     # the k-th used tuple of every row that has one: distinct rows
                s = slot[rows[tt]]
                dg = cl[tt] == 2
                if dg.any():
                    d[s[dg]] = dr.add(d[s[dg]], vals[tt[dg]])
                od = ~dg
                if od.any():
                    p = dr.mul(vals[tt[od]][:, None], X[cols[tt[od]], :])
                    acc[s[od], :] = sub(acc[s[od], :], p)
        X[r, :] = acc if diag == UNIT else div(acc, d[:, None])
    return X.reshape(np.shape(B))


def schedule_stats(S, n, uplo=LOWER, diag=NONUNIT):
    """(levels, max_level_rows) of the schedule."""
    if n == 0:
        return 0, 0
    cnt = np.bincount(levels(S, n, uplo, diag))
    return int(cnt.size), int(cnt.max())
