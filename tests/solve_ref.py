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
peel_plan   the peel launches of the analysis for a sequence of level sizes (the host loop of `analyse` restated)
by_levels, mirrored, pattern_noise, far_rows   operands built with their level vector known, for the cases too large for
            `levels` (pass lev= to solve_fast)
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


def peel_plan(sizes, thin_max, batch):
    """(thin, wide): the peel launches the analysis issues for a schedule whose level l has sizes[l] rows -- the host loop
    of `analyse` (k_solve.hip) restated.  The host reads the frontier size; a frontier of at most thin_max rows is one thin
    launch, which walks on to the first level above thin_max or to the end; if levels remain, `batch` wide launches follow,
    one level each (those past the last level find an empty frontier and still count); then the host looks again.  One
    level means no used off-diagonal tuple: no peel at all."""
    sizes = [int(s) for s in sizes]
    thin = wide = 0
    l, n = 0, len(sizes)
    if n <= 1:
        return 0, 0
    while l < n:
        if sizes[l] <= thin_max:
            thin += 1
            while l < n and sizes[l] <= thin_max:
                l += 1
        if l < n:
            wide += batch
            l += batch
    return thin, wide


def by_levels(rng, sizes, fan=None, gather=None, scatter=True):
    """Lower-triangular operand with a known level vector: level l has sizes[l] rows.  Every row has a diagonal in
    [2, 3); a row of level l > 0 has one off-diagonal tuple in level l - 1 and, one time in two, a second one.
    fan = {l: H}: row 0 of level l is the one parent of H rows of level l + 1; the other rows of level l + 1 share out the
        other rows of level l in turn (one parent each), so with fewer than twice as many of them every such parent has one
        or two dependants.
    gather = {l: H}: one row of level l has H off-diagonal tuples, naming H distinct rows of level l - 1.
    scatter: the rows are renumbered by a random order that keeps every parent in front of its dependants, so a level's
        rows are scattered over the triangle; without it they are numbered level after level.
    Returns ((rows, cols, vals) sorted by (row, col), n, lev) with lev the level of every row."""
    sizes = [int(s) for s in sizes]
    fan, gather = dict(fan or {}), dict(gather or {})
    start = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    n = int(start[-1])
    lev = np.repeat(np.arange(len(sizes)), sizes)
    per_level = [(np.zeros(0, np.int64), np.zeros(0, np.int64))]
    for l in range(1, len(sizes)):
        r = np.arange(start[l], start[l + 1])
        lo, hi = int(start[l - 1]), int(start[l])
        if l - 1 in fan:
            H = int(fan[l - 1])
            rest = r.size - H
            assert rest >= 0 and (rest == 0 or hi - lo > 1)
            p = np.full(r.size, lo, np.int64)
            if rest:
                p[H:] = lo + 1 + rng.permutation(rest) % (hi - lo - 1)
            per_level.append((r, p))
            continue
        p = rng.integers(lo, hi, r.size)
        q = rng.integers(lo, hi, r.size)
        two = (rng.random(r.size) < 0.5) & (q != p)
        rr, cc = [r, r[two]], [p, q[two]]
        if l in gather:
            H = int(gather[l])
            assert H <= hi - lo
            own = np.concatenate(rr) != r[0]
            rr, cc = [np.concatenate(rr)[own]], [np.concatenate(cc)[own]]
            rr.append(np.full(H, r[0])); cc.append(lo + rng.choice(hi - lo, H, replace=False))
        per_level.append((np.concatenate(rr), np.concatenate(cc)))
    if scatter:
        key = np.empty(n)
        key[:sizes[0]] = rng.random(sizes[0]) * len(sizes)
        for l in range(1, len(sizes)):
            r, c = per_level[l]
            m = np.full(sizes[l], -np.inf)
            np.maximum.at(m, r - start[l], key[c])
            key[start[l]:start[l + 1]] = m + 1e-6 + rng.exponential(1.0, sizes[l])
        new = np.empty(n, np.int64)
        new[np.argsort(key, kind="stable")] = np.arange(n)
    else:
        new = np.arange(n)
    rows = np.concatenate([np.arange(n)] + [x[0] for x in per_level])
    cols = np.concatenate([np.arange(n)] + [x[1] for x in per_level])
    rows, cols = new[rows], new[cols]
    assert np.all(cols <= rows)
    out = np.empty(n, np.int64)
    out[new] = lev
    vals = np.where(rows == cols, 2.0 + rng.random(rows.size), 0.5 * rng.standard_normal(rows.size))
    o = np.lexsort((cols, rows))
    return (rows[o].astype(np.int32), cols[o].astype(np.int32), vals[o]), n, out


def mirrored(A, n, lev=None):
    """The operand under the numbering i -> n - 1 - i: a lower triangle becomes an upper one with the same dependencies,
    every row's tuples in the order they had.  Rows ascending.  Returns (A', lev')."""
    r, c = n - 1 - np.asarray(A[0], np.int64), n - 1 - np.asarray(A[1], np.int64)
    o = np.argsort(r, kind="stable")
    return (r[o].astype(np.int32), c[o].astype(np.int32), np.asarray(A[2])[o]), None if lev is None else lev[::-1].copy()


def pattern_noise(rng, A, n, lev, drop_diag, neg_zero_diag):
    """A by_levels operand made awkward without moving a level: of every row's off-diagonal tuples the one with the
    smallest column stays as it is (so a consolidation that merges duplicates or drops zeros leaves the row a parent of
    the level below); of the others a third is stored two or three times with different values and a fifth becomes an
    explicit 0.0; the upper triangle is populated (half of it NaN: never to be read); row drop_diag loses its diagonal
    and row neg_zero_diag's becomes -0.0.  Rows ascending, a row's tuples in random order: a trusted operand."""
    rows, cols, vals = (np.asarray(x).copy() for x in A)
    off = np.flatnonzero(cols < rows)
    first = off[np.r_[True, rows[off][1:] != rows[off][:-1]]]
    other = np.setdiff1d(off, first)
    u = rng.random(other.size)
    dup, zero = other[u < 1 / 3], other[(u >= 1 / 3) & (u < 1 / 3 + 1 / 5)]
    vals[zero] = 0.0
    dup = np.r_[dup, dup[rng.random(dup.size) < 0.5], zero[: zero.size // 2]]
    ur = rng.integers(0, n - 1, n)
    uc = rng.integers(ur + 1, n)
    uv = np.where(rng.random(n) < 0.5, np.nan, rng.standard_normal(n))
    keep = np.ones(rows.size, bool)
    keep[(rows == drop_diag) & (cols == drop_diag)] = False
    vals[(rows == neg_zero_diag) & (cols == neg_zero_diag)] = -0.0
    rows = np.r_[rows[keep], rows[dup], ur]
    cols = np.r_[cols[keep], cols[dup], uc]
    vals = np.r_[vals[keep], 0.5 * rng.standard_normal(dup.size), uv]
    o = rng.permutation(rows.size)
    o = o[np.argsort(rows[o], kind="stable")]
    return rows[o].astype(np.int32), cols[o].astype(np.int32), vals[o]


def far_rows(rng, n, tail=40):
    """A positive diagonal everywhere and dependencies among rows 0, 1 and the last `tail` rows only: row 1 names row 0;
    the k-th of the last rows names row 0 (k even), row 1 (k a multiple of 3) and every one of the last rows before it.
    Returns (A sorted by (row, col), lev, the rows named): lev is 0 elsewhere, 1 for row 1, 2 + k for the k-th last row."""
    last = n - tail + np.arange(tail)
    rr, cc = [np.arange(n), [1]], [np.arange(n), [0]]
    for k in range(tail):
        c = np.r_[[0] if k % 2 == 0 else [], [1] if k % 3 == 0 else [], last[:k]].astype(np.int64)
        rr.append(np.full(c.size, last[k])); cc.append(c)
    rows, cols = np.concatenate(rr).astype(np.int64), np.concatenate(cc).astype(np.int64)
    vals = np.where(rows == cols, 1.0 + rng.random(rows.size), 0.3 * rng.standard_normal(rows.size))
    o = np.lexsort((cols, rows))
    lev = np.zeros(n, np.int64)
    lev[1] = 1
    lev[last] = 2 + np.arange(tail)
    return (rows[o].astype(np.int32), cols[o].astype(np.int32), vals[o]), lev, np.r_[0, 1, last]
