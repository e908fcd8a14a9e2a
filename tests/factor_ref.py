"""Host restatement of spsamd_factor_ilu0 (include/spsparse_amd.h): the yardstick of the device kernels.

S = (rows, cols, vals) is op(A) as the call takes it (tests/select_ref.operand_S), strictly ascending in (row, col).  F has
S's keys and the values of

    f_t = value of tuple t of S
    for i = 0 .. n-1:
      for each tuple t = (i, k) of row i with k < i, in ascending k:
          f_t = f_t / p_k               p_k: f of row k's diagonal tuple; +0.0 if row k stores none
          for each tuple s = (k, j) of row k with j > k:
              if row i stores a tuple u = (i, j):   f_u = f_u - f_t * f_s

every operation rounded on its own and a NaN result with the bits x86-64 gives it (dense_ref.mul, solve_ref.sub / div: the
left operand's NaN quieted, else the right one's, else 0xFFF8000000000000).

ilu0_ref    the loop as written, tuple by tuple (small cases)
ilu0_fast   the same by levels: the rows of a level vectorised, one lower-tuple rank at a time and inside it one rank of
            the named rows' upper parts at a time (every f_u still sees its updates in ascending k)
row_work    w_i, the lookups of row i; classes() the kernel class of every row under given thresholds
plan        (launches, fused_levels) of the numeric phase for a schedule: the host loop of k_factor.hip restated
and the input makers.  Both return (f, stats) with stats = dict(updates, lookups, zero_pivot, missing_diag).
"""
import numpy as np

from tests import dense_ref as dr
from tests import solve_ref as sr


def _spans(rows, n):
    return np.searchsorted(np.asarray(rows, np.int64), np.arange(n + 1), side="left")


def strictly_ascending(S):
    key = np.asarray(S[0], np.int64) << 32 | np.asarray(S[1], np.int64)
    return bool(np.all(key[1:] > key[:-1]))


def first_violation(S):
    """The first position whose key does not exceed the key in front of it, or -1."""
    key = np.asarray(S[0], np.int64) << 32 | np.asarray(S[1], np.int64)
    bad = np.flatnonzero(key[1:] <= key[:-1])
    return int(bad[0]) + 1 if bad.size else -1


def structure(S, n):
    """(beg, dpos, ustart): row spans, the diagonal's position (-1: none) and the first tuple right of it, per row."""
    rows, cols = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64)
    beg = _spans(rows, n)
    key = rows << 32 | cols
    i = np.arange(n, dtype=np.int64)
    p = np.searchsorted(key, i << 32 | i, side="left")
    has = (p < beg[1:]) & (key[np.minimum(p, max(len(key) - 1, 0))] == (i << 32 | i)) if len(key) else np.zeros(n, bool)
    dpos = np.where(has, p, -1)
    ustart = np.where(has, p + 1, p)
    return beg, dpos, ustart


def row_work(S, n):
    """w_i = sum over the lower tuples (i, k) of the tuples of row k right of its diagonal."""
    rows, cols = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64)
    beg, _d, ustart = structure(S, n)
    up = beg[1:] - ustart
    low = cols < rows
    w = np.zeros(n, np.int64)
    np.add.at(w, rows[low], up[cols[low]])
    return w


def _pivot_stats(S, n, f, dpos):
    miss = np.flatnonzero(dpos < 0)
    piv = np.where(dpos >= 0, f[np.maximum(dpos, 0)] if len(f) else 0.0, 0.0)
    z = np.flatnonzero(piv == 0)
    return (int(z[0]) if z.size else -1), (int(miss[0]) if miss.size else -1)


def ilu0_ref(S, n):
    """The loop as written."""
    assert strictly_ascending(S)
    rows, cols = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64)
    f = np.array(S[2], np.float64)
    beg, dpos, ustart = structure(S, n)
    updates = lookups = 0
    for i in range(n):
        b, e = int(beg[i]), int(beg[i + 1])
        where = {int(cols[u]): u for u in range(b, e)}
        for t in range(b, e):
            k = int(cols[t])
            if k >= i:
                break
            p = f[dpos[k]] if dpos[k] >= 0 else np.float64(0.0)
            f[t] = sr.div(f[t], p)
            for s in range(int(ustart[k]), int(beg[k + 1])):
                lookups += 1
                u = where.get(int(cols[s]))
                if u is not None:
                    f[u] = sr.sub(f[u], dr.mul(f[t], f[s]))
                    updates += 1
    zp, md = _pivot_stats(S, n, f, dpos)
    return f, dict(updates=updates, lookups=lookups, zero_pivot=zp, missing_diag=md)


_CHUNK = 1 << 22          # (t, s) pairs ilu0_fast looks up at a time


def ilu0_fast(S, n, lev=None):
    """The same by levels (for large cases).  lev: the level vector of S's LOWER triangle, where the caller knows it."""
    assert strictly_ascending(S)
    rows, cols = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64)
    f = np.array(S[2], np.float64)
    m = len(f)
    beg, dpos, ustart = structure(S, n)
    up = beg[1:] - ustart
    zero = np.float64(0.0)
    if lev is None:
        lev = sr.levels(S, n, sr.LOWER, sr.NONUNIT)
    key = rows << 32 | cols
    low = np.flatnonzero(cols < rows)                               # the lower tuples, S's order: ascending k inside a row
    rank = low - beg[rows[low]]                                     # (the lower tuples lead their row)
    tlev = lev[rows[low]]
    order = np.lexsort((rank, tlev))
    nlev = int(lev.max()) + 1 if n else 0
    tb = np.searchsorted(tlev[order], np.arange(nlev + 1), side="left")
    updates = 0
    lookups = int(up[cols[low]].sum())
    for L in range(1, nlev):
        sel = order[tb[L]:tb[L + 1]]
        if not sel.size:
            continue
        rk = rank[sel]
        bounds = np.searchsorted(rk, np.arange(rk[-1] + 2), side="left")
        for r in range(len(bounds) - 1):
            t = low[sel[bounds[r]:bounds[r + 1]]]                   # the r-th lower tuple of every row that has one: distinct rows
            k = cols[t]
            p = np.where(dpos[k] >= 0, f[np.maximum(dpos[k], 0)], zero)
            f[t] = sr.div(f[t], p)
            width = up[k]
            tot = int(width.sum())
            if not tot:
                continue
            # every (t, s) pair of this rank, a few million at a time: distinct rows i, and inside one k distinct j, so no u
            # occurs twice
            ends = np.cumsum(width)
            cuts = [0]
            while cuts[-1] < t.size:
                cuts.append(max(cuts[-1] + 1, int(np.searchsorted(ends, ends[cuts[-1]] - width[cuts[-1]] + _CHUNK, side="right"))))
            for c0, c1 in zip(cuts[:-1], cuts[1:]):
                wd = width[c0:c1]
                tot = int(wd.sum())
                tt = np.repeat(t[c0:c1], wd)
                s = np.repeat(ustart[k[c0:c1]] - (np.cumsum(wd) - wd), wd) + np.arange(tot)
                want = rows[tt] << 32 | cols[s]
                u = np.searchsorted(key, want, side="left")
                hit = (u < m) & (key[np.minimum(u, m - 1)] == want)
                if hit.any():
                    uu, th, sh = u[hit], tt[hit], s[hit]
                    f[uu] = sr.sub(f[uu], dr.mul(f[th], f[sh]))
                    updates += int(hit.sum())
    zp, md = _pivot_stats(S, n, f, dpos)
    return f, dict(updates=updates, lookups=lookups, zero_pivot=zp, missing_diag=md)


def classes(S, n, serial_work, lds_row, factor_row=0):
    """Per row: 0 no lower tuple | 1 serial | 2 wave | 3 block -- fac_class of k_factor.hip."""
    rows, cols = np.asarray(S[0], np.int64), np.asarray(S[1], np.int64)
    length = np.bincount(rows, minlength=n)
    nlow = np.bincount(rows[cols < rows], minlength=n)
    w = row_work(S, n)
    long_cl = np.where(length <= lds_row, 2, 3)
    if factor_row == 1:
        cl = np.ones(n, np.int64)
    elif factor_row == 3:
        cl = np.full(n, 3)
    elif factor_row == 2:
        cl = long_cl
    else:
        cl = np.where(w <= serial_work, 1, long_cl)
    return np.where(nlow == 0, 0, cl)


def plan(sizes, level_work, level_len, fuse_rows, serial_work, lds_row, factor_path=0, factor_row=0):
    """(launches, fused_levels) for a schedule whose level l has sizes[l] rows, the largest row work level_work[l] and the
    longest row level_len[l]: level 0 is never launched; a level whose rows are all serial-class is thin when factor_path is
    2 or (factor_path 0 and) it has at most fuse_rows rows, and a maximal run of thin levels is one launch; any other level
    is a serial launch (unless a wave or block kernel is forced), a wave launch where a row has more work (unless block is
    forced), and a block launch where a row is longer than lds_row (or block is forced)."""
    launches = fused = 0
    prev_thin = False
    for l in range(1, len(sizes)):
        all_serial = factor_row == 1 or (factor_row == 0 and level_work[l] <= serial_work)
        thin = factor_path != 1 and all_serial and (factor_path == 2 or sizes[l] <= fuse_rows)
        if thin:
            fused += 1
            launches += 0 if prev_thin else 1
        else:
            launches += 1 if factor_row <= 1 else 0
            if not all_serial:
                launches += 1 if factor_row != 3 else 0
                launches += 1 if factor_row == 3 or level_len[l] > lds_row else 0
        prev_thin = thin
    return launches, fused


# ---------------------------------------------------------------- inputs

def fuzz_operand(rng, n, kind, transpose):
    """A small n x n operand as stored, and its sort0.  kind 0: raw, every key once, shuffled; 1: raw with duplicate keys
    (finite values on them: a folded NaN's bits are the consolidation's business), shuffled; 2: trusted, strictly ascending
    in op()'s (row, col), sort0 naming op()'s rows.  Four rows in five store a diagonal; a tenth of the values (a third under
    kind 2) are special: NaN, +-Inf, +-0.0 (under kind 2 explicit zeros stay as pattern)."""
    from tests import select_ref as sel
    nnz = int(rng.integers(0, 6 * n))
    flat = rng.choice(n * n, min(nnz, n * n), replace=False)
    d = np.flatnonzero(rng.random(n) < 0.8)
    flat = np.union1d(flat, d * n + d)
    r, c = flat // n, flat % n                                      # op()'s (row, col), ascending
    v = sel.special_values(rng, flat.size, 0.3 if kind == 2 else 0.1)
    plain = (r == c) & (rng.random(flat.size) < 0.9)
    v[plain] = rng.choice((-1.0, 1.0), int(plain.sum())) * (1.0 + rng.random(int(plain.sum())))
    if kind == 1 and flat.size:
        dup = rng.integers(0, flat.size, max(1, flat.size // 3))
        v[dup] = rng.standard_normal(dup.size)
        r, c, v = np.r_[r, r[dup]], np.r_[c, c[dup]], np.r_[v, rng.standard_normal(dup.size)]
    if kind != 2:
        o = rng.permutation(r.size)
        r, c, v = r[o], c[o], v[o]
    i0, i1 = (c, r) if transpose == 'T' else (r, c)
    sort0 = (1 if transpose == 'T' else 0) if kind == 2 else -1
    return (i0.astype(np.int32), i1.astype(np.int32), v), sort0


def sorted_unique(rows, cols, vals):
    """Tuples by (row, col), the first of every key kept."""
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float64)
    o = np.lexsort((cols, rows))
    rows, cols, vals = rows[o], cols[o], vals[o]
    keep = np.r_[True, (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])] if len(rows) else np.zeros(0, bool)
    return rows[keep].astype(np.int32), cols[keep].astype(np.int32), vals[keep]


def symmetrised(A, n, rng, diag=None):
    """L u L^T of a lower-triangular operand (strict lower part mirrored, new values drawn); diag: the value of every
    diagonal entry (None: A's own)."""
    r, c, v = (np.asarray(x) for x in A)
    off = c < r
    rr = np.r_[r, c[off]]
    cc = np.r_[c, r[off]]
    vv = np.r_[v, 0.5 * rng.standard_normal(int(off.sum()))]
    if diag is not None:
        vv = np.where(rr == cc, diag, vv)
    return sorted_unique(rr, cc, vv)


def product_lu(rng, n, pattern):
    """A = L0 * U0 on `pattern` (a boolean n x n array that LU without pivoting does not fill): L0 unit lower with entries
    in -3 .. 3, U0 with integer off-diagonals and +-2^e diagonals.  Returns (S of A on the pattern, tril(L0, -1) + U0 on
    the pattern): every operation of the factorisation is exact."""
    L0 = np.tril(rng.integers(-3, 4, (n, n)).astype(np.float64), -1) * np.tril(pattern, -1) + np.eye(n)
    U0 = np.triu(rng.integers(-3, 4, (n, n)).astype(np.float64), 1) * np.triu(pattern, 1)
    U0 += np.diag(rng.choice((-1.0, 1.0), n) * 2.0 ** rng.integers(-2, 3, n))
    A = L0 @ U0
    assert not np.any(A[~pattern]), "the pattern fills"
    r, c = np.nonzero(pattern)
    want = np.tril(L0, -1) + U0
    return (r.astype(np.int32), c.astype(np.int32), A[r, c]), want[r, c]


def band(n, lo, hi):
    i, j = np.indices((n, n))
    return (i - j <= lo) & (j - i <= hi)


def arrow(n):
    """Down-right arrow: the diagonal, the last row and the last column."""
    i, j = np.indices((n, n))
    return (i == j) | (i == n - 1) | (j == n - 1)


def rmat_sym(scale, edge_factor, seed, diag):
    """The symmetrised R-MAT pattern plus a diagonal: values U(0, 1] off the diagonal (the first drawn of a key), `diag` on it."""
    from spsparse_amd import workloads as wl
    r, c, v, _shape = wl.rmat(scale, seed, edge_factor)
    n = 1 << scale
    i = np.arange(n)
    off = r != c
    return sorted_unique(np.r_[i, r[off], c[off]], np.r_[i, c[off], r[off]], np.r_[np.full(n, float(diag)), v[off], v[off]]), n
