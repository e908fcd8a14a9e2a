"""spsamd_solve_tri on the device against tests/solve_ref.py (pinned on the host by tests/test_solve_host.py): every value of
X as an int64 bit pattern, zero tolerance -- each is defined by one serial chain, so there is nothing to tolerate -- and the
schedule's figures (levels, max_level_rows, tuples_used, zero_pivot) equal.  The solve_path, solve_row and solve_fuse_rows
knobs run so that every row meets every row kernel and every level both ways of running it."""
import ctypes as C

import numpy as np
import pytest

from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests import select_ref as sel
from tests import solve_ref as sr
from tests.gpu_util import SENT, bits_same as _bits_same, coo as _coo, ctx, forced, rhs as _rhs, solve as _solve  # noqa: F401

pytestmark = pytest.mark.gpu

NRHS = (1, 2, 3, 15, 16, 17, 64, 65)


def test_semantic_fuzz(ctx):
    """200 small operands: raw unique, raw duplicate-key and trusted (sorted by the leading index only, duplicates and special
    values anywhere), both triangles, both diagonals, both transposes, the three policies, zero_nan, the eight nrhs, in and
    out of place, host and device memory.  The kind of operand is the trial's base-3 digit and (solve_path, solve_row) its
    base-12 digit above that, so every kind meets every setting; the rest is drawn."""
    rng = np.random.default_rng(2020)
    seen = set()
    for trial in range(200):
        n = int(rng.integers(1, 41))
        nnz = int(rng.integers(0, 6 * n))
        t = '.' if rng.integers(2) == 0 else 'T'
        lead = 1 if t == 'T' else 0
        kind, combo = trial % 3, (trial // 3) % 12
        path, row = combo % 3, combo // 3
        uplo, diag = int(rng.integers(2)), int(rng.integers(2))
        pol, zn = int(rng.integers(3)), bool(rng.integers(5) == 0)
        nrhs = NRHS[int(rng.integers(len(NRHS)))]
        device, in_place, dev_a = bool(rng.integers(2)), bool(rng.integers(2)), bool(rng.integers(2))
        sort0 = -1
        shape = (n, n)
        if kind == 0:
            A = sel.unique_key_operand(rng, shape, nnz)
        elif kind == 1:
            A = sel.duplicate_key_operand(rng, shape, nnz)
        else:
            i0 = rng.integers(0, n, nnz).astype(np.int32)
            i1 = rng.integers(0, n, nnz).astype(np.int32)
            v = sel.special_values(rng, nnz, 0.3)
            o = np.argsort(i1 if lead else i0, kind="stable")
            A, sort0 = (i0[o], i1[o], v[o]), lead
        S = sel.operand_S(A, t, pol, zn, sort0)
        B = _rhs(rng, n, nrhs)
        keep = []
        a = _coo(A, shape, sort0, device=dev_a, keep=keep)
        what = "trial %d n %d kind %d %s uplo %d diag %d pol %d zn %d nrhs %d path %d row %d dev %d inplace %d" % (
            trial, n, kind, t, uplo, diag, pol, zn, nrhs, path, row, device, in_place)
        with forced(ctx, "solve_path", path), forced(ctx, "solve_row", row):
            X, st = _solve(ctx, a, B, uplo, diag, t, pol, zn, device, in_place, pad=1 + trial % 3)
        _bits_same(X, sr.solve_ref(S, n, B, uplo, diag), what)
        assert (st.levels, st.max_level_rows) == sr.schedule_stats(S, n, uplo, diag), what
        assert st.tuples_used == sr.tuples_used(S, uplo, diag), what
        assert st.zero_pivot == sr.zero_pivot(S, n, uplo, diag), what
        assert st.analysis_reused == 0
        seen.add((uplo, diag, t)); seen.add(("mem", device, in_place)); seen.add(("nrhs", nrhs)); seen.add(("pol", pol, zn))
    assert len([s for s in seen if len(s) == 3 and s[0] in (0, 1)]) == 8
    assert len([s for s in seen if s[0] == "mem"]) == 4 and len([s for s in seen if s[0] == "nrhs"]) == len(NRHS)
    assert len([s for s in seen if s[0] == "pol"]) == 6


def _by_levels(rng, sizes):
    """Lower-triangular operand whose level l has sizes[l] rows (numbered level after level): each row of level l > 0 has
    one or two off-diagonal tuples in level l - 1, and a diagonal."""
    start = np.r_[0, np.cumsum(sizes)]
    rows, cols = [np.arange(start[-1])], [np.arange(start[-1])]
    for l in range(1, len(sizes)):
        r = np.arange(start[l], start[l + 1])
        p = rng.integers(start[l - 1], start[l], r.size)
        rows.append(r); cols.append(p)
        two = rng.random(r.size) < 0.5
        q = rng.integers(start[l - 1], start[l], r.size)
        two &= q != p
        rows.append(r[two]); cols.append(q[two])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.where(rows == cols, 2.0 + rng.random(rows.size), 0.5 * rng.standard_normal(rows.size))
    o = np.lexsort((cols, rows))
    return (rows[o].astype(np.int32), cols[o].astype(np.int32), vals[o]), int(start[-1])


def test_level_widths_at_the_edges(ctx):
    """Levels of 1 .. 5000 rows around the wave, workgroup and fuse widths; under the default, solve_fuse_rows 256 and 1024 the
    fused runs begin and end at those widths, under solve_path 1 / 2 none / all of the levels are fused."""
    from spsparse_amd import capi
    rng = np.random.default_rng(7)
    sizes = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000, 1, 1, 1, 5000, 2]
    A, n = _by_levels(rng, sizes)
    B = _rhs(rng, n, 3, 0.0)
    want = sr.solve_fast(A, n, B)
    keep = []
    a = _coo(A, (n, n), -1, device=True, keep=keep)
    for knob, value in (("solve_fuse_rows", 0), ("solve_fuse_rows", 256), ("solve_fuse_rows", 1024), ("solve_path", 1), ("solve_path", 2)):
        with forced(ctx, knob, value):
            X, st = _solve(ctx, a, B, device=True)
        what = "%s %d" % (knob, value)
        _bits_same(X, want, what)
        assert (st.levels, st.max_level_rows) == (16, 5000), what
        fuse = {("solve_fuse_rows", 0): min(capi.solve_fuse_rows, capi.solve_fuse_work // 3), ("solve_fuse_rows", 256): 256,
                ("solve_fuse_rows", 1024): 1024, ("solve_path", 1): 0, ("solve_path", 2): 10 ** 9}[(knob, value)]
        thin = [s <= fuse for s in sizes]                              # (every row is short: three tuples at most)
        runs = sum(1 for l, x in enumerate(thin) if x and (l == 0 or not thin[l - 1]))
        assert st.fused_levels == sum(thin), what
        assert st.launches == runs + len(sizes) - sum(thin), what


def test_levels_not_monotone_in_the_row(ctx):
    """Row i depends on row i - 2: two interleaved chains, so a level's rows are not consecutive.  And random sparse lower
    operands with up to 3 tuples per row, where a level's rows are scattered."""
    rng = np.random.default_rng(8)
    n = 3001
    i = np.arange(n)
    A = (np.r_[i, i[2:]].astype(np.int32), np.r_[i, i[2:] - 2].astype(np.int32), np.r_[1.5 + rng.random(n), rng.standard_normal(n - 2)])
    B = _rhs(rng, n, 2, 0.0)
    keep = []
    X, st = _solve(ctx, _coo(A, (n, n), -1, keep=keep), B)
    S = sel.operand_S(A)
    _bits_same(X, sr.solve_fast(S, n, B), "i - 2")
    assert (st.levels, st.max_level_rows) == (1501, 2)
    n = 3000
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        r = np.repeat(np.arange(n), 3)
        c = (rng.random(3 * n) * (r + 1)).astype(np.int64)             # columns 0 .. i: lower, diagonal included at times
        R = (r.astype(np.int32), c.astype(np.int32), 0.7 * rng.standard_normal(3 * n) + 1.0)
        S = sel.operand_S(R)
        B = _rhs(rng, n, 3, 0.0)
        for uplo, t in ((0, '.'), (1, 'T')):
            St = sel.operand_S(R, t)
            X, st = _solve(ctx, _coo(R, (n, n), -1, keep=keep), B, uplo=uplo, t=t, device=True)
            _bits_same(X, sr.solve_fast(St, n, B, uplo), "random lower seed %d %s" % (seed, t))
            assert (st.levels, st.max_level_rows) == sr.schedule_stats(St, n, uplo), (seed, t)
            assert st.zero_pivot == sr.zero_pivot(St, n, uplo)


def test_chain_is_one_launch(ctx):
    """A bidiagonal matrix is n levels of one row: the default path serves it in a fused run (a handful of launches, not
    n), solve_path 1 in a launch per level, and the bits are the same."""
    n = 20000
    rng = np.random.default_rng(9)
    i = np.arange(n)
    A = (np.r_[i, i[1:]].astype(np.int32), np.r_[i, i[1:] - 1].astype(np.int32), np.r_[1.0 + rng.random(n), 0.9 * rng.random(n - 1)])
    S = sel.operand_S(A)
    B = _rhs(rng, n, 3, 0.0)
    want = sr.solve_fast(S, n, B, lev=np.arange(n))
    keep = []
    a = _coo(A, (n, n), -1, device=True, keep=keep)
    for nrhs in (1, 3):
        X, st = _solve(ctx, a, B[:, :nrhs], device=True)
        _bits_same(X, want[:, :nrhs], "chain nrhs %d" % nrhs)
        assert st.levels == n and st.max_level_rows == 1
        assert st.launches < st.levels / 1000 and st.fused_levels >= st.levels - 1
        with forced(ctx, "solve_path", 1):
            X, st = _solve(ctx, a, B[:, :nrhs], device=True)
        _bits_same(X, want[:, :nrhs], "chain, a launch per level, nrhs %d" % nrhs)
        assert st.launches >= st.levels and st.fused_levels == 0


def test_row_lengths(ctx):
    """Rows with 0, 1, 63, 64, 65, 128, 129, 4096 and 4097 used off-diagonal tuples (and the other triangle present, to be
    skipped) among short random rows, nrhs 1, 16 and 17 under every solve_row: the serial, lanes and fold kernels at the
    edges of spmm_long_min and of the fold's 64-tuple steps."""
    rng = np.random.default_rng(10)
    n = 4200
    special = {0: 0, 1: 1, 100: 63, 101: 64, 102: 65, 200: 128, 201: 129, 4150: 4096, 4199: 4097}
    rows, cols = [], []
    for i in range(n):
        k = special.get(i, min(i, int(rng.integers(0, 4))))
        c = rng.choice(i, k, replace=False) if k else np.zeros(0, np.int64)
        up = rng.integers(i + 1, n, 2) if i + 1 < n else np.zeros(0, np.int64)      # the other triangle: never read
        c = np.r_[c, i, up]
        rows.append(np.full(c.size, i)); cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = np.where(rows == cols, 3.0 + rng.random(rows.size), 0.02 * rng.standard_normal(rows.size))
    o = rng.permutation(rows.size)
    o = o[np.argsort(rows[o], kind="stable")]                          # trusted: row order, columns in any order inside a row
    A = (rows[o].astype(np.int32), cols[o].astype(np.int32), vals[o])
    used = np.bincount(A[0][A[1] < A[0]], minlength=n)
    assert all(used[i] == k for i, k in special.items())
    B = _rhs(rng, n, 17, 0.0)
    want = sr.solve_fast(A, n, B)
    keep = []
    a = _coo(A, (n, n), 0, device=True, keep=keep)
    for row in (0, 1, 2, 3):
        for nrhs in (1, 16, 17):
            with forced(ctx, "solve_row", row):
                X, st = _solve(ctx, a, B[:, :nrhs], device=True)
            _bits_same(X, want[:, :nrhs], "solve_row %d nrhs %d" % (row, nrhs))
            assert st.tuples_used == int(np.count_nonzero(A[1] <= A[0]))


def test_poisson(ctx):
    """tril of the 5-point Poisson matrix on 64 x 64 points: taken from the whole matrix by the fill-mode rule, and as a
    chained spsamd_select(TRIL) result read in place; that result under 'T' is the upper triangle.  2 * 64 - 1 levels, the
    level of a point its x + y."""
    import torch
    from spsparse_amd import capi
    N = 64
    n = N * N
    P = wl.poisson2d(N)[:3]
    m = len(P[2])
    dev = torch.device("cuda:0")
    t = (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
         torch.empty(m, dtype=torch.float64, device=dev))
    ctx.gen_poisson2d(N, *[x.data_ptr() for x in t])
    torch.cuda.synchronize()
    a = capi.device_coo(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), m, (n, n), 0)
    rng = np.random.default_rng(11)
    B = _rhs(rng, n, 3, 0.0)
    want = sr.solve_fast(P, n, B)
    lev = sr.levels(P, n)
    assert np.array_equal(lev, np.arange(n) // N + np.arange(n) % N)
    X, st = _solve(ctx, a, B, device=True)
    _bits_same(X, want, "whole matrix, LOWER")
    assert (st.levels, st.max_level_rows) == (2 * N - 1, N)
    res = ctx.select(a, capi.SELECT_TRIL)
    L = capi.result_operand(res)
    X, st = _solve(ctx, L, B, device=True)
    _bits_same(X, want, "select(TRIL) chained")
    assert st.levels == 2 * N - 1 and st.tuples_used == int(res.nnz)
    keep = np.flatnonzero(P[1] <= P[0])
    Lh = tuple(x[keep] for x in P)
    St = sel.operand_S(Lh, 'T')
    X, st = _solve(ctx, L, B, uplo=1, t='T', device=True)
    _bits_same(X, sr.solve_fast(St, n, B, sr.UPPER), "select(TRIL) under 'T', UPPER")
    assert st.levels == 2 * N - 1
    assert ctx.fetch(res)[2].size == keep.size                          # neither output set was written: still fetchable


def test_prepared_keeps_the_schedule(ctx):
    """Handles for '.' and 'T', each solved under both transposes: with its own transpose the second solve of an
    (uplo, diag) reuses the schedule (analysis_reused, equal bits, spsamd_operand_bytes grown once), another (uplo, diag) is
    analysed again; with the other transpose the handle is an ordinary device operand, analysed per call."""
    from spsparse_amd import capi
    rng = np.random.default_rng(12)
    n = 500
    r = np.repeat(np.arange(n), 4)
    c = rng.integers(0, n, 4 * n)
    R = (np.r_[r, np.arange(n)].astype(np.int32), np.r_[c, np.arange(n)].astype(np.int32), np.r_[0.1 * rng.standard_normal(4 * n), 2.0 + rng.random(n)])
    B = _rhs(rng, n, 5, 0.0)
    keep = []
    for tprep in ('.', 'T'):
        h = capi.Operand(ctx, _coo(R, (n, n), -1, False, keep), tprep, capi.AS_A, capi.ADD, False)
        try:
            for t in ('.', 'T'):
                S = sel.operand_S(R, t)
                own = t == tprep
                bytes0 = h.bytes
                for uplo, diag in ((0, 0), (1, 0), (0, 1)):
                    want = sr.solve_fast(S, n, B, uplo, diag)
                    before = h.bytes
                    X, st = _solve(ctx, h.coo, B, uplo, diag, t, device=True)
                    what = "prepared %s used %s uplo %d diag %d" % (tprep, t, uplo, diag)
                    _bits_same(X, want, what)
                    assert st.analysis_reused == 0, what
                    grown = h.bytes
                    assert (grown > before) if own else (grown == before), what
                    X, st2 = _solve(ctx, h.coo, B, uplo, diag, t, device=False, in_place=True)
                    _bits_same(X, want, what + " again")
                    assert st2.analysis_reused == (1 if own else 0), what
                    assert h.bytes == grown, what
                    assert (st2.levels, st2.max_level_rows, st2.tuples_used, st2.zero_pivot) == \
                        (st.levels, st.max_level_rows, st.tuples_used, st.zero_pivot) == \
                        sr.schedule_stats(S, n, uplo, diag) + (sr.tuples_used(S, uplo, diag), sr.zero_pivot(S, n, uplo, diag)), what
                assert (h.bytes > bytes0) == own
        finally:
            h.close()


def test_zero_pivots(ctx):
    """A missing diagonal at row 3 and a zero diagonal at row 7: zero_pivot 3, the Inf / NaN outputs bit for bit.  A
    diagonal of one explicit -0.0 (trusted) folds to +0.0 + -0.0 = +0.0; duplicate diagonal tuples -0.0, -0.0 (trusted) fold to
    +0.0 as well: zero pivots both.  Under UNIT the same operands report none."""
    n = 10
    rng = np.random.default_rng(13)
    i = np.arange(n)
    keep = []
    d = 1.0 + rng.random(n)
    d[7] = 0.0
    rows, cols, vals = np.r_[i, i[1:]], np.r_[i, i[1:] - 1], np.r_[d, rng.standard_normal(n - 1)]
    m = ~((rows == 3) & (cols == 3))
    o = np.lexsort((cols[m], rows[m]))
    A = (rows[m][o].astype(np.int32), cols[m][o].astype(np.int32), vals[m][o])
    B = _rhs(rng, n, 2, 0.0)
    B[3, 1] = 0.0
    for sort0 in (0,):                                                 # (raw, the zero at (7, 7) would be dropped: trusted keeps it)
        X, st = _solve(ctx, _coo(A, (n, n), sort0, keep=keep), B)
        _bits_same(X, sr.solve_ref(A, n, B), "missing and zero diagonal")
        assert st.zero_pivot == 3 and not np.all(np.isfinite(X))
        X, st = _solve(ctx, _coo(A, (n, n), sort0, keep=keep), B, diag=1)
        _bits_same(X, sr.solve_ref(A, n, B, diag=1), "the same, UNIT")
        assert st.zero_pivot == -1 and np.all(np.isfinite(X))
    for dv in ((-0.0,), (-0.0, -0.0)):
        rows = np.r_[0, 1, np.full(len(dv), 2), 3]
        cols = np.r_[0, 1, np.full(len(dv), 2), 3]
        A = (rows.astype(np.int32), cols.astype(np.int32), np.r_[1.0, 2.0, dv, 4.0])
        B = np.array([[1.0], [1.0], [-3.0], [1.0]])
        X, st = _solve(ctx, _coo(A, (4, 4), 0, keep=keep), B)
        _bits_same(X, sr.solve_ref(A, 4, B), "diagonal %r" % (dv,))
        assert st.zero_pivot == 2 and X[2, 0] == -np.inf               # -3 / +0.0
        X, st = _solve(ctx, _coo(A, (4, 4), 0, keep=keep), B, diag=1)
        assert st.zero_pivot == -1 and X[2, 0] == -3.0


def test_errors_leave_x_untouched(ctx):
    from spsparse_amd import capi
    keep = []
    A = (np.array([0, 1, 2], np.int32), np.array([0, 0, 2], np.int32), np.array([1.0, 2.0, 3.0]))
    a = _coo(A, (3, 3), -1, keep=keep)
    B = np.ones((3, 2))
    X = np.full((3, 2), SENT)
    L = ctx.L

    def call(a=a, uplo=0, diag=0, pb=B.ctypes.data, ldb=2, px=X.ctypes.data, ldx=2, nrhs=2, mem=capi.MEM_HOST, pol=capi.ADD, pa=None):
        rc = L.spsamd_solve_tri(ctx.h, C.byref(a) if pa is None else pa, b'.', uplo, diag, pb, ldb, px, ldx, nrhs, mem, pol, 0, None, None)
        assert np.all(X == SENT), "X was written"
        return rc

    assert call(pa=C.POINTER(capi.Coo)()) == -2                        # A NULL
    assert call(pb=None) == -2 and call(px=None) == -2
    assert call(uplo=2) == -2 and call(uplo=-1) == -2 and call(diag=2) == -2
    assert call(ldb=1) == -2 and call(ldx=1) == -2
    assert call(mem=2) == -2 and call(mem=7) == -2 and call(pol=3) == -2
    assert call(a=_coo((A[0], np.array([0, 3, 2], np.int32), A[2]), (3, 3), -1, keep=keep)) == -2          # index out of bounds
    assert call(a=_coo((np.array([2, 1, 0], np.int32), A[1], A[2]), (3, 3), 0, keep=keep)) == -2           # a false sort0
    assert call(a=_coo(A, (3, 4), -1, keep=keep)) == -1                                                   # not square
    assert b"square" in L.spsamd_last_error(ctx.h)
    big = _coo(A, (3, 3), -1, keep=keep)
    big.nnz = 1 << 31
    assert call(a=big) == -2
    assert call(px=B.ctypes.data + 8) == -2                            # X overlaps B, not in place
    assert call(px=B.ctypes.data, ldb=3) == -2                         # X == B, but ldx != ldb
    assert call(px=keep[0][2].ctypes.data) == -2                       # X overlaps A's values
    assert call(nrhs=0) == 0 and call(nrhs=0, pb=None, px=None) == 0
    assert call(a=_coo((A[0][:0], A[1][:0], A[2][:0]), (0, 0), -1, keep=keep)) == 0
    st = capi.SolveStats()
    res = capi.Result()
    rc = L.spsamd_solve_tri(ctx.h, C.byref(a), b'.', 0, 0, B.ctypes.data, 2, X.ctypes.data, 2, 2, capi.MEM_HOST, capi.ADD, 0,
                            C.byref(st), C.byref(res))
    assert rc == 0 and (res.shape0, res.shape1, res.nnz_a) == (3, 3, 3) and st.levels == 2 and st.tuples_used == 3
    _bits_same(X, sr.solve_ref(sel.operand_S(A), 3, B), "after the errors")


def test_device_x_in_an_output_set_is_refused(ctx):
    from spsparse_amd import capi
    keep = []
    n = 4
    A = (np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.0))
    res = ctx.consolidate(_coo(A, (n, n), -1, keep=keep), 0)
    import torch
    B = torch.ones(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.L.spsamd_solve_tri(ctx.h, C.byref(capi.result_operand(res)), b'.', 0, 0, B.data_ptr(), 1, res.val, 1, 1,
                                capi.MEM_DEVICE, capi.ADD, 0, None, None)
    assert rc == -2
    assert np.array_equal(ctx.fetch(res)[2], np.full(n, 2.0))
    X = ctx.solve_tri(capi.result_operand(res), B)                      # the result itself as A: read in place
    assert np.array_equal(X.cpu().numpy(), np.full(n, 0.5))
