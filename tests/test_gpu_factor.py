"""spsamd_factor_ilu0 on the device against tests/factor_ref.py (pinned on the host by tests/test_factor_host.py): the keys
equal to S's, every value as an int64 bit pattern with zero tolerance -- each is defined by one serial chain, so there is
nothing to tolerate -- and the counters that are functions of S alone (levels, lookups, updates, zero_pivot, missing_diag)
equal.  The factor_path, factor_row and threshold knobs run so that every row meets every row kernel and every level both
ways of running it."""
import ctypes as C

import numpy as np
import pytest

from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests import factor_ref as fr
from tests import select_ref as sel
from tests import solve_ref as sr
from tests.gpu_util import Knobs, bits_same as _bits_same, check_tuples as _check, coo as _coo, ctx, rhs as _rhs, solve as _solve  # noqa: F401

pytestmark = pytest.mark.gpu


def _counters(st, rs, S, n, what):
    assert (st.lookups, st.updates, st.zero_pivot, st.missing_diag) == \
        (rs["lookups"], rs["updates"], rs["zero_pivot"], rs["missing_diag"]), "%s: counters %r, want %r" % (
            what, (st.lookups, st.updates, st.zero_pivot, st.missing_diag), rs)


def _digest_same(res, tuples, what):
    """gpu_util.check_digest's checks on a digest result against the tuples of the COO result: count and index hash exact;
    the value sum to the rounding of a sum of that many terms in any order (F's values are not exactly summable, unlike the
    integer-valued inputs check_digest was written for), and equal in kind where it is not finite."""
    from oracle import binding as orc
    i, j, v = tuples
    cnt, vsum, h = orc.digest(i, j, v)
    assert (res.nnz, res.hash) == (cnt, h), "%s: digest sink: nnz %d hash %x, want %d %x" % (what, res.nnz, res.hash, cnt, h)
    if np.isfinite(vsum) and np.all(np.isfinite(v)):
        assert abs(res.sum - vsum) <= 2 * max(cnt, 1) * 2.0 ** -53 * float(np.abs(v).sum()), "%s: digest sum %r, want %r" % (what, res.sum, vsum)
    else:
        assert not np.isfinite(res.sum), what


def test_semantic_fuzz(ctx):
    """200 small operands: raw unique-key, raw duplicate-key (consolidated by the three policies, zero_nan) and trusted
    strictly ascending with special values (NaN, +-Inf, +-0.0, explicit zeros, rows without a diagonal); both transposes,
    host and device operands, the COO sink plain and permuted and the digest sink.  The kind is the trial's base-3 digit and
    (factor_path, factor_row) its base-12 digit above that, so every kind meets every setting; the rest is drawn."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2121)
    seen = set()
    for trial in range(200):
        n = int(rng.integers(1, 41))
        t = '.' if rng.integers(2) == 0 else 'T'
        kind, combo = trial % 3, (trial // 3) % 12
        path, row = combo % 3, combo // 3
        pol, zn = int(rng.integers(3)), bool(rng.integers(5) == 0)
        dev_a, mode = bool(rng.integers(2)), int(rng.integers(3))
        A, sort0 = fr.fuzz_operand(rng, n, kind, t)
        S = sel.operand_S(A, t, pol, zn, sort0)
        f, rs = fr.ilu0_ref(S, n)
        keep = []
        a = _coo(A, (n, n), sort0, device=dev_a, keep=keep)
        what = "trial %d n %d kind %d %s pol %d zn %d path %d row %d dev %d mode %d" % (trial, n, kind, t, pol, zn, path, row, dev_a, mode)
        with Knobs(ctx, {"factor_path": path, "factor_row": row}):
            flags = capi.SINK_PERMUTE if mode == 1 else 0
            res, st = ctx.factor_ilu0(a, t, pol, zn, flags=flags, stats=True)
            got = ctx.fetch(res)
            want = (S[1], S[0], f) if mode == 1 else (S[0], S[1], f)
            _check(got, want, what)
            assert (res.shape0, res.shape1, res.nnz, res.nnz_a, res.products) == (n, n, len(f), len(f), rs["lookups"]), what
            _counters(st, rs, S, n, what)
            assert (st.levels, st.max_level_rows) == sr.schedule_stats(S, n), what
            assert st.analysis_reused == 0, what
            cl = fr.classes(S, n, capi.factor_serial_work, capi.factor_lds_row, row)
            assert (st.rows_serial, st.rows_wave, st.rows_block) == tuple(int(np.count_nonzero(cl == k)) for k in (1, 2, 3)), what
            if mode == 2:
                d, st2 = ctx.factor_ilu0(a, t, pol, zn, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS * int(trial % 2), stats=True)
                _digest_same(d, got, what)
                _counters(st2, rs, S, n, what + " digest")
                if trial % 2:
                    assert np.array_equal(ctx.to_host(d.row_nnz, n, np.int64), np.bincount(S[0], minlength=n)), what
        seen.add(("combo", kind, path, row)); seen.add(("op", t, dev_a)); seen.add(("mode", mode)); seen.add(("pol", pol, zn))
    assert len([s for s in seen if s[0] == "combo"]) == 36
    assert len([s for s in seen if s[0] == "op"]) == 4 and len([s for s in seen if s[0] == "mode"]) == 3
    assert len([s for s in seen if s[0] == "pol"]) == 6


def _level_max(x, lev, nlev):
    m = np.zeros(nlev, np.int64)
    np.maximum.at(m, lev, x)
    return m


def test_level_widths_at_the_edges(ctx):
    """Levels of 1 .. 5000 rows around the wave, workgroup and fuse widths, symmetrised so that every lower tuple has its
    diagonal update, plus seeded tuples that close triangles -- (i, g) and (g, i) for rows i and a parent g of a parent of
    theirs: a tuple between two rows sharing a parent would put one of them a level up, one to the level two below keeps
    the sixteen levels -- so updates exceed the lower tuples.  Under the default, factor_fuse_rows 256 and 1024 the fused runs
    begin and end at those widths; under factor_path 1 / 2 none / all of the levels (from level 1 on) are fused."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2122)
    sizes = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000, 1, 1, 1, 5000, 2]
    L, n, lev = sr.by_levels(rng, sizes, scatter=False)
    r, c = np.asarray(L[0], np.int64), np.asarray(L[1], np.int64)
    off = c < r
    parent = np.full(n, -1, np.int64)
    parent[r[off]] = c[off]                                            # one parent of every row beyond level 0
    pick = np.flatnonzero((lev >= 2) & (rng.random(n) < 0.3))
    g = parent[parent[pick]]
    rr, cc = np.r_[r, pick], np.r_[c, g]
    S = fr.symmetrised(fr.sorted_unique(rr, cc, np.r_[L[2], 0.25 * rng.standard_normal(pick.size)]), n, rng)
    assert np.array_equal(sr.levels(S, n), lev)
    f, rs = fr.ilu0_fast(S, n, lev)
    assert rs["updates"] > int(np.count_nonzero(S[1] < S[0]))
    w, length = fr.row_work(S, n), np.bincount(S[0], minlength=n)
    lw, ll = _level_max(w, lev, len(sizes)), _level_max(length, lev, len(sizes))
    keep = []
    a = _coo(S, (n, n), 0, device=True, keep=keep)
    for knob, value in (("factor_fuse_rows", 0), ("factor_fuse_rows", 256), ("factor_fuse_rows", 1024), ("factor_path", 1), ("factor_path", 2)):
        with Knobs(ctx, {knob: value}):
            res, st = ctx.factor_ilu0(a, stats=True)
        what = "%s %d" % (knob, value)
        _check(ctx.fetch(res), (S[0], S[1], f), what)
        _counters(st, rs, S, n, what)
        assert (st.levels, st.max_level_rows) == (16, 5000), what
        fuse = value if knob == "factor_fuse_rows" and value else capi.factor_fuse_rows
        want = fr.plan(sizes, lw, ll, fuse, capi.factor_serial_work, capi.factor_lds_row, factor_path=value if knob == "factor_path" else 0)
        assert (st.launches, st.fused_levels) == want, "%s: launches %d fused %d, want %r" % (what, st.launches, st.fused_levels, want)
    # (the one-row levels make the 5000 rows after them wave-class -- each names a row with 5000 tuples right of its diagonal --
    # and the row before them, 5000 tuples long, is block-class: the plan counts those launches)
    assert lw[14] > capi.factor_serial_work and ll[13] > capi.factor_lds_row and lw[13] > capi.factor_serial_work


def _row_shapes(rng, n, lds_row):
    """One operand for test_row_shapes_at_their_edges; returns S (sorted, unique)."""
    hot = np.arange(n - 100, n)
    rows = {i: {i} for i in range(n)}
    for k in range(100, 700):                                          # base rows: one tuple right of the diagonal, in a hot column
        rows[k].add(int(rng.choice(hot)))
    rows[5] |= set(int(x) for x in rng.choice(np.arange(6, n), 5000, replace=False))
    for k, m in ((19, 32), (20, 32), (21, 33)):
        rows[k] |= set(int(x) for x in rng.choice(np.r_[np.arange(1000, 1300), hot], m, replace=False))

    def add(i, lower, length=None):
        rows[i] |= set(int(x) for x in lower) | set(int(x) for x in rng.choice(hot, 40, replace=False))
        if length is not None:
            rest = np.setdiff1d(np.arange(i + 1, n), np.fromiter(rows[i], np.int64))
            rows[i] |= set(int(x) for x in rng.choice(rest, length - len(rows[i]), replace=False))
            assert len(rows[i]) == length
    add(1000, (19, 20)); add(1001, (19, 21))                           # work 64 and 65 with two lower tuples
    for i, m in ((1100, 63), (1101, 64), (1102, 65)):                  # 63 / 64 / 65 lower tuples, one lookup each
        add(i, rng.choice(np.arange(100, 700), m, replace=False))
    add(1200, (5,))                                                    # a short row naming a row with 5000 tuples right of its diagonal
    for i, length in ((2000, lds_row - 1), (2001, lds_row), (2002, lds_row + 1), (2100, 3 * lds_row)):
        add(i, rng.choice(np.arange(100, 700), lds_row // 4 + 16, replace=False), length)     # (more work than factor_serial_work)
    add(3000, (1200, 2000, 2002, 2100)); add(3001, (3000, 1102, 5))    # levels 2 and 3: the long rows' upper parts are read
    r = np.concatenate([np.full(len(cs), i) for i, cs in rows.items()])
    c = np.concatenate([np.fromiter(cs, np.int64) for cs in rows.values()])
    v = np.where(r == c, 3.0 + rng.random(r.size), 0.02 * rng.standard_normal(r.size))
    return fr.sorted_unique(r, c, v)


def test_row_shapes_at_their_edges(ctx):
    """Rows of 63 / 64 / 65 lower tuples, of factor_lds_row - 1, + 0, + 1 and 3 x factor_lds_row tuples, a short row whose work is
    5000 lookups, a row whose work is exactly factor_serial_work and one with one more; under the default and each factor_row:
    the bits, and the rows by kernel class as computed on the host from w_i and the row lengths."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2123)
    n, lds = 8000, capi.factor_lds_row
    S = _row_shapes(rng, n, lds)
    w, length = fr.row_work(S, n), np.bincount(S[0], minlength=n)
    assert [int(w[i]) for i in (1000, 1001, 1100, 1101, 1102)] == [64, 65, 63, 64, 65] and w[1200] == 5000
    assert [int(length[i]) for i in (2000, 2001, 2002, 2100)] == [lds - 1, lds, lds + 1, 3 * lds]
    f, rs = fr.ilu0_fast(S, n)
    assert rs["updates"] > 200
    cl0 = fr.classes(S, n, capi.factor_serial_work, lds)
    assert [int(cl0[i]) for i in (1000, 1001, 1100, 1101, 1102, 1200, 2000, 2001, 2002, 2100)] == [1, 2, 1, 1, 2, 2, 2, 2, 3, 3]
    keep = []
    a = _coo(S, (n, n), 0, device=True, keep=keep)
    for row in (0, 1, 2, 3):
        with Knobs(ctx, {"factor_row": row}):
            res, st = ctx.factor_ilu0(a, stats=True)
        what = "factor_row %d" % row
        _check(ctx.fetch(res), (S[0], S[1], f), what)
        _counters(st, rs, S, n, what)
        cl = fr.classes(S, n, capi.factor_serial_work, lds, row)
        assert (st.rows_serial, st.rows_wave, st.rows_block) == tuple(int(np.count_nonzero(cl == k)) for k in (1, 2, 3)), what
    # the thresholds moved: the same rows through other kernels, the same bits
    with Knobs(ctx, {"factor_serial_work": 63, "factor_lds_row": 64}):
        res, st = ctx.factor_ilu0(a, stats=True)
    _check(ctx.fetch(res), (S[0], S[1], f), "serial_work 63, lds_row 64")
    cl = fr.classes(S, n, 63, 64)
    assert (st.rows_serial, st.rows_wave, st.rows_block) == tuple(int(np.count_nonzero(cl == k)) for k in (1, 2, 3))


@pytest.fixture(scope="module")
def rmat12():
    S, n = fr.rmat_sym(12, 8, 3, 50.0)
    lev = sr.levels(S, n)
    f, rs = fr.ilu0_fast(S, n, lev)
    return S, n, lev, f, rs


def _factor_both_paths(ctx, S, n, f, rs, nlev, what, fused=None):
    keep = []
    a = _coo(S, (n, n), 0, device=True, keep=keep)
    for path in (0, 1):
        with Knobs(ctx, {"factor_path": path}):
            res, st = ctx.factor_ilu0(a, stats=True)
        _check(ctx.fetch(res), (S[0], S[1], f), "%s path %d" % (what, path))
        _counters(st, rs, S, n, "%s path %d" % (what, path))
        assert st.levels == nlev, what
        if path == 1:
            assert st.fused_levels == 0 and st.launches >= nlev - 1, what
        elif fused is not None:
            assert (st.fused_levels > 0) == fused, what


def test_stencils(ctx):
    """Poisson 64^2 (2 * 64 - 1 levels) and Laplace 16^3 (3 * 16 - 2) under the default and a launch per level."""
    for what, P, nlev in (("poisson", wl.poisson2d(64)[:3], 127), ("laplace", wl.laplace3d(16)[:3], 46)):
        S = fr.sorted_unique(*P)
        n = int(S[0].max()) + 1
        f, rs = fr.ilu0_fast(S, n)
        assert rs["zero_pivot"] == -1 and rs["updates"] == int(np.count_nonzero(S[1] < S[0]))    # no triangles: the diagonal updates alone
        _factor_both_paths(ctx, S, n, f, rs, nlev, what, fused=True)       # (every level at most 64 / 256 rows wide, every row serial-class)


def test_skew(ctx, rmat12):
    """The symmetrised R-MAT scale 12, edge factor 8, seed 3, plus a diagonal of 50: rows of every class in one level."""
    S, n, lev, f, rs = rmat12
    assert rs["lookups"] > 10 * len(f) and rs["updates"] > len(f)
    _factor_both_paths(ctx, S, n, f, rs, int(lev.max()) + 1, "rmat")


def test_chain(ctx):
    """The operand is itself a chained result (a spsamd_add of two halves) sitting in the current output set: F lands in the
    other set and the operand's tuples are intact afterwards; then solve_tri(F, LOWER, UNIT) and solve_tri(F, UPPER, NONUNIT)
    with 3 right-hand sides give the bits of solve_ref applied to ilu0_ref's F."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2124)
    n = 150
    m = 6 * n
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    S = fr.sorted_unique(np.r_[np.arange(n), r, c], np.r_[np.arange(n), c, r], np.r_[4.0 + rng.random(n), 0.3 * rng.standard_normal(2 * m)])
    half = np.arange(len(S[2])) % 2 == 0
    keep = []
    h1 = _coo(tuple(x[half] for x in S), (n, n), 0, keep=keep)
    h2 = _coo(tuple(x[~half] for x in S), (n, n), 0, keep=keep)
    sres = ctx.add(h1, h2)
    _check(ctx.fetch(sres), S, "the sum of the halves")
    op = capi.result_operand(sres)
    res, st = ctx.factor_ilu0(op, stats=True)
    f, rs = fr.ilu0_ref(S, n)
    assert res.val != sres.val and res.idx0 != sres.idx0
    _check(ctx.fetch(res), (S[0], S[1], f), "F")
    _check(ctx.fetch(sres), S, "the operand after the factorisation")
    _counters(st, rs, S, n, "chain")
    B = _rhs(rng, n, 3, 0.0)
    F = (S[0], S[1], f)
    Fop = capi.result_operand(res)
    Y, _ = _solve(ctx, Fop, B, sr.LOWER, sr.UNIT, device=True)
    X, _ = _solve(ctx, Fop, Y, sr.UPPER, sr.NONUNIT, device=True)
    want = sr.solve_ref(F, n, sr.solve_ref(F, n, B, sr.LOWER, sr.UNIT), sr.UPPER, sr.NONUNIT)
    _bits_same(X, want, "U^-1 L^-1 B")
    assert np.all(np.isfinite(X))


def test_prepared_keeps_the_schedule(ctx):
    """A handle factored twice: analysis_reused 0 then 1, spsamd_operand_bytes grown once.  A factorisation after a
    solve_tri(LOWER, NONUNIT) on a fresh handle reuses that solve's schedule, and the reverse.  A handle of the other
    transpose is analysed per call and still gives the right bits."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2125)
    n = 400
    m = 4 * n
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    R = fr.sorted_unique(np.r_[np.arange(n), r], np.r_[np.arange(n), c], np.r_[3.0 + rng.random(n), 0.3 * rng.standard_normal(m)])
    B = _rhs(rng, n, 2, 0.0)
    keep = []
    want = {t: (sel.operand_S(R, t),) for t in ('.', 'T')}
    want = {t: (S,) + fr.ilu0_fast(S, n) for t, (S,) in want.items()}
    for tprep in ('.', 'T'):
        S, f, rs = want[tprep]
        h = capi.Operand(ctx, _coo(R, (n, n), -1, False, keep), tprep, capi.AS_A, capi.ADD, False)
        try:
            b0 = h.bytes
            res, st = ctx.factor_ilu0(h.coo, tprep, stats=True)
            _check(ctx.fetch(res), (S[0], S[1], f), "prepared %s" % tprep)
            b1 = h.bytes
            assert st.analysis_reused == 0 and b1 > b0
            res, st2 = ctx.factor_ilu0(h.coo, tprep, stats=True)
            _check(ctx.fetch(res), (S[0], S[1], f), "prepared %s again" % tprep)
            assert st2.analysis_reused == 1 and h.bytes == b1
            assert (st2.levels, st2.launches, st2.fused_levels) == (st.levels, st.launches, st.fused_levels)
            _counters(st2, rs, S, n, "prepared again")
            X, sst = _solve(ctx, h.coo, B, sr.LOWER, sr.NONUNIT, tprep, device=True)        # ... and the solve finds it
            assert sst.analysis_reused == 1 and h.bytes == b1
            _bits_same(X, sr.solve_fast(S, n, B), "solve after factor")
            other = 'T' if tprep == '.' else '.'
            So, fo, rso = want[other]
            for k in range(2):
                res, st3 = ctx.factor_ilu0(h.coo, other, stats=True)
                _check(ctx.fetch(res), (So[0], So[1], fo), "prepared %s used %s" % (tprep, other))
                assert st3.analysis_reused == 0 and h.bytes == b1
                _counters(st3, rso, So, n, "other transpose")
        finally:
            h.close()
        h = capi.Operand(ctx, _coo(R, (n, n), -1, False, keep), tprep, capi.AS_A, capi.ADD, False)
        try:
            _solve(ctx, h.coo, B, sr.LOWER, sr.NONUNIT, tprep, device=True)
            b1 = h.bytes
            res, st = ctx.factor_ilu0(h.coo, tprep, stats=True)
            assert st.analysis_reused == 1 and h.bytes == b1
            _check(ctx.fetch(res), (S[0], S[1], f), "factor after solve, %s" % tprep)
        finally:
            h.close()


def test_refusals_leave_the_output_sets(ctx):
    """Every refusal leaves both output sets as they were: a result made before them is fetched whole after them."""
    from spsparse_amd import capi
    keep = []
    base = (np.array([0, 1, 1, 2], np.int32), np.array([0, 0, 1, 2], np.int32), np.array([1.0, 2.0, 3.0, 4.0]))
    r0 = ctx.consolidate(_coo(base, (3, 3), -1, keep=keep), 0)
    r1 = ctx.add(capi.result_operand(r0), _coo(base, (3, 3), 0, keep=keep))               # into the other set: r0 is its operand
    assert r1.val != r0.val
    L = ctx.L
    res = capi.Result()

    def call(a, t=b'.', pol=capi.ADD, sink=capi.SINK_COO, pa=None, pres=None):
        rc = L.spsamd_factor_ilu0(ctx.h, C.byref(a) if pa is None else pa, t, pol, 0, sink, 0, None, C.byref(res) if pres is None else pres)
        return rc, L.spsamd_last_error(ctx.h).decode()

    A = (np.array([0, 1, 2], np.int32), np.array([0, 0, 2], np.int32), np.array([1.0, 2.0, 3.0]))
    a = _coo(A, (3, 3), -1, keep=keep)
    assert call(a, pa=C.POINTER(capi.Coo)())[0] == -2 and call(a, pres=C.POINTER(capi.Result)())[0] == -2
    rc, msg = call(_coo(A, (3, 4), -1, keep=keep))
    assert rc == -1 and "square" in msg                                # non-square
    assert call(a, pol=3)[0] == -2 and call(a, sink=0)[0] == -2 and call(a, sink=3)[0] == -2
    assert call(_coo((A[0], np.array([0, 3, 2], np.int32), A[2]), (3, 3), -1, keep=keep))[0] == -2           # index out of bounds
    assert call(_coo((np.array([2, 1, 0], np.int32), A[1], A[2]), (3, 3), 0, keep=keep))[0] == -2            # a false sort0
    big = _coo(A, (3, 3), -1, keep=keep)
    big.nnz = 1 << 31
    assert call(big)[0] == -2
    for device in (False, True):
        dup = (np.array([0, 1, 1, 1, 2], np.int32), np.array([0, 0, 1, 1, 2], np.int32), np.ones(5))
        rc, msg = call(_coo(dup, (3, 3), 0, device=device, keep=keep))
        assert rc == -2 and "position 3" in msg, msg                   # a trusted operand with a duplicate key
        desc = (np.array([0, 1, 1, 2, 2], np.int32), np.array([0, 1, 0, 1, 2], np.int32), np.ones(5))
        rc, msg = call(_coo(desc, (3, 3), 0, device=device, keep=keep))
        assert rc == -2 and "position 2" in msg, msg                   # ... and one whose columns descend in row 1
    for r, want in ((r0, base), (r1, (base[0], base[1], 2 * base[2]))):
        _check(ctx.fetch(r), want, "a result made before the refusals")
    # a chained select result whose rows descend: a subsequence of a trusted operand is taken as it is, so only this call's own check sees it
    desc = (np.array([0, 1, 1, 2, 2], np.int32), np.array([0, 1, 0, 2, 1], np.int32), np.array([1.0, 2.0, 3.0, 4.0, 5.0]))
    sres = ctx.select(_coo(desc, (3, 3), 0, keep=keep), sel.ABS_GE, dparam=1.5)
    _check(ctx.fetch(sres), tuple(x[1:] for x in desc), "the select result")
    rc, msg = call(capi.result_operand(sres))
    assert rc == -2 and "position 1" in msg, msg
    _check(ctx.fetch(sres), tuple(x[1:] for x in desc), "the select result after the refusal")
    # n = 0 and an empty S
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    res0, st = ctx.factor_ilu0(_coo(e, (0, 0), -1, keep=keep), stats=True)
    assert (res0.shape0, res0.shape1, res0.nnz) == (0, 0, 0) and (st.levels, st.zero_pivot, st.missing_diag) == (0, -1, -1)
    res0, st = ctx.factor_ilu0(_coo(e, (5, 5), -1, keep=keep), stats=True)
    assert (res0.shape0, res0.shape1, res0.nnz) == (5, 5, 0) and ctx.fetch(res0)[2].size == 0
    assert (st.levels, st.max_level_rows, st.zero_pivot, st.missing_diag, st.lookups) == (1, 5, 0, 0, 0)
    d = ctx.factor_ilu0(_coo(e, (5, 5), -1, keep=keep), sink=capi.SINK_DIGEST)
    assert (d.nnz, d.hash) == (0, 0)
    zeros = (np.array([0, 1], np.int32), np.array([0, 1], np.int32), np.zeros(2))          # raw: consolidated to nothing
    res0 = ctx.factor_ilu0(_coo(zeros, (2, 2), -1, keep=keep))
    assert res0.nnz == len(sel.operand_S(zeros)[2]) == 0
    res, st = ctx.factor_ilu0(a, stats=True)                           # and the context still works
    _check(ctx.fetch(res), (A[0], A[1], np.array([1.0, 2.0, 3.0])), "after the refusals")
    assert (st.levels, st.zero_pivot, st.missing_diag) == (2, 1, 1)
