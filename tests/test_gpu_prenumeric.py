"""What a multiply runs before its first numeric kernel, at its own edges, against the test oracle bit for bit: the operand
consolidation behind both forms of the sort (key and position in one 64-bit word where they fit, two arrays where not), the
list of op(A)'s non-empty rows in both of its forms (from the dense row pointer, from the tuples) and the cell grouping of
the heavy rows over a number of windows that is no multiple of four.

Every value is a small integer (or a NaN on a key of its own), so a sum is exact in whatever order it is added."""
import numpy as np
import pytest

from oracle import binding as orc
from tests.gpu_util import check_tuples as _check, coo as _coo, ctx  # noqa: F401
from tests.test_gpu_prims_edges import _heavy, _ints

pytestmark = pytest.mark.gpu

SHAPE = (1500, 2000)                    # 11 + 11 key bits: one word with any position
BIG = (2 ** 31 - 1, 2 ** 31 - 1)        # 62 key bits: no room for a position of three bits or more
POLICIES = (orc.LEAVE_ALONE, orc.ADD, orc.REPLACE)

# ---------------------------------------------------------------- consolidation

_RAW = {}


def _raw(n, shape):
    """n stored tuples in no order.  In sorted order (position = place in the stable sort):
        0 and n - 1        explicit zeros
        1 and 5            NaNs on keys of their own: before and after the first kept key, which is at 2 (n >= 8)
        10 .. 13           one key, zeros only: no output (n >= 20)
        60 .. 69           one key across position 64, its first two tuples zeros (n >= 63)
        4090 .. 4100       one key across position 4096, its first two tuples zeros (n >= 4095)
    and every other position a key of its own.  Runs are cut at n."""
    if (n, shape) not in _RAW:
        rng = np.random.default_rng(2000 + n)
        gid = np.arange(n)
        runs = [(a, min(b, n)) for a, b in ((10, 14), (60, 70), (4090, 4101)) if a < n]
        for a, b in runs:
            gid[a:b] = a
        lin = np.unique(rng.integers(0, shape[0] * shape[1], 2 * n + 8))
        lin = np.sort(rng.choice(lin, n, replace=False))[gid]
        v = _ints(rng, n)
        if n >= 8:
            v[1] = v[5] = np.nan
        for a, b in runs:
            v[a:min(a + 2, b)] = 0.0
        if n >= 20:
            v[10:14] = 0.0
        v[0] = v[n - 1] = 0.0
        at = rng.permutation(n)                             # sorted position t is stored at at[t] ...
        for a, b in runs:
            at[a:b] = np.sort(at[a:b])                      # ... the tuples of a run in their order (the sort is stable)
        i0, i1, val = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n)
        i0[at], i1[at], val[at] = lin // shape[1], lin % shape[1], v
        _RAW[n, shape] = (i0, i1, val), {}
    return _RAW[n, shape]


CASES = [(n, SHAPE) for n in (1, 2, 8, 63, 64, 65, 4095, 4096, 4097)] + [(8, BIG), (4097, BIG)]
_ids = ["%d-%s" % (n, "big" if s is BIG else "small") for n, s in CASES]


@pytest.mark.parametrize("zero_nan", (False, True))
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n,shape", CASES, ids=_ids)
def test_consolidate(ctx, n, shape, policy, zero_nan):  # noqa: F811
    X, memo = _raw(n, shape)
    if (policy, zero_nan) not in memo:
        memo[policy, zero_nan] = orc.consolidate(X[0], X[1], X[2], 0, policy, zero_nan)
    want = memo[policy, zero_nan]
    if n >= 8:
        assert (np.count_nonzero(np.isnan(want[2])) == (1 if zero_nan else 2)), "the oracle drops the leading NaN alone"
    keep = []
    res = ctx.consolidate(_coo(X, shape, keep=keep), 0, policy, zero_nan)
    _check(ctx.fetch(res), want, "consolidate n %d shape %s policy %d zero_nan %d" % (n, shape, policy, zero_nan))


SMALL = {"kept": ([3], [4], [2.0]), "zero_kept": ([3, 5], [4, 6], [0.0, 2.0]), "kept_zero": ([3, 5], [4, 6], [2.0, 0.0]),
         "pair": ([5, 5], [6, 6], [2.0, 3.0]), "zero_pair": ([5, 5], [6, 6], [0.0, 3.0]), "unsorted_pair": ([5, 3, 5], [6, 4, 6], [2.0, 1.0, 3.0])}


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("case", sorted(SMALL))
def test_consolidate_one_to_three_tuples(ctx, case, policy):  # noqa: F811
    """The sizes at which _raw holds zeros only: a kept tuple alone, beside a zero, and a pair on one key."""
    X = tuple(np.asarray(x, t) for x, t in zip(SMALL[case], (np.int32, np.int32, np.float64)))
    want = orc.consolidate(X[0], X[1], X[2], 0, policy, False)
    assert len(want[2]) >= 1
    keep = []
    res = ctx.consolidate(_coo(X, SHAPE, keep=keep), 0, policy, False)
    _check(ctx.fetch(res), want, "consolidate %s policy %d" % (case, policy))


@pytest.mark.parametrize("n,shape", CASES, ids=_ids)
def test_sorted_permutation(ctx, n, shape):  # noqa: F811
    X, memo = _raw(n, shape)
    if "perm" not in memo:
        memo["perm"] = orc.sorted_permutation(X[0], X[1], 0)
    want = memo["perm"]
    keep = []
    got = ctx.sorted_permutation(_coo(X, shape, keep=keep), 0)
    assert np.array_equal(got, want), "sorted_permutation n %d: first difference at %d" % (n, np.flatnonzero(got != want)[0])


# ---------------------------------------------------------------- row lists

_ROWS = {}


def _rows_of(rng, rows, per_row, ncol):
    """per_row tuples in each of `rows`, columns distinct inside a row."""
    r = np.repeat(np.asarray(rows), per_row)
    c = np.concatenate([rng.choice(ncol, per_row, replace=False) for _ in rows])
    return r.astype(np.int32), c.astype(np.int32), _ints(rng, len(r))


def _rowlist(case):
    """(A, B or None for A * A, the oracle's product).  The longest rows of A and B hold ten tuples or more each, so no product
    is all light and every one builds the row list of A.  A multiply builds the dense row pointer of A in every case (it reads
    the longest row off it), also where A is not the right operand, so the path is chosen by nrow + 1 <= nnz alone:
        ends     60 x 60, rows 1 .. 58 of ten tuples, the first and the last row empty; A * A: A's pointer is B's; pointer form
        single   5 x 40, row 2 alone, 40 tuples; B 40 x 12: pointer form, one flagged entry of five
        sparse   100000 x 40, rows 3 and 99998 of twelve tuples: nrow >> nnz; the same B: the one case of the tuples' form
        a_only   50 x 40, ten tuples a row; the same B: A is the left operand only, its pointer is built for it; pointer form,
                 the same path as `ends` with no empty row"""
    if case not in _ROWS:
        rng = np.random.default_rng({"ends": 31, "single": 32, "sparse": 33, "a_only": 34}[case])
        B = _rows_of(rng, range(40), 10, 12) + ((40, 12),)
        if case == "ends":
            A, B = _rows_of(rng, range(1, 59), 10, 60) + ((60, 60),), None
        elif case == "single":
            A = _rows_of(rng, [2], 40, 40) + ((5, 40),)
        elif case == "sparse":
            A = _rows_of(rng, [3, 99998], 12, 40) + ((100000, 40),)
        else:
            A = _rows_of(rng, range(50), 10, 40) + ((50, 40),)
        _ROWS[case] = (A, B, orc.multiply(orc.Mat(*A), orc.Mat(*(B or A)), rowwise=True)[:3])
    return _ROWS[case]


@pytest.mark.parametrize("case", ("ends", "single", "sparse", "a_only"))
def test_row_list(ctx, case):  # noqa: F811
    from spsparse_amd import capi
    A, B, want = _rowlist(case)
    assert (A[3][0] + 1 <= len(A[2])) == (case != "sparse")
    keep = []
    a = _coo(A[:3], A[3], keep=keep)
    b = a if B is None else _coo(B[:3], B[3], keep=keep)
    res = ctx.multiply(a, b, sink=capi.SINK_COO)
    assert res.rows_light + res.rows_mid + res.rows_heavy == len(np.unique(A[0])), "%s: the rows of the three classes" % case
    _check(ctx.fetch(res), want, "row list %s" % case)
    d = ctx.multiply(a, b, sink=capi.SINK_DIGEST)
    cnt, _, hsh = orc.digest(*want)
    assert (d.nnz, d.hash) == (cnt, hsh), "%s digest: nnz %d hash %x, want %d %x" % (case, d.nnz, d.hash, cnt, hsh)
    assert d.sum == want[2].sum(), "%s digest: sum %r, want %r" % (case, d.sum, want[2].sum())


# ---------------------------------------------------------------- cell grouping

NCOL = 5 * 8192 + 1                     # six windows of 8192 columns, the last of one column
HS = (1, 63, 64, 65, 127, 128, 129)     # heavy rows, one thread of k_cells each: around one wave and one workgroup
_CELLS = {}


def _spread(j):
    """Column of B's j-th tuple of a row: j = 0 in the last window, the others over the five whole windows in turn."""
    j = np.asarray(j)
    return np.where(j == 0, NCOL - 1, ((j - 1) % 5) * 8192 + 7 * j).astype(np.int32)


def _cells(h, variant):
    """_heavy(h) with B's columns placed in NCOL columns.  "dense": every column in window 2, 4160 products of a row in one
    window; "tiles": over all six windows, 65 to 845 products a window; "long": the same, B 300 rows (the further ones one
    tuple each) and the last row of A 300 tuples -- too long for a tile, 65 to 892 products a window."""
    if (h, variant) not in _CELLS:
        A, B, _ = _heavy(h)
        a0, a1, av = A[0], A[1], A[2]
        bj = np.tile(np.arange(64), 65)
        b0, b1, bv = B[0], (2 * 8192 + 3 * bj).astype(np.int32) if variant == "dense" else _spread(bj), B[2]
        inner = 65
        if variant == "long":
            rng = np.random.default_rng(7500 + h)
            inner = 300
            more = np.arange(65, 300)
            b0 = np.r_[b0, more].astype(np.int32)
            b1 = np.r_[b1, _spread(1 + more % 5)].astype(np.int32)
            bv = np.r_[bv, _ints(rng, len(more))]
            cut = 65 * (h - 1)
            a0 = np.r_[a0[:cut], np.full(300, h - 1)].astype(np.int32)
            a1 = np.r_[a1[:cut], np.arange(300)].astype(np.int32)
            av = np.r_[av[:cut], _ints(rng, 300)]
        A, B = (a0, a1, av, (h, inner)), (b0, b1, bv, (inner, NCOL))
        _CELLS[h, variant] = (A, B, orc.multiply(orc.Mat(*A), orc.Mat(*B), rowwise=True, nthreads=8)[:3])
    return _CELLS[h, variant]


@pytest.mark.parametrize("variant", ("dense", "tiles", "long"))
@pytest.mark.parametrize("h", HS)
def test_cell_grouping(ctx, h, variant):  # noqa: F811
    from spsparse_amd import capi
    A, B, want = _cells(h, variant)
    what = "%s cells, h %d" % (variant, h)
    keep = []
    a, b = _coo(A[:3], A[3], keep=keep), _coo(B[:3], B[3], keep=keep)
    cnt, _, hsh = orc.digest(*want)
    for sink in (capi.SINK_COO, capi.SINK_DIGEST):
        res = ctx.multiply(a, b, sink=sink)
        assert res.rows_heavy == h, "%s: %d heavy rows, want %d" % (what, res.rows_heavy, h)
        assert res.window == 8192
        # which cells the rows were cut into: all dense | all tile cells | the long row's hash cells beside the others' tiles
        dense, tiles = (4160 * h, 0) if variant == "dense" else (0, 4160 * (h if variant == "tiles" else h - 1))
        assert (res.products_dense, res.products_tiles) == (dense, tiles), "%s: %d products in dense cells, %d in tiles" % (
            what, res.products_dense, res.products_tiles)
        if variant == "dense":
            assert res.cells_dense == h
        if sink == capi.SINK_COO:
            _check(ctx.fetch(res), want, what)
        else:
            assert (res.nnz, res.hash) == (cnt, hsh), "%s digest: nnz %d hash %x, want %d %x" % (what, res.nnz, res.hash, cnt, hsh)
            assert res.sum == want[2].sum(), "%s digest: sum %r, want %r" % (what, res.sum, want[2].sum())
