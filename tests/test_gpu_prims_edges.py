"""The host-launched primitives of prims.hip -- the tiled exclusive scan in each of its instantiations, the sort frame and the
side-stream scope -- at their own edges, through the public API, against the test oracle and the host references, bit for bit.

The scan tile is T = 1024 elements (one launch up to T, two levels up to T * T, three from T * T + 1 on); the sort tile is
4096 keys.  Which call reaches which scan, read off the code:

    u8 -> u32    spsamd_consolidate: the keep flags and the run heads of the n stored tuples (consolidate_operand) -- the
                 operand is unsorted with a duplicate key and an explicit zero, so the flag, compact and merge passes run
    sort         the same call and spsamd_sorted_permutation: n keys (its digit histograms go through the u32 -> u32 scan)
    u32 -> i64   spsamd_extract: the tuple counts of the nR output rows
    u32 -> u32   spsamd_select, a tuple-wise predicate: one count per wave tile of 512 tuples, two levels from 1025 counts on
    u64 -> u64   spsamd_multiply_stream: the bounds of the nrow rows of op(A)
    batch        spsamd_multiply with h heavy rows: the per-row counters of heavy_prepare, h elements per array

Every value is a small integer, so a sum is exact in whatever order it is added."""
import numpy as np
import pytest

from oracle import binding as orc
from tests import extract_ref as xr
from tests import select_ref as sr
from tests import stream_ref as st
from tests.gpu_util import check_tuples as _check, coo as _coo, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

T = 1024
SHAPE = (1500, 2000)


def _ints(rng, n, lo=1, hi=4):
    return rng.integers(lo, hi, n).astype(np.float64) * rng.choice((-1.0, 1.0), n)


# ---------------------------------------------------------------- u8 -> u32 scan and the sort

_RAW = {}


def _raw(n):
    """n stored tuples in no order; from three tuples on one key twice and one explicit zero (one tuple: the zero).
    Made once per size, with the oracle's permutation and consolidation of it."""
    if n not in _RAW:
        rng = np.random.default_rng(1000 + n)
        i0 = rng.integers(0, SHAPE[0], n).astype(np.int32)
        i1 = rng.integers(0, SHAPE[1], n).astype(np.int32)
        v = _ints(rng, n)
        if n >= 3:
            i0[n - 1], i1[n - 1] = i0[0], i1[0]
            v[n // 2] = 0.0
        else:
            v[0] = 0.0
        _RAW[n] = ((i0, i1, v), orc.sorted_permutation(i0, i1, 0), orc.consolidate(i0, i1, v, 0))
    return _RAW[n]


SORT_N = (1, 1023, 1024, 1025, 4095, 4096, 4097, T * T + 1)


@pytest.mark.parametrize("n", SORT_N)
def test_consolidate_flags_compacts_and_merges(ctx, n):  # noqa: F811
    X, _, want = _raw(n)
    assert len(want[2]) < n                                # something was dropped or merged: the passes behind the sort ran
    keep = []
    res = ctx.consolidate(_coo(X, SHAPE, keep=keep), 0)
    _check(ctx.fetch(res), want, "consolidate n %d" % n)


@pytest.mark.parametrize("n", SORT_N)
def test_sorted_permutation(ctx, n):  # noqa: F811
    X, want, _ = _raw(n)
    keep = []
    got = ctx.sorted_permutation(_coo(X, SHAPE, keep=keep), 0)
    assert np.array_equal(got, want), "sorted_permutation n %d: first difference at %d" % (n, np.flatnonzero(got != want)[0])


# ---------------------------------------------------------------- u32 -> i64 scan

@pytest.mark.parametrize("nR", (T, T + 1, T * T + 1))
def test_extract_row_counts(ctx, nR):  # noqa: F811
    """Every 97th row of the source holds one tuple or two, the last row two; the output rows are the source's, last first."""
    rng = np.random.default_rng(nR)
    r = np.unique(np.r_[np.arange(5, nR, 97), nR - 1])
    rows = np.repeat(r, np.where(r % 2 == 1, 2, 1))
    first = np.searchsorted(rows, rows)
    S = (rows.astype(np.int32), (3 + 4 * (np.arange(len(rows)) - first)).astype(np.int32), _ints(rng, len(rows)))
    I = np.arange(nR - 1, -1, -1, dtype=np.int32)
    want = xr.extract_ref(S, I, None, nR, 8)
    assert len(want[2]) == len(rows) and want[0][0] == 0 and want[0][-1] == nR - 1 - 5
    keep = []
    res = ctx.extract(_coo(S, (nR, 8), 0, keep=keep), rows=I)
    _check(ctx.fetch(res), want, "extract nR %d" % nR)


# ---------------------------------------------------------------- u32 -> u32 scan, two levels

@pytest.mark.parametrize("n", (512 * T + 1, 512 * (T + 1) + 1))
def test_select_two_scan_levels(ctx, n):  # noqa: F811
    """ABS_GE over n tuples: T + 1 and T + 2 wave tiles, the last of one tuple, which is kept."""
    i = np.arange(n)
    A = ((i // 7).astype(np.int32), (i % 7).astype(np.int32), np.where((i % 3 == 0) | (i == n - 1), 2.0, 0.5) * np.where(i % 2, -1.0, 1.0))
    shape = (int(A[0][-1]) + 1, 7)
    want = sr.select_ref(A, shape[0], sr.ABS_GE, dparam=1.0)
    assert want[0][-1] == A[0][-1] and len(want[2]) == np.sum(i % 3 == 0) + (1 if (n - 1) % 3 else 0)
    keep = []
    res = ctx.select(_coo(A, shape, 0, True, keep), sr.ABS_GE, dparam=1.0)
    _check(ctx.fetch(res), want, "select n %d" % n)


# ---------------------------------------------------------------- u64 scan

@pytest.mark.parametrize("nrow", (1, T, T + 1, T * T + 1))
def test_stream_row_bounds(ctx, nrow):  # noqa: F811
    """Every 200th row of A and the last one hold one tuple or two; every row of B holds three.  The budget is a third of
    the bounds' sum: three blocks or more wherever A has three rows with tuples."""
    from spsparse_amd import capi
    rng = np.random.default_rng(nrow)
    inner, ncol = 64, 50
    r = np.unique(np.r_[np.arange(0, nrow, 200), nrow - 1])
    rows = np.repeat(r, np.where(r % 400 == 0, 2, 1))
    first = np.searchsorted(rows, rows)
    A = (rows.astype(np.int32), ((rows * 7 + 31 * (np.arange(len(rows)) - first)) % inner).astype(np.int32), _ints(rng, len(rows)))
    bk = np.repeat(np.arange(inner), 3)
    B = (bk.astype(np.int32), ((bk * 5 + 17 * (np.arange(len(bk)) % 3)) % ncol).astype(np.int32), _ints(rng, len(bk)))
    bound = st.row_bounds(A[0], A[1], nrow, np.full(inner, 3), ncol)
    budget = max(int(bound.max()), int(bound.sum()) // 3)
    edges = st.blocks(bound, budget)
    assert len(edges) - 1 >= (3 if len(r) >= 3 else 1)
    wi, wj, wv, _ = orc.multiply(orc.Mat(*A, (nrow, inner)), orc.Mat(*B, (inner, ncol)), rowwise=True)
    keep, parts = [], []
    a, b = _coo(A, (nrow, inner), keep=keep), _coo(B, (inner, ncol), keep=keep)
    res, stats = ctx.multiply_stream(a, b, flags=capi.SINK_ORDERED, block_tuples=budget,
                                     on_chunk=lambda i, j, v: parts.append((i.copy(), j.copy(), v.copy())))
    assert stats.blocks == len(edges) - 1, "nrow %d: %d blocks, the model has %d" % (nrow, stats.blocks, len(edges) - 1)
    got = tuple(np.concatenate([p[q] for p in parts]) for q in range(3))
    _check(got, (wi, wj, wv), "multiply_stream nrow %d against the oracle" % nrow)
    assert res.nnz == len(wv)
    plain = ctx.fetch(ctx.multiply(a, b, flags=capi.SINK_ORDERED))
    _check(plain, (wi, wj, wv), "multiply nrow %d against the oracle" % nrow)


# ---------------------------------------------------------------- batch scan, side-stream scope

_HEAVY = {}


def _heavy(h):
    """A: h rows of 65 tuples; B: 65 x 64, dense -- 4160 products a row, which is a heavy row.  With the oracle's product."""
    if h not in _HEAVY:
        rng = np.random.default_rng(7000 + h)
        A = (np.repeat(np.arange(h), 65).astype(np.int32), np.tile(np.arange(65), h).astype(np.int32), _ints(rng, 65 * h), (h, 65))
        B = (np.repeat(np.arange(65), 64).astype(np.int32), np.tile(np.arange(64), 65).astype(np.int32), _ints(rng, 65 * 64), (65, 64))
        _HEAVY[h] = (A, B, orc.multiply(orc.Mat(*A), orc.Mat(*B), rowwise=True, nthreads=8)[:3])
    return _HEAVY[h]


def _heavy_product(c, h, what):
    """Both sinks of A * B on context c against the oracle; every row must have gone the heavy rows' way."""
    from spsparse_amd import capi
    A, B, want = _heavy(h)
    keep = []
    a, b = _coo(A[:3], A[3], keep=keep), _coo(B[:3], B[3], keep=keep)
    res = c.multiply(a, b, sink=capi.SINK_COO)
    assert res.rows_heavy == h, "%s: %d heavy rows, want %d" % (what, res.rows_heavy, h)
    _check(c.fetch(res), want, what)
    d = c.multiply(a, b, sink=capi.SINK_DIGEST)
    cnt, vsum, hsh = orc.digest(*want)
    assert d.rows_heavy == h
    assert (d.nnz, d.hash) == (cnt, hsh), "%s digest: nnz %d hash %x, want %d %x" % (what, d.nnz, d.hash, cnt, hsh)
    assert d.sum == want[2].sum(), "%s digest: sum %r, want %r" % (what, d.sum, want[2].sum())


@pytest.mark.parametrize("h", (1, T, T + 1))
def test_heavy_rows_batch_scan(ctx, h):  # noqa: F811
    _heavy_product(ctx, h, "heavy rows h %d" % h)


def test_side_streams_leave_the_context_on_its_main_stream():
    """h = 1025 builds the window-major copy of B on the second stream and sorts the lists on the third.  Twice on one
    context, then an all-light product on it: a stream left swapped, or a join left out, shows in one of the three."""
    from spsparse_amd import capi
    c = capi.Context(0)
    try:
        for turn in (1, 2):
            _heavy_product(c, T + 1, "side streams, turn %d" % turn)
        rng = np.random.default_rng(5)
        n = 300
        L = (rng.integers(0, n, 900).astype(np.int32), rng.integers(0, n, 900).astype(np.int32), _ints(rng, 900), (n, n))
        want = orc.multiply(orc.Mat(*L), orc.Mat(*L), rowwise=True)[:3]
        keep = []
        a = _coo(L[:3], L[3], keep=keep)
        res = c.multiply(a, a, sink=capi.SINK_COO)
        assert res.rows_heavy == 0 and res.rows_mid == 0 and res.rows_light > 0
        _check(c.fetch(res), want, "the light product after the heavy ones")
    finally:
        c.close()
