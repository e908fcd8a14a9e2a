"""k_dense (csrc/k_dense.hip) on planned dense cells: the row's A-tuple count against the chunk of NT tuples (the clamped
prefetches of chunk c + 1 and c + 2 and of the next cell), segment lengths against the item of R tuples and the 64-item
block, chunks whose segments are empty in some lanes or in all of them (the path that skips barriers B2 and B3), chunks
of more than W items (later batches: the re-marked bitmap, the carried segment count, a boundary inside a segment and on
a first item), and lists of one cell to 4200 cells whose shape changes from each cell to the next (in the list and in
every workgroup's walk), under the three ways the list is dealt.  GPU only.

The plans come from tests/dense_plan.py; tests/test_dense_plan_host.py shows on the CPU that each is what it claims.
Every case goes through the C ABI in both sinks and compares bit for bit with the oracle (small integers: every sum is
exact in any order of the atomics): the COO sink tuple for tuple in order, the digest sink in count, hash and value sum.
Every case also asserts that the planned cut happened: the window width and every counter of the result equal the
plan's.  A cut that differs from the plan is a failure.

Every plan runs plain at both window widths.  A representative of each group -- L = NT + 1, the segment lengths, the
empty middle chunk, the straddling batch, the second chunk of two batches, the 2450-cell list -- also runs ORDERED, under
EXACT_PATTERN with planned cancellations (where the plan has more than one chunk or batch to put a pair in), with C,
scalei and scalek (the general instantiation and the COUNT launch's col_allowed walk), through the row-major window index
(no_wmajor) and with op(B) as a prepared handle multiplied twice; the lists with ROWSTATS.

Not here: the slot layout and the scan-out's group edges (tests/test_gpu_bank_layout.py has them), B operands too large
for 32-bit piece offsets (3.5e8 tuples), the DENSE_DEPTH 2 and ablation builds, and any timing."""
import numpy as np
import pytest

from tests import dense_plan as dp
from tests import emit_ref as er
from tests import tile_plan as tp
from tests.gpu_util import Knobs, check_digest, check_tuples, ctx, operands, sink_flags  # noqa: F401  (ctx: fixture)
from tests.tile_plan import BITMAP

pytestmark = pytest.mark.gpu


class Tuned(Knobs):
    """Knobs whose "xcd" goes back to its default, 2 (the others' default is 0)."""

    def __exit__(self, *exc):
        super().__exit__(*exc)
        if "xcd" in self.knobs:
            self.ctx.set_tuning("xcd", 2)


def run_plan(ctx, p, flag="plain", emit="plain", extra=None, b=None, rowstats=False, what=""):
    """The plan under a sink flag, an emit variant and further knobs, in both sinks: the planned cut (every counter) and
    the oracle's tuples, bit for bit.  b: a prepared op(B) in place of the plan's.  Returns (COO result, digest result)."""
    from spsparse_amd import capi
    want = tp.oracle_tuples(p, emit)
    what = "%s%s, %s, %s" % (what, flag, emit, extra or {})
    keep, out = [], []
    a, b0, C_, si, sk = operands(p, emit, keep)
    planned = p.cut(tp.effective_scheme(BITMAP, flag)).counters()
    assert planned["cells_dense"] == p.ndense and planned["cells_hash"] == 0
    for sink in (capi.SINK_COO, capi.SINK_DIGEST):
        flags = sink_flags(flag) | (capi.SINK_ROWSTATS if rowstats and sink == capi.SINK_DIGEST else 0)
        with Tuned(ctx, dict(p.knobs, **(extra or {}))):
            res = ctx.multiply(a, b if b is not None else b0, C_, si, ".", None, ".", sk, capi.ADD, False, sink, flags)
        got = {name: getattr(res, name) for name in planned}
        print("%s: sink %d window %d %r" % (what, sink, res.window, got))
        assert res.window == p.W
        for name, n in planned.items():
            assert got[name] == n, "%s: %s %d, planned %d" % (what, name, got[name], n)
        if sink == capi.SINK_COO:
            check_tuples(tuple(ctx.fetch(res)), want, what + ": COO sink")
        else:
            check_digest(res, want, what)
            if rowstats:
                nrow = p.A.shape[0]
                rn, rh = er.row_stats(want, nrow)
                rs = np.bincount(want[0], weights=want[2], minlength=nrow)          # (integers: exact in any order)
                assert np.array_equal(ctx.to_host(res.row_nnz, nrow, np.int64), rn), what + ": row_nnz"
                assert np.array_equal(ctx.to_host(res.row_hash, nrow, np.uint64), rh), what + ": row_hash"
                assert np.array_equal(ctx.to_host(res.row_sum, nrow, np.float64), rs), what + ": row_sum"
        out.append(res)
    return out


# ---- every plan, plain

@pytest.mark.parametrize("name", list(dp.CATALOGUE))
def test_planned_cells(ctx, name):
    """A: L = 1, 2, NT - 1 .. 3 NT + 1.  B: segment lengths 0 .. 513, the whole window as one segment, one column, every
    column once.  C: eight lane patterns, empty chunks first, middle, last and two in a row.  D: W - 1, W, W + 1 items, two
    and three batches, the boundary inside a segment and on a first item, a second chunk of two batches.  E: one cell, 210,
    2450 (static stride) and 4200 (claimed XCD parts) cells.  And the variants with planned cancellations."""
    p = dp.plan(name)
    coo, dig = run_plan(ctx, p, what=name + ": ")
    assert coo.cells_dense == p.ndense and coo.products_dense == coo.products


# ---- the representatives under flags, emit variants and knobs

REPS = ["chunk_L513_8192", "chunk_L1025_16384", "seg_lens_8192", "seg_lens_16384", "empty_middle_8192", "empty_middle_16384",
        "straddle_8192", "straddle_16384", "second_chunk_8192", "second_chunk_16384", "list_static_8192", "list_static_16384"]
CANCELS = [n for n in dp.CATALOGUE if n.endswith("_cancel")]


@pytest.mark.parametrize("name", REPS + ["three_batches_8192", "lanes_8192"])
def test_ordered(ctx, name):
    """SINK_ORDERED: the ascending-k accumulation, one segment at a time, and its own clean-up of the bitmap."""
    run_plan(ctx, dp.plan(name), "ordered", what=name + ": ")


@pytest.mark.parametrize("emit", ["plain", "all"])
@pytest.mark.parametrize("name", CANCELS)
def test_exact_pattern_with_planned_cancellations(ctx, name, emit):
    """SINK_EXACT_PATTERN on sums that cancel to exactly 0: the pair of a cancelled column lies in different chunks, for
    the batch plans in different batches; one window of every plan cancels completely and emits nothing."""
    p = dp.plan(name)
    coo, dig = run_plan(ctx, p, "exact", emit, what=name + ": ")
    assert p.cancelled > 0


@pytest.mark.parametrize("emit", ["C", "scalei", "scalek", "all"])
@pytest.mark.parametrize("name", REPS + ["chunk_L513_8192_cancel"])
def test_emit_variants(ctx, name, emit):
    """C, scalei, scalek with absent columns, and all three: the general instantiation instead of PLAIN, and the COUNT
    launch's col_allowed walk."""
    run_plan(ctx, dp.plan(name), "plain", emit, what=name + ": ")


@pytest.mark.parametrize("name", ["list_few_8192", "list_few_16384", "list_static_8192", "lanes_8192"])
def test_rowstats(ctx, name):
    """SINK_DIGEST | SINK_ROWSTATS on rows with dense cells in several windows: row_nnz, row_sum and row_hash."""
    run_plan(ctx, dp.plan(name), rowstats=True, what=name + ": ")


@pytest.mark.parametrize("name", REPS + ["columns_8192", "giant_16384"])
def test_row_major_window_index(ctx, name):
    """no_wmajor = 1: the segment bounds come from the row-major window index and B is read in place."""
    run_plan(ctx, dp.plan(name), extra={"no_wmajor": 1}, what=name + ": ")


@pytest.mark.parametrize("name", REPS)
def test_prepared_right_operand_twice(ctx, name):
    """op(B) as a prepared handle, multiplied twice in a row: the second product reads the handle's window-major copy."""
    from spsparse_amd import capi
    p = dp.plan(name)
    s, k = capi.host_coo(p.B.idx0, p.B.idx1, p.B.val, p.B.shape, p.B.sort0)
    op = capi.Operand(ctx, s, role=capi.AS_B)
    try:
        for rep in ("first", "second"):
            run_plan(ctx, p, b=op.coo, what="%s: prepared, %s: " % (name, rep))
    finally:
        op.close()
    del k


# ---- the three ways the list is dealt

@pytest.mark.parametrize("xcd", [0, 1, 2])
@pytest.mark.parametrize("name", ["list_parts_8192", "list_static_8192"])
def test_list_walks(ctx, name, xcd):
    """4200 cells (cut into XCD parts: claimed under xcd 2, static parts under 1, one list under 0) and 2450 (below 4096:
    one list with the static stride whatever the knob), twice in one context: the claim counters start afresh."""
    p = dp.plan(name)
    first = run_plan(ctx, p, extra={"xcd": xcd}, what=name + ": ")[1]
    again = run_plan(ctx, p, extra={"xcd": xcd}, what=name + ", again: ")[1]
    assert (again.nnz, again.hash, again.sum) == (first.nnz, first.hash, first.sum)
