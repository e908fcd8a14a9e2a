"""The two emit paths of the heavy-row kernels.  k_dense has a PLAIN instantiation (C = 1, no scale vector: the emitted
value is the sum itself, known at compile time) beside the general one (C, scalei, scalek applied per output), and both
scan a cell out in batches: a batch's slots are exchanged with the clean value before the first of them is looked at.
k_bm_tiles takes the same calls through its one instantiation.  A product must not depend on which of them ran.

The inputs are the plans of tests/test_gpu_bank_layout.py (every slot, group edge and window edge; small integers, so
every sum is exact in any order) and one of its own with more dense cells than the launch has workgroups.  Everything
compares bit for bit with the oracle: the COO sink tuple for tuple, the digest sink in count, hash and value sum.  The
counters of the result show that the kernel under test took the products.  The plans are checked on the CPU first."""
import functools

import numpy as np
import pytest

from oracle import binding as orc
from tests.gpu_util import check_tuples, ctx, forced  # noqa: F401  (ctx: fixture)
from tests.test_gpu_bank_layout import (BITMAP_TILES, MID_MAX, W_LARGE, W_SMALL, column_scale, every_slot, few_columns,
                                        tile_rows, window_products)

gpu = pytest.mark.gpu

# (a) plain: the PLAIN instantiation; (b) .. (e): the general one
EMITS = ["plain", "C", "scalei", "scalek", "all"]
DROP = 3                    # scalek: every third column absent (its outputs are skipped), the others scaled by 1 or 2

PLANS = {
    "every_slot_8192": (every_slot, (W_SMALL, False)), "every_slot_8192_signed": (every_slot, (W_SMALL, True)),
    "every_slot_16384": (every_slot, (W_LARGE, False)), "every_slot_16384_signed": (every_slot, (W_LARGE, True)),
    "few_columns": (few_columns, ()),
    "tile_rows": (tile_rows, (False,)), "tile_rows_signed": (tile_rows, (True,)),
}


def emit_args(A, B, emit):
    """(C, scalei, scalek) of an emit variant as oracle operands: all factors small integers."""
    C_ = 2.0 if emit in ("C", "all") else 1.0
    rows = np.arange(A.shape[0])
    scalei = orc.Vec(rows, 1.0 + rows % 3 + (2.0 if A.shape[0] == 1 else 0.0), A.shape[0]) if emit in ("scalei", "all") else None
    scalek = column_scale(B.shape[1], DROP, 2) if emit in ("scalek", "all") else None
    return C_, scalei, scalek


@functools.lru_cache(maxsize=None)
def planned(plan, emit):
    """(A, B, C, scalei, scalek, the oracle's tuples) of a plan under an emit variant: computed once, never changed."""
    make, args = PLANS[plan] if plan in PLANS else (many_cells, ())
    A, B = make(*args)
    C_, scalei, scalek = emit_args(A, B, emit)
    want = orc.multiply(A, B, C_, scalei, '.', None, '.', scalek, rowwise=True, nthreads=4)[:3]
    return A, B, C_, scalei, scalek, want


# ---- more dense cells than workgroups ---------------------------------------------------------------------------------

MANY_ROWS = 2 * 256 + 64                # 2 x CUs + 64 on a 256-CU device (checked against the device at run time)
MANY_K = 41                             # B rows behind a row's second window: 41 x 100 products make the row heavy
# 100 columns each.  Window 0: two per group, in the even groups (set 0) or the odd ones (set 1).  Window 1: one per group
# in groups 27 .. 126, at different places of the group.  No two of the four sets share a slot of the accumulator.
SET_W0 = [np.sort(np.concatenate([[g * 64 + (5 * g) % 64, g * 64 + (5 * g + 33) % 64] for g in range(p, 100, 2)])) for p in (0, 1)]
SET_W1 = [np.asarray([g * 64 + (5 * g + 11 + 17 * p) % 64 for g in range(27, 127)]) + W_SMALL for p in (0, 1)]


def many_set(r):
    """Which pair of column sets row r takes: it alternates along the rows and flips from one sweep of 512 workgroups
    to the next, so cells that one workgroup takes in a row differ whether it walks by stride or by claim."""
    return (r + r // 512) % 2


@functools.lru_cache(maxsize=None)
def many_cells():
    """A: 576 x 84, row r has 1 + 41 tuples of value 1 + r mod 3.  B: 84 x 16384; rows 0 and 1 hold the 100 columns of
    window 0's two sets, rows 2 .. 42 and 43 .. 83 those of window 1's two sets, value 1 + column mod 7.  Row r takes
    B row s and the 41 rows of set s = many_set(r): a window of 100 products (one per column) and one of 4100 (41 per
    column), 4200 in all: a heavy row of two dense cells at dense_min = 64."""
    ai, ak, av, bk, bj = [], [], [], [], []
    for r in range(MANY_ROWS):
        s = many_set(r)
        ks = np.concatenate([[s], 2 + MANY_K * s + np.arange(MANY_K)])
        ai.append(np.full(ks.size, r)); ak.append(ks); av.append(np.full(ks.size, 1.0 + r % 3))
    for s in (0, 1):
        bk.append(np.full(100, s)); bj.append(SET_W0[s])
    for s in (0, 1):
        for q in range(MANY_K):
            bk.append(np.full(100, 2 + MANY_K * s + q)); bj.append(SET_W1[s])
    bj = np.concatenate(bj)
    A = orc.Mat(np.concatenate(ai), np.concatenate(ak), np.concatenate(av), (MANY_ROWS, 2 + 2 * MANY_K))
    return A, orc.Mat(np.concatenate(bk), bj, 1.0 + bj % 7, (2 + 2 * MANY_K, 2 * W_SMALL))


# ---- the plans, on the CPU -----------------------------------------------------------------------------------------------

def test_emit_variants_give_the_planned_outputs():
    """What the docstrings promise, from the operands and the oracle alone: which columns each variant keeps, that the
    cancelling columns are gone under every variant, and that all values are integers (exact in any order)."""
    for W in (W_SMALL, W_LARGE):
        cols = np.arange(W)
        for emit in EMITS:
            keep = cols % DROP != 0 if emit in ("scalek", "all") else np.ones(W, bool)
            factor = (2.0 if emit in ("C", "all") else 1.0) * (3.0 if emit in ("scalei", "all") else 1.0)
            kscale = np.where(cols % 2 == 0, 1.0, 2.0) if emit in ("scalek", "all") else np.ones(W)
            i, j, v = planned("every_slot_%d" % W, emit)[5]
            assert np.array_equal(j, cols[keep]) and np.array_equal(v, (4.0 * (cols + 1) * factor * kscale)[keep])
            i, j, v = planned("every_slot_%d_signed" % W, emit)[5]
            assert np.array_equal(j, cols[keep & (cols % 5 != 0)])          # the sums that cancel are not emitted
    for plan in PLANS:
        for emit in EMITS:
            i, j, v = planned(plan, emit)[5]
            assert len(v) and np.all(v == np.rint(v)) and np.all(v != 0)
    assert len(planned("tile_rows_signed", "plain")[5][1]) == len(planned("tile_rows", "plain")[5][1]) - 14
    assert len(planned("tile_rows", "scalek")[5][1]) < len(planned("tile_rows", "plain")[5][1])


def test_many_cells_plan():
    A, B = many_cells()
    assert len({int(c) for s in (0, 1) for c in SET_W0[s] % W_SMALL} | {int(c) for s in (0, 1) for c in SET_W1[s] % W_SMALL}) == 400
    assert not ({int(c) >> 6 for c in SET_W0[0]} & {int(c) >> 6 for c in SET_W0[1]})        # window 0: the sets' groups differ
    deg = np.zeros((B.shape[0], 2), np.int64)
    np.add.at(deg, (B.idx0, B.idx1 >> 13), 1)
    for r in (0, 1, 511, 512, 513, MANY_ROWS - 1):
        wp = deg[A.idx1[A.idx0 == r]].sum(axis=0)
        assert wp.tolist() == [100, 100 * MANY_K] and wp.sum() > MID_MAX      # heavy; each window above dense_min = 64
    assert all(many_set(r) != many_set(r + 1) for r in range(511)) and all(many_set(r) != many_set(r + 512) for r in range(64))
    i, j, v = planned("many_cells", "plain")[5]
    assert len(i) == MANY_ROWS * 200
    r = 5
    s = many_set(r)
    assert np.array_equal(j[i == r], np.concatenate([SET_W0[s], SET_W1[s]]))
    assert np.array_equal(v[i == r], (1.0 + r % 3) * np.concatenate([1.0 + SET_W0[s] % 7, MANY_K * (1.0 + SET_W1[s] % 7)]))


# ---- on the GPU ------------------------------------------------------------------------------------------------------------

def run_both_sinks(ctx, plan, emit):
    """The planned product through the C ABI in both sinks against the oracle's tuples; returns the COO result."""
    from spsparse_amd import capi
    A, B, C_, scalei, scalek, want = planned(plan, emit)
    keep = []

    def vec(x):
        if x is None:
            return None
        s, k = capi.host_vec(x.idx, x.val, x.shape0)
        keep.append(k)
        return s
    a, ka = capi.host_coo(A.idx0, A.idx1, A.val, A.shape, A.sort0)
    b, kb = capi.host_coo(B.idx0, B.idx1, B.val, B.shape, B.sort0)
    si, sk = vec(scalei), vec(scalek)
    res = ctx.multiply(a, b, C_, si, ".", None, ".", sk, capi.ADD, False, capi.SINK_COO, 0)
    got = tuple(ctx.fetch(res))
    check_tuples(got, want, "%s, %s: COO sink" % (plan, emit))
    dig = ctx.multiply(a, b, C_, si, ".", None, ".", sk, capi.ADD, False, capi.SINK_DIGEST, 0)
    cnt, vsum, h = orc.digest(*want)
    assert (dig.nnz, dig.hash) == (cnt, h), "%s, %s: digest sink: nnz %d hash %x, want %d %x" % (plan, emit, dig.nnz, dig.hash, cnt, h)
    assert dig.sum == vsum                                          # integers: exact in any order
    assert dig.products_dense == res.products_dense and dig.products_tiles == res.products_tiles
    return res


@gpu
@pytest.mark.parametrize("emit", EMITS)
@pytest.mark.parametrize("plan", ["every_slot_8192", "every_slot_8192_signed", "few_columns"])
def test_dense_cell_emit_paths(ctx, plan, emit):
    """One dense cell of the 8192-column window kernel, every slot or twenty columns at the edges, under each emit
    variant; signed: a fifth of the sums cancel to exactly 0 and must not be emitted by either instantiation."""
    res = run_both_sinks(ctx, plan, emit)
    assert res.window == W_SMALL and res.cells_dense >= 1 and res.products_dense == res.products > MID_MAX and res.products_tiles == 0


@gpu
@pytest.mark.parametrize("emit", EMITS)
@pytest.mark.parametrize("plan", ["every_slot_16384", "every_slot_16384_signed"])
def test_dense_cell_emit_paths_16384_column_window(ctx, plan, emit):
    """The same through the 16384-column window kernel (1024 threads, sixteen groups a wave as well)."""
    with forced(ctx, "window", W_LARGE):
        res = run_both_sinks(ctx, plan, emit)
    assert res.window == W_LARGE and res.cells_dense >= 1 and res.products_dense == res.products == 4 * W_LARGE and res.products_tiles == 0


@gpu
@pytest.mark.parametrize("emit", EMITS)
@pytest.mark.parametrize("plan", ["tile_rows", "tile_rows_signed"])
def test_bitmap_tiles_emit_paths(ctx, plan, emit):
    """One heavy row in bitmap tiles (keyed columns in the digest launch, columns in the store launch) under each emit
    variant."""
    with forced(ctx, "tiles_v1", BITMAP_TILES):
        res = run_both_sinks(ctx, plan, emit)
    assert res.products_tiles == res.products == 5120 and res.cells_dense == 0


@gpu
@pytest.mark.parametrize("emit", EMITS)
def test_consecutive_dense_cells_in_one_workgroup(ctx, emit):
    """1152 dense cells for at most 512 workgroups: every workgroup scans out several cells in a row, on column sets that
    share no slot.  A slot that a batch's clean left dirty is a wrong value, or a tuple too many, in the next cell."""
    import torch
    assert MANY_ROWS >= 2 * torch.cuda.get_device_properties(0).multi_processor_count + 64
    with forced(ctx, "dense_min", 64):
        res = run_both_sinks(ctx, "many_cells", emit)
    assert res.rows_heavy == MANY_ROWS and res.cells_dense == 2 * MANY_ROWS
    assert res.products_dense == res.products == MANY_ROWS * 100 * (1 + MANY_K) and res.products_tiles == 0
