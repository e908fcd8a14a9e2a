"""The four tile kernels (k_bm_tiles, k_hash_tiles2, k_direct_tiles in csrc/k_tiles.hip, k_hash_tiles in csrc/k_hash.hip)
on planned tiles: every class of A-tuple count, the edges of a cell (distinct columns at the emission loop's trips, the
full column range, cancelled sums, absent columns), of its items and segments, of the hash tables (full, one column,
probe runs that wrap), the direct cells, and long lists of tiles whose shape changes from one tile to the next.  GPU only.

The plans come from tests/tile_plan.py; tests/test_tile_plan_host.py shows on the CPU that each is what it claims.  Every
case goes through the C ABI in both sinks and compares bit for bit with the oracle (small integers: every sum is exact in
any order): the COO sink tuple for tuple in order, the digest sink in count, hash and value sum.  Every case also asserts
that the planned cut happened: the symbolic phase's trace line (tiles, tile cells) and the result's counters equal the
plan's.  A cut that differs from the plan is a failure."""
import re

import pytest

from tests import tile_plan as tp
from tests.gpu_util import Knobs, check_digest, check_tuples, ctx, operands, sink_flags  # noqa: F401  (ctx: fixture)
from tests.tile_plan import BITMAP, HASH1, HASH2

pytestmark = pytest.mark.gpu

SCHEMES = {"bitmap": BITMAP, "hash2": HASH2, "hash1": HASH1}


def run_plan(ctx, capfd, p, scheme, flag="plain", emit="plain", extra=None):
    """The plan under a scheme, sink flag and emit variant, in both sinks: the planned cut (trace line and counters) and
    the oracle's tuples, bit for bit.  Returns (the COO result, the digest result)."""
    from spsparse_amd import capi
    want = tp.oracle_tuples(p, emit)
    what = "%s, %s, %s" % (tp.SCHEME_IDS[scheme], flag, emit)
    keep, out = [], []
    a, b, C_, si, sk = operands(p, emit, keep)
    knobs = dict(p.knobs, tiles_v1=tp.TILES_V1[scheme], trace=1, **(extra or {}))
    for sink in (capi.SINK_COO, capi.SINK_DIGEST):
        cut = p.cut(tp.effective_scheme(scheme, flag), coo=sink == capi.SINK_COO)
        with Knobs(ctx, knobs):
            capfd.readouterr()
            res = ctx.multiply(a, b, C_, si, ".", None, ".", sk, capi.ADD, False, sink, sink_flags(flag))
            err = capfd.readouterr().err
        m = re.search(r"tiles (\d+) cells (\d+):", err)
        got_cut = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
        assert got_cut == (cut.tiles, cut.tile_cells), "%s: tiles, cells %r, planned %r" % (what, got_cut, (cut.tiles, cut.tile_cells))
        assert res.window == p.W
        for name, planned in cut.counters().items():
            assert getattr(res, name) == planned, "%s: %s %d, planned %d" % (what, name, getattr(res, name), planned)
        if sink == capi.SINK_COO:
            check_tuples(tuple(ctx.fetch(res)), want, what + ": COO sink")
        else:
            check_digest(res, want, what)
        out.append(res)
    return out


# ---- A. classes of A-tuple count

@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("L", tp.L_CLASSES + (257,))
def test_tuple_count_classes(ctx, capfd, L, scheme):
    """A row of exactly G cells in one tile and a row of G + 1 (its last cell opens a second tile), for every class of L:
    the thread-to-(cell, tuple) mapping at lsh 0 .. 8, lanes ei >= L idle inside a wave that holds other cells, sixteen
    one-thread cells in wave 0 at L = 1.  L = 257: the other side of the boundary, windowed hash cells and no tile."""
    coo, dig = run_plan(ctx, capfd, tp.l_class(L), SCHEMES[scheme])
    assert (coo.products_tiles == 0) == (L == 257)


# ---- B. bitmap cell edges

@pytest.mark.parametrize("flag", ["plain", "exact"])
@pytest.mark.parametrize("name", ["bm_distinct", "bm_few_columns", "bm_range_8192", "bm_range_16384"])
def test_bitmap_cell_edges(ctx, capfd, name, flag):
    """Distinct columns at the trip edges of the emission loop (two ranks a trip in the digest launch) up to the full acc
    and colof, once a product per column and once many products on 7 columns; a cell over all 2048 bitmap words, whose row's
    next window starts a new cell, at both window widths."""
    run_plan(ctx, capfd, tp.plan(name), BITMAP, flag)


@pytest.mark.parametrize("flag", ["plain", "exact"])
@pytest.mark.parametrize("where", tp.CANCELS)
def test_bitmap_cancelled_sums(ctx, capfd, where, flag):
    """Sums that cancel to exactly 0 in the first emission trip only, the last only, every trip, or all of a cell (its
    segment empty, nothing counted for it): the COO launch compacts with its run carried over the trips."""
    run_plan(ctx, capfd, tp.bm_cancel(where), BITMAP, flag)


@pytest.mark.parametrize("emit", ["scalek", "C", "scalei", "all"])
@pytest.mark.parametrize("where", ["first", "every"])
def test_bitmap_absent_columns_and_scales(ctx, capfd, where, emit):
    """scalek with absent columns (the COUNT launch walks the bitmap words, the COO launch stores compacted), alone and
    with cancelled sums in the same cell; C and scalei through the general emit."""
    run_plan(ctx, capfd, tp.bm_cancel(where), BITMAP, "plain", emit)


@pytest.mark.parametrize("emit", ["scalek", "all"])
def test_bitmap_absent_columns_alone(ctx, capfd, emit):
    """scalek on cells none of whose sums cancels, at every distinct-column edge: the stored count is the allowed columns'."""
    run_plan(ctx, capfd, tp.bm_distinct(False), BITMAP, "plain", emit)


# ---- C. items and segments

@pytest.mark.parametrize("flag", ["plain", "exact"])
@pytest.mark.parametrize("scheme", ["bitmap", "hash2"])
def test_items_and_segments(ctx, capfd, scheme, flag):
    """Segment lengths 1, 3, 4, 5, 8, 17 in one cell, tuples without a segment in a cell and tuples whose B row is empty,
    64 k items beside 64 k + 1, and a bitmap cell of 1200 items (19 blocks: the third, unprefetched step) before a small
    one."""
    run_plan(ctx, capfd, tp.segments(), SCHEMES[scheme], flag)


@pytest.mark.parametrize("scheme", ["bitmap", "hash2"])
def test_tile_filled_to_its_item_capacity(ctx, capfd, scheme):
    """Sixteen cells whose costs add up to exactly 8192 items in one tile, and a row whose sixteenth cell no longer fits."""
    run_plan(ctx, capfd, tp.full_tile(), SCHEMES[scheme])


# ---- D. hash tables

@pytest.mark.parametrize("flag", ["plain", "exact", "ordered"])
@pytest.mark.parametrize("scheme", ["hash2", "hash1"])
def test_hash_tile_tables(ctx, capfd, scheme, flag):
    """A cell of 1500 columns whose probe runs wrap from the last slot to the first, one of exactly 2048 distinct columns,
    one with 256 products on one column; ORDERED runs them on the first generation, EXACT_PATTERN on the second."""
    run_plan(ctx, capfd, tp.hash_tiles(), SCHEMES[scheme], flag)


@pytest.mark.parametrize("flag", ["plain", "exact", "ordered"])
@pytest.mark.parametrize("T", tp.HASH_T)
def test_windowed_hash_tables(ctx, capfd, T, flag):
    """The same wrap in each table of the windowed hash cells of a row too long for tiles (3072: the table that is no
    power of two), and 2048 products on one column in the table of 4096."""
    p = tp.hash_windowed(T)
    run_plan(ctx, capfd, p, p.schemes[0], flag)


# ---- E. direct tiles

@pytest.mark.parametrize("scheme", ["bitmap", "hash2"])
def test_direct_cells(ctx, capfd, scheme):
    """Every product its own column (every lane an owner), 1280 products on 5 columns, columns that cancel to exactly 0
    (products without an owner: a rank gap), cells in the first and the last window of the matrix."""
    coo, dig = run_plan(ctx, capfd, tp.direct_cells(), SCHEMES[scheme])
    assert coo.products_direct == coo.products == 5120


# ---- F. sequences

def sequence_rows():
    import torch
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1


@pytest.mark.parametrize("scheme,walk", [("bitmap", 0), ("bitmap", 1), ("hash2", 0), ("hash2", 1), ("hash1", 1)],
                         ids=["bitmap-claimed", "bitmap-static", "hash2-claimed", "hash2-static", "hash1-static"])
def test_tile_sequences(ctx, capfd, scheme, walk):
    """8 x CUs + 1 one-tile rows whose shape changes from each tile to the next (lsh 4 .. 8, 1 .. 16 cells, cells of one
    block and of more than sixteen, one window and sixteen) on column sets that neighbours do not share: a bitmap word,
    accumulator slot, table key or expansion left behind by a tile is a wrong tuple in the next.  Claimed and static walk
    (the first generation never claims); the claimed kernels twice in one context."""
    from spsparse_amd import capi
    nrows = sequence_rows()
    p = tp.sequence("tiles", nrows)
    coo, dig = run_plan(ctx, capfd, p, SCHEMES[scheme], extra={"tile_walk": walk})
    assert coo.rows_heavy == nrows
    if walk == 0:
        keep = []
        a, b, C_, si, sk = operands(p, "plain", keep)
        with Knobs(ctx, dict(p.knobs, tiles_v1=tp.TILES_V1[SCHEMES[scheme]])):
            again = ctx.multiply(a, b, C_, si, ".", None, ".", sk, capi.ADD, False, capi.SINK_DIGEST, 0)
        assert (again.nnz, again.hash, again.sum) == (dig.nnz, dig.hash, dig.sum)


def test_direct_tile_sequence(ctx, capfd):
    """The same for the direct tiles: 8 x CUs + 1 one-tile rows of five shapes on disjoint column sets."""
    nrows = sequence_rows()
    coo, dig = run_plan(ctx, capfd, tp.sequence("direct", nrows), BITMAP)
    assert coo.products_direct == coo.products and coo.rows_heavy == nrows
