"""The plans of tests/dense_plan.py on the CPU: every plan is what it claims, from the operands and the oracle alone.  For
each plan: every row is heavy and the cut (Cut.counters) has the planned dense cells and no tile or hash cell; each planned
cell has the pinned L, items per chunk of NT tuples, batches, empty chunks, batch boundaries, segment lengths and non-empty
lanes; the planned cancellations pair tuples of different chunks or batches; the oracle's output lacks exactly the
cancelled columns.  One test asserts that the catalogue as a whole holds every edge the dense cells' suite is about.  No GPU."""
import numpy as np
import pytest

from tests import dense_plan as dp
from tests import tile_plan as tp
from tests.dense_plan import NT
from tests.tile_plan import BITMAP, HASH1, HASH2
from tests.test_tile_plan_host import row_columns


def check_cut(p):
    """Heavy rows; dense cells only, as many as planned, under every scheme a flag can select; every window none or more
    than dense_min products."""
    for s in (BITMAP, HASH2, HASH1):
        c = p.cut(s)
        assert c.rows_heavy == p.A.shape[0] and all(wp.sum() > tp.MID_MAX for L, wp, cells, tiles in c.rows)
        assert all(np.all((wp == 0) | (wp > dp.DENSE_MIN)) for L, wp, cells, tiles in c.rows)
        k = c.counters()
        assert k["cells_dense"] == p.ndense and k["cells_hash"] == 0 and c.tiles == c.direct_tiles == 0
        assert k["products_dense"] == k["products"] and k["products_tiles"] == k["products_direct"] == 0
        assert p.knobs == {"dense_min": 64, "window": p.W}


def check_values(p):
    i, j, v = tp.oracle_tuples(p)
    assert np.all(v == np.rint(v)) and np.all(v != 0)
    assert np.all((v < 0) == (j % 4 == 3)) and np.any(v < 0)
    assert len(j) == sum(len(c) for c in row_columns(p)) - p.cancelled
    assert np.all(np.abs(p.A.val) <= 3) and np.all(np.abs(p.B.val) <= 3) and np.all(p.B.val != 0)


def check_claims(p):
    for cl in p.claims:
        sh = dp.shape_of(p, cl["row"], cl["window"])
        what = (cl["row"], cl["window"])
        assert sh["L"] == cl["L"] and sh["items"] == cl["items"], (what, sh["L"], sh["items"])
        assert sh["products"] > dp.DENSE_MIN and len(sh["items"]) == -(-cl["L"] // NT[p.W])
        if "bounds" in cl:
            assert sh["bounds"] == cl["bounds"], (what, sh["bounds"])
        else:
            assert all(n <= p.W for n in sh["items"]), what         # one batch a chunk unless the plan says otherwise
        if "lens" in cl:
            assert sh["lens"] == cl["lens"], (what, sh["lens"])
        if "lanes" in cl:
            assert np.array_equal(sh["live"], dp.lane_mask(cl["lanes"], NT[p.W])), what


def check_cancellations(p):
    """Every cancelling pair's columns are absent from the output, their products lie in different chunks or batches, and
    the window that cancels completely emits nothing."""
    if not p.cancelled:
        assert not p.pairs or not any(p.pairs.values())
        return
    i, j, v = tp.oracle_tuples(p)
    zwin = p.B.shape[1] // p.W - 1
    assert not np.any(j // p.W == zwin)                             # one window cancels completely
    dp.degrees(p)
    for r in list(p.pairs)[:3]:
        cols = row_columns(p)[r]
        gone = np.setdiff1d(cols, j[i == r])
        assert len(gone) == len(p.pairs[r]) * (1 + dp.ZCOLS)
        for w in np.unique(gone // p.W):
            for col, places in dp.holder_places(p, r, gone[gone // p.W == w]).items():
                # (in the window that cancels completely a one-chunk plan's pair shares its one batch)
                assert len(places) == 2 and (places[0] != places[1] or w == zwin), (r, col, places)
            assert w == zwin or all(c % p.W >= p.W - dp.MARGIN for c in gone[gone // p.W == w])
    for emit in ("C", "scalei", "scalek", "all"):
        assert not np.any(tp.oracle_tuples(p, emit)[1] // p.W == zwin)


@pytest.mark.parametrize("name", list(dp.CATALOGUE))
def test_plan_is_what_it_claims(name):
    p = dp.plan(name)
    check_cut(p)
    check_values(p)
    check_claims(p)
    if name.endswith("_cancel"):
        assert p.cancelled
        check_cancellations(p)
    else:
        assert not p.cancelled


def test_dense_min_knob_in_the_grouping_model():
    """cells_of_row with the dense_min knob: 65 products are a dense cell, 64 are not; a long row takes the smaller of the
    two thresholds; a value outside 64 .. 4096 is ignored, as heavy_prepare ignores it."""
    wp = np.zeros(8, np.int64)
    wp[[1, 3, 5]] = 65, 64, 5000
    cells, tiles = tp.cells_of_row(10, wp, BITMAP, 8192, dense_min=64)
    assert cells == [("dense", 1, 2, 65), ("tile", 3, 4, 64), ("dense", 5, 6, 5000)]
    assert tp.cells_of_row(10, wp, BITMAP, 8192, dense_min=63)[0] == tp.cells_of_row(10, wp, BITMAP, 8192)[0]
    assert tp.cells_of_row(300, wp, HASH2, 8192, dense_min=64)[0][0] == ("dense", 1, 2, 65)
    wp[1] = 1025
    assert tp.cells_of_row(300, wp, HASH2, 8192, dense_min=4096)[0][0] == ("dense", 1, 2, 1025)      # long_dense_min's default
    assert tp.cells_of_row(256, wp, HASH2, 8192, dense_min=4096)[0][0][0] == "tile"


def planned_shapes(names):
    for name in names:
        p = dp.plan(name)
        for cl in p.claims:
            yield name, p, cl, dp.shape_of(p, cl["row"], cl["window"])


@pytest.mark.parametrize("W", dp.WIDTHS)
def test_catalogue_holds_every_edge(W):
    """Every edge of the groups A to E is attained by some plan of the catalogue at this width (the lists' long forms at
    8192 only): a plan that is simplified later cannot drop one silently."""
    nt = NT[W]
    names = [n for n in dp.CATALOGUE if n.endswith("_%d" % W)]
    shapes = list(planned_shapes(names))
    Ls = {sh["L"] for n, p, cl, sh in shapes}
    # A: the row's tuple count against NT, three items a tuple with a last item of one tuple
    want_L = {nt - 1, nt, nt + 1, 2 * nt + 1, 3 * nt + 1} | ({1, 2, 2 * nt - 1, 2 * nt} if W == 8192 else set())
    assert want_L <= Ls and set(dp.CHUNK_L[W]) <= Ls
    for n, p, cl, sh in shapes:
        if n.startswith("chunk_L") and cl["L"] > 2:
            assert sh["lens"] == {9} and sh["items"][-1] == 3 * (((cl["L"] - 1) % nt) + 1)
    assert dp.shape_of(dp.chunk_edge(513, 8192), 0, 1)["items"] == [1536, 3]
    if W == 8192:
        assert dp.shape_of(dp.plan("chunk_L1_8192"), 0, 1)["lens"] == {4105} and dp.shape_of(dp.plan("chunk_L2_8192"), 0, 1)["lens"] == {2053}
    # B: segment lengths against R and the 64-item block; the longest segment; one column; every column once
    lens = set().union(*[sh["lens"] for n, p, cl, sh in shapes])
    assert set(dp.SEG_LENS) | {W} <= lens
    sl = dp.segment_lengths(dp.seg_lens(W), 0, 1)
    it = (sl + 3) // 4
    assert set(it[sl == 257]) == {65} and set(it[sl == 513]) == {129} and set(it[sl == 5]) == {2} and set(it[sl == 4]) == {1}
    gl = dp.segment_lengths(dp.giant(W), 0, 1)
    assert gl.tolist() == [1, W, 9] and ((gl + 3) // 4).tolist() == [1, {8192: 2048, 16384: 4096}[W], 3]     # the whole window behind one item
    assert dp.shape_of(dp.giant(W), 0, 1)["items"] == [{8192: 2052, 16384: 4100}[W]]
    st = tp.cell_stats(dp.columns(W).A, dp.columns(W).B, 0, 0, 1, W)
    assert (st["products"], st["distinct"]) == (4100, 1)
    st = tp.cell_stats(dp.columns(W).A, dp.columns(W).B, 1, 1, 2, W)
    assert st["products"] == st["distinct"] == W
    # C: every lane pattern in a chunk of NT segments; a wholly empty chunk first, in the middle, last; two in a row
    pats = {cl["lanes"] for n, p, cl, sh in shapes if "lanes" in cl and sh["L"] == nt}
    assert pats == set(dp.LANES) and len(dp.LANES) == 8
    empties = {(tuple(sh["empty"]), len(sh["items"])) for n, p, cl, sh in shapes if n.startswith("empty_") and cl["window"] == 0}
    assert {((0,), 3), ((1,), 3), ((2,), 3), ((1, 2), 4)} <= empties
    assert dp.shape_of(dp.empty_chunks("middle", 8192), 0, 0)["items"] == [1536, 0, 1536]
    # D: W - 1, W, W + 1 items; two and three batches; a boundary inside a segment and one on a first item; a second chunk
    # of two batches between ordinary ones
    single = {sh["items"][0] for n, p, cl, sh in shapes if len(sh["items"]) == 1}
    assert {W - 1, W, W + 1} <= single
    batches = {b for n, p, cl, sh in shapes for b in sh["batches"]}
    assert {0, 1, 2, 3} <= batches
    kinds = {(len(b), k) for n, p, cl, sh in shapes for b in sh["bounds"] for k in b}
    assert {(1, "inside"), (1, "first"), (2, "inside")} <= kinds
    sc = dp.shape_of(dp.second_chunk(W), 0, 1)
    assert sc["batches"] == [1, 2, 1] and sc["bounds"] == [[], ["inside"], []]
    assert dp.shape_of(dp.straddle(8192), 0, 1)["items"] == [9000]
    # E: one cell, fewer cells than workgroups, a list dealt by the static stride, a list cut into XCD parts
    ncells = {k: dp.plan("list_%s_%d" % (k, W)).ndense for k in dp.LISTS if "list_%s_%d" % (k, W) in dp.CATALOGUE}
    assert ncells["few"] == 210 < 256 and 3 * 3 * 256 < ncells["static"] == 2450 < 4096
    if W == 8192:
        assert ncells["one"] == 1 and ncells["parts"] == 4200 >= 4096
        assert dp.plan("list_parts_8192").A.shape[0] * dp.LIST_WINDOWS * dp.LIST_PRODUCTS < 300000


@pytest.mark.parametrize("name", ["list_static_8192", "list_static_16384", "list_parts_8192"])
def test_list_cells_change_shape(name):
    """In a list plan every cell has 66 products (one size key: the sorted list keeps the rows' order inside a window).  Rows
    r .. r + 4 are a one-tuple cell, a three-chunk cell, a cell whose first chunk is empty, a cell whose second chunk is one
    tuple and a cell of NT - 1 tuples, on columns of different residues mod 5.  The rows are a multiple of five and no
    static stride is: under every launch's stride a workgroup's next cell has another shape."""
    p = dp.plan(name)
    W, nt = p.W, NT[p.W]
    c = p.cut(BITMAP)
    assert all(cell[0] == "dense" and cell[3] == dp.LIST_PRODUCTS and cell[3] >> 8 == 0 for L, wp, cells, tiles in c.rows for cell in cells)
    Ls = [1, 2 * nt + 1, nt + dp.LIST_LIVE, nt + 1, nt - 1]
    assert [L for L, wp, cells, tiles in c.rows[:10]] == Ls * 2 and len(set(Ls)) == dp.LIST_PERIOD == 5
    nrows = len(c.rows)
    assert nrows % dp.LIST_PERIOD == 0 and all(len(cells) == dp.LIST_WINDOWS for L, wp, cells, tiles in c.rows)
    shape_of_cell = [r % dp.LIST_PERIOD for w in range(dp.LIST_WINDOWS) for r in range(nrows)]      # the sorted list: window-major, rows in order
    for stride in dp.LIST_STRIDES:
        assert stride % dp.LIST_PERIOD != 0
        assert all(shape_of_cell[i] != shape_of_cell[i + stride] for i in range(len(shape_of_cell) - stride))
    for w in (0, dp.LIST_WINDOWS - 1):
        one, three, late, tail, short = (dp.shape_of(p, r, w) for r in range(5))
        assert one["items"] == [17] and len(three["items"]) == 3 and min(three["items"]) > 0 and late["items"] == [0, dp.LIST_LIVE]
        assert tail["items"] == [dp.LIST_LIVE - 1, 1] and short["items"] == [dp.LIST_LIVE]
        assert three["live"][0] and dp.segment_lengths(p, 1, w)[-1] > 0         # the row's first and last tuple
    cols = row_columns(p)
    for r in range(10):
        assert np.all(cols[r] % W % 5 == r % 5) and len(cols[r]) == dp.LIST_WINDOWS * dp.LIST_PRODUCTS


def test_batch_bounds():
    assert dp.batch_bounds([1500] * 6, 8192) == ["inside"] and dp.batch_bounds([1024] * 9, 8192) == ["first"]
    assert dp.batch_bounds([1500] * 12, 8192) == ["inside", "inside"] and dp.batch_bounds([8192], 8192) == []
    assert dp.batch_bounds([0, 8192, 0, 1], 8192) == ["first"]
