"""The plans of tests/tile_plan.py on the CPU: every plan is what it claims, from the operands and the oracle alone.  For
each plan: every row is heavy; its window histogram gives the planned tiles and cells through cells_of_row (the numbers
pinned here and in the catalogue, not taken from the cut itself); each named edge value is attained exactly; the oracle's
output has the planned tuple count, the planned cancelled columns absent.  No GPU."""
import math

import numpy as np
import pytest

from tests import tile_plan as tp
from tests.tile_plan import BITMAP, HASH1, HASH2


def row_columns(p):
    """Per row of A: the distinct columns its products fall on."""
    lo, hi = tp.row_tuples(p.A)
    blo = np.searchsorted(p.B.idx0, np.arange(p.B.shape[0] + 1))
    memo, out = {}, []
    for r in range(p.A.shape[0]):
        ks = p.A.idx1[lo[r]:hi[r]]
        key = ks.tobytes()
        if key not in memo:
            memo[key] = np.unique(np.concatenate([p.B.idx1[blo[k]:blo[k + 1]] for k in ks]))
        out.append(memo[key])
    return out


def check_common(p):
    """Heavy rows, the pinned cut under every scheme the plan runs, integer values, the oracle's tuple count."""
    for s in p.schemes:
        for coo in (True, False):
            c = p.cut(s, coo)
            assert c.rows_heavy == p.A.shape[0] and all(wp.sum() > tp.MID_MAX for L, wp, cells, tiles in c.rows)
            if coo or s != HASH1:
                assert (c.tiles, c.tile_cells) == p.expect[s], (tp.SCHEME_IDS[s], coo, c.tiles, c.tile_cells)
            for L, wp, cells, tiles in c.rows:                  # no tile beyond its capacity, no cell beyond its kernel's
                cap = tp.TILE_ITEMS if s != HASH1 else (tp.TILE_PB_STORE if coo else tp.TILE_PB)
                assert all(cost <= (cap if kd == "tile" else p.W) for cost, (kd, idx) in zip(tp.tile_costs(L, cells, tiles, s), tiles))
                assert all(len(idx) <= tp.cells_per_tile(L) for kd, idx in tiles)
                assert all(c_[3] <= (tp.BM_MAXOUT if s == BITMAP else tp.HASH_TILE_CAP) for c_ in cells if c_[0] == "tile")
    i, j, v = tp.oracle_tuples(p)
    assert np.all(v == np.rint(v)) and np.all(v != 0)
    assert np.all((v < 0) == (j % 4 == 3)) and np.any(v < 0)      # sums of both signs
    assert len(j) == sum(len(c) for c in row_columns(p)) - getattr(p, "cancelled", 0)
    assert np.all(np.abs(p.A.val) <= 3) and np.all(np.abs(p.B.val) <= 3) and np.all(p.B.val != 0)


@pytest.mark.parametrize("name", list(tp.CATALOGUE))
def test_plan_is_cut_as_pinned(name):
    check_common(tp.plan(name))


def test_cells_of_row_follows_the_grouping_rules():
    """The restated grouping on histograms small enough to cut by hand."""
    wp = np.zeros(40, np.int64)
    wp[[0, 1, 16, 17]] = 1000
    cells, tiles = tp.cells_of_row(64, wp, BITMAP, 8192)          # span cap: window 16 is the 17th from window 0
    assert cells == [("tile", 0, 2, 2000), ("tile", 16, 18, 2000)] and tiles == [("tile", [0, 1])]
    cells, tiles = tp.cells_of_row(64, wp, HASH2, 8192)           # 2048 products: 1000 + 1000, no span cap
    assert cells == [("tile", 0, 2, 2000), ("tile", 16, 18, 2000)]
    wp[1] = 1049
    assert tp.cells_of_row(64, wp, HASH2, 8192)[0] == [("tile", 0, 1, 1000), ("tile", 1, 2, 1049), ("tile", 16, 18, 2000)]      # 2049 > 2048, twice
    assert tp.cells_of_row(64, wp, BITMAP, 16384)[0][0] == ("tile", 0, 2, 2049)
    assert tp.cells_of_row(64, wp, BITMAP, 16384)[0][1][1] == 16                # W = 16384: 8 windows a cell, 0 .. 7
    wp[5] = 3072
    assert ("dense", 5, 6, 3072) in tp.cells_of_row(64, wp, HASH2, 8192)[0] and ("dense", 5, 6, 3072) not in tp.cells_of_row(64, wp, BITMAP, 8192)[0]
    wp[5] = 3073
    assert ("dense", 5, 6, 3073) in tp.cells_of_row(64, wp, BITMAP, 8192)[0]
    assert ("direct", 0, 1, 1000) not in tp.cells_of_row(64, wp, BITMAP, 8192, direct_min=1000)[0]
    assert ("direct", 1, 2, 1049) in tp.cells_of_row(64, wp, BITMAP, 8192, direct_min=1000)[0]
    long_ = tp.cells_of_row(257, wp, BITMAP, 8192)[0]              # too long for tiles: dense from 1025 products on
    assert ("dense", 1, 2, 1049) in long_ and ("hash1024", 0, 1, 1000) not in long_ and long_[0] == ("hash3072", 0, 1, 1000)
    assert tp.cells_per_tile(1) == 16 and tp.cells_per_tile(32) == 16 and tp.cells_per_tile(33) == 8 and tp.cells_per_tile(129) == 2 == tp.cells_per_tile(256)
    assert tp.item_cost(1500, 32) == 512 and tp.item_cost(1700, 32) == 576


def test_hash_and_key_functions():
    """hash_slot<T> and tile_key / tile_rel as the kernels compute them: ranges, the multiply-shift of 3072, inverses."""
    cols = np.arange(1 << 17)
    for T in (1024, 3072, 4096, 8192):
        h = tp.hash_slot(T, cols)
        assert h.min() == 0 and h.max() == T - 1
        assert tp.hash_slot(T, 1) == ((0x9E3779B1 * T) >> 32 if T == 3072 else 0x9E3779B1 >> (32 - int(math.log2(T))))
    assert tp.hash_slot(4096, 2 ** 31 + 5) == ((2 ** 31 + 5) * 0x9E3779B1 % 2 ** 32) >> 20
    k = tp.tile_key(cols)
    assert np.array_equal(np.sort(k), cols) and np.array_equal(tp.tile_rel(k), cols)
    assert np.array_equal(k >> 14, cols >> 14)                      # a key stays in its column's 256 bitmap words


@pytest.mark.parametrize("L", tp.L_CLASSES + (257,))
def test_class_plan(L):
    p = tp.l_class(L)
    G = tp.cells_per_tile(min(L, 256))
    assert G == {1: 16, 2: 16, 3: 16, 31: 16, 32: 16, 33: 8, 63: 8, 64: 8, 65: 4, 128: 4, 129: 2, 255: 2, 256: 2, 257: 2}[L]
    for s in (BITMAP, HASH2):
        c = p.cut(s)
        if L == 257:
            assert c.products_tiles == 0 and c.cells_windowed == 3 and c.cells_dense == 2
            assert [[cell[0] for cell in row[2]] for row in c.rows] == [["hash4096", "dense"], ["hash4096", "hash3072", "dense"]]
            continue
        (L0, wp0, cells0, tiles0), (L1, wp1, cells1, tiles1) = c.rows
        assert [len(idx) for kd, idx in tiles0] == [G] and [len(idx) for kd, idx in tiles1] == [G, 1]
        assert all(cell[3] == tp.CLASS_CELL and cell[2] == cell[1] + 1 for cell in cells0 + cells1 if cell[0] == "tile")
    if L <= 256:
        st = tp.cell_stats(p.A, p.B, 0, 0, 1)
        assert st["nonempty"] == L and st["products"] == st["distinct"] == tp.CLASS_CELL      # every lane ei < L of the cell has a segment
        assert tp.lsh_of(L) == {1: 0, 2: 1, 3: 2, 31: 5, 32: 5, 33: 6, 63: 6, 64: 6, 65: 7, 128: 7, 129: 8, 255: 8, 256: 8}[L]


def test_bitmap_distinct_plans():
    p = tp.bm_distinct(False)
    cells = p.cut(BITMAP).rows[0][2]
    st = [tp.cell_stats(p.A, p.B, 0, wa, wb) for kd, wa, wb, prods in cells]
    assert [x["distinct"] for x in st] == list(tp.BM_DISTINCT) == [x["products"] for x in st]
    assert tp.BM_DISTINCT[-1] == tp.BM_MAXOUT                       # acc and colof full
    p = tp.bm_distinct(True)
    cells = p.cut(BITMAP).rows[0][2]
    st = [tp.cell_stats(p.A, p.B, 0, wa, wb) for kd, wa, wb, prods in cells]
    assert [(x["products"], x["distinct"]) for x in st] == [(1792, 7), (4096, 4096), (1792, 7), (256, 1)]


@pytest.mark.parametrize("W", [8192, 16384])
def test_bitmap_range_plan(W):
    p = tp.bm_range(W)
    wshift = {8192: 13, 16384: 14}[W]
    span = {8192: 16, 16384: 8}[W]
    cells = p.cut(BITMAP).rows[0][2]
    assert [c[:3] for c in cells[:2]] == [("tile", 1, 1 + span), ("tile", 1 + span, 2 + span)]     # the next window starts a new cell
    assert ((cells[0][2] - cells[0][1]) << (wshift - 6)) == tp.BM_WORDS == 2048                  # nwords
    st = tp.cell_stats(p.A, p.B, 0, 1, 1 + span, W)
    assert st["columns"][0] == W and st["columns"][-1] == (1 + span) * W - 1                   # first column of the first window, last of the last
    keys = tp.tile_key(st["columns"] - W)
    assert keys.min() < 64 * 256 and keys.max() >= 64 * (2048 - 256)                           # keys in the first and the last wave's words


@pytest.mark.parametrize("where", tp.CANCELS)
def test_bitmap_cancel_plan(where):
    p = tp.bm_cancel(where)
    cells = p.cut(BITMAP).rows[0][2]
    st = [tp.cell_stats(p.A, p.B, 0, wa, wb) for kd, wa, wb, prods in cells]
    assert [x["distinct"] for x in st] == [1537] * 3
    assert not np.any(st[0]["sums"] == 0) and not np.any(st[2]["sums"] == 0)
    zero = np.flatnonzero(st[1]["sums"] == 0)
    trips = sorted(set((zero // tp.TRIP).tolist()))
    assert trips == {"first": [0], "last": [3], "every": [0, 1, 2, 3], "all": [0, 1, 2, 3]}[where]
    assert len(zero) == p.cancelled == {"first": 3, "last": 1, "every": 8, "all": 1537}[where]
    gone = st[1]["columns"][zero]
    for emit in p.emits:
        assert not np.any(np.isin(gone, tp.oracle_tuples(p, emit)[1]))
    assert len(tp.oracle_tuples(p, "scalek")[1]) < len(tp.oracle_tuples(p)[1])


def test_segments_plan():
    p = tp.segments()
    c = p.cut(BITMAP)
    cells0, cells1 = c.rows[0][2], c.rows[1][2]
    st = [tp.cell_stats(p.A, p.B, 0, wa, wb) for kd, wa, wb, prods in cells0 if kd == "tile"]
    assert set(st[0]["lens"].tolist()) == set(tp.SEG_LENS) | {0}
    assert st[1]["nonempty"] == 16 and (st[1]["lens"] == 0).sum() == 32
    assert st[2]["items"] == 256 and st[3]["items"] == 257                      # 64 k and 64 k + 1
    deg = np.bincount(p.B.idx0, minlength=p.B.shape[0])
    assert (deg[:48] == 0).sum() == 16                                          # A tuples whose B row is empty
    long_ = tp.cell_stats(p.A, p.B, 1, cells1[0][1], cells1[0][2])
    assert (long_["products"], long_["items"], long_["nonempty"]) == (4080, 1200, 240) and set(long_["lens"].tolist()) == {17}
    assert (long_["items"] + 63) // 64 == 19 > 16                               # blocks: waves 0 .. 2 take a third step
    assert cells1[0][2] - cells1[0][1] == 2 and len(c.rows[1][3]) == 1 and len(cells1) == 2


def test_full_tile_plan():
    p = tp.full_tile()
    for s in (BITMAP, HASH2):
        c = p.cut(s)
        costs = [tp.tile_costs(L, cells, tiles, s) for L, wp, cells, tiles in c.rows]
        assert costs == [[8192], [7680, 576]] and tp.TILE_ITEMS == 8192
        assert [len(idx) for kd, idx in c.rows[0][3]] == [16] and [len(idx) for kd, idx in c.rows[1][3]] == [15, 1]


def wraps(T, cols):
    """The columns' home slots are the table's last two and first two, with more at the end than there are slots left."""
    h = tp.hash_slot(T, cols)
    return set(h.tolist()) == {T - 2, T - 1, 0, 1} and (h >= T - 2).sum() > 2


def test_hash_tile_plan():
    p = tp.hash_tiles()
    for s in (HASH2, HASH1):
        c = p.cut(s)
        cl = [cell for cell in c.rows[0][2] if cell[0] == "tile"]
        assert len(cl) == 1 and cl[0][3] == tp.NCLUSTER >= 1500
        st = tp.cell_stats(p.A, p.B, 0, cl[0][1], cl[0][2])
        assert st["distinct"] == tp.NCLUSTER and wraps(4096, st["columns"])
        full = [cell for cell in c.rows[1][2] if cell[0] == "tile"]
        st = tp.cell_stats(p.A, p.B, 1, full[0][1], full[0][2])
        assert len(full) == 1 and st["distinct"] == st["products"] == 2048 == tp.HASH_TILE_CAP
        one, seven = [tp.cell_stats(p.A, p.B, 2, cell[1], cell[2]) for cell in c.rows[2][2] if cell[0] == "tile"]
        assert (one["products"], one["distinct"]) == (356, 101) and (seven["products"], seven["distinct"]) == (1792, 7)


@pytest.mark.parametrize("T", tp.HASH_T)
def test_hash_windowed_plan(T):
    p = tp.hash_windowed(T)
    c = p.cut(p.schemes[0])
    cells = c.rows[0][2]
    assert [cell[0] for cell in cells] == ["hash%d" % T, "dense"] and c.products_tiles == 0
    st = tp.cell_stats(p.A, p.B, 0, cells[0][1], cells[0][2])
    assert st["products"] <= T // 2 and st["products"] > {1024: 0, 3072: 512, 4096: 1536, 8192: 2048}[T]
    home = tp.hash_slot(T, st["columns"])
    assert wraps(T, st["columns"][(home >= T - 2) | (home <= 1)]) and ((home >= T - 2) | (home <= 1)).sum() == tp.WINDOWED[T]
    if T == 4096:
        cells = c.rows[1][2]
        st = tp.cell_stats(p.A, p.B, 1, cells[0][1], cells[0][2])
        assert cells[0][0] == "hash4096" and (st["products"], st["distinct"]) == (2048, 1)


def test_direct_plan():
    p = tp.direct_cells()
    for s in p.schemes:
        c = p.cut(s)
        cells = c.rows[0][2]
        assert [cell[0] for cell in cells] == ["direct"] * 4 and (c.direct_tiles, c.products_direct) == (2, 5120)
        assert cells[0][1] == 0 and cells[3][2] == p.B.shape[1] // 8192                # first and last window of the matrix
        st = [tp.cell_stats(p.A, p.B, 0, cell[1], cell[2]) for cell in cells]
        assert [(x["products"], x["distinct"]) for x in st] == [(1280, 1280), (1280, 5), (1280, 640), (1280, 1280)]
        assert (st[2]["sums"] == 0).sum() == p.cancelled == 100 and st[0]["columns"][0] == 0 and st[3]["columns"][-1] == p.B.shape[1] - 1


def test_cut_without_direct_cells_has_none():
    p = tp.direct_cells()
    assert tp.Cut(p.A, p.B, BITMAP, p.W).direct_cells == 0


@pytest.mark.parametrize("kind", ["tiles", "direct"])
def test_sequence_plan(kind):
    """8 x 256 + 1 rows (an MI355X has 256 CUs): one tile a row under every scheme, five shapes, the period coprime to every
    grid, neighbours on disjoint columns."""
    nrows = 8 * 256 + 1
    p = tp.sequence(kind, nrows)
    check_common(p)
    shapes = tp.sequence_shapes(kind)
    assert len(shapes) == tp.PERIOD == 5 and sorted(tp.lsh_of(L) for L, cells in shapes) == [4, 5, 6, 7, 8]
    for grid in (256, 512, 768, 1024):                              # 2 x CUs (bitmap, direct) and 1 .. 4 resident workgroups x CUs
        assert math.gcd(tp.PERIOD, grid) == 1
    assert math.gcd(tp.PERIOD, 3) == 1
    for s in p.schemes:
        c = p.cut(s)
        per_row = [[len(idx) for kd, idx in tiles] for L, wp, cells, tiles in c.rows]
        assert all(len(t) == 1 for t in per_row)                    # one tile a row
        if kind == "tiles":
            assert tuple(t[0] for t in per_row[:5]) == tp.SEQUENCE_TILE_CELLS[s] and c.tiles == nrows
            assert all(cells[0][1] == 0 for L, wp, cells, tiles in c.rows)      # every tile starts in window 0: the sorted list keeps the rows' order
        else:
            assert c.direct_tiles == nrows and c.products_direct == c.products
    cols = row_columns(p)
    for r in range(10):
        assert np.all(cols[r] % tp.PERIOD == r % tp.PERIOD)         # shape s on columns = s (mod 5)
    if kind == "tiles":
        c = p.cut(BITMAP)
        items = [[tp.cell_stats(p.A, p.B, r, cell[1], cell[2])["items"] for cell in c.rows[r][2] if cell[0] == "tile"] for r in range(5)]
        assert max(items[0]) <= 128 and min(items[1][:2]) > 16 * 64 // 4 and items[4][1] <= 64       # small cells, cells of many blocks, a one-block cell
        spans = {cell[2] - cell[1] for r in range(5) for cell in c.rows[r][2] if cell[0] == "tile"}
        assert spans == {1, 16}
