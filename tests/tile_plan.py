"""Planned tiles for the four tile kernels (k_bm_tiles, k_hash_tiles2, k_direct_tiles, k_hash_tiles): a plain-Python
restatement of the cell grouping, builders that make operands whose heavy rows fall into chosen cells, the hash and key
functions of the kernels in numpy, and the catalogue of plans that tests/test_tile_plan_host.py checks on the CPU and
tests/test_gpu_tile_shapes.py runs on the GPU.  Importing it needs no GPU.

All values are small integers (A in 1 .. 3, B in 1 .. 3 with a sign by column, planned cancellations in pairs + / -): every sum is exact in any
order, so a result compares bit for bit with the oracle."""
import functools
import math

import numpy as np

from oracle import binding as orc

# ---- the constants of csrc/spgemm_dev.h that the grouping uses
R = 4                                   # DENSE_R: B tuples of one item
MID_MAX = 4096                          # a row above MID_MAX products is heavy
TILE_LMAX, TILE_NT, TILE_MAXCELLS = 256, 512, 16
BM_MAXOUT, HASH_TILE_CAP = 4096, 2048   # products of a bitmap cell / of a hash tile's cell (TILE_T / 2)
DENSE_MIN_BITMAP, DENSE_MIN_DEFAULT, LONG_DENSE_MIN_DEFAULT = 3072, 2048, 1024
CELL_CAP_DEFAULT, DIRECT_MIN_DEFAULT = 2048, 4096
BM_WORDS = 2048                         # 64-bit words of the bitmap: 131072 columns
TILE_ITEMS = 8192                       # TILE2_ITEMS, BM_ITEMS
TILE_PB, TILE_PB_STORE = 16384, 12288   # products of a first-generation tile: digest sink / COO sink
BITMAP, HASH1, HASH2 = 0, 1, 2          # heavy_prepare's set_scheme
TILES_V1 = {BITMAP: 3, HASH1: 1, HASH2: 2}      # ... and the "tiles_v1" knob value that forces each
SCHEME_IDS = {BITMAP: "bitmap", HASH1: "hash1", HASH2: "hash2"}
HASH_T = (1024, 3072, 4096, 8192)       # tables of the windowed k_hash launches, by hash_class


def hash_class(prods):
    return 0 if prods <= 512 else (1 if prods <= 1536 else (2 if prods <= 2048 else 3))


def lsh_of(L):
    lsh = 0
    while (1 << lsh) < L:
        lsh += 1
    return lsh


def cells_per_tile(L):
    """G: the cells one tile of a row with L A tuples holds."""
    return min(TILE_NT >> lsh_of(L), TILE_MAXCELLS)


def item_cost(prods, L):
    """A cell's cost against a tile's TILE_ITEMS (or a direct tile's W) items."""
    return ((prods // R + L + 63) & ~63) + 64


def cells_of_row(L, window_products, scheme, W, direct_min=None, coo=True, no_tiles=False, long_cap=0, long_dense_min=None, dense_min=None):
    """k_cells (csrc/symbolic_heavy.hip) for one row of L A tuples and its products per column window, under the limits
    heavy_prepare sets for a scheme.  direct_min: the knob (None: direct cells off, their default); coo: the COO sink
    (the first generation's tiles then hold fewer products); long_cap, long_dense_min: the knobs for rows too long for
    tiles; dense_min: the knob (64 .. 4096, else the scheme's default).  Returns (cells, tiles): cells in the row's order as
    (kind, wa, wb, products), kind one of "tile", "direct", "dense", "hash1024" .. "hash8192"; tiles as (kind, [indices
    into cells])."""
    wshift = {8192: 13, 16384: 14}[W]
    tiles_on = not no_tiles
    tileable = tiles_on and L <= TILE_LMAX
    user_dense_min = dense_min is not None and 64 <= dense_min <= 4096
    dense_min = dense_min if user_dense_min else (DENSE_MIN_BITMAP if scheme == BITMAP and tiles_on else DENSE_MIN_DEFAULT)
    tile_cap = BM_MAXOUT if scheme == BITMAP else HASH_TILE_CAP
    span_cap = BM_WORDS >> (wshift - 6) if scheme == BITMAP else 0
    pb = {"tile": TILE_ITEMS if scheme != HASH1 else (TILE_PB_STORE if coo else TILE_PB), "direct": W}
    by_items = {"tile": scheme != HASH1, "direct": True}
    dmin = direct_min if direct_min else DIRECT_MIN_DEFAULT
    direct_ok = tileable and dmin < dense_min
    cell_cap = CELL_CAP_DEFAULT
    if tileable and tile_cap > cell_cap:
        cell_cap = tile_cap
    if not tileable and long_cap > cell_cap:
        cell_cap = min(long_cap, 4096)
    ldm = (LONG_DENSE_MIN_DEFAULT if W == 8192 else 0) if not long_dense_min else long_dense_min
    if not tileable and ldm and ldm < dense_min:
        dense_min = ldm
    G = cells_per_tile(L)
    cells, tiles = [], []
    open_ = {"tile": None, "direct": None}            # the open tile of each kind: [cell indices, cost]

    def close_tile(kd):
        if open_[kd]:
            tiles.append((kd, open_[kd][0]))
        open_[kd] = None

    def tile_cell(kd, wa, wb, prods):
        cost = item_cost(prods, L) if by_items[kd] else prods
        if open_[kd] and (len(open_[kd][0]) == G or open_[kd][1] + cost > pb[kd]):
            close_tile(kd)
        if not open_[kd]:
            open_[kd] = [[], 0]
        open_[kd][0].append(len(cells))
        open_[kd][1] += cost
        cells.append((kd, wa, wb, prods))

    cur = start = last = 0

    def flush():
        nonlocal cur
        if not cur:
            return
        if tileable and cur <= tile_cap:
            tile_cell("tile", start, last + 1, cur)
        else:
            cells.append(("hash%d" % HASH_T[hash_class(cur)], start, last + 1, cur))
        cur = 0

    for w, c in enumerate(window_products):
        c = int(c)
        if c > dense_min:
            flush()
            cells.append(("dense", w, w + 1, c))
        elif direct_ok and c > dmin:
            flush()
            tile_cell("direct", w, w + 1, c)
        elif c > cell_cap:
            flush()
            cur, start, last = c, w, w
            flush()
        elif c > 0:
            if cur + c > cell_cap or (cur and tileable and span_cap and w - start >= span_cap):
                flush()
            if not cur:
                start = w
            cur += c
            last = w
    flush()
    close_tile("tile")
    close_tile("direct")
    return cells, tiles


def tile_costs(L, cells, tiles, scheme):
    """The summed cost of every tile against its capacity (items, or products in the first generation)."""
    return [sum(item_cost(cells[i][3], L) if (kd == "direct" or scheme != HASH1) else cells[i][3] for i in idx) for kd, idx in tiles]


# ---- the kernels' hash and key functions

def hash_slot(T, col):
    """hash_slot<T> (csrc/spgemm_hash.h): multiplicative hash; shift for a power of two, multiply-shift for 3072."""
    h = (np.asarray(col, np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    if T & (T - 1) == 0:
        return (h >> np.uint64(32 - int(math.log2(T)))).astype(np.int64)
    return ((h * np.uint64(T)) >> np.uint64(32)).astype(np.int64)


TILE_KEY_LOW, TILE_KEY_K, TILE_KEY_KINV = (1 << 14) - 1, 40503, 96135


def tile_key(rel):
    rel = np.asarray(rel, np.int64)
    return rel ^ ((rel ^ (rel * TILE_KEY_K)) & TILE_KEY_LOW)


def tile_rel(key):
    key = np.asarray(key, np.int64)
    return key ^ ((key ^ (key * TILE_KEY_KINV)) & TILE_KEY_LOW)


def wrap_cluster(T, n, ncol, first=0):
    """The first n columns from `first` on whose home slot in a table of T is one of its last two or first two: inserted
    in any order they fill a run of slots that passes T - 1 and goes on at 0."""
    cols = np.arange(first, ncol)
    h = hash_slot(T, cols)
    cols = cols[(h >= T - 2) | (h <= 1)]
    assert cols.size >= n, (T, n, cols.size)
    return cols[:n]


# ---- operands from a specification

class Builder:
    """Heavy rows given by their B segments.  row(segs): one row of A with L = len(segs) tuples; segs[e] holds the columns
    of the B row that A tuple e selects (that B row belongs to this A tuple alone).  cancel: columns whose sum in this row
    must be exactly 0 -- each held by an even number of the row's tuples, whose B values then pair off as + a', - a.
    again(r): one more row of A on the B rows of row r, with r's values.  A values 1 + (seed + 2 e) % 3, B values
    1 + (column + B row) % 3, negative in the columns = 3 (mod 4): sums of both signs, none that cancels unplanned."""

    def __init__(self, nwin, W=8192):
        self.W, self.nwin, self.ncol = W, nwin, nwin * W
        self.rows = []                  # (first B row, L, A values)
        self.bcols, self.bvals = [], []

    def row(self, segs, cancel=(), seed=0):
        k0, L = len(self.bcols), len(segs)
        a = 1.0 + (seed + 2 * np.arange(L)) % 3
        holders = {}
        for e, s in enumerate(segs):
            s = np.unique(np.asarray(s, np.int64))
            assert s.size == len(segs[e]) and (s.size == 0 or (s[0] >= 0 and s[-1] < self.ncol)), "segment %d: columns" % e
            self.bcols.append(s)
            self.bvals.append(np.where(s % 4 == 3, -1.0, 1.0) * (1.0 + (s + k0 + e) % 3))
        for j in cancel:
            hs = [e for e in range(L) if np.any(self.bcols[k0 + e] == j)]
            assert hs and len(hs) % 2 == 0, "column %d: %d holders" % (j, len(hs))
            for h0, h1 in zip(hs[::2], hs[1::2]):
                self.bvals[k0 + h0][self.bcols[k0 + h0] == j] = a[h1]
                self.bvals[k0 + h1][self.bcols[k0 + h1] == j] = -a[h0]
            holders[j] = hs
        self.rows.append((k0, L, a))
        return len(self.rows) - 1

    def again(self, r):
        self.rows.append(self.rows[r])
        return len(self.rows) - 1

    def operands(self):
        nb = len(self.bcols)
        ai = np.concatenate([np.full(L, r) for r, (k0, L, a) in enumerate(self.rows)])
        ak = np.concatenate([k0 + np.arange(L) for k0, L, a in self.rows])
        av = np.concatenate([a for k0, L, a in self.rows])
        bk = np.concatenate([np.full(len(s), k) for k, s in enumerate(self.bcols)])
        A = orc.Mat(ai, ak, av, (len(self.rows), nb))
        B = orc.Mat(bk, np.concatenate(self.bcols), np.concatenate(self.bvals), (nb, self.ncol))
        return A, B


def deal(L, cols, products=None):
    """`products` products (default: one per column) of one cell on the distinct columns `cols`, dealt to L tuples in runs
    of consecutive columns (cyclically): every column is taken, no tuple takes one twice.  Returns the L segments."""
    cols = np.asarray(cols, np.int64)
    D = cols.size
    P = D if products is None else products
    assert P >= D and P <= L * D
    lens = np.full(L, P // L) + (np.arange(L) < P % L)
    segs, off = [], 0
    for n in lens:
        segs.append(cols[(off + np.arange(n)) % D])
        off += n
    return segs


def spread(n, lo, hi):
    """n distinct columns of [lo, hi) at even steps, lo and hi - 1 among them (n >= 2)."""
    if n == 1:
        return np.asarray([lo], np.int64)
    return np.unique(lo + (np.arange(n, dtype=np.int64) * (hi - 1 - lo)) // (n - 1))


def join(*cells):
    """The segments of one row from its cells' segments (each a list of L segments)."""
    return [np.concatenate([c[e] for c in cells]) for e in range(len(cells[0]))]


# ---- what a product is cut into

@functools.lru_cache(maxsize=None)
def _degrees(B_id, nwin, wshift):
    B = _KEEP[B_id]
    deg = np.zeros((B.shape[0], nwin), np.int64)
    np.add.at(deg, (B.idx0, B.idx1 >> wshift), 1)
    return deg


_KEEP = {}


def row_tuples(A):
    """Per row of A (rows sorted, as the builder makes them): (first, one past last) of its tuples."""
    beg = np.searchsorted(A.idx0, np.arange(A.shape[0] + 1))
    return beg[:-1], beg[1:]


def window_histograms(A, B, W):
    """Per row of A: L and the products per column window."""
    wshift = {8192: 13, 16384: 14}[W]
    nwin = (B.shape[1] + W - 1) >> wshift
    _KEEP[id(B)] = B
    deg = _degrees(id(B), nwin, wshift)
    lo, hi = row_tuples(A)
    out, memo = [], {}
    for r in range(A.shape[0]):
        key = A.idx1[lo[r]:hi[r]].tobytes()
        if key not in memo:
            memo[key] = deg[A.idx1[lo[r]:hi[r]]].sum(axis=0)
        out.append((int(hi[r] - lo[r]), memo[key]))
    return out


class Cut:
    """The cut of a whole product: per row its cells and tiles, and the counters a result reports."""

    def __init__(self, A, B, scheme, W=8192, **kw):
        self.rows, memo = [], {}
        for L, wp in window_histograms(A, B, W):
            key = (L, wp.tobytes())
            if key not in memo:
                memo[key] = cells_of_row(L, wp, scheme, W, **kw)
            self.rows.append((L, wp) + memo[key])
        self.scheme = scheme
        self.rows_heavy = sum(1 for L, wp, c, t in self.rows if wp.sum() > MID_MAX)
        kinds = [c[0] for L, wp, cells, t in self.rows for c in cells]
        prods = lambda kind: sum(c[3] for L, wp, cells, t in self.rows for c in cells if c[0] == kind)      # noqa: E731
        self.tiles = sum(1 for L, wp, c, tiles in self.rows for t in tiles if t[0] == "tile")
        self.direct_tiles = sum(1 for L, wp, c, tiles in self.rows for t in tiles if t[0] == "direct")
        self.tile_cells, self.direct_cells, self.cells_dense = kinds.count("tile"), kinds.count("direct"), kinds.count("dense")
        self.cells_windowed = len(kinds) - self.tile_cells - self.direct_cells - self.cells_dense
        self.products_tiles, self.products_direct, self.products_dense = prods("tile"), prods("direct"), prods("dense")
        self.products = sum(int(wp.sum()) for L, wp, c, t in self.rows)

    def counters(self):
        return dict(rows_heavy=self.rows_heavy, products=self.products, products_tiles=self.products_tiles,
                    products_direct=self.products_direct, products_dense=self.products_dense, cells_dense=self.cells_dense,
                    cells_hash=self.tile_cells + self.direct_cells + self.cells_windowed)


def cell_stats(A, B, r, wa, wb, W=8192):
    """One cell of row r, from the operands: products, distinct columns, items (sum of ceil(len / R)), non-empty
    segments, the segment lengths, and (columns, exact sums) of its outputs."""
    lo, hi = row_tuples(A)
    blo = np.searchsorted(B.idx0, np.arange(B.shape[0] + 1))
    lens, cols, vals = [], [], []
    for e in range(lo[r], hi[r]):
        k = A.idx1[e]
        j, v = B.idx1[blo[k]:blo[k + 1]], B.val[blo[k]:blo[k + 1]]
        m = (j >= wa * W) & (j < wb * W)
        lens.append(int(m.sum())); cols.append(j[m]); vals.append(A.val[e] * v[m])
    lens = np.asarray(lens)
    cols, vals = np.concatenate(cols), np.concatenate(vals)
    u, inv = np.unique(cols, return_inverse=True)
    sums = np.zeros(u.size)
    np.add.at(sums, inv, vals)
    return dict(products=int(lens.sum()), distinct=int(u.size), items=int(((lens + R - 1) // R).sum()),
                nonempty=int((lens > 0).sum()), lens=lens, columns=u, sums=sums)


# ---- the plans -----------------------------------------------------------------------------------------------------
# A plan: operands, the knobs and schemes it runs under, and what it claims (checked on the CPU from the operands).

STRIDE = 16                             # windows from one planned cell's first window to the next one's (the bitmap span cap at W = 8192)
DENSE_FILL = 3100                       # products of the dense window that makes a row heavy whatever its tile cells hold


class Plan:
    def __init__(self, b, schemes=(BITMAP, HASH2, HASH1), knobs=None, flags=("plain",), emits=("plain",), expect=None, **cut_kw):
        self.A, self.B = b.operands()
        self.W, self.schemes, self.flags, self.emits = b.W, schemes, flags, emits
        self.knobs = dict(knobs or {}, window=b.W)
        self.cut_kw = cut_kw            # direct_min, long_cap, long_dense_min, no_tiles: as the knobs say
        self.expect = expect or {}      # scheme -> (tiles, tile cells) for the COO sink: pinned by the host test

    def cut(self, scheme, coo=True):
        return Cut(self.A, self.B, scheme, self.W, coo=coo, **self.cut_kw)


def window_cols(w, W=8192, margin=0):
    """(first column, one past the last) of window w; margin: columns kept free at its end."""
    return w * W, (w + 1) * W - margin


def dense_window(L, w, W=8192, n=DENSE_FILL):
    """n products in window w, every column its own: a dense cell under every scheme."""
    lo, hi = window_cols(w, W)
    return deal(L, spread(n, lo, hi))


L_CLASSES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 128, 129, 255, 256)
CLASS_CELL = 1100                       # products of a class plan's cell: two of them pass a hash cell's 2048, one window is below every dense threshold


@functools.lru_cache(maxsize=None)
def l_class(L):
    """Two rows of L tuples: G cells in windows 0, 16, 32, .. (one tile: a window gap ends a bitmap cell, the product sum
    a hash cell), and G + 1 cells (the last one opens the row's second tile); a dense window makes either row heavy.  At
    L = 257 the cells hold 1000 products (below the long rows' dense threshold) and go to the windowed hash cells."""
    G = cells_per_tile(min(L, 256))
    b = Builder((TILE_MAXCELLS + 2) * STRIDE)
    per = CLASS_CELL if L <= 256 else 1000
    for n in (G, G + 1):
        cells = [deal(L, spread(per, *window_cols(STRIDE * i, margin=8)) + (i % 5)) for i in range(n)]
        b.row(join(*cells, dense_window(L, (TILE_MAXCELLS + 1) * STRIDE)), seed=n)
    if L > 256:
        return Plan(b, expect={s: (0, 0) for s in (BITMAP, HASH2, HASH1)})
    # the first generation counts products: a tile of a COO call ends at 12288 of them, after 11 of these cells, so its
    # rows of 16 and 17 cells are two tiles each
    return Plan(b, expect={BITMAP: (3, 2 * G + 1), HASH2: (3, 2 * G + 1), HASH1: (3 if G <= 8 else 4, 2 * G + 1)})


BM_DISTINCT = (1, 511, 512, 513, 1024, 1025, 1536, 1537, 4095, 4096)


def bm_cell(L, w0, distinct, products=None, nwin=2, shift=0):
    """A bitmap cell from window w0 on: `distinct` columns spread over nwin windows (each window below the dense
    threshold), `products` products dealt to L tuples."""
    lo, hi = w0 * 8192 + shift, (w0 + nwin) * 8192
    return deal(L, spread(distinct, lo, hi), products)


@functools.lru_cache(maxsize=None)
def bm_distinct(few):
    """One row of 64 tuples, a bitmap cell for every count of BM_DISTINCT (the emission loop's trip edges; 4096 fills
    acc and colof), every product its own column.  few: instead one row of 256 tuples whose cells hold 1792 products on
    7 columns (a tile row has at most 256 products on a column) beside cells of 1 and 4096 distinct columns."""
    b = Builder(12 * STRIDE)
    if not few:
        cells = [bm_cell(64, STRIDE * i, d) for i, d in enumerate(BM_DISTINCT)]
        b.row(join(*cells))
        return Plan(b, schemes=(BITMAP,), expect={BITMAP: (2, 10)}, flags=("plain", "exact"))
    cells = [bm_cell(256, 0, 7, 1792), bm_cell(256, STRIDE, 4096, 4096), bm_cell(256, 2 * STRIDE, 7, 1792, shift=5), bm_cell(256, 3 * STRIDE, 1, 256)]
    b.row(join(*cells))
    return Plan(b, schemes=(BITMAP,), expect={BITMAP: (2, 4)}, flags=("plain", "exact"))


@functools.lru_cache(maxsize=None)
def bm_range(W):
    """A cell whose columns go from the first of window 1 to the last of window 1 + span - 1 (span = 16 windows of 8192,
    8 of 16384: all 2048 bitmap words); the row's next window, the span cap's 17th (9th), starts a new cell."""
    span = BM_WORDS * 64 // W
    b = Builder(2 * span + 4, W)
    L = 80
    full = deal(L, spread(2600, W, (1 + span) * W))
    nxt = deal(L, spread(1400, (1 + span) * W, (2 + span) * W))
    b.row(join(full, nxt, dense_window(L, 2 * span + 3, W)))
    return Plan(b, schemes=(BITMAP,), expect={BITMAP: (1, 2)}, flags=("plain", "exact"))


TRIP = 512                              # ranks of one trip of the COO emission loop (a digest trip takes two of them)
CANCELS = ("first", "last", "every", "all")


@functools.lru_cache(maxsize=None)
def bm_cancel(where):
    """One row of 64 tuples, three bitmap cells of 1537 distinct columns (four emission trips, the last of one rank),
    every column held by two tuples.  The middle cell's sums cancel to exactly 0 in the first trip only (ranks 3, 100 and
    511), in the last only (rank 1536), in every trip, or all of them; its neighbours keep all their columns."""
    b = Builder(4 * STRIDE)
    cols = [spread(1537, *(STRIDE * i * 8192 + 3 * i, (STRIDE * i + 2) * 8192)) for i in range(3)]
    ranks = {"first": [3, 100, 511], "last": [1536], "every": [0, 511, 512, 700, 1023, 1024, 1535, 1536], "all": range(1537)}[where]
    b.row(join(*[deal(64, c, 2 * 1537) for c in cols]), cancel=[int(cols[1][q]) for q in ranks])
    p = Plan(b, schemes=(BITMAP,), expect={BITMAP: (1, 3)}, flags=("plain", "exact"), emits=("plain", "scalek", "C", "scalei", "all"))
    p.cancelled = len(ranks)
    return p


SEG_LENS = (1, 3, 4, 5, 8, 17)


@functools.lru_cache(maxsize=None)
def segments():
    """Row 0 (48 tuples), four cells: (0) segment lengths 1, 3, 4, 5, 8 and 17 mixed; (1) only every third tuple has a
    segment here; (2) 256 items, a multiple of 64; (3) 257 items, 64 k + 1.  A third of its tuples select an empty B
    row.  Row 1 (240 tuples): a bitmap cell of 4080 products in segments of 17 (1200 items: 19 blocks, the third step of
    waves 0 .. 2) followed by a small cell, whose two prefetched blocks come after the long one.  (For the hash tiles
    the long cell's windows are dense cells.)"""
    b = Builder(8 * STRIDE)
    L = 48
    live = [e for e in range(L) if e % 3 != 2]                      # tuples with a B row that is not empty
    none = np.zeros(0, np.int64)
    c0, lo = [], 0
    for e in range(L):
        n = SEG_LENS[live.index(e) % 6] if e in live else 0
        c0.append(np.arange(lo, lo + n) * 5)
        lo += n if e % 4 else 0                                     # some neighbours share columns
    c1 = [spread(40, *window_cols(STRIDE, margin=64)) + e if e % 3 == 0 else none for e in range(L)]
    c2 = [spread(32, *window_cols(2 * STRIDE, margin=8)) + (e % 7) if e in live else none for e in range(L)]       # 32 live tuples x 8 items
    c3 = [spread(32 if e else 33, *window_cols(3 * STRIDE, margin=8)) + (e % 7) if e in live else none for e in range(L)]
    fill = iter(dense_window(len(live), 7 * STRIDE))
    b.row(join(c0, c1, c2, c3, [next(fill) if e in live else none for e in range(L)]))
    long_ = [np.arange(17) * 900 + 4 * STRIDE * 8192 + 3 * e for e in range(240)]        # 17 columns over two windows
    small = [np.arange(2) * 64 + 5 * STRIDE * 8192 + e for e in range(240)]
    b.row(join(long_, small))
    return Plan(b, schemes=(BITMAP, HASH2), expect={BITMAP: (2, 6), HASH2: (2, 4)}, flags=("plain", "exact"))


@functools.lru_cache(maxsize=None)
def full_tile():
    """Rows of 32 tuples (16 cells a tile).  Row 0: 16 cells of cost 512 items, 8192 in all: one tile filled to the item
    capacity.  Row 1: the same but for a 16th cell of cost 576, which no longer fits and opens a second tile."""
    b = Builder(17 * STRIDE)
    for last in (1500, 1700):
        cells = [deal(32, spread(1500 if i < 15 else last, *window_cols(STRIDE * i, margin=4)) + i % 3) for i in range(16)]
        b.row(join(*cells), seed=last)
    return Plan(b, schemes=(BITMAP, HASH2), expect={BITMAP: (3, 32), HASH2: (3, 32)})


NCLUSTER = 1500


@functools.lru_cache(maxsize=None)
def hash_tiles():
    """Row 0 (16 tuples): one hash cell of 1500 columns whose home slots in the tiles' table of 4096 are 4094, 4095, 0
    and 1 -- the probe runs wrap.  Row 1 (64 tuples): a cell of exactly 2048 distinct columns (occ full, the table half
    full).  Row 2 (256 tuples): a cell of 256 products on one column (the most a tile row can put on one) and 100 on columns of
    their own, then one of 1792 products on 7 columns."""
    nwin = 260
    b = Builder(nwin)
    cl = wrap_cluster(4096, NCLUSTER, 256 * 8192)
    b.row(join(deal(16, cl), dense_window(16, 258)))
    b.row(join(deal(64, spread(2048, 0, 6 * 8192)), dense_window(64, 258)), seed=1)
    one = join(deal(256, np.asarray([8192 + 77]), 256), deal(256, spread(100, *window_cols(2))))
    b.row(join(one, deal(256, spread(7, 20 * 8192, 21 * 8192), 1792), dense_window(256, 258)), seed=2)
    return Plan(b, schemes=(HASH2, HASH1), expect={HASH2: (3, 4), HASH1: (3, 4)}, flags=("plain", "exact", "ordered"))


WINDOWED = {1024: 400, 3072: 1200, 4096: 1800, 8192: 1500}      # wrapping columns of the cell per windowed table


@functools.lru_cache(maxsize=None)
def hash_windowed(T):
    """A row of 300 tuples (too long for tiles): one windowed hash cell in the table of T slots whose columns' home slots
    are the table's last two and first two (for 8192, 700 further columns bring the cell above 2048 products), and a
    dense window.  A second row, of 2048 tuples, puts 2048 products on one column (table 4096)."""
    nwin = 512
    b = Builder(nwin)
    L = 300
    cols = wrap_cluster(T, WINDOWED[T], 500 * 8192)
    if T == 8192:
        rest = np.setdiff1d(spread(720, 0, 500 * 8192), cols)[:700]
        cols = np.union1d(cols, rest)
    b.row(join(deal(L, cols), dense_window(L, 510, n=3900)))
    # (a long row's window above 1024 products is a dense cell unless the knob says otherwise)
    kn = {"long_cap": 4096, "long_dense_min": 4096} if T == 8192 else ({"long_dense_min": 2048} if T == 4096 else {})
    if T == 4096:
        b.row(join(deal(2048, np.asarray([3 * 8192 + 5]), 2048), dense_window(2048, 510, n=4096)), seed=1)
    return Plan(b, schemes=(BITMAP,) if T == 8192 else (HASH2,), knobs=kn, flags=("plain", "exact", "ordered"),
                expect={BITMAP: (0, 0), HASH2: (0, 0)}, **kn)


@functools.lru_cache(maxsize=None)
def direct_cells():
    """Direct cells (one window above direct_min = 1024 products) of rows of 256 tuples.  Row 0: 1280 products, every one
    its own column, in the matrix's first window; 1280 products on 5 columns (a tile row has at most 256 on one); 1280
    products on 640 columns of which 100 cancel to exactly 0 (products, no owner); 1280 own columns in the last window."""
    nwin = 64
    b = Builder(nwin)
    L = 256
    own = deal(L, spread(1280, 0, 8192))
    five = deal(L, spread(5, *window_cols(9)), 1280)
    ccols = spread(640, *window_cols(20))
    canc = deal(L, ccols, 1280)
    lastw = deal(L, spread(1280, *window_cols(nwin - 1)))
    b.row(join(own, five, canc, lastw), cancel=[int(c) for c in ccols[::6][:100]])
    p = Plan(b, schemes=(BITMAP, HASH2), knobs={"direct_min": 1024}, direct_min=1024, expect={BITMAP: (0, 0), HASH2: (0, 0)})
    p.cancelled = 100
    return p


PERIOD = 5
# tile cells of the five shapes: the bitmap cells end at window gaps, the hash cells of shape 0 where 2048 products are full
SEQUENCE_TILE_CELLS = {BITMAP: (16, 3, 3, 1, 2), HASH2: (3, 3, 3, 1, 2), HASH1: (3, 3, 3, 1, 2)}


def sequence_shapes(kind):
    """The five row shapes of a sequence, as (L, [(first window, windows, products) per cell]); every row is one tile.
    They differ in lsh (4, 5, 6, 7, 8: both sides of 6), tile cells (16, 3, 3, 1, 2), cell size (one block of 64 items,
    or more than 16) and column range (one window, or 16).  kind "tiles": cells of at most 2048 products (a window of
    more would be a dense cell for the hash tiles; the row of one tile cell has a dense window besides, which makes it
    heavy); "direct": every cell one window of 1030 .. 2100 products."""
    if kind == "direct":
        return [(16, [(0, 1, 1100), (1, 1, 1100), (2, 1, 1100), (3, 1, 1100)]), (32, [(0, 1, 1300), (5, 1, 1300), (9, 1, 1300), (11, 1, 1300)]),
                (64, [(0, 1, 1030), (1, 1, 1030), (2, 1, 1030), (3, 1, 1030)]), (100, [(0, 1, 1250), (7, 1, 1250), (8, 1, 1250), (15, 1, 1250)]),
                (256, [(0, 1, 2100), (6, 1, 2100)])]
    return [(16, [(STRIDE * i, 1, 260) for i in range(16)]),                              # lsh 4: 16 cells of 65 items
            (32, [(0, 16, 2000), (16, 16, 2000), (32, 1, 200)]),                          # lsh 5: 500 items over 16 windows
            (64, [(0, 1, 1500), (STRIDE, 1, 1500), (2 * STRIDE, 1, 1500)]),               # lsh 6
            (100, [(0, 16, 2000), (16 * STRIDE, 1, DENSE_FILL)]),                         # lsh 7: one tile cell (and a dense one)
            (256, [(0, 1, 2000), (STRIDE, 1, 64), (16 * STRIDE, 1, DENSE_FILL)])]         # lsh 8: two tile cells, the second one block


@functools.lru_cache(maxsize=None)
def sequence(kind, nrows):
    """nrows one-tile rows whose shapes cycle with period 5 through sequence_shapes(kind).  Shape s takes only columns
    = s (mod 5): neighbours in the list -- and, the period being coprime to every grid, a workgroup's consecutive tiles
    under the static walk -- share no column, so whatever a tile leaves behind in LDS shows as a wrong tuple.  Every
    tile starts in window 0: the list, sorted by first window, keeps the rows' order."""
    shapes = sequence_shapes(kind)
    nwin = 16 * STRIDE + 1 if kind == "tiles" else 16
    b = Builder(nwin)
    base = []
    for s, (L, cells) in enumerate(shapes):
        segs = []
        for w0, nw, prods in cells:
            distinct = min(prods, nw * 8192 // PERIOD - 2)
            cols = spread(distinct, w0 * 8192 // PERIOD + 1, (w0 + nw) * 8192 // PERIOD - 1) * PERIOD + s
            segs.append(deal(L, cols, prods))
        base.append(b.row(join(*segs), seed=s))
    for r in range(PERIOD, nrows):
        b.again(base[r % PERIOD])
    if nrows < PERIOD:
        raise ValueError("a sequence has at least one period")
    if kind == "direct":
        return Plan(b, schemes=(BITMAP,), knobs={"direct_min": 1024}, direct_min=1024, expect={BITMAP: (0, 0)})
    return Plan(b, expect={s: (nrows, sum(SEQUENCE_TILE_CELLS[s][r % PERIOD] for r in range(nrows))) for s in (BITMAP, HASH2, HASH1)})


# ---- the catalogue: name -> (maker, arguments); the sequences, whose length follows the device, come from sequence()

CATALOGUE = {"class_L%d" % L: (l_class, (L,)) for L in L_CLASSES + (257,)}
CATALOGUE.update({"bm_distinct": (bm_distinct, (False,)), "bm_few_columns": (bm_distinct, (True,)),
                  "bm_range_8192": (bm_range, (8192,)), "bm_range_16384": (bm_range, (16384,))})
CATALOGUE.update({"bm_cancel_" + w: (bm_cancel, (w,)) for w in CANCELS})
CATALOGUE.update({"segments": (segments, ()), "full_tile": (full_tile, ()), "hash_tiles": (hash_tiles, ())})
CATALOGUE.update({"hash_windowed_%d" % T: (hash_windowed, (T,)) for T in HASH_T})
CATALOGUE["direct_cells"] = (direct_cells, ())


def plan(name):
    make, args = CATALOGUE[name]
    return make(*args)


DROP = 3                                # scalek: every third column absent, the others scaled by 1 or 2


def emit_args(A, B, emit):
    """(C, scalei, scalek) of an emit variant as oracle operands (the variants of tests/test_gpu_plain_emit.py)."""
    C_ = 2.0 if emit in ("C", "all") else 1.0
    rows = np.arange(A.shape[0])
    scalei = orc.Vec(rows, 3.0 + rows % 3, A.shape[0]) if emit in ("scalei", "all") else None
    scalek = None
    if emit in ("scalek", "all"):                                   # (an entry per column: not for the plans of 2^25 columns)
        j = np.arange(B.shape[1])
        j = j[j % DROP != 0]
        scalek = orc.Vec(j, np.where(j % 2 == 0, 1.0, 2.0), B.shape[1])
    return C_, scalei, scalek


_WANT = {}


def oracle_tuples(p, emit="plain"):
    """The oracle's (i, j, v) of a plan under an emit variant: computed once per plan, never changed."""
    key = (id(p), emit)
    if key not in _WANT:
        C_, scalei, scalek = emit_args(p.A, p.B, emit)
        _WANT[key] = (p, orc.multiply(p.A, p.B, C_, scalei, '.', None, '.', scalek, rowwise=True, nthreads=4)[:3])
    return _WANT[key][1]


def effective_scheme(scheme, flag):
    """The scheme heavy_prepare takes: ORDERED runs on the first generation, EXACT_PATTERN never does."""
    if flag == "ordered":
        return HASH1
    return HASH2 if (flag == "exact" and scheme == HASH1) else scheme
