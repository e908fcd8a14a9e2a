"""Planned dense cells for k_dense (csrc/k_dense.hip): operands whose heavy rows are cut into chosen dense cells -- one
output row times one column window -- at the edges of the kernel's product loop: the A-tuple count against the chunk of NT
tuples, segment lengths against the item of R tuples and the 64-item block, chunks without a product, chunks of more than
W items (several batches) and long lists of cells of changing shape.  Built on tests/tile_plan.py (Builder, Cut, Plan, the
oracle); tests/test_dense_plan_host.py checks every plan on the CPU, tests/test_gpu_dense_cells.py runs them on the GPU.
Importing it needs no GPU.

Every plan runs with the knob dense_min = 64: a window of more than 64 products is a dense cell, for rows of every
length, and every window of a plan holds either none or more than 64 -- no tile or hash cell is cut.  The last MARGIN
columns of every window stay free of planned products; the planned cancellations take them.

A segment is the part of one B row inside one window: at most W tuples, W / R items.  (So no segment has more than 4096
items at W = 16384, and no 4096-item lane group of the bitmap is ever without a first-item bit; the plan `giant` holds the
longest segment there is, the whole window, placed behind a one-item segment so that it crosses the lane groups' edge.)"""
import functools

import numpy as np

from tests import tile_plan as tp
from tests.tile_plan import BITMAP, HASH1, HASH2, R

NT = {8192: 512, 16384: 1024}           # A tuples of a chunk = threads of a workgroup
WIDTHS = (8192, 16384)
MARGIN = 64                             # columns at a window's end that only planned cancellations use
DENSE_MIN = 64                          # the knob every plan runs under
ZCOLS = 40                              # columns a cancelling pair shares in the window that cancels completely


class DensePlan(tp.Plan):
    """A plan of dense cells only.  ndense: its dense cells; claims: per planned cell a dict (row, window, L, items per
    chunk, and where stated `bounds` per chunk, `lens`, `lanes`), pinned by the maker and checked from the operands;
    cancelled: output columns whose sum is exactly 0; pairs: per row the cancelling (tuple, tuple) pairs."""

    def __init__(self, b, ndense, claims, cancelled=0, pairs=None):
        super().__init__(b, schemes=(BITMAP,), knobs={"dense_min": DENSE_MIN}, dense_min=DENSE_MIN)
        self.ndense, self.claims, self.cancelled, self.pairs = ndense, claims, cancelled, pairs or {}


def few(e, w, W, n=9):
    """n <= 9 columns of window w for tuple e, 911 apart: tuples share columns, no segment holds one twice."""
    return w * W + (e * 7 + np.arange(n) * 911) % (W - MARGIN)


def run(e, n, w, W):
    """n consecutive columns (cyclically, outside the margin) of window w for tuple e."""
    assert n <= W - MARGIN
    return w * W + (e * 1001 + np.arange(n)) % (W - MARGIN)


NONE = np.zeros(0, np.int64)


def add_cancel(segs, pairs, w, wz, W):
    """Every pair (e0, e1) of tuples gets one column of its own in the margin of window w and ZCOLS of its own in window
    wz, which holds nothing else: all of them cancel.  Returns the cancelled columns."""
    assert len(pairs) <= MARGIN
    out = []
    for q, (e0, e1) in enumerate(pairs):
        extra = np.concatenate([[(w + 1) * W - MARGIN + q], wz * W + ZCOLS * q + np.arange(ZCOLS)])
        for e in (e0, e1):
            segs[e] = np.concatenate([segs[e], extra])
        out += extra.tolist()
    return out


def items_of(lens):
    return [(n + R - 1) // R for n in lens]


def chunk_sums(per_tuple_items, nt):
    return [int(sum(per_tuple_items[c:c + nt])) for c in range(0, len(per_tuple_items), nt)]


# ---- A. chunk edges

CHUNK_L = {8192: (1, 2, 511, 512, 513, 1023, 1024, 1025, 1537), 16384: (1023, 1024, 1025, 2049, 3073)}


@functools.lru_cache(maxsize=None)
def chunk_edge(L, W, cancel=False):
    """One row of L tuples, one dense cell in window 1: nine columns a tuple (three items, the last of one tuple); L = 1
    is one segment of 4105 columns, L = 2 two of 2053.  cancel: two pairs of tuples from different chunks share a
    cancelling column in the cell, and window 2 cancels completely."""
    nt = NT[W]
    b = tp.Builder(3, W)
    lens = {1: [4105], 2: [2053, 2053]}.get(L, [9] * L)
    segs = [few(e, 1, W) if n == 9 else run(e, n, 1, W) for e, n in enumerate(lens)]
    pairs = [(0, nt), (nt - 1, L - 1)] if cancel else []
    canc = add_cancel(segs, pairs, 1, 2, W)
    b.row(segs, cancel=canc)
    claims = [dict(row=0, window=1, L=L, items=chunk_sums(items_of([n + (1 if cancel and e in sum(pairs, ()) else 0) for e, n in enumerate(lens)]), nt))]
    return DensePlan(b, 2 if cancel else 1, claims, len(canc), {0: pairs})


# ---- B. segments and items

SEG_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def seg_lens(W):
    """One chunk of 60 tuples whose segment lengths run four times through SEG_LENS: every fill of an item's R tuples,
    65 items (257 tuples: a block and one item) and 129 (513 tuples: bitmap words without a bit)."""
    b = tp.Builder(2, W)
    lens = list(SEG_LENS) * 4
    b.row([run(e, n, 1, W) for e, n in enumerate(lens)])
    return DensePlan(b, 1, [dict(row=0, window=1, L=60, items=[4 * sum(items_of(SEG_LENS))], lens=set(SEG_LENS))])


@functools.lru_cache(maxsize=None)
def giant(W):
    """Three segments in one chunk: one tuple, the whole window (W tuples, W / R items: the longest segment there is, from
    item 1 on: it leaves all but the first of its W / 256 bitmap words without a bit) and nine tuples."""
    b = tp.Builder(2, W)
    b.row([np.asarray([W + 5]), W + np.arange(W), few(2, 1, W)])
    return DensePlan(b, 1, [dict(row=0, window=1, L=3, items=[1 + W // R + 3], lens={1, W, 9})])


@functools.lru_cache(maxsize=None)
def columns(W):
    """Row 0: 4100 tuples (nine chunks at NT = 512), every product on one column of window 0.  Row 1: 64 tuples, every
    column of window 1 hit exactly once."""
    b = tp.Builder(2, W)
    b.row([np.asarray([77])] * 4100)
    b.row(tp.deal(64, W + np.arange(W)), seed=1)
    nt = NT[W]
    return DensePlan(b, 2, [dict(row=0, window=0, L=4100, items=[min(nt, 4100 - c) for c in range(0, 4100, nt)], lens={1}),
                            dict(row=1, window=1, L=64, items=[W // R], lens={W // 64})])


# ---- C. empty segments

LANES = ("all", "thread_0", "thread_last", "every_other", "lanes_0_63", "not_wave_0", "not_last_wave", "one_in_wave_5")


def lane_mask(name, nt):
    t = np.arange(nt)
    return {"all": t >= 0, "thread_0": t == 0, "thread_last": t == nt - 1, "every_other": t % 2 == 0,
            "lanes_0_63": (t % 64 == 0) | (t % 64 == 63), "not_wave_0": t >= 64, "not_last_wave": t < nt - 64,
            "one_in_wave_5": t == 5 * 64 + 17}[name]


@functools.lru_cache(maxsize=None)
def lanes(W):
    """Eight rows of NT tuples, one per pattern of LANES: the tuples of the pattern have a segment in window 0 (nine
    columns; 130 where at most two tuples have one), the others none.  Window 1 is a filler cell with a segment from
    every tuple, which makes the row heavy."""
    nt = NT[W]
    b = tp.Builder(2, W)
    claims = []
    for r, name in enumerate(LANES):
        live = lane_mask(name, nt)
        n = 130 if live.sum() <= 2 else 9
        cell = [(few(e, 0, W) if n == 9 else run(e, n, 0, W)) if live[e] else NONE for e in range(nt)]
        b.row(tp.join(cell, tp.dense_window(nt, 1, W, n=4100)), seed=r)
        claims.append(dict(row=r, window=0, L=nt, items=[int(live.sum()) * ((n + R - 1) // R)], lanes=name))
    return DensePlan(b, 16, claims)


EMPTY_CHUNKS = {"first": (0,), "middle": (1,), "last": (2,), "two": (1, 2)}


@functools.lru_cache(maxsize=None)
def empty_chunks(where, W, cancel=False):
    """A row of three chunks (four for "two") whose first, middle or last chunk -- or the two middle ones -- has no product
    in window 0: those tuples select B rows with one tuple in window 1 (the even ones) or none at all.  Window 1 is then a
    dense cell with the complementary empty chunks.  cancel: pairs of tuples of the first and the last chunk."""
    nt = NT[W]
    dead = EMPTY_CHUNKS[where]
    nch = 4 if where == "two" else 3
    L = nch * nt
    cell = [few(e, 0, W) if e // nt not in dead else NONE for e in range(L)]
    other = [np.asarray([W + (e * 5) % (W - MARGIN)]) if (e // nt in dead and e % 2 == 0) else NONE for e in range(L)]
    segs = tp.join(cell, other)
    pairs = [(0, L - nt), (nt - 1, L - 1)] if cancel else []
    assert not cancel or where == "middle"
    canc = add_cancel(segs, pairs, 0, 2, W)
    b = tp.Builder(3, W)
    b.row(segs, cancel=canc)
    claims = [dict(row=0, window=0, L=L, items=[0 if c in dead else 3 * nt for c in range(nch)]),
              dict(row=0, window=1, L=L, items=[nt // 2 if c in dead else 0 for c in range(nch)])]
    return DensePlan(b, 3 if cancel else 2, claims, len(canc), {0: pairs})


# ---- D. batches

SEG_ITEMS = 1024                        # items of the D plans' even segments (4096 tuples)
STRADDLE = 6000                         # tuples of the straddling plans' segments (1500 items)


@functools.lru_cache(maxsize=None)
def items_edge(W, d):
    """One chunk of W + d items (d = -1, 0, 1): segments of 1024 items and a last one that ends on a one-tuple item.
    W + 1: a second batch of one item, the boundary on its segment's first item."""
    n = W + d
    full, rest = divmod(n, SEG_ITEMS)
    lens = [R * SEG_ITEMS] * full + ([R * rest - 3] if rest else [])
    b = tp.Builder(2, W)
    b.row([run(e, m, 1, W) for e, m in enumerate(lens)])
    return DensePlan(b, 1, [dict(row=0, window=1, L=len(lens), items=[n], bounds=[["first"] if d == 1 else []])])


@functools.lru_cache(maxsize=None)
def straddle(W, nbatch=2, cancel=False):
    """One chunk of 6 (12 at W = 16384) segments of 1500 items: two batches, the boundary inside a segment.  nbatch 3:
    twice as many segments (one less at W = 16384), three batches.  cancel: the first segment (batch 0) and the last
    (its last item in the last batch) share cancelling columns."""
    S = {(8192, 2): 6, (16384, 2): 12, (8192, 3): 12, (16384, 3): 23}[(W, nbatch)]
    segs = [run(e, STRADDLE, 1, W) for e in range(S)]
    pairs = [(0, S - 1)] if cancel else []
    canc = add_cancel(segs, pairs, 1, 2, W)
    b = tp.Builder(3, W)
    b.row(segs, cancel=canc)
    items = S * (STRADDLE // R) + (2 if cancel else 0)
    return DensePlan(b, 2 if cancel else 1, [dict(row=0, window=1, L=S, items=[items], bounds=[["inside"] * (nbatch - 1)])],
                     len(canc), {0: pairs})


@functools.lru_cache(maxsize=None)
def first_item(W):
    """One chunk of W / 1024 + 1 segments of 1024 items: the second batch begins on a segment's first item."""
    S = W // SEG_ITEMS + 1
    b = tp.Builder(2, W)
    b.row([run(e, R * SEG_ITEMS, 1, W) for e in range(S)])
    return DensePlan(b, 1, [dict(row=0, window=1, L=S, items=[S * SEG_ITEMS], bounds=[["first"]])])


@functools.lru_cache(maxsize=None)
def second_chunk(W, cancel=False):
    """A row of 2 NT + 40 tuples: an ordinary first chunk (nine columns a tuple), a second chunk whose first 6 (12) tuples
    have segments of 1500 items -- two batches -- and an ordinary third.  cancel: pairs across the chunks and across the
    second chunk's batches."""
    nt = NT[W]
    S = 6 if W == 8192 else 12
    L = 2 * nt + 40
    lens = [STRADDLE if nt <= e < nt + S else 9 for e in range(L)]
    segs = [few(e, 1, W) if n == 9 else run(e, n, 1, W) for e, n in enumerate(lens)]
    pairs = [(0, nt), (nt, nt + S - 1), (nt + S - 1, L - 1)] if cancel else []
    canc = add_cancel(segs, pairs, 1, 2, W)
    b = tp.Builder(3, W)
    b.row(segs, cancel=canc)
    mid = S * (STRADDLE // R) + 3 * (nt - S) + (2 if cancel else 0)
    return DensePlan(b, 2 if cancel else 1, [dict(row=0, window=1, L=L, items=[3 * nt, mid, 120], bounds=[[], ["inside"], []])],
                     len(canc), {0: pairs})


# ---- E. lists of cells

LIST_WINDOWS, LIST_PRODUCTS, LIST_LIVE = 70, 66, 22
LIST_PERIOD = 5
LISTS = {"one": 0, "few": 3, "static": 35, "parts": 60}          # rows of the list plans ("one": a single cell)
# workgroups of a launch on 256 CUs (one, two or three a CU) and, for a list in eight XCD parts, an eighth of them: the
# static strides.  None is a multiple of LIST_PERIOD.
LIST_STRIDES = (256, 512, 768, 32, 64, 96)


def list_shapes(W):
    """The five row shapes of a list, as (L, tuples with a segment): one tuple; three chunks, the 22 segments spread
    over them with the row's first and last tuple among them; two chunks, the first one empty; two chunks, the second of
    one tuple; one chunk of NT - 1 tuples."""
    nt = NT[W]
    return [(1, np.asarray([0])), (2 * nt + 1, tp.spread(LIST_LIVE, 0, 2 * nt + 1)), (nt + LIST_LIVE, nt + np.arange(LIST_LIVE)),
            (nt + 1, tp.spread(LIST_LIVE, 0, nt + 1)), (nt - 1, tp.spread(LIST_LIVE, 0, nt - 1))]


@functools.lru_cache(maxsize=None)
def cell_list(nrows, W=8192, cancel=False):
    """nrows rows of 70 dense cells of 66 products each (every product its own column).  The rows cycle through the five
    shapes of list_shapes; every size key being equal, the cells of one window keep the rows' order in the sorted list,
    so consecutive cells go from a one-tuple cell to a three-chunk cell to a cell whose first chunk is empty, and on.
    The long lists have a multiple of five rows: cell i has shape i mod 5, and since no static stride (LIST_STRIDES) is a
    multiple of five, a workgroup's next cell has another shape in every launch, the COUNT launch's three workgroups a CU
    included.  Shape s takes only the window's columns = s (mod 5): what a cell leaves behind in LDS is a wrong tuple in
    the next.  The rows of a shape share their B rows.  nrows 0: a single cell, 4100 products of one row of three
    tuples.  cancel: in the three-chunk rows the first and the last tuple share a cancelling column in window 0, and
    window 70 cancels completely."""
    if nrows == 0:
        b = tp.Builder(1, W)
        b.row(tp.deal(3, tp.spread(4100, 0, W - MARGIN)))
        return DensePlan(b, 1, [dict(row=0, window=0, L=3, items=[342 + 342 + 342])])
    nt = NT[W]
    b = tp.Builder(LIST_WINDOWS + (1 if cancel else 0), W)
    claims, pairs, ncanc = [], {}, 0
    shapes = list_shapes(W)[:min(nrows, LIST_PERIOD)]
    for s, (L, live) in enumerate(shapes):
        per = LIST_PRODUCTS // len(live)                            # 66 columns of the one tuple, or 3 of each of the 22
        segs = [NONE] * L
        for q, e in enumerate(live):
            slots = per * q + np.arange(per)
            segs[e] = np.concatenate([w * W + LIST_PERIOD * 23 * slots + s for w in range(LIST_WINDOWS)])
        canc = []
        if cancel and s == 1:
            pairs[s] = [(int(live[0]), int(live[-1]))]
            canc = add_cancel(segs, pairs[s], 0, LIST_WINDOWS, W)
            ncanc = len(canc)
        b.row(segs, cancel=canc, seed=s)
        lens = np.zeros(L, np.int64)
        lens[live] = per
        for w in (0, 1, LIST_WINDOWS - 1):
            it = np.asarray(items_of(lens))
            if canc and w == 0:
                it[[live[0], live[-1]]] = 1                         # 3 + 1 tuples: still one item
            claims.append(dict(row=s, window=w, L=L, items=chunk_sums(it, nt)))
    for r in range(len(shapes), nrows):
        b.again(r % LIST_PERIOD)
    ncancel_rows = sum(1 for r in range(nrows) if r % LIST_PERIOD in pairs)
    p = DensePlan(b, LIST_WINDOWS * nrows + ncancel_rows, claims, ncanc * ncancel_rows, pairs)
    for r in range(len(shapes), nrows):
        if r % LIST_PERIOD in pairs:
            p.pairs[r] = pairs[r % LIST_PERIOD]
    return p


# ---- the catalogue: name -> (maker, arguments)

CATALOGUE = {}
for _W in WIDTHS:
    CATALOGUE.update({"chunk_L%d_%d" % (L, _W): (chunk_edge, (L, _W)) for L in CHUNK_L[_W]})
    CATALOGUE.update({"seg_lens_%d" % _W: (seg_lens, (_W,)), "giant_%d" % _W: (giant, (_W,)), "columns_%d" % _W: (columns, (_W,)),
                      "lanes_%d" % _W: (lanes, (_W,))})
    CATALOGUE.update({"empty_%s_%d" % (k, _W): (empty_chunks, (k, _W)) for k in EMPTY_CHUNKS})
    CATALOGUE.update({"items_W%+d_%d" % (d, _W): (items_edge, (_W, d)) for d in (-1, 0, 1)})
    CATALOGUE.update({"straddle_%d" % _W: (straddle, (_W,)), "three_batches_%d" % _W: (straddle, (_W, 3)),
                      "first_item_%d" % _W: (first_item, (_W,)), "second_chunk_%d" % _W: (second_chunk, (_W,))})
    CATALOGUE.update({"list_%s_%d" % (k, _W): (cell_list, (n, _W)) for k, n in LISTS.items() if _W == 8192 or k in ("few", "static")})
# the variants with planned cancellations (EXACT_PATTERN's representatives)
CATALOGUE.update({"chunk_L513_8192_cancel": (chunk_edge, (513, 8192, True)), "chunk_L1025_16384_cancel": (chunk_edge, (1025, 16384, True)),
                  "empty_middle_8192_cancel": (empty_chunks, ("middle", 8192, True)), "empty_middle_16384_cancel": (empty_chunks, ("middle", 16384, True)),
                  "straddle_8192_cancel": (straddle, (8192, 2, True)), "straddle_16384_cancel": (straddle, (16384, 2, True)),
                  "second_chunk_8192_cancel": (second_chunk, (8192, True)), "second_chunk_16384_cancel": (second_chunk, (16384, True)),
                  "list_static_8192_cancel": (cell_list, (35, 8192, True))})


def plan(name):
    make, args = CATALOGUE[name]
    return make(*args)


# ---- a planned cell, measured from the operands

def degrees(p):
    """Per (B row, window): the tuples of the segment."""
    if not hasattr(p, "_deg"):
        wshift = {8192: 13, 16384: 14}[p.W]
        p._deg = np.zeros((p.B.shape[0], p.B.shape[1] >> wshift), np.int64)
        np.add.at(p._deg, (p.B.idx0, p.B.idx1 >> wshift), 1)
        p._rows = tp.row_tuples(p.A)
    return p._deg


def segment_lengths(p, r, w):
    deg = degrees(p)
    return deg[p.A.idx1[p._rows[0][r]:p._rows[1][r]], w]


def batch_bounds(items, W):
    """For one chunk's items per tuple: per batch boundary k W below the total, "first" if item k W is a segment's first,
    else "inside"."""
    items = np.asarray(items, np.int64)
    first = np.cumsum(items) - items
    firsts = set(first[items > 0].tolist())
    return ["first" if k in firsts else "inside" for k in range(W, int(items.sum()), W)]


def shape_of(p, r, w):
    """What k_dense meets in the cell of row r and window w: L, items and batch boundaries per chunk of NT tuples, the
    set of segment lengths, the non-empty lanes of the first chunk."""
    lens = segment_lengths(p, r, w)
    nt = NT[p.W]
    it = (lens + R - 1) // R
    chunks = [it[c:c + nt] for c in range(0, len(lens), nt)]
    items = [int(c.sum()) for c in chunks]
    return dict(L=len(lens), products=int(lens.sum()), items=items, batches=[(n + p.W - 1) // p.W for n in items],
                empty=[c for c, n in enumerate(items) if n == 0], bounds=[batch_bounds(c, p.W) for c in chunks],
                lens=set(lens.tolist()), live=np.pad(lens[:nt] > 0, (0, max(0, nt - len(lens)))))


def cell_products(p, r, w):
    """Every product of the cell of row r and window w: (tuple of the row, position in its segment, column)."""
    degrees(p)
    lo, hi = p._rows[0][r], p._rows[1][r]
    blo = np.searchsorted(p.B.idx0, np.arange(p.B.shape[0] + 1))
    es, pos, cols = [], [], []
    for e in range(hi - lo):
        k = p.A.idx1[lo + e]
        j = p.B.idx1[blo[k]:blo[k + 1]]
        j = j[(j >= w * p.W) & (j < (w + 1) * p.W)]
        es.append(np.full(j.size, e)); pos.append(np.arange(j.size)); cols.append(j)
    return np.concatenate(es), np.concatenate(pos), np.concatenate(cols)


def holder_places(p, r, cols):
    """Per column of `cols` (all of one window): the (chunk, batch) of every product of row r on it."""
    w = int(cols[0]) // p.W
    e, pos, j = cell_products(p, r, w)
    nt = NT[p.W]
    it = (segment_lengths(p, r, w) + R - 1) // R
    before = np.concatenate([np.cumsum(it[c:c + nt]) - it[c:c + nt] for c in range(0, len(it), nt)])     # items of the chunk in front of the tuple
    out = {}
    for col in cols:
        assert int(col) // p.W == w
        m = j == col
        out[int(col)] = [(int(x) // nt, int(before[x] + q // R) // p.W) for x, q in zip(e[m], pos[m])]
    return out
