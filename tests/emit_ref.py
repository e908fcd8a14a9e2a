"""Inputs for hash_emit (csrc/spgemm_hash.h), the column-ordered emission of a finished LDS hash table, and a restatement
of what decides its ordering.  Needs numpy and the oracle only: tests/test_emit_host.py pins the restatement and the
records without a GPU, tests/test_gpu_emit_edges.py runs the cases.

In the COO sink hash_emit picks one of three orderings from the table size T, the block size NT and colbits, the bits of
the cell's column range: the bitmap rank, the LDS radix sort of 32-bit keys (col - colbase) << PBITS | position, the
bitonic network of 64-bit keys.  For a mid row (65 .. 4096 products) colbits is the bits of ncol - 1, so the column count
of op(B) alone decides; for a cell of a heavy row it is wshift + bits(windows - 1).

Mid rows: case(ncol, rows) builds op(B) of ncol columns by hand; a row of A is given by the column sets of the B rows it
multiplies.  Values are small integers (A: 1 .. 3 with a sign by row, B: 1 .. 3 with a sign by column, planned
cancellations in pairs + a', - a): every sum is exact in any order, so a result compares bit for bit with the oracle.
Every row is recorded as (L, products, outputs, kernel, T, path).  width_case(ncol) is the catalogue's case of a width.

Heavy rows: window_case(T, W, where) puts one hash cell of 1, 2, 3, 4, 5 (and 9) windows per row, in the lowest or in the
highest windows of 2048, with tests/tile_plan.py's Builder; its Cut predicts the cells."""
import collections
import functools

import numpy as np

from oracle import binding as orc
from tests import tile_plan as tp

# ---- the restatement -----------------------------------------------------------------------------------------------

FEW_MAX_DEFAULT, FEW_LMAX, MID_MAX = 8, 16, 4096
CLASSES = ((1024, 65, 512), (4096, 513, 2048), (8192, 2049, 4096))         # (T, fewest, most products) of the mid rows' tables
# threads of a workgroup by kernel and table: k_hash (mid rows and windowed cells), k_few, the hash tiles of both generations
NT = {"k_hash": {1024: 256, 3072: 512, 4096: 512, 8192: 512}, "k_few": {1024: 256, 4096: 512, 8192: 1024}, "tiles": {4096: 512}}
BITMAP, RADIX, BITONIC = "bitmap", "radix", "bitonic"


def colbits(ncol):
    """EmitParams::ncolbits (emit_params, csrc/spgemm.hip): the bits of the largest column index, 1 for a single column."""
    return max(1, (int(ncol) - 1).bit_length())


def table_class(P):
    """bin_of (csrc/spgemm.hip) for a mid row: the table of a row of P products; None: the row is light or heavy."""
    for T, lo, hi in CLASSES:
        if lo <= P <= hi:
            return T
    return None


def few_limit(few_max=0, ordered=False):
    """classify_rows: the most A tuples of a k_few row under the knob (0: the default, -1: none, at most 16); the ORDERED
    sink and EXACT_PATTERN keep every mid row on k_hash."""
    if ordered or few_max < 0:
        return -1
    return FEW_MAX_DEFAULT if few_max == 0 else min(few_max, FEW_LMAX)


def kernel(L, few_max=0, ordered=False):
    """k_classify: the kernel of a mid row of L A tuples."""
    return "k_few" if L <= few_limit(few_max, ordered) else "k_hash"


def pbits(T):
    """Bits of a position in the occupied list (below T / 2) in the radix key."""
    return 9 if T <= 1024 else (11 if T <= 4096 else 12)


def emit_path(kern, T, cbits, knob=0):
    """hash_emit's choice in the COO sink.  knob (emit_path): 1 skips the bitmap rank, 2 the radix sort as well; it never
    forces a radix sort whose key would not fit."""
    nt = NT[kern][T]
    colrange = 0xFFFFFFFF if cbits >= 32 else 1 << cbits
    if T // 8 <= nt and colrange <= 32 * T and knob < 1:
        return BITMAP
    if cbits + pbits(T) <= 32 and knob < 2:
        return RADIX
    return BITONIC


def thresholds(kern, T):
    """(widest colbits on the bitmap rank or None, widest colbits on the radix sort) with no knob set."""
    on = [emit_path(kern, T, b) for b in range(33)]
    bm = [b for b in range(33) if on[b] == BITMAP]
    return (max(bm) if bm else None), max(b for b in range(33) if on[b] == RADIX)


# ---- mid rows: operands from column sets -----------------------------------------------------------------------------

Rec = collections.namedtuple("Rec", "L products outputs kernel T path")


class Case:
    """Operands, the records of A's rows, the distinct columns a row's products fall on (hit: the occupied list's
    length) and the tuples the construction itself gives (want: i, j, v)."""

    def __init__(self, A, B, ncol, rec, hit, want):
        self.A, self.B, self.ncol, self.rec, self.hit, self.want = A, B, ncol, rec, hit, want
        self.colbits = colbits(ncol)

    def few_rows(self, few_max=0, ordered=False):
        """The mid rows that k_few takes under the knob: the N of the trace line "few cells: mid N"."""
        return sum(1 for r in self.rec if r.T and r.L <= few_limit(few_max, ordered))

    def mid(self):
        """(rows, products, A tuples) of the mid rows: the result's rows_mid, products_mid, tuples_mid."""
        m = [r for r in self.rec if r.T]
        return len(m), sum(r.products for r in m), sum(r.L for r in m)

    def paths(self, knob=0, few_max=0, ordered=False):
        """{(kernel, T, path)} that the case's mid rows reach under the knobs."""
        out = set()
        for r in self.rec:
            if r.T:
                k = kernel(r.L, few_max, ordered)
                out.add((k, r.T, emit_path(k, r.T, self.colbits, knob)))
        return out


def case(ncol, rows):
    """rows[i] = (segments, cancel): segments[e] the sorted columns of the B row that A tuple e of row i selects, cancel the
    columns whose sum in the row must be exactly 0 (each held by an even number of the row's tuples, whose B values pair
    off as + a', - a, as tile_plan.Builder.row does).  Equal column sets of different rows of A are one row of B (two in
    one row of A are two rows of B); the B rows of a row with cancellations are its own.  A value of tuple e in row i:
    1 + (i + 2 e) % 3, negative in the rows i = 1 (mod 3); B value: 1 + (column + B row) % 3, negative in the columns = 3 (mod 4):
    sums of both signs, none that cancels unplanned."""
    bcols, bvals, known = [], [], {}
    ai, ak, av, rec, hit = [], [], [], [], []
    wi, wj, wv = [], [], []
    for i, (segs, cancel) in enumerate(rows):
        L = len(segs)
        e = np.arange(L)
        a = (1.0 + (i + 2 * e) % 3) * (-1.0 if i % 3 == 1 else 1.0)
        ks, seen = [], collections.Counter()
        for q, s in enumerate(segs):
            s = np.asarray(s, np.int64)
            assert np.all(s[1:] > s[:-1]) and (s.size == 0 or (s[0] >= 0 and s[-1] < ncol)), "row %d, segment %d: columns" % (i, q)
            key = (i, q) if len(cancel) else (s.tobytes(), seen[s.tobytes()])
            seen[s.tobytes()] += 1
            if key not in known:
                known[key] = len(bcols)
                bcols.append(s)
                bvals.append(np.where(s % 4 == 3, -1.0, 1.0) * (1.0 + (s + len(bcols) - 1) % 3))
            ks.append(known[key])
        assert len(set(ks)) == L
        for j in cancel:
            hs = [q for q in range(L) if np.any(bcols[ks[q]] == j)]
            assert hs and len(hs) % 2 == 0, "row %d, column %d: %d holders" % (i, j, len(hs))
            for h0, h1 in zip(hs[::2], hs[1::2]):
                bvals[ks[h0]][bcols[ks[h0]] == j] = a[h1]
                bvals[ks[h1]][bcols[ks[h1]] == j] = -a[h0]
        ai.append(np.full(L, i)); ak.append(np.asarray(ks, np.int64)); av.append(a)
        cols = np.concatenate([bcols[k] for k in ks]) if L else np.zeros(0, np.int64)
        prods = np.concatenate([a[q] * bvals[ks[q]] for q in range(L)]) if L else np.zeros(0)
        u, inv = np.unique(cols, return_inverse=True)
        sums = np.zeros(u.size)
        np.add.at(sums, inv, prods)
        keep = sums != 0
        P, T = int(cols.size), table_class(int(cols.size))
        assert P <= MID_MAX, "row %d: %d products, a heavy row" % (i, P)
        kern = kernel(L) if T else None
        rec.append(Rec(L, P, int(keep.sum()), kern, T, emit_path(kern, T, colbits(ncol)) if T else None))
        hit.append(int(u.size))
        wi.append(np.full(int(keep.sum()), i)); wj.append(u[keep]); wv.append(sums[keep])
    nb = len(bcols)
    A = orc.Mat(np.concatenate(ai), np.concatenate(ak), np.concatenate(av), (len(rows), nb))
    B = orc.Mat(np.concatenate([np.full(s.size, k) for k, s in enumerate(bcols)]), np.concatenate(bcols), np.concatenate(bvals), (nb, ncol))
    want = (np.concatenate(wi).astype(np.int32), np.concatenate(wj).astype(np.int32), np.concatenate(wv))
    return Case(A, B, ncol, rec, hit, want)


# ---- the columns of a row ----------------------------------------------------------------------------------------------

def ends(ncol):
    return [0, 1, ncol - 2, ncol - 1]


def bitmap_edges(ncol):
    """The bitmap's word and superblock edges (a word is 64 columns, a superblock 4 words) and the first and last bit of
    its last word that holds a column."""
    return [63, 64, 255, 256, ((ncol - 1) >> 6) << 6, ncol - 1]


def bit_pairs(ncol):
    """Pairs of columns that differ only in the top bit of colbits, only in bit 0, only in bit 15, 16 or 30."""
    top = 1 << (colbits(ncol) - 1)
    x = 37 & (top - 1)
    out = [x if (x | top) < ncol else 0, (x if (x | top) < ncol else 0) | top]
    m = 2 * (ncol // 3)
    out += [m, m + 1]
    for b in (15, 16, 30):
        out += [(1 << b) - 3, (2 << b) - 3]
    return out


LAYOUTS = {"ends": lambda n: ends(n), "bitmap": lambda n: ends(n) + bitmap_edges(n), "pairs": lambda n: ends(n) + bit_pairs(n),
           "all": lambda n: ends(n) + bitmap_edges(n) + bit_pairs(n)}


def columns(ncol, D, rng, layout):
    """min(D, ncol) sorted distinct columns: the layout's special columns that exist (both ends always), the rest a seeded
    random spread."""
    D = min(D, ncol)
    sp = np.unique([c for c in LAYOUTS[layout](ncol) if 0 <= c < ncol])[:D]
    if ncol <= 4 * D:
        rest = np.setdiff1d(rng.permutation(ncol), sp)
        rest = rng.permutation(rest)[:D - sp.size]
    else:
        rest = np.zeros(0, np.int64)
        while rest.size < D - sp.size:
            rest = np.setdiff1d(np.union1d(rest, rng.integers(0, ncol, 2 * D, dtype=np.int64)), sp)
        rest = rng.permutation(rest)[:D - sp.size]
    out = np.union1d(sp, rest).astype(np.int64)
    assert out.size == D
    return out


def deal(L, cols, P):
    """tile_plan.deal with every segment sorted."""
    return [np.sort(s) for s in tp.deal(L, cols, P)]


def ceil_div(a, b):
    return -(-a // b)


def width_rows(ncol):
    """The rows of a width, as (name, segments, cancel).  Per table class: its fewest and its most products with as few
    A tuples as the width allows (one on a wide matrix: k_few; the most products on T / 2 distinct columns fill the
    occupied list), a row of few_max tuples whose columns repeat, and a row of few_max + 1 tuples on T / 2 distinct columns
    (k_hash).  Then three B rows of one column set (every output a sum of three), and rows of 4 and 12 tuples whose three
    middle columns cancel to exactly 0.  On a narrow matrix the rows need more tuples (ncol = 1: one per product) and some
    coincide: a shape is taken once.  Every row has another count of products or columns."""
    rng = np.random.default_rng([ncol, 7])
    F = FEW_MAX_DEFAULT
    rows, shapes = [], set()
    kinds = ["all", "bitmap", "pairs", "ends"]

    def add(name, L, P, D, cancel=0):
        D = min(D, ncol, P)
        L = max(L, ceil_div(P, D))
        if (L, P, D) in shapes:
            return
        shapes.add((L, P, D))
        cols = columns(ncol, D, rng, "all" if name.startswith("full") else kinds[len(rows) % 4])
        canc = [int(c) for c in cols[max(0, D // 2 - 1):D // 2 + 2]] if cancel else []
        rows.append((name, deal(L, cols, P), canc))

    for T, lo, hi in CLASSES:
        add("lo%d" % T, 1, lo, lo)
        add("full%d_few" % T, 1, hi, hi)
        mid = (lo + hi) // 2 + T // 512
        if F * ncol >= lo:
            add("few_max%d" % T, F, min(mid, F * ncol), (2 * mid) // 3)
        add("full%d_hash" % T, F + 1, hi, hi)
    D = min(ncol, 100)
    add("repeat", 3, max(3, ceil_div(70, D)) * D, D)
    for name, m, D in (("cancel_few", 1, 150), ("cancel_hash", 3, 170)):
        D = min(ncol, D)
        m = max(m, ceil_div(33, D))
        add(name, 4 * m, 2 * m * D, D, cancel=1)
    return rows


SMALL = (1, 2, 64, 65, 513)
EDGES = tuple(w for k in (15, 17, 18, 20, 21, 23) for w in (1 << k, (1 << k) + 1))
TOP = 1 << 31                           # the widest shape check_operand accepts
WIDTHS = SMALL + EDGES + (TOP,)
SCALE_BELOW = 1 << 26                   # upload_scale allocates four bytes per column: no scale vectors from here on


@functools.lru_cache(maxsize=None)
def width_case(ncol):
    rows = width_rows(ncol)
    c = case(ncol, [(segs, canc) for name, segs, canc in rows])
    c.names = {name: i for i, (name, segs, canc) in enumerate(rows)}
    return c


def scales(c):
    """C != 1, scalei (a row absent, one 0) and scalek over the columns op(B) holds (every fifth of them absent: dropped
    outputs shift the ranks behind them), all powers of two."""
    nrow = c.A.shape[0]
    i = np.arange(nrow)
    si = orc.Vec(i[i % 7 != 3], np.where(i % 5 == 4, 0.0, np.array([0.5, 1.0, 2.0, -1.0])[i % 4])[i % 7 != 3], nrow)
    j = np.unique(c.B.idx1)
    j = j[np.arange(j.size) % 5 != 2]
    sk = orc.Vec(j, np.array([1.0, 2.0, -0.5])[j % 3], c.ncol)
    return dict(C_=-2.0, scalei=si, scalek=sk)


_WANT = {}


def oracle_tuples(c, scaled=False, **kw):
    """The oracle's (i, j, v) of a case: computed once, never changed."""
    key = (id(c), scaled, tuple(sorted(kw.items())))
    if key not in _WANT:
        args = dict(scales(c), **kw) if scaled else kw
        _WANT[key] = (c, orc.multiply(c.A, c.B, rowwise=True, nthreads=1, **args)[:3])
    return _WANT[key][1]


def row_stats(want, nrow):
    """(row_nnz, row_hash) of tuples, as SINK_ROWSTATS reports them."""
    i, j = np.asarray(want[0], np.int64), np.asarray(want[1], np.int64)
    nnz = np.bincount(i, minlength=nrow).astype(np.int64)
    h = np.zeros(nrow, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(h, i, orc.mix64(i, j))
    return nnz, h


# ---- heavy rows: one hash cell per row, at the bottom and at the top of the column range ---------------------------------

NWIN = 2048                             # the most windows of one pass: 2^24 columns of 8192, 2^25 of 16384
SPANS = (1, 2, 3, 4, 5)
# (distinct columns, products) of a cell per table: 3072 with more than 1024 outputs (the bitonic network then sorts 2048 keys)
CELL = {1024: (400, 500), 3072: (1300, 1500), 4096: (1700, 2000), 8192: (2600, 3000), "tiles": (1500, 1900)}
WINDOW_CASES = [(T, W, where) for T in (1024, 3072, 4096, 8192, "tiles") for W in (8192, 16384) for where in ("low", "high")]


def spans_of(T, W):
    """1 .. 5 windows; 9 of 16384 columns for the tables of 4096, whose first radix width is 18 bits."""
    return SPANS + ((9,) if W == 16384 and T in (4096, "tiles") else ())


def cell_colbits(W, wa, wb):
    """colbits of a cell over the windows [wa, wb), as the kernels compute it."""
    return {8192: 13, 16384: 14}[W] + (int(wb - wa - 1).bit_length() if wb - wa > 1 else 0)


@functools.lru_cache(maxsize=None)
def window_case(T, W, where):
    """One row per span: a cell of CELL[T] over exactly that many windows, from the matrix's first column (low) or up to
    its last (high), whose columns take the range's ends, the bitmap's word and superblock edges and a spread between;
    a third of its columns are held by two tuples.  A dense window makes every row heavy.  Rows of 300 tuples are too long
    for a tile (windowed k_hash), those of 64 go to the hash tiles.  The knobs are hash_windowed's (tile_plan)."""
    b = tp.Builder(NWIN, W)
    L = 64 if T == "tiles" else 300
    D, P = CELL[T]
    dmin = tp.DENSE_MIN_BITMAP if T == 8192 else tp.DENSE_MIN_DEFAULT
    for span in spans_of(T, W):
        wa = 0 if where == "low" else NWIN - span
        lo, hi = wa * W, (wa + span) * W
        sp = [lo + 1, lo + 63, lo + 64, lo + 255, lo + 256, hi - 64, hi - 2]
        cols = np.union1d(tp.spread(D, lo, hi), sp)
        spare = np.setdiff1d(cols, sp + [lo, hi - 1])
        cols = np.setdiff1d(cols, spare[1:1 + cols.size - (D - span)])       # D - span distinct columns: every row another count
        fill = tp.dense_window(L, NWIN // 2 + span, W, n=max(dmin + 52, MID_MAX + 64 - P))
        b.row(tp.join(tp.deal(L, cols, P + cols.size - D), fill), seed=span)
    if T == 8192:
        kn, schemes = {"long_cap": 4096, "long_dense_min": 4096}, (tp.BITMAP,)
    elif T == "tiles":
        kn, schemes = {}, (tp.HASH2, tp.HASH1)
    else:
        kn, schemes = {"long_dense_min": 2048}, (tp.HASH2,)
    p = tp.Plan(b, schemes=schemes, knobs=kn, **kn)
    p.kind = "tile" if T == "tiles" else "hash%d" % T
    return p


def planned_cells(p, scheme, kind):
    """[(wa, wb, products, colbase, colbits, path)] of the plan's cells of a kind under a scheme (COO sink)."""
    kern, T = ("tiles", 4096) if kind == "tile" else ("k_hash", int(kind[4:]))
    out = []
    for L, wp, cells, tiles in p.cut(scheme).rows:
        for k, wa, wb, prods in cells:
            if k == kind:
                cb = cell_colbits(p.W, wa, wb)
                out.append((wa, wb, prods, wa * p.W, cb, emit_path(kern, T, cb)))
    return out
