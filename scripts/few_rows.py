"""Developer tool, CPU only: the rows of R-MAT scale-S A*A whose A row has few tuples, and what they cost today.

    python scripts/few_rows.py [scale] [window shift]

Mid rows (65 .. 4096 products): how many A tuples they have (L), how long the B segments are that they read.  Heavy rows
by L: rows, products, and a replay of k_cells' greedy grouping -- the tile cells of today (dense threshold 3072, cap 4096,
at most 16 windows a cell) and the cells the same rows would make with no span cap at caps 4096 and 2048.  What
profiles/few/README.md quotes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spsparse_amd import workloads as wl

S = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WSH = int(sys.argv[2]) if len(sys.argv) > 2 else 13
MID_MIN, MID_MAX, DENSE_MIN, TILE_CAP, TILE_SPAN = 64, 4096, 3072, 4096, 16
CLASSES = ((1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 64))

n = 1 << S
r, c, _, _ = wl.rmat(S, seed=1)
key = np.unique(r.astype(np.int64) * n + c)
row, col = key // n, key % n
blen = np.bincount(row, minlength=n)
ptr = np.concatenate([[0], np.cumsum(blen)])
nwin = max(1, n >> WSH)
P = np.bincount(row, weights=blen[col], minlength=n).astype(np.int64)


def label(lo, hi):
    return "%d" % lo if lo == hi else "%d-%d" % (lo, hi)


# ---- mid rows
mid = (P > MID_MIN) & (P <= MID_MAX)
print("mid rows %d, A tuples %d (%.2f a row), products %.4g" % (mid.sum(), blen[mid].sum(), blen[mid].sum() / max(1, mid.sum()), P[mid].sum()))
for lo, hi in CLASSES + ((65, 1 << 30),):
    sel = mid & (blen >= lo) & (blen <= hi)
    print("  L %-8s rows %8d  products %.4g" % (label(lo, hi) if hi < 1 << 30 else "above 64", sel.sum(), P[sel].sum()))
for name, lo, hi in (("T = 1024", 64, 512), ("T = 4096", 512, 2048), ("T = 8192", 2048, 4096)):
    sel = (P > lo) & (P <= hi)
    print("  class %s: rows %d (L <= 8: %d, L <= 16: %d), products %.4g" % (name, sel.sum(), (sel & (blen <= 8)).sum(), (sel & (blen <= 16)).sum(), P[sel].sum()))
seg = blen[col[mid[row]]]                                           # one entry per A tuple of a mid row: the B segment it selects
seg = seg[seg > 0]
order = np.sort(seg)
cum = np.cumsum(order)
print("  B segments read: %d non-empty, median %d tuples; by products: median segment %d tuples, %.3f %% of the products in segments of <= 10" % (
    seg.size, np.median(seg), order[np.searchsorted(cum, cum[-1] / 2)], 100.0 * order[order <= 10].sum() / cum[-1]))
print("  bytes of B read: %.3g" % (12.0 * seg.sum()))

# ---- heavy rows by L: the greedy grouping of k_cells replayed
heavy = np.flatnonzero((P > MID_MAX) & (blen <= 64))
cnt_kw = np.bincount(row * nwin + (col >> WSH), minlength=n * nwin).reshape(n, nwin).astype(np.uint16)


def greedy(wp, cap, span):
    """(hash cells, dense cells) of a row with window products wp: a window above DENSE_MIN is a dense cell, the others
    are grouped in window order into cells of at most `cap` products and `span` windows (0: any)."""
    cells = dense = cur = start = 0
    for w in np.flatnonzero(wp):
        cw = int(wp[w])
        if cw > DENSE_MIN:
            cells += cur > 0
            cur = 0
            dense += 1
            continue
        if cur and (cur + cw > cap or (span and w - start >= span)):
            cells += 1
            cur = 0
        if not cur:
            start = w
        cur += cw
    return cells + (cur > 0), dense


stats = {k: [0, 0, 0, 0, 0, 0] for k in CLASSES}                    # rows, products, tile cells, dense cells, any-span cells at 4096, at 2048
for rr in heavy:
    wp = cnt_kw[col[ptr[rr]:ptr[rr + 1]]].sum(axis=0, dtype=np.int64)
    k = next(kk for kk in CLASSES if kk[0] <= blen[rr] <= kk[1])
    t, d = greedy(wp, TILE_CAP, TILE_SPAN)
    s = stats[k]
    s[0] += 1; s[1] += int(P[rr]); s[2] += t; s[3] += d
    s[4] += greedy(wp, 4096, 0)[0]; s[5] += greedy(wp, 2048, 0)[0]
print("heavy rows with at most 64 A tuples: %d" % heavy.size)
print("  %-6s %8s %10s %12s %8s %14s %10s" % ("L", "rows", "products", "tile cells", "dense", "any span 4096", "cap 2048"))
for k in CLASSES:
    s = stats[k]
    print("  %-6s %8d %10.3g %12d %8d %14d %10d" % ((label(*k),) + tuple(s)))
le8 = [sum(stats[k][i] for k in CLASSES[:4]) for i in range(6)]
print("  L <= 8: tile cells %d, products %.4g, any-span cells %d (cap 4096)" % (le8[2], le8[1], le8[4]))
