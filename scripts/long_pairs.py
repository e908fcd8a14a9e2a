"""Developer tool, CPU only: what the hash cells of the long rows (more than 256 A tuples) of R-MAT scale-S A*A visit.

    python scripts/long_pairs.py [scale] [window shift]

A port of scripts/window_stats.py restricted to the rows the windowed k_hash launches run, with the greedy grouping of
k_cells (cell cap 2048, the long rows' dense threshold 1024): the long rows and their lengths, the hash cells by class,
the (cell, A tuple) pairs a cell's walk over its row visits, and how many of them select a non-empty B segment -- counted
exactly and as the sum over the cell's windows, which is an upper bound.  What profiles/longrows/README.md quotes."""
import sys

import numpy as np

from spsparse_amd import workloads as wl

S = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WSH = int(sys.argv[2]) if len(sys.argv) > 2 else 13
CELL_CAP, LONG_DENSE_MIN, TILE_LMAX, HEAVY = 2048, 1024, 256, 4096

n = 1 << S
r, c, _, _ = wl.rmat(S, seed=1)
key = np.unique(r.astype(np.int64) * n + c)
row, col = key // n, key % n
blen = np.bincount(row, minlength=n)
ptr = np.concatenate([[0], np.cumsum(blen)])
nwin = max(1, n >> WSH)
P = np.bincount(row, weights=blen[col], minlength=n)
long_rows = np.flatnonzero((P > HEAVY) & (blen > TILE_LMAX))
cnt_kw = np.bincount(row * nwin + (col >> WSH), minlength=n * nwin).reshape(n, nwin).astype(np.uint16)
L = blen[long_rows]
print("long rows %d, A tuples %.4g; lengths: median %d, 99th percentile %d, maximum %d" % (
    long_rows.size, L.sum(), np.median(L), np.quantile(L, 0.99), L.max()))

ncls = [0, 0, 0]
cells = pairs = prods = ne_exact = ne_bound = 0
for rr in long_rows:
    ks = col[ptr[rr]:ptr[rr + 1]]
    seg = cnt_kw[ks]                                                # [tuple][window]: the segment lengths
    wp = seg.sum(axis=0, dtype=np.int64)
    occ = np.concatenate([np.zeros((ks.size, 1), np.int32), np.cumsum(seg > 0, axis=1, dtype=np.int32)], axis=1)
    cur = start = last = 0

    def flush():
        global cells, pairs, prods, ne_exact, ne_bound, cur
        if not cur:
            return
        ncls[0 if cur <= 512 else (1 if cur <= 1536 else 2)] += 1
        cells += 1
        pairs += ks.size
        prods += cur
        hit = occ[:, last + 1] - occ[:, start]
        ne_exact += int(np.count_nonzero(hit))
        ne_bound += int(hit.sum())
        cur = 0
    for w in range(nwin):
        cw = int(wp[w])
        if cw > LONG_DENSE_MIN:
            flush()
        elif cw > CELL_CAP:
            flush()
            cur, start, last = cw, w, w
            flush()
        elif cw > 0:
            if cur + cw > CELL_CAP:
                flush()
            if not cur:
                start = w
            cur += cw
            last = w
    flush()
print("hash cells %d: %d of at most 512 products, %d of at most 1536, %d of at most 2048; products %d" % (cells, ncls[0], ncls[1], ncls[2], prods))
print("(cell, A tuple) pairs %.4g, %.3f products per pair" % (pairs, prods / max(1, pairs)))
print("pairs with a non-empty B segment: %.4g exactly (%.1f %%); summed over windows %.4g (%.1f %%, an upper bound)" % (
    ne_exact, 100.0 * ne_exact / max(1, pairs), ne_bound, 100.0 * ne_bound / max(1, pairs)))
