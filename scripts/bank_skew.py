#!/usr/bin/env python3
"""How unevenly the product columns of an R-MAT A*A fall on the LDS banks of k_dense and k_bm_tiles, and what a
bijective remap of the address returns (CPU only).

    python scripts/bank_skew.py [scale=16] [rows=60]

The generator scrambles no vertices: every column bit is set with probability 0.24, independently, so addresses taken
from low column bits crowd the banks whose index has few set bits.
  real columns  the product columns of the heaviest rows: share of the products in the fullest bank
                (k_dense: bank pair = slot mod 16 of the ds_add_f64; k_bm_tiles: dword = (rel >> 5) mod 32 of the ds_or)
  model         64 lanes draw independent columns with that bit distribution; a wave-instruction costs, per lane
                group, the largest number of distinct addresses on one bank (issue and latency effects ignored)
The constants of csrc/bank_layout.h were chosen with the candidate lists below.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spsparse_amd import workloads as wl  # noqa: E402

W = 8192
TILE_BITS = 17
TILE_MASK = (1 << TILE_BITS) - 1
TILE_LOW = (1 << 14) - 1
P1 = 0.24


# ---- candidate remaps (uint32 arrays in, uint32 arrays out) --------------------------------------------------------
def dense_plain(slot):
    return slot


def dense_xor(slot):
    g = slot >> 6
    return slot ^ ((g ^ (g >> 5)) & 31)


def dense_mul(c, sh):
    def f(slot):
        return slot ^ ((((slot >> 6) * np.uint32(c)) >> np.uint32(sh)) & np.uint32(63))
    f.__name__ = "dense_mul(%d,%d)" % (c, sh)
    return f


def tile_plain(rel):
    return rel


def tile_mul(c):
    def f(rel):
        return (rel & np.uint32(TILE_MASK & ~TILE_LOW)) | ((rel * np.uint32(c)) & np.uint32(TILE_LOW))      # (bits 14..16 stay: bank_layout.h)
    f.__name__ = "tile_mul(%d)" % c
    return f


DENSE = [dense_plain, dense_xor] + [dense_mul(c, sh) for c, sh in ((37, 2), (45, 2), (109, 3), (181, 3), (91, 2), (211, 4))]
TILES = [tile_plain] + [tile_mul(c) for c in (40503, 25743, 60493, 46021, 77821, 109441, 2654435761 & TILE_MASK | 1)]


# ---- inputs --------------------------------------------------------------------------------------------------------
def product_columns(scale, nrows):
    r, c, _, (n, _) = wl.rmat(scale, seed=1)
    key = np.unique(r.astype(np.int64) * n + c)
    r, c = (key // n).astype(np.int64), (key % n).astype(np.uint32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
    deg = np.diff(ptr)
    prods = np.bincount(r, weights=deg[c], minlength=n)
    out = []
    for i in np.argsort(-prods)[:nrows]:
        for k in c[ptr[i]:ptr[i + 1]]:
            out.append(c[ptr[k]:ptr[k + 1]])
    return np.concatenate(out)


def iid_columns(rng, n, bits, p):
    x = np.zeros(n, dtype=np.uint32)
    for b in range(bits):
        x |= (rng.random(n) < p).astype(np.uint32) << np.uint32(b)
    return x


# ---- measures ------------------------------------------------------------------------------------------------------
def fullest(bank, nbank):
    return np.bincount(bank, minlength=nbank).max() / bank.size


def cycles(addr, bank, nbank, group):
    """Mean cycles of a 64-lane instruction: per lane group, the most distinct addresses on one bank."""
    n = addr.size // 64 * 64
    a = addr[:n].astype(np.int64).reshape(-1, group)
    b = bank[:n].astype(np.int64).reshape(-1, group)
    k = np.sort(b * (1 << 32) + a, axis=1)
    first = np.ones(k.shape, dtype=bool)
    first[:, 1:] = k[:, 1:] != k[:, :-1]
    gi = np.repeat(np.arange(k.shape[0]), group).reshape(k.shape)
    load = np.bincount((gi * nbank + (k >> 32))[first], minlength=k.shape[0] * nbank).reshape(-1, nbank)
    return load.max(axis=1).reshape(-1, 64 // group).sum(axis=1).mean()


def dense_row(f, cols, model):
    s = f(cols & np.uint32(W - 1))
    m = f(model & np.uint32(W - 1))
    return fullest(s & 15, 16), cycles(m, m & 15, 16, 16), cycles(m, m & 15, 16, 32)


def tiles_row(f, cols, model):
    k = f(cols & np.uint32(TILE_MASK))
    m = f(model & np.uint32(TILE_MASK))
    return (fullest((k >> 5) & 31, 32), cycles(m >> 5, (m >> 5) & 31, 32, 32), cycles(m >> 6, (m >> 6) & 31, 32, 32),
            cycles(m >> 7, (m >> 7) & 31, 32, 32))


def main():
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    nrows = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    cols = product_columns(scale, nrows)
    rng = np.random.default_rng(1)
    model = iid_columns(rng, 64 * 20000, TILE_BITS, P1)
    uni = rng.integers(0, 1 << TILE_BITS, size=model.size, dtype=np.uint32)
    print("R-MAT scale %d, %d heaviest rows, %d products; bits 0..12 set in %s %% of them" % (scale, nrows, cols.size,
          " ".join("%.0f" % (100.0 * ((cols >> b) & 1).mean()) for b in range(13))))
    print("\nk_dense: fullest bank pair (real) | ds_add_f64 cycles 4 x 16 lanes | 2 x 32 lanes (model)")
    for f in DENSE:
        print("  %-22s %5.1f %%   %5.1f   %5.1f" % ((f.__name__,) + tuple(x * (100 if i == 0 else 1) for i, x in enumerate(dense_row(f, cols, model)))))
    print("  %-22s %5.1f %%   %5.1f   %5.1f" % (("uniform columns",) + tuple(x * (100 if i == 0 else 1) for i, x in enumerate(dense_row(dense_plain, uni, uni)))))
    print("\nk_bm_tiles: fullest dword of the ds_or (real) | cycles of ds_or | bm[w] read | bpre[w] read (model)")
    for f in TILES:
        print("  %-22s %5.1f %%   %5.1f   %5.1f   %5.1f" % ((f.__name__,) + tuple(x * (100 if i == 0 else 1) for i, x in enumerate(tiles_row(f, cols, model)))))
    print("  %-22s %5.1f %%   %5.1f   %5.1f   %5.1f" % (("uniform columns",) + tuple(x * (100 if i == 0 else 1) for i, x in enumerate(tiles_row(tile_plain, uni, uni)))))


if __name__ == "__main__":
    main()
