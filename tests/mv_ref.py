"""Seeded inputs for the matrix x vector entry point and for products with a narrow right operand, and the row classes
they reach (tests/test_mv_host.py pins them without a GPU, tests/test_gpu_mv.py runs them on the device).

    row_lengths(rng, k)               every class boundary of the product path and its neighbours, the two very long
                                      rows, a full row, and ~180 random lengths
    long_row_matrix(rng, k, lens..)   COO matrix, row r with exactly lens[r] distinct columns, shuffled storage order
    dense_vec / sparse_vec / messy_vec / ones_vec
    cancel_matrix(k)                  rows of (+x, -x) pairs, rows that cancel only in ascending k, rows that do not
    narrow_b(rng, k, n, nnz)          k x n right operand whose first DENSE_K rows are full
    row_classes(A, B_or_V, ...)       products per output row and the light / mid / heavy counts, in numpy, from the
                                      consolidated operands -- what spsamd_result's rows_* / products_* must report

The classes are those of spsparse_amd/csrc/spgemm.hip: a row with P_r scalar products is light for 1 <= P_r <= 64, mid
up to 4096, heavy above; a heavy row with at most 256 tuples of op(A) is a tile row.  In an MV product P_r is the number
of the row's tuples whose inner index V holds, so with a dense V it is the row's length.
"""
import numpy as np

from oracle import binding as orc

LIGHT_MAX, MID_MAX, TILE_LMAX = 64, 4096, 256
BOUNDARY_LENS = (0, 1, 2, 63, 64, 65, 66, 255, 256, 257, 1024, 1025, 3072, 3073, 4095, 4096, 4097, 4098,
                 8191, 8192, 8193, 20000, 150000)
NARROW_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193)
DENSE_K = 512                       # narrow_b fills its first DENSE_K rows; the tile rows of long_row_matrix live on them


def row_lengths(rng, k, n_random=180):
    """The boundary lengths that fit k columns, a full row, and n_random lengths in 1 ... min(9000, k)."""
    fixed = [n for n in BOUNDARY_LENS if n <= k] + [k]
    return np.concatenate([np.array(fixed, np.int64), rng.integers(1, min(9000, k) + 1, n_random)])


def _values(rng, n, signed):
    v = rng.uniform(0.1, 1.0, n)
    return v * rng.choice([-1.0, 1.0], n) if signed else v


def long_row_matrix(rng, k, lens, signed=False, dups=0, zeros=0, tile_rows=0):
    """orc.Mat of len(lens) + tile_rows rows over k columns.  Row r holds lens[r] distinct columns with non-zero values;
    `dups` more tuples repeat the indices of random ones (new values), `zeros` more are explicit zeros at random
    places.  The tile_rows extra rows hold 200 ... 256 columns below DENSE_K each.  Storage order is shuffled."""
    lens = np.asarray(lens, np.int64)
    assert lens.max(initial=0) <= k
    cols = [rng.choice(k, size=int(n), replace=False) for n in lens]
    rows = [np.full(int(n), r, np.int64) for r, n in enumerate(lens)]
    for t in range(tile_rows):
        n = int(rng.integers(200, TILE_LMAX + 1))
        cols.append(rng.choice(min(DENSE_K, k), size=n, replace=False))
        rows.append(np.full(n, len(lens) + t, np.int64))
    i0, i1 = np.concatenate(rows), np.concatenate(cols)
    v = _values(rng, i0.size, signed)
    nrow = len(lens) + tile_rows
    if dups:
        pick = rng.integers(0, i0.size, dups)
        i0, i1, v = np.concatenate([i0, i0[pick]]), np.concatenate([i1, i1[pick]]), np.concatenate([v, _values(rng, dups, signed)])
    if zeros:
        i0 = np.concatenate([i0, rng.integers(0, nrow, zeros)])
        i1 = np.concatenate([i1, rng.integers(0, k, zeros)])
        v = np.concatenate([v, np.zeros(zeros)])
    o = rng.permutation(i0.size)
    return orc.Mat(i0[o], i1[o], v[o], (nrow, k))


def transposed(A):
    """The same matrix stored the other way round (to be used with 'T')."""
    return orc.Mat(A.idx1, A.idx0, A.val, (A.shape[1], A.shape[0]), -1)


def absolute(X):
    """|X| for the error bound: the oracle run on it gives the sum of |terms| of every output."""
    if X is None:
        return None
    if isinstance(X, orc.Vec):
        return orc.Vec(X.idx, np.abs(X.val), X.shape0, X.sort0)
    return orc.Mat(X.idx0, X.idx1, np.abs(X.val), X.shape, X.sort0)


def dense_vec(rng, k, signed=False):
    """Every index once, in shuffled storage order."""
    return orc.Vec(rng.permutation(k), rng.uniform(0.5, 2.0, k) * (rng.choice([-1.0, 1.0], k) if signed else 1.0), k)


def sparse_vec(rng, k, density=0.3, signed=False):
    idx = rng.permutation(np.flatnonzero(rng.random(k) < density))
    if idx.size == 0:
        idx = np.array([0])
    return orc.Vec(idx, rng.uniform(0.5, 2.0, idx.size) * (rng.choice([-1.0, 1.0], idx.size) if signed else 1.0), k)


def messy_vec(rng, k, draws=None):
    """Indices drawn with replacement (duplicates), a tenth of the values explicit zeros, unsorted."""
    n = int(draws if draws is not None else max(1, k // 2))
    idx = rng.integers(0, k, n)
    val = rng.uniform(0.5, 2.0, n)
    val[rng.random(n) < 0.1] = 0.0
    return orc.Vec(idx, val, k)


def ones_vec(k):
    return orc.Vec(np.arange(k), np.ones(k), k, 0)


def scale_vec(rng, n, density=0.8):
    """Ascending scale vector over part of [0, n) with some zero entries (absent and zero scales both occur)."""
    idx = np.flatnonzero(rng.random(n) < density)
    if idx.size == 0:
        idx = np.array([0])
    val = rng.uniform(0.5, 2.0, idx.size)
    val[rng.random(idx.size) < 0.1] = 0.0
    return orc.Vec(idx, val, n)


# lengths of the rows of cancel_matrix: light, mid and heavy against an all-ones V (multiples of 6)
CANCEL_LENS = (6, 60, 600, 3000, 6000, 12000)


def cancel_matrix(k):
    """Three rows per length L of CANCEL_LENS, on the columns 0 ... L-1, for a product with ones_vec(k):
      row 3q      (+x, -x) pairs of small integers: the sum is exactly 0 in every order
      row 3q + 1  triples (1e16, 1, -1e16): 0 only when summed in ascending k ((1e16 + 1) - 1e16 == 0)
      row 3q + 2  triples (1e16, -1e16, 1): 1 in ascending k, never 0
    Returns (orc.Mat, kinds) with kinds[r] in {"pairs", "ascending", "kept"}."""
    assert k >= max(CANCEL_LENS)
    i0, i1, v, kinds = [], [], [], []
    for q, L in enumerate(CANCEL_LENS):
        x = np.repeat(np.arange(1, L // 2 + 1) % 7 + 1.0, 2) * np.tile([1.0, -1.0], L // 2)
        for kind, vals in (("pairs", x), ("ascending", np.tile([1e16, 1.0, -1e16], L // 3)), ("kept", np.tile([1e16, -1e16, 1.0], L // 3))):
            i0.append(np.full(L, len(kinds)))
            i1.append(np.arange(L))
            v.append(vals)
            kinds.append(kind)
    return orc.Mat(np.concatenate(i0), np.concatenate(i1), np.concatenate(v), (len(kinds), k)), kinds


def narrow_b(rng, k, n, nnz, signed=False):
    """orc.Mat of shape (k, n): nnz tuples at random places (duplicates occur, the more the narrower) and the first
    min(DENSE_K, k) rows full, in shuffled storage order."""
    d = min(DENSE_K, k)
    i0 = np.concatenate([rng.integers(0, k, nnz), np.repeat(np.arange(d), n)])
    i1 = np.concatenate([rng.integers(0, n, nnz), np.tile(np.arange(n), d)])
    o = rng.permutation(i0.size)
    return orc.Mat(i0[o], i1[o], _values(rng, i0.size, signed), (k, n))


def as_column(V):
    """The vector as the k x 1 matrix the MV entry point multiplies by."""
    return orc.Mat(V.idx, np.zeros(V.nnz, np.int32), V.val, (V.shape0, 1), 0 if V.sort0 == 0 else -1)


class RowClasses:
    """products[r] for every row of op(A); the counts of the three classes and their products."""

    def __init__(self, products, a_len, b_maxlen):
        P = self.products = products
        self.a_len = a_len
        light, mid, heavy = (P >= 1) & (P <= LIGHT_MAX), (P > LIGHT_MAX) & (P <= MID_MAX), P > MID_MAX
        self.rows_light, self.rows_mid, self.rows_heavy = int(light.sum()), int(mid.sum()), int(heavy.sum())
        self.products_light, self.products_mid, self.products_heavy = int(P[light].sum()), int(P[mid].sum()), int(P[heavy].sum())
        self.total = int(P.sum())
        self.tile_rows_heavy = int((heavy & (a_len <= TILE_LMAX)).sum())
        # (longest row of op(A)) x (longest row of op(B)) <= 64: the product takes the direct kernel, which reports every
        # row of op(A), empty ones included, as light
        self.all_light = int(a_len.max(initial=0)) * int(b_maxlen) <= LIGHT_MAX

    def at(self, p):
        return int((self.products == p).sum())


def row_classes(A, B, tA='.', tB='.', scalei=None, scalej=None, duplicate_policy=orc.ADD, zero_nan=False):
    """RowClasses of op(A) * op(B); B an orc.Mat or an orc.Vec (MV).  Both operands are consolidated first (duplicate
    policy, zero drop) as the product does.  A tuple of A whose inner index scalej lacks gives no product; a row that
    scalei lacks or scales by 0 gives none either; scalek does not enter."""
    a0, a1, _ = orc.consolidate(A.idx0, A.idx1, A.val, 1 if tA == 'T' else 0, duplicate_policy, zero_nan)
    arow, ainner = (a1, a0) if tA == 'T' else (a0, a1)
    nrow, ninner = (A.shape[1], A.shape[0]) if tA == 'T' else A.shape
    if isinstance(B, orc.Vec):
        binner = orc.consolidate(B.idx, None, B.val, 0, duplicate_policy, zero_nan)[0]
    else:
        b0, b1, _ = orc.consolidate(B.idx0, B.idx1, B.val, 1 if tB == 'T' else 0, duplicate_policy, zero_nan)
        binner = b1 if tB == 'T' else b0
    blen = np.bincount(binner, minlength=ninner).astype(np.int64)
    if scalej is not None:
        present = np.zeros(ninner, bool)
        present[scalej.idx] = True
        blen = blen * present
    P = np.bincount(arow, weights=blen[ainner].astype(np.float64), minlength=nrow).astype(np.int64)
    if scalei is not None:
        live = np.zeros(nrow, bool)
        live[scalei.idx[scalei.val != 0]] = True
        P = P * live
    return RowClasses(P, np.bincount(arow, minlength=nrow).astype(np.int64), np.bincount(binner, minlength=ninner).max(initial=0))
