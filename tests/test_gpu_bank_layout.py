"""The LDS bank layouts of the heavy-row kernels (csrc/bank_layout.h): k_dense accumulates column s of a window in a
swizzled slot and un-swizzles at the scan-out; k_bm_tiles' digest and plain COUNT launches know a column by a scrambled
key and recover it per output.  A slot or key mapped back wrongly moves a value to another column, so the inputs give
every output column its own value and touch every slot, group edge and window edge.

All values are small integers: every sum is exact in any order, and results compare bit for bit with the oracle -- the
COO sink tuple for tuple in ascending order, the digest sink in count, hash and value sum.  The counters of the result
show that the kernel under test took the products.  The input plans are checked on the CPU first (no GPU needed)."""
import functools

import numpy as np
import pytest

from oracle import binding as orc
from tests.gpu_util import check_tuples, ctx, forced  # noqa: F401  (ctx: fixture)

gpu = pytest.mark.gpu

BITMAP_TILES = 3            # the "tiles_v1" value that forces k_bm_tiles (tests/test_gpu_parity.py, every cell scheme)
W_SMALL, W_LARGE = 8192, 16384
MID_MAX, DENSE_MIN_BITMAP, BM_CELL = 4096, 3072, 4096          # a row above MID_MAX products is heavy; a window from DENSE_MIN_BITMAP on is a dense cell; a bitmap cell holds BM_CELL products


# ---- inputs ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def every_slot(W, signed):
    """A: 1 x 8, all ones.  B: 8 x W, row k holds every column j with (j + k) even, value j + 1: 4 W products, every
    column hit four times, C(0, j) = 4 (j + 1).  signed: in the columns j = 0 mod 5 the four terms are +, -, +, - and
    cancel exactly."""
    A = orc.Mat(np.zeros(8, np.int32), np.arange(8), np.ones(8), (1, 8))
    k = np.repeat(np.arange(8), W // 2)
    j = np.concatenate([np.arange(kk & 1, W, 2) for kk in range(8)])
    v = (j + 1).astype(np.float64)
    if signed:
        v = np.where((j % 5 == 0) & ((k // 2) % 2 == 1), -v, v)
    return A, orc.Mat(k, j, v, (8, W))


FEW_COLUMNS = [0, 1, 31, 32, 63, 64, 65, 4095, 4096, 8127, 8128, 8191] + [g * 64 + (g * 7) % 64 for g in (5, 17, 33, 50, 77, 90, 101, 120)]


@functools.lru_cache(maxsize=None)
def few_columns():
    """A: 1 x 4200, all ones.  B: 4200 x 8192, one tuple a row, its column cycling through FEW_COLUMNS (the edges of
    64-slot groups, of the window's halves and of the window, and one column in each of eight further groups); the
    value is the column's place in the list + 1, so C(0, column q) = 210 (q + 1)."""
    n = 4200
    A = orc.Mat(np.zeros(n, np.int32), np.arange(n), np.ones(n), (1, n))
    q = np.arange(n) % len(FEW_COLUMNS)
    return A, orc.Mat(np.arange(n), np.asarray(FEW_COLUMNS)[q], (q + 1).astype(np.float64), (n, W_SMALL))


TILE_NCOL = 17 * W_SMALL                                          # 139 264: one window more than a bitmap cell spans
TILE_EDGES = [0, 63, 64, 131071, 131072, 139263]


@functools.lru_cache(maxsize=None)
def tile_rows(signed):
    """A: 1 x 64, all ones.  B: 64 x 139264, 80 columns a row: 40 shared by every row (the edges of the first bitmap
    word, of the 2^17 keys and of the matrix among them) and 40 that no other row has.  5120 products over 17 windows,
    no window near a dense cell's size.  A shared column's value is 1 + its place mod 3, a unique one's 1 + row mod 4.
    signed: every third shared column has + on even rows and - on odd rows and cancels exactly."""
    rng = np.random.default_rng(77)
    rest = np.setdiff1d(np.arange(TILE_NCOL), TILE_EDGES)
    pick = rng.choice(rest, 34 + 64 * 40, replace=False)
    shared = np.concatenate([TILE_EDGES, pick[:34]])
    uniq = pick[34:].reshape(64, 40)
    rows, cols, vals = [], [], []
    for r in range(64):
        sv = 1.0 + (np.arange(40) % 3)
        if signed:
            sv = np.where((np.arange(40) % 3 == 0) & (r % 2 == 1), -sv, sv)
        c = np.concatenate([shared, uniq[r]])
        v = np.concatenate([sv, np.full(40, 1.0 + r % 4)])
        o = np.argsort(c)
        rows.append(np.full(80, r)); cols.append(c[o]); vals.append(v[o])
    A = orc.Mat(np.zeros(64, np.int32), np.arange(64), np.ones(64), (1, 64))
    return A, orc.Mat(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals), (64, TILE_NCOL))


def column_scale(ncol, drop, scale):
    """scalek: columns with j % drop == 0 absent (their outputs are skipped), the others scaled by 1 or `scale`."""
    j = np.arange(ncol)
    j = j[j % drop != 0]
    return orc.Vec(j, np.where(j % 2 == 0, 1.0, float(scale)), ncol)


@functools.lru_cache(maxsize=None)
def oracle_tuples(name, *args, scalek=None):
    A, B = INPUTS[name](*args)
    kw = {"scalek": column_scale(B.shape[1], *scalek)} if scalek else {}
    return orc.multiply(A, B, rowwise=True, nthreads=4, **kw)[:3]


INPUTS = {"every_slot": every_slot, "few_columns": few_columns, "tile_rows": tile_rows}


def window_products(A, B, wshift):
    """Products of A's single row per column window of B."""
    deg_in_window = np.zeros((B.shape[0], (B.shape[1] >> wshift) + 1), np.int64)
    np.add.at(deg_in_window, (B.idx0, B.idx1 >> wshift), 1)
    return deg_in_window[A.idx1].sum(axis=0)


# ---- the plans, on the CPU -----------------------------------------------------------------------------------------

def test_inputs_give_the_planned_cells():
    """Row classes and cell kinds follow from the products per row and window: checked here from the operands and the
    oracle's output alone."""
    for W, wshift in ((W_SMALL, 13), (W_LARGE, 14)):
        A, B = every_slot(W, False)
        wp = window_products(A, B, wshift)
        assert wp.sum() == 4 * W > MID_MAX and wp[0] == 4 * W >= DENSE_MIN_BITMAP        # heavy, one dense window
        i, j, v = oracle_tuples("every_slot", W, False)
        assert np.array_equal(j, np.arange(W)) and np.array_equal(v, 4.0 * (np.arange(W) + 1))     # every column its own value
        i, j, v = oracle_tuples("every_slot", W, True)
        assert np.array_equal(j, np.flatnonzero(np.arange(W) % 5 != 0))                     # the cancelling columns are gone
    i, j, v = oracle_tuples("every_slot", W_SMALL, False, scalek=(3, 2))
    assert np.array_equal(j, np.flatnonzero(np.arange(W_SMALL) % 3 != 0))
    A, B = few_columns()
    wp = window_products(A, B, 13)
    assert wp.sum() == wp[0] == 4200 > MID_MAX
    i, j, v = oracle_tuples("few_columns")
    assert np.array_equal(j, np.sort(FEW_COLUMNS)) and len(set(FEW_COLUMNS)) == 20 and len(set(v)) == 20
    assert len({c >> 6 for c in FEW_COLUMNS}) == 14                # six groups at the edges, eight further ones
    for signed in (False, True):
        A, B = tile_rows(signed)
        wp = window_products(A, B, 13)
        assert wp.sum() == 5120 > BM_CELL and wp[:17].max() < DENSE_MIN_BITMAP and wp[16] > 0      # >= two cells, none dense, one past 2^17 columns
        i, j, v = oracle_tuples("tile_rows", signed)
        assert set(TILE_EDGES) <= set(j.tolist()) if not signed else len(j) == 40 - 14 + 64 * 40
    assert len(oracle_tuples("tile_rows", False)[1]) == 40 + 64 * 40


# ---- on the GPU ----------------------------------------------------------------------------------------------------

def run_both_sinks(ctx, A, B, want, flags=0, scalek=None, sinks=("coo", "digest")):
    """The product through the C ABI in the given sinks against the oracle's tuples; returns the COO (or only) result."""
    from spsparse_amd import capi
    keep, out = [], None
    a, ka = capi.host_coo(A.idx0, A.idx1, A.val, A.shape, A.sort0)
    b, kb = capi.host_coo(B.idx0, B.idx1, B.val, B.shape, B.sort0)
    keep += [ka, kb]
    sk = None
    if scalek is not None:
        sk, kk = capi.host_vec(scalek.idx, scalek.val, scalek.shape0)
        keep.append(kk)
    for sink in sinks:
        res = ctx.multiply(a, b, 1.0, None, ".", None, ".", sk, capi.ADD, False, capi.SINK_COO if sink == "coo" else capi.SINK_DIGEST, flags)
        if sink == "coo":
            check_tuples(tuple(ctx.fetch(res)), want, "COO sink")
            gi, gj, _ = ctx.fetch(res)
            assert np.all(np.diff(gj[gi == 0]) > 0)
        else:
            cnt, vsum, h = orc.digest(*want)
            assert (res.nnz, res.hash) == (cnt, h), "digest sink: nnz %d hash %x, want %d %x" % (res.nnz, res.hash, cnt, h)
            assert res.sum == vsum                                  # integers: exact in any order
        out = out or res
    return out


DENSE_VARIANTS = ["plain", "scalek", "ordered", "exact_pattern"]


def dense_every_slot(ctx, W, variant):
    from spsparse_amd import capi
    signed = variant == "exact_pattern"
    A, B = every_slot(W, signed)
    flags = {"ordered": capi.SINK_ORDERED, "exact_pattern": capi.SINK_EXACT_PATTERN}.get(variant, 0)
    scalek = (3, 2) if variant == "scalek" else None
    want = oracle_tuples("every_slot", W, signed, scalek=scalek)
    res = run_both_sinks(ctx, A, B, want, flags, column_scale(W, *scalek) if scalek else None)
    assert res.window == W and res.products == 4 * W
    assert res.cells_dense >= 1 and res.products_dense == 4 * W and res.products_tiles == 0


@gpu
@pytest.mark.parametrize("variant", DENSE_VARIANTS)
def test_dense_cell_every_slot(ctx, variant):
    """One dense cell whose 32 768 products hit every slot of the 8192-column window four times: plain, with scalek (the
    COUNT launch walks its flag bytes back to columns), ORDERED (plain read-add-write on the same slots) and
    EXACT_PATTERN with exactly cancelling terms (clean slots told from cancelled ones at the swizzled address)."""
    dense_every_slot(ctx, W_SMALL, variant)


@gpu
def test_dense_cell_few_live_columns(ctx):
    """4200 products on twenty columns at the edges of groups, halves and the window: a scan-out that reads a group
    with another group's swizzle finds them in the wrong lanes."""
    A, B = few_columns()
    res = run_both_sinks(ctx, A, B, oracle_tuples("few_columns"))
    assert res.cells_dense >= 1 and res.products_dense == res.products == 4200 and res.products_tiles == 0


@gpu
@pytest.mark.parametrize("variant", DENSE_VARIANTS)
def test_dense_cell_16384_column_window(ctx, variant):
    """The 16384-column window kernel (1024 threads, 256 groups): every slot again."""
    with forced(ctx, "window", W_LARGE):
        dense_every_slot(ctx, W_LARGE, variant)


@gpu
@pytest.mark.parametrize("variant", ["coo", "digest", "exact_pattern", "scalek_coo"])
def test_bitmap_tiles_keyed_columns(ctx, variant):
    """One heavy row in bitmap tiles, its columns over 17 windows (more than one cell; the last cell starts past 2^17):
    shared columns take many products on one key, unique ones a single product.  The digest launch and the COO sink's
    plain COUNT launch run keyed; the store launch and the scalek COUNT launch keep the columns and must agree with them."""
    from spsparse_amd import capi
    signed = variant == "exact_pattern"
    A, B = tile_rows(signed)
    scalek = (4, 2) if variant == "scalek_coo" else None
    want = oracle_tuples("tile_rows", signed, scalek=scalek)
    sinks = {"coo": ("coo",), "digest": ("digest",), "exact_pattern": ("coo", "digest"), "scalek_coo": ("coo",)}[variant]
    with forced(ctx, "tiles_v1", BITMAP_TILES):
        res = run_both_sinks(ctx, A, B, want, capi.SINK_EXACT_PATTERN if signed else 0, column_scale(TILE_NCOL, *scalek) if scalek else None, sinks)
    assert res.products_tiles == res.products == 5120 and res.cells_dense == 0
