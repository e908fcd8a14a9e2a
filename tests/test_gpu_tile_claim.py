"""The heavy rows' tiles claimed from a counter (k_bm_tiles, k_hash_tiles2): same tuples, same digest as the oracle, call
after call, with the static walk (the `tile_walk` knob) beside it; the same walk dealing statically in the first-generation
and the direct tiles (k_hash_tiles, k_direct_tiles) at the same list lengths.  GPU only.

The few-tile products are built so that every heavy row is exactly one tile (80 A tuples, 5120 products spread over four
column windows: two or three cells, four in the first generation, whose cells hold 2048 products); the symbolic phase's
trace line confirms the count.  A claim can go wrong where the list is shorter than the grid (most workgroups claim
nothing), where it holds one tile, and where it is one longer than the grid (one workgroup's second claim is the last
tile, every other second claim finds the list used up)."""
import functools
import re

import numpy as np
import pytest

from oracle import binding as orc
from spsparse_amd import workloads as wl
from tests.gpu_util import Knobs as _Knobs, ctx  # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu

REL = 1e-12          # values, as tests/test_gpu_parity.py
DIGEST_REL = 1e-11   # the digest's value sum, as tests/test_gpu_parity.py


def _coo(M, keep):
    from spsparse_amd import capi
    s, k = capi.host_coo(M.idx0, M.idx1, M.val, M.shape, M.sort0)
    keep.append(k)
    return s


def _multiply(ctx, A, B, sink, flags=0):
    """(i, j, v, res); i, j, v None for the digest sink."""
    from spsparse_amd import capi
    keep = []
    res = ctx.multiply(_coo(A, keep), _coo(B, keep), sink=sink, flags=flags)
    if sink == capi.SINK_COO:
        return tuple(ctx.fetch(res)) + (res,)
    return None, None, None, res


def _check_tuples(got, want, exact=False):
    gi, gj, gv = got[:3]
    wi, wj, wv = want[:3]
    assert len(gi) == len(wi), (len(gi), len(wi))
    assert np.array_equal(gi, wi) and np.array_equal(gj, wj)
    if exact:
        assert np.array_equal(gv, wv)
    else:
        assert np.max(np.abs(gv - wv) / np.abs(wv)) <= REL


def _check_digest(res, tuples):
    cnt, s_, h = orc.digest(*tuples[:3])
    assert res.nnz == cnt and res.hash == h
    assert abs(res.sum - s_) <= DIGEST_REL * abs(s_)


# ---- few tiles

L_TILE, B_LEN, B_ROWS, NCOL = 80, 64, 512, 4 * 8192


@functools.lru_cache(maxsize=None)
def _one_tile_rows(nrows):
    """A (nrows x B_ROWS, 80 tuples a row) and B (B_ROWS x 32768, 64 tuples a row, columns over four windows of 8192):
    every row of A * B is heavy (5120 products) and one tile.  Returns (A, B, oracle tuples)."""
    rng = np.random.default_rng(500 + nrows)
    bj = np.concatenate([np.sort(rng.choice(NCOL, B_LEN, replace=False)) for _ in range(B_ROWS)])
    B = orc.Mat(np.repeat(np.arange(B_ROWS), B_LEN), bj, rng.uniform(0.5, 1.5, B_ROWS * B_LEN), (B_ROWS, NCOL))
    aj = np.concatenate([np.sort(rng.choice(B_ROWS, L_TILE, replace=False)) for _ in range(nrows)])
    A = orc.Mat(np.repeat(np.arange(nrows), L_TILE), aj, rng.uniform(0.5, 1.5, nrows * L_TILE), (nrows, B_ROWS))
    return A, B, orc.multiply(A, B, rowwise=True, nthreads=8)


def _tile_grid():
    return 2 * _cus()


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# grid_plus_one: one more than k_bm_tiles' grid (two workgroups a CU).  The hash kernels size their grids by the workgroups
# resident on a CU -- at 512 threads never more than four, eight waves a SIMD -- so "beyond_every_grid" is a list longer
# than any of the grids: there every kernel's static walk goes on to a second tile.
_FEW = {"one": lambda: 1, "few": lambda: 7, "grid_plus_one": lambda: _tile_grid() + 1, "beyond_every_grid": lambda: 8 * _cus() + 1}
_FEW_IDS = list(_FEW)


@pytest.mark.parametrize("scheme", [3, 2, 1], ids=["bitmap", "hash2", "hash1"])
@pytest.mark.parametrize("ntiles", _FEW_IDS)
def test_few_tiles(ctx, capfd, ntiles, scheme):
    """One tile, fewer tiles than workgroups, one tile more than workgroups: the COO result tuple by tuple against the
    oracle, the digest against the digest of those tuples, the three tile kernels of the hash-class cells."""
    from spsparse_amd import capi
    nrows = _FEW[ntiles]()
    A, B, want = _one_tile_rows(nrows)
    with _Knobs(ctx, {"tiles_v1": scheme, "trace": 1}):
        capfd.readouterr()
        got = _multiply(ctx, A, B, capi.SINK_COO)
        err = capfd.readouterr().err
        d = _multiply(ctx, A, B, capi.SINK_DIGEST)[3]
    m = re.search(r"tiles (\d+) cells (\d+):", err)
    assert m, err
    assert int(m.group(1)) == nrows                             # one tile a row
    assert got[3].rows_heavy == nrows and got[3].products_tiles == got[3].products == nrows * L_TILE * B_LEN
    _check_tuples(got, want)
    _check_digest(d, got)                                       # ... of the stored tuples
    _check_digest(d, want)


@pytest.mark.parametrize("ntiles", _FEW_IDS)
def test_few_direct_tiles(ctx, ntiles):
    """The same three list lengths for the direct tiles: with direct cells from 1024 products on, each of a row's four
    windows (1280 products) is a direct cell and the row one direct tile."""
    from spsparse_amd import capi
    A, B, want = _one_tile_rows(_FEW[ntiles]())
    with _Knobs(ctx, {"direct_min": 1024}):
        got = _multiply(ctx, A, B, capi.SINK_COO)
        d = _multiply(ctx, A, B, capi.SINK_DIGEST)[3]
    assert got[3].products_direct > 0 and d.products_direct > 0
    # every window a direct cell: the row's four cells fill one 512-thread tile (128 threads a cell), so the direct list
    # has one tile a row
    nrows = A.shape[0]
    assert got[3].products_direct == got[3].products == d.products_direct == nrows * L_TILE * B_LEN
    _check_tuples(got, want)
    _check_digest(d, got)
    _check_digest(d, want)


# ---- R-MAT, every walk and scheme

@functools.lru_cache(maxsize=None)
def _rmat(scale, signed):
    a = wl.rmat(scale, seed=8)
    vals = a[2]
    if signed:                                                  # small integers of both signs: sums are exact in every order, cancellation is common
        vals = np.random.default_rng(30 + scale).integers(-3, 4, size=a[2].size).astype(np.float64)
        vals[vals == 0] = 1.0
    A = orc.Mat(a[0], a[1], vals, a[3])
    return A, orc.multiply(A, A, rowwise=True, nthreads=8)


@pytest.mark.parametrize("walk", [0, 1], ids=["claimed", "static"])
@pytest.mark.parametrize("scheme", [3, 2], ids=["bitmap", "hash2"])
@pytest.mark.parametrize("scale", [13, 15])
def test_rmat_walks_and_schemes(ctx, scale, scheme, walk):
    """R-MAT A * A with either tile kernel, tiles claimed or dealt statically: the oracle's tuples in its order from the
    COO sink (claimed in both of its passes), its digest from the digest sink."""
    from spsparse_amd import capi
    A, want = _rmat(scale, False)
    with _Knobs(ctx, {"tiles_v1": scheme, "tile_walk": walk}):
        got = _multiply(ctx, A, A, capi.SINK_COO)
        d = _multiply(ctx, A, A, capi.SINK_DIGEST)[3]
    assert (got[3].products_tiles > 0) == (scale == 15)         # (scale 13: one column window, every heavy row a dense cell -- no tile list at all)
    _check_tuples(got, want)
    _check_digest(d, want)


@pytest.mark.parametrize("walk", [0, 1], ids=["claimed", "static"])
@pytest.mark.parametrize("scheme", [3, 2], ids=["bitmap", "hash2"])
@pytest.mark.parametrize("scale", [13, 15])
def test_rmat_exact_pattern_both_signs(ctx, scale, scheme, walk):
    """EXACT_PATTERN on values of both signs (small integers: every order of a sum is exact, many sums cancel): the
    oracle's pattern and values bit for bit from both sinks."""
    from spsparse_amd import capi
    A, want = _rmat(scale, True)
    with _Knobs(ctx, {"tiles_v1": scheme, "tile_walk": walk}):
        got = _multiply(ctx, A, A, capi.SINK_COO, capi.SINK_EXACT_PATTERN)
        d = _multiply(ctx, A, A, capi.SINK_DIGEST, capi.SINK_EXACT_PATTERN)[3]
    assert (got[3].products_tiles > 0) == (scale == 15)
    _check_tuples(got, want, exact=True)
    cnt, s_, h = orc.digest(*want[:3])
    assert (d.nnz, d.hash, d.sum) == (cnt, h, s_)


# ---- the same product again

def test_repeatable_in_one_context_and_a_fresh_one(ctx):
    """The same scale-15 digest twice in one context and once in a fresh one: identical count and hash (a counter that
    was not reset would show here), and the oracle's."""
    from spsparse_amd import capi
    A, want = _rmat(15, False)
    d = [_multiply(ctx, A, A, capi.SINK_DIGEST)[3] for _ in range(2)]
    fresh = capi.Context(0)
    try:
        d.append(_multiply(fresh, A, A, capi.SINK_DIGEST)[3])
        coo = _multiply(fresh, A, A, capi.SINK_COO)              # (and the COO sink behind a digest call, claimed tiles in both passes)
        d.append(_multiply(fresh, A, A, capi.SINK_DIGEST)[3])
    finally:
        fresh.close()
    for x in d:
        assert (x.nnz, x.hash) == (d[0].nnz, d[0].hash)
        _check_digest(x, want)
    _check_tuples(coo, want)


# ---- every kind of row in one product

@pytest.mark.parametrize("knobs", [{"dense_min": 4096, "long_dense_min": 4096}, {"no_tiles": 1}], ids=["tiles", "windowed"])
def test_digest_matches_stored_tuples(ctx, knobs):
    """Light, mid and dense-cell rows with the heavy rows' hash-class cells in tiles (dense thresholds at the cells'
    capacity) or in the windowed k_hash launches (no tiles): the digest, with the row statistics, has the count and hash
    of the tuples the COO sink stores."""
    from spsparse_amd import capi
    A, want = _rmat(15, False)
    with _Knobs(ctx, knobs):
        got = _multiply(ctx, A, A, capi.SINK_COO)
        d = _multiply(ctx, A, A, capi.SINK_DIGEST, capi.SINK_ROWSTATS)[3]
    r = got[3]
    assert r.rows_light > 0 and r.rows_mid > 0 and r.cells_dense > 0
    windowed = r.products_heavy - r.products_dense - r.products_tiles - r.products_direct
    assert (r.products_tiles > 0 and windowed == 0) if "dense_min" in knobs else (r.products_tiles == 0 and windowed > 0)
    _check_tuples(got, want)
    _check_digest(d, got)
    # the benchmark takes the windowed cells' time as this difference: never negative
    assert d.ms_heavy - d.ms_dense - d.ms_tiles - d.ms_direct >= -1e-3
