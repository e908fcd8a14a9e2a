"""The hash cells of rows too long for a tile (more than 256 A tuples: the windowed k_hash launches), which test the
window-occupancy words of op(B), queue the A tuples whose B segment is not empty, and read bounds for those alone.  GPU only.

Operands are built by hand.  Every row of A is a scenario of its own: L A tuples whose columns k are consecutive rows of
op(B) owned by that row alone, so the tuple at position p of the row selects B row base + p, and what that B row holds in
a column window decides whether the tuple survives in the cell of that window.  A row's hash windows are kept apart by
dense windows (40 filler positions x 30 tuples = 1200 products, above the long rows' dense threshold of 1024), so each
hash window is a cell of its own unless two are meant to merge.  Values are small integers (scale vectors powers of two):
every order of a sum is exact, so the COO sink is compared bit for bit with the oracle and the digest exactly.

Per row length (257, 513, 1025, 1300: one and several chunk boundaries for NT = 256 and 512) and class (at most 512
products: T = 1024, NT = 256; 513 .. 1024: T = 3072, NT = 512) the cells have 1 survivor, exactly NT, NT + 1, survivors
only among the last 64 A tuples, only among the first 64, and with NT consecutive empty tuples in the middle; one more is
two windows of 1000 products that merge (T = 4096).  The windows sit at the edges of the occupancy words: op(B) has
130 windows, cells end at window 31 / 32, 63 / 64, 127 / 128, and one spans 120 .. 129.  A scan round is 768 A tuples for
T = 1024 (256 in STORE), 1024 for T = 3072, 1536 for T = 4096, 2048 for T = 8192: the rows of 1025 and 1300 tuples take a
second round in the first two, test_ring_wraps in the others; a cell with NT + 1 survivors leaves one in the ring for a
chunk of its own."""
import functools

import numpy as np
import pytest

from oracle import binding as orc
from tests.gpu_util import Knobs, check_digest, check_tuples, ctx  # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu

NWIN = 130
LENGTHS = (257, 513, 1025, 1300)
# hash windows of a row, ascending, never adjacent (a dense window goes behind each); the last entry of Z is a pair that
# merges into one cell across the second 16-byte group of the occupancy words
WSETS = ([3, 31, 47, 63, 127, 129], [0, 32, 64, 100, 112, 128], [2, 20, 40, 60, 80, (120, 129)])
PATTERNS = ("one", "nt", "nt_plus_1", "last64", "first64", "hole")


def _survivors(pattern, L, nt):
    """Positions of the row's A tuples that hold tuples of the cell's window, and tuples per survivor for `prods` in all."""
    if pattern == "one":
        return np.array([L // 2])
    if pattern == "nt":
        return np.sort(np.random.default_rng(L).choice(L, min(nt, L), replace=False))
    if pattern == "nt_plus_1":
        return np.sort(np.random.default_rng(L + 1).choice(L, min(nt + 1, L), replace=False))
    if pattern == "last64":
        return np.arange(L - 64, L)[::2]
    if pattern == "first64":
        return np.arange(0, 64)[1::2]
    head = np.arange(0, 40)                                         # "hole": nt consecutive empty tuples, survivors on both sides where the row is long enough
    tail = np.arange(40 + nt, L)[:40]
    return np.concatenate([head, tail])


def _spread(total, n):
    """n positive integers that sum to total (total >= n)."""
    per = np.full(n, total // n)
    per[: total - per.sum()] += 1
    return per


class _Builder:
    def __init__(self, W):
        self.W, self.rng = W, np.random.default_rng(77)
        self.ai, self.aj, self.bi, self.bj = [], [], [], []
        self.nrow = self.nk = 0

    def _put(self, k, w, n):
        """n tuples of B row k in window w."""
        self.bi.append(np.full(n, k))
        self.bj.append(w * self.W + np.sort(self.rng.choice(self.W, n, replace=False)))

    def row(self, L, cells, dense):
        """One row of A with L tuples; cells: (windows, survivors, products); dense: the separating windows."""
        base = self.nk
        self.ai.append(np.full(L, self.nrow))
        self.aj.append(base + np.arange(L))
        for wins, surv, prods in cells:
            wins = wins if isinstance(wins, tuple) else (wins,)
            for x, w in enumerate(wins):                                # (a pair: the survivors' halves in either window)
                part = surv[x::len(wins)] if len(wins) > 1 and surv.size > 1 else surv
                for p, n in zip(part, _spread(max(prods // len(wins), part.size), part.size)):
                    self._put(base + p, w, int(n))
        filler = np.unique(np.linspace(0, L - 1, 40).astype(int))
        for w in dense:
            for p in filler:
                self._put(base + p, w, 30)
        self.nrow += 1
        self.nk += L

    def finish(self):
        bi, bj = np.concatenate(self.bi), np.concatenate(self.bj)
        ai, aj = np.concatenate(self.ai), np.concatenate(self.aj)
        rng = np.random.default_rng(78)

        def vals(n):
            v = rng.integers(-3, 4, n).astype(np.float64)
            v[v == 0] = 2.0
            return v
        A = orc.Mat(ai, aj, vals(ai.size), (self.nrow, self.nk))
        B = orc.Mat(bi, bj, vals(bi.size), (self.nk, NWIN * self.W))
        return A, B


def _scenario_rows(b):
    i = 0
    for L in LENGTHS:
        for cls in (0, 1):
            nt, prods = (256, 512) if cls == 0 else (512, 1024)
            wset = WSETS[i % 3]
            cells, dense = [], []
            for x, w in enumerate(wset):
                pattern = PATTERNS[(x + i) % len(PATTERNS)]
                surv = _survivors(pattern, L, nt)
                if isinstance(w, tuple):
                    cells.append((w, surv if surv.size > 1 else np.arange(0, L, 3), 2000))       # two windows of 1000: one cell of 2000
                    dense.append(w[0] - 1)
                else:
                    p = prods if surv.size > 1 or cls == 0 else 1024
                    cells.append((w, surv, max(min(p, 300) if surv.size == 1 else p, surv.size)))
                    if w + 1 < NWIN:
                        dense.append(w + 1)
            b.row(L, cells, dense)
            i += 1


@functools.lru_cache(maxsize=None)
def _edges(W):
    b = _Builder(W)
    _scenario_rows(b)
    return b.finish()


@functools.lru_cache(maxsize=None)
def _want(W, tB=".", scaled=False):
    A, B = _edges(W)
    kw = _scales(A, B) if scaled else {}
    if tB == "T":
        B = _transposed(B)
    return orc.multiply(A, B, rowwise=True, nthreads=8, tB=tB, **kw)


def _transposed(B):
    return orc.Mat(B.idx1, B.idx0, B.val, (B.shape[1], B.shape[0]))


def _scales(A, B):
    rng = np.random.default_rng(79)

    def vec(n):
        return orc.Vec(np.arange(n), rng.choice([0.5, 1.0, 2.0, -1.0], n), n)
    return dict(C_=2.0, scalei=vec(A.shape[0]), scalej=vec(A.shape[1]), scalek=vec(B.shape[1]))


def _multiply(ctx, A, B, sink, flags=0, **kw):
    """(i, j, v, res) like tests/test_gpu_parity.py's _dev; B may be a prepared operand's Coo."""
    from spsparse_amd import capi
    keep = []

    def coo(M):
        if isinstance(M, capi.Coo):
            return M
        s, k = capi.host_coo(M.idx0, M.idx1, M.val, M.shape, M.sort0)
        keep.append(k)
        return s

    def vec(V):
        if V is None:
            return None
        s, k = capi.host_vec(V.idx, V.val, V.shape0)
        keep.append(k)
        return s
    res = ctx.multiply(coo(A), coo(B), kw.get("C_", 1.0), vec(kw.get("scalei")), ".", vec(kw.get("scalej")), kw.get("tB", "."),
                       vec(kw.get("scalek")), sink=sink, flags=flags)
    if sink == capi.SINK_COO:
        return tuple(ctx.fetch(res)) + (res,)
    return None, None, None, res


def _windowed(res):
    """Products of the windowed k_hash launches."""
    return res.products_heavy - res.products_dense - res.products_tiles - res.products_direct


def _both_sinks(ctx, A, B, want, what, flags=0, **kw):
    from spsparse_amd import capi
    got = _multiply(ctx, A, B, capi.SINK_COO, flags, **kw)
    check_tuples(got[:3], want[:3], what + ": COO sink")
    d = _multiply(ctx, A, B, capi.SINK_DIGEST, flags, **kw)[3]
    check_digest(d, want, what)
    return got[3], d


KNOBS = {
    "default": {},
    "t8192": {"long_cap": 4096, "long_dense_min": 4096},
    "dense_from_64": {"long_dense_min": 64},
}


@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
def test_chunk_and_word_edges(ctx, knobs):
    """Every scenario row in one product, 8192-column windows: default grouping, 4096-product cells (T = 8192: the windows
    between the cells are hash windows too and merge with them) and nearly every window a dense cell."""
    A, B = _edges(8192)
    with Knobs(ctx, KNOBS[knobs]):
        res, d = _both_sinks(ctx, A, B, _want(8192), knobs)
    assert res.rows_heavy == A.shape[0] == 2 * len(LENGTHS)
    assert res.products_tiles == 0                               # every row is too long for a tile
    if knobs != "dense_from_64":
        assert _windowed(res) > 0 and _windowed(d) > 0
    if knobs == "default":
        # per row: five or six single-window cells of 300 .. 1024 products and (every third row) a merged pair of 2000
        assert res.cells_dense >= 5 * A.shape[0]
        assert _windowed(res) >= A.shape[0] * 5 * 256


def test_window_16384(ctx):
    """The same rows on 16384-column windows (130 of them again: op(B) twice as wide), long rows' dense threshold as for 8192."""
    A, B = _edges(16384)
    with Knobs(ctx, {"window": 16384, "long_dense_min": 1024}):
        res, d = _both_sinks(ctx, A, B, _want(16384), "window 16384")
    assert _windowed(res) >= A.shape[0] * 5 * 256 and res.products_tiles == 0


@functools.lru_cache(maxsize=None)
def _many_survivors():
    """A row of 3000 A tuples and two windows in which nearly all of them survive with one B tuple each: 2700 and 2000
    products."""
    b = _Builder(8192)
    rng = np.random.default_rng(94)
    L = 3000
    b.row(L, [(10, np.sort(rng.choice(L, 2700, replace=False)), 2700), (50, np.sort(rng.choice(L, 2000, replace=False)), 2000)], [])
    A, B = b.finish()
    return A, B, orc.multiply(A, B, rowwise=True, nthreads=8)


def test_ring_wraps(ctx):
    """With 4096-product cells the two windows are a cell of 2700 products (T = 8192: two rounds of 2048 tuples, and the
    second round's survivors wrap around the ring of 2560 entries) and one of 2000 (T = 4096: two rounds of 1536)."""
    A, B, want = _many_survivors()
    with Knobs(ctx, {"long_cap": 4096, "long_dense_min": 4096}):
        res, d = _both_sinks(ctx, A, B, want, "ring")
        _both_sinks(ctx, A, B, want, "ring, ordered", _flags("ordered"))
    assert _windowed(res) == res.products == 4700 and res.cells_dense == 0


def _flags(mode):
    from spsparse_amd import capi
    return capi.SINK_EXACT_PATTERN if mode == "exact_pattern" else capi.SINK_ORDERED


@pytest.mark.parametrize("mode", ["exact_pattern", "ordered"])
def test_modes(ctx, mode):
    from spsparse_amd import capi
    A, B = _edges(8192)
    flags = capi.SINK_EXACT_PATTERN if mode == "exact_pattern" else capi.SINK_ORDERED
    res, d = _both_sinks(ctx, A, B, _want(8192), mode, flags)
    assert _windowed(res) > 0


def test_scale_vectors_on_all_sides(ctx):
    A, B = _edges(8192)
    res, d = _both_sinks(ctx, A, B, _want(8192, scaled=True), "scaled", **_scales(A, B))
    assert _windowed(res) > 0


def test_transposed_b(ctx):
    A, B = _edges(8192)
    res, d = _both_sinks(ctx, A, _transposed(B), _want(8192, tB="T"), "op(B) = T", tB="T")
    assert _windowed(res) > 0


def test_prepared_right_operand_twice(ctx):
    """A prepared op(B) brings its own index and occupancy words: two products in a row read the handle's tables (the
    second builds nothing), with another product on plain operands between them in the same context."""
    from spsparse_amd import capi
    A, B = _edges(8192)
    keep = []
    s, k = capi.host_coo(B.idx0, B.idx1, B.val, B.shape, B.sort0)
    keep.append(k)
    op = capi.Operand(ctx, s, role=capi.AS_B)
    try:
        r1, _ = _both_sinks(ctx, A, op.coo, _want(8192), "prepared, first")
        A2, B2 = _one_row_most_cells()
        _both_sinks(ctx, A2, B2, _want_of("most"), "plain operands between")
        r2, _ = _both_sinks(ctx, A, op.coo, _want(8192), "prepared, second")
    finally:
        op.close()
    assert _windowed(r1) == _windowed(r2) > 0


def test_no_tiles_sends_ordinary_rows_to_the_windowed_kernel(ctx):
    """Rows of 80 A tuples beside the long ones, tiles switched off: their hash cells run in the windowed launches too
    (one chunk, most of whose tuples survive)."""
    A, B = _short_and_long()
    want = _want_of("short_and_long")
    with Knobs(ctx, {"no_tiles": 1}):
        res, d = _both_sinks(ctx, A, B, want, "no_tiles")
    assert res.products_tiles == 0 and _windowed(res) > 0
    _both_sinks(ctx, A, B, want, "tiles")


# ---- list lengths (the cases of tests/test_gpu_tile_claim.py for this kernel)

def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _merging_rows(nrows, L=257, nwindows=10, first=0):
    """Rows that share B rows 0 .. L-1: nwindows hash windows of 500 products each, no dense window between them, so the
    greedy grouping cuts cells of four windows (2000 products, T = 4096) and a rest."""
    b = _Builder(8192)
    b.nk = L
    rng = np.random.default_rng(90 + nrows)
    for w in range(first, first + nwindows):
        surv = np.sort(rng.choice(L, 100, replace=False))
        for p, n in zip(surv, _spread(500, surv.size)):
            b._put(p, (w * 7) % NWIN if nwindows > 64 else w, int(n))
    for r in range(nrows):
        b.ai.append(np.full(L, r))
        b.aj.append(np.arange(L))
    b.nrow = nrows
    return b.finish()


def _grid_plus_one():
    """One cell more than the workgroups of the T = 4096 launch (78 KB of LDS: two workgroups a CU in DIGEST and STORE): a
    row of ten windows of 500 products is two cells of 2000 and one of 1000, the last row six windows and a dense one --
    a single cell of 2000."""
    b = _Builder(8192)
    rng = np.random.default_rng(93)
    L = 257

    def win(w):
        return (w, np.sort(rng.choice(L, 20, replace=False)), 500)
    for r in range(_cus()):
        b.row(L, [win(w) for w in range(r % 100, r % 100 + 10)], [])
    b.row(L, [win(w) for w in range(7, 13)], [60])
    return b.finish()


@functools.lru_cache(maxsize=None)
def _list_case(name):
    if name == "few":                                               # 3 rows x 3 cells: far fewer cells than workgroups
        return _merging_rows(3)
    if name == "grid_plus_one":
        return _grid_plus_one()
    return _merging_rows(4 * _cus() + 1)                            # "beyond_every_grid": 2 cells of a class per row, at most 8 workgroups a CU


@functools.lru_cache(maxsize=None)
def _one_row_most_cells():
    """One row owns 120 windows of 500 products (30 cells); three more rows have one cell each in the same class."""
    b = _Builder(8192)
    L = 700
    rng = np.random.default_rng(91)
    cells = [(w, np.sort(rng.choice(L, 90, replace=False)), 500) for w in range(4, 124)]
    b.row(L, cells, [])
    for r in range(3):
        b.row(300, [(w, np.sort(rng.choice(300, 120, replace=False)), 500) for w in range(10 + r, 14 + r)] +
              [(60 + r, np.arange(0, 300, 2), 700)], [20 + r, 30 + r, 40 + r, 50 + r])
    return b.finish()


@functools.lru_cache(maxsize=None)
def _short_and_long():
    b = _Builder(8192)
    rng = np.random.default_rng(92)
    for r in range(6):
        L = 80 if r % 2 == 0 else 400
        cells = [(w, np.sort(rng.choice(L, 60, replace=False)), 900) for w in (1 + r, 33 + r, 65 + r, 97 + r, 127)]
        b.row(L, cells, [20 + r, 50 + r] if r % 2 else [])
    return b.finish()


@functools.lru_cache(maxsize=None)
def _want_of(name):
    A, B = {"most": _one_row_most_cells, "short_and_long": _short_and_long}[name]() if name in ("most", "short_and_long") else _list_case(name)
    return orc.multiply(A, B, rowwise=True, nthreads=8)


@pytest.mark.parametrize("name", ["few", "grid_plus_one", "beyond_every_grid", "most"])
def test_list_lengths(ctx, name):
    """Fewer cells than workgroups, one cell more than workgroups (one workgroup goes on to a second cell, every other
    finds the list used up), a list longer than any grid, and a list most of whose cells belong to one row; twice in a
    row, for what a launch leaves behind."""
    A, B = _one_row_most_cells() if name == "most" else _list_case(name)
    want = _want_of(name)
    for rep in range(2):
        res, d = _both_sinks(ctx, A, B, want, "%s, call %d" % (name, rep))
        assert res.products_tiles == 0 and _windowed(res) == res.products_heavy - res.products_dense > 0
