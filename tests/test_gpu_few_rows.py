"""Mid rows with few A tuples (65 .. 4096 products, at most `few_max` A tuples): the k_few launches, which hold a row's B
segments in registers, find a product's segment by comparing against their prefixes and request the next row's B tuples
a row ahead.  GPU only.

Operands are built by hand.  op(B) has 40 rows by 2^20 columns whose lengths are the class edges and the odd cases (an
empty row, eight rows of one 16-column pattern, two rows with the same columns and values, a last row that ends at the
last tuple of B's arrays); a row of A names the B rows it multiplies.  Values are small integers (scale vectors powers
of two): every order of a sum is exact, so the COO sink is compared bit for bit with the oracle and the digest exactly.

Which kernel ran is read from the `trace` line "few cells: mid N": N is the number of rows with 65 .. 4096 products and
at most few_max A tuples, counted here from the construction.  Every case also runs with few_max = -1 (every mid row in
k_hash) and must give the same tuples."""
import functools
import re

import numpy as np
import pytest

from oracle import binding as orc
from tests.gpu_util import Knobs, check_digest, check_tuples, ctx  # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu

NCOL = 1 << 20
FEW_MAX = 8                                                         # the knob's default
# B rows by name -> (row index, tuples)
EDGE = {65: 0, 512: 1, 513: 2, 2048: 3, 2049: 4, 4096: 5, 4097: 6}     # rows of exactly that many tuples
EMPTY = (7, 37, 38)
SAME16 = tuple(range(8, 16))                                        # eight rows, one pattern of 16 columns
RUN30 = tuple(range(16, 16 + 16 + 1))                               # seventeen rows of 30 tuples: L up to FEW_LMAX + 1
PAIR = (33, 34)                                                     # the same 100 columns and values twice
ONE = 35                                                            # one tuple
ALSO2048 = 36
LAST = 39                                                           # 70 tuples, the last of B's arrays
NB = 40


@functools.lru_cache(maxsize=None)
def _b():
    rng = np.random.default_rng(501)
    rows = {}

    def cols(n):
        return np.sort(rng.choice(NCOL, n, replace=False))

    def vals(n):
        v = rng.integers(-3, 4, n).astype(np.float64)
        v[v == 0] = 2.0
        return v
    for n, r in EDGE.items():
        rows[r] = (cols(n), vals(n))
    pat = cols(16)
    for r in SAME16:
        rows[r] = (pat, vals(16))
    for r in RUN30:
        rows[r] = (cols(30), vals(30))
    pc, pv = cols(100), vals(100)
    for r in PAIR:
        rows[r] = (pc, pv)
    rows[ONE] = (cols(1), vals(1))
    rows[ALSO2048] = (cols(2048), vals(2048))
    rows[LAST] = (np.concatenate([np.sort(rng.choice(NCOL - 1, 69, replace=False)), [NCOL - 1]]), vals(70))
    bi = np.concatenate([np.full(rows[r][0].size, r) for r in sorted(rows)])
    bj = np.concatenate([rows[r][0] for r in sorted(rows)])
    bv = np.concatenate([rows[r][1] for r in sorted(rows)])
    lens = np.zeros(NB, np.int64)
    for r in rows:
        lens[r] = rows[r][0].size
    return orc.Mat(bi, bj, bv, (NB, NCOL)), lens


def _a(rowlists, values=None):
    """A whose row i holds the B rows rowlists[i] (values: per row, else small integers)."""
    rng = np.random.default_rng(502)
    ai = np.concatenate([np.full(len(ks), i) for i, ks in enumerate(rowlists)])
    aj = np.concatenate([np.sort(np.asarray(ks)) for ks in rowlists])
    av = rng.integers(1, 4, ai.size).astype(np.float64) * rng.choice([-1.0, 1.0], ai.size)
    if values:
        for i, v in values.items():
            av[ai == i] = v
    return orc.Mat(ai, aj, av, (len(rowlists), NB))


def _few_rows(rowlists, few_max=FEW_MAX):
    """Rows that k_few takes: 65 .. 4096 products and at most few_max A tuples."""
    lens = _b()[1]
    return sum(1 for ks in rowlists if 64 < sum(lens[k] for k in ks) <= 4096 and len(ks) <= few_max)


# every row a case of its own; the comment is (L, products)
EDGE_ROWS = [
    [EDGE[65]], [EDGE[512]], [EDGE[513]], [EDGE[2048]], [EDGE[2049]], [EDGE[4096]],      # L = 1 at the class edges
    [EDGE[4097]],                                                   # (1, 4097): a heavy row
    [EDGE[512], ONE], [EDGE[2048], ONE],                            # (2, 513), (2, 2049)
    [EDGE[2048], ALSO2048],                                         # (2, 4096): a full table
    [EDGE[2048], ALSO2048, ONE],                                    # (3, 4097): heavy
    [EDGE[65], EDGE[512], EDGE[513]],                               # (3, 1090)
    list(RUN30[:FEW_MAX]), list(RUN30[:FEW_MAX + 1]),               # L = few_max, and few_max + 1: k_hash
    list(RUN30[:16]), list(RUN30[:17]),                             # L = 16 and 17 (for few_max = 16)
    [EMPTY[0], EMPTY[1], EDGE[512], EMPTY[2]],                      # one segment of four is not empty (the second by k)
    [EMPTY[0], EMPTY[1], EMPTY[2], LAST],                           # ... the last one, which ends at B's last tuple
    [EDGE[65], EMPTY[0], EMPTY[1], EMPTY[2]],                       # ... the first one
    list(SAME16),                                                   # 128 products, 16 outputs
    list(PAIR),                                                     # a and -a: every sum is exactly 0
    [LAST],                                                         # (1, 70), the segment that ends B's arrays
    [EDGE[65], ONE],                                                # the last cell: its A tuples are the last of A's
]
PAIR_ROW = EDGE_ROWS.index(list(PAIR))


@functools.lru_cache(maxsize=None)
def _edges():
    return _a(EDGE_ROWS, {PAIR_ROW: np.array([3.0, -3.0])}), _b()[0]


def _transposed(B):
    return orc.Mat(B.idx1, B.idx0, B.val, (B.shape[1], B.shape[0]))


def _scales(A, B):
    rng = np.random.default_rng(503)

    def vec(n):
        return orc.Vec(np.arange(n), rng.choice([0.5, 1.0, 2.0, -1.0], n), n)
    return dict(C_=2.0, scalei=vec(A.shape[0]), scalej=vec(A.shape[1]), scalek=vec(B.shape[1]))


@functools.lru_cache(maxsize=None)
def _want_edges(tB=".", scaled=False):
    A, B = _edges()
    kw = _scales(A, B) if scaled else {}
    return orc.multiply(A, _transposed(B) if tB == "T" else B, rowwise=True, nthreads=8, tB=tB, **kw)


def _multiply(ctx, A, B, sink, flags=0, **kw):
    """(i, j, v, res); B may be a prepared operand's Coo."""
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


def _few_cells(err):
    """The count of every "few cells: mid N" line the symbolic phase printed."""
    return [int(x) for x in re.findall(r"few cells: mid (\d+)", err)]


def _both_sinks(ctx, capfd, A, B, want, what, expect_few, knobs=None, flags=0, **kw):
    """Both sinks with the knobs (and trace), the k_few cell count of every call asserted; then with few_max = -1."""
    from spsparse_amd import capi
    for kn, few in ((dict(knobs or {}), expect_few), (dict(knobs or {}, few_max=-1), 0)):
        with Knobs(ctx, dict(kn, trace=1)):
            capfd.readouterr()
            got = _multiply(ctx, A, B, capi.SINK_COO, flags, **kw)
            d = _multiply(ctx, A, B, capi.SINK_DIGEST, flags, **kw)[3]
            err = capfd.readouterr().err
        assert _few_cells(err) == [few, few], "%s %r: %s" % (what, kn, err)
        check_tuples(got[:3], want[:3], "%s %r: COO sink" % (what, kn))
        check_digest(d, want, "%s %r" % (what, kn))
    return got[3], d


def test_class_edges_and_odd_rows(ctx, capfd):
    """Every row of EDGE_ROWS in one product at the default few_max: L = 1, 2, few_max go to k_few, few_max + 1 and the
    rows of 16 and 17 tuples to k_hash, 4097 products to the heavy rows."""
    A, B = _edges()
    res, d = _both_sinks(ctx, capfd, A, B, _want_edges(), "edges", _few_rows(EDGE_ROWS))
    assert res.rows_heavy == 2 and res.rows_mid == len(EDGE_ROWS) - 2 and res.rows_light == 0
    assert _few_rows(EDGE_ROWS) == len(EDGE_ROWS) - 2 - 3          # all mid rows but L = 9, 16, 17
    lens = _b()[1]
    assert res.products_mid == d.products_mid == sum(int(sum(lens[k] for k in ks)) for ks in EDGE_ROWS) - 2 * 4097
    assert res.tuples_mid == sum(len(ks) for ks in EDGE_ROWS) - 1 - 3


@pytest.mark.parametrize("few_max", [1, 2, 4, 16, 100])
def test_few_max_settings(ctx, capfd, few_max):
    """The routing threshold: rows of more A tuples stay on k_hash; a setting above 16 is 16."""
    A, B = _edges()
    _both_sinks(ctx, capfd, A, B, _want_edges(), "few_max %d" % few_max, _few_rows(EDGE_ROWS, min(few_max, 16)), {"few_max": few_max})


def test_cancelling_pair_leaves_nothing(ctx):
    """a and -a on two B rows with the same columns and values: the COO sink closes the holes, the digest counts nothing."""
    from spsparse_amd import capi
    A = _a([list(PAIR)], {0: np.array([3.0, -3.0])})
    B = _b()[0]
    got = _multiply(ctx, A, B, capi.SINK_COO)
    d = _multiply(ctx, A, B, capi.SINK_DIGEST)[3]
    assert got[0].size == 0 and got[3].nnz == 0 and got[3].products_mid == 200
    assert (d.nnz, d.hash, d.sum) == (0, 0, 0.0)


def test_scale_vectors_on_all_sides(ctx, capfd):
    A, B = _edges()
    _both_sinks(ctx, capfd, A, B, _want_edges(scaled=True), "scaled", _few_rows(EDGE_ROWS), **_scales(A, B))


def test_transposed_b(ctx, capfd):
    A, B = _edges()
    _both_sinks(ctx, capfd, A, _transposed(B), _want_edges(tB="T"), "op(B) = T", _few_rows(EDGE_ROWS), tB="T")


def test_prepared_right_operand_twice(ctx, capfd):
    from spsparse_amd import capi
    A, B = _edges()
    keep = []
    s, k = capi.host_coo(B.idx0, B.idx1, B.val, B.shape, B.sort0)
    keep.append(k)
    op = capi.Operand(ctx, s, role=capi.AS_B)
    try:
        for rep in range(2):
            _both_sinks(ctx, capfd, A, op.coo, _want_edges(), "prepared, call %d" % rep, _few_rows(EDGE_ROWS))
    finally:
        op.close()


@pytest.mark.parametrize("mode", ["exact_pattern", "ordered"])
def test_ordered_modes_stay_on_k_hash(ctx, capfd, mode):
    """EXACT_PATTERN and the ORDERED sink: no row goes to k_few, whatever few_max says, and the oracle's values come back
    bit for bit."""
    from spsparse_amd import capi
    A, B = _edges()
    flags = capi.SINK_EXACT_PATTERN if mode == "exact_pattern" else capi.SINK_ORDERED
    _both_sinks(ctx, capfd, A, B, _want_edges(), mode, 0, flags=flags)
    _both_sinks(ctx, capfd, A, B, _want_edges(), mode, 0, {"few_max": 16}, flags=flags)


# ---- the pipeline's ramp: lists of 1, 2, 3 cells, one grid, one more, two grids and one more

def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# A list's cells alternate between the smallest and the largest of its class (consecutive cells differ in shape) and
# between one and two A tuples.  T = 8192: one 1024-thread workgroup a CU in every mode (104 KB of LDS and more).
# T = 1024: 256-thread workgroups, six a CU in DIGEST, five in STORE, eight in COUNT by their registers -- the lengths
# are one DIGEST grid, one more, and more than two grids of any mode.
RAMP = {
    "t8192": ([[EDGE[2049]], [EDGE[4096]], [EDGE[2048], ONE], [EDGE[2048], ALSO2048]], lambda cu: (1, 2, 3, cu, cu + 1, 2 * cu + 1)),
    "t1024": ([[EDGE[65]], [EDGE[512]], [EDGE[65], ONE], [RUN30[0], RUN30[1], RUN30[2]]], lambda cu: (1, 2, 3, 6 * cu, 6 * cu + 1, 16 * cu + 1)),
}


@functools.lru_cache(maxsize=None)
def _ramp(cls, n):
    shapes = RAMP[cls][0]
    rows = [shapes[i % len(shapes)] for i in range(n)]
    A, B = _a(rows), _b()[0]
    return A, B, orc.multiply(A, B, rowwise=True, nthreads=8)


@pytest.mark.parametrize("which", range(6), ids=["1", "2", "3", "grid", "grid+1", "2grid+1"])
@pytest.mark.parametrize("cls", list(RAMP))
def test_list_lengths(ctx, capfd, cls, which):
    n = RAMP[cls][1](_cus())[which]
    A, B, want = _ramp(cls, n)
    res, d = _both_sinks(ctx, capfd, A, B, want, "%s, %d cells" % (cls, n), n)
    assert res.rows_mid == d.rows_mid == n
