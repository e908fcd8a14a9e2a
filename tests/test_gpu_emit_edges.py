"""hash_emit (csrc/spgemm_hash.h), the column-ordered emission of the LDS hash cells, at every column width.  GPU only.

The cases come from tests/emit_ref.py; tests/test_emit_host.py shows on the CPU which (kernel, table, ordering) each row
reaches and that the catalogue reaches them all.  Mid rows: op(B) of 1 column to 2^31, both sides of every width at which
a table changes its ordering (bitmap rank, LDS radix sort, bitonic network).  Every case runs through the C ABI against the
oracle, bit for bit (small integers: every sum is exact in any order): the COO sink (count and store pass) under the
emit_path knob at 0, 1 and 2 and with few_max at its default and at -1, the digest sink with and without ROWSTATS.  Which
kernel ran is read from the trace line "few cells: mid N" and the result's counters; which ordering ran cannot be seen
from here -- the host file's coverage assertions and the restatement stand for that.  Heavy rows: one hash cell of 1 .. 5
(9) windows per row in the lowest and in the highest of 2048 windows, for every windowed table and the hash tiles of both
generations, the planned cut asserted as in tests/test_gpu_tile_shapes.py."""
import re

import numpy as np
import pytest

from tests import emit_ref as er
from tests import test_gpu_tile_shapes as shapes
from tests.gpu_util import Knobs, check_digest, check_tuples, ctx  # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu


def _multiply(ctx, c, sink, flags=0, **kw):
    """(i, j, v, res) of the case's product; kw: C_, scalei, scalek."""
    from spsparse_amd import capi
    keep = []

    def coo(M):
        s, k = capi.host_coo(M.idx0, M.idx1, M.val, M.shape, M.sort0)
        keep.append(k)
        return s

    def vec(V):
        if V is None:
            return None
        s, k = capi.host_vec(V.idx, V.val, V.shape0)
        keep.append(k)
        return s
    res = ctx.multiply(coo(c.A), coo(c.B), kw.get("C_", 1.0), vec(kw.get("scalei")), ".", None, ".", vec(kw.get("scalek")), sink=sink, flags=flags)
    if sink == capi.SINK_COO:
        return tuple(ctx.fetch(res)) + (res,)
    return None, None, None, res


def _few_cells(err):
    return [int(x) for x in re.findall(r"few cells: mid (\d+)", err)]


def _traced(ctx, capfd, c, knobs, sink, flags=0, **kw):
    """One call under the knobs with the trace on: (i, j, v, res, the k_few cell counts the symbolic phase printed)."""
    with Knobs(ctx, dict(knobs, trace=1)):
        capfd.readouterr()
        out = _multiply(ctx, c, sink, flags, **kw)
        err = capfd.readouterr().err
    return out + (_few_cells(err),)


def _check_routing(c, res, few, few_max, what, on=None):
    """The result's counters and the trace line against the records (on: the rows that scalei leaves)."""
    rec = [r for i, r in enumerate(c.rec) if on is None or on[i]]
    assert few == [sum(1 for r in rec if r.L <= er.few_limit(few_max))], "%s: few cells %r" % (what, few)
    assert (res.rows_mid, res.products_mid, res.tuples_mid) == (len(rec), sum(r.products for r in rec), sum(r.L for r in rec)), what
    assert res.rows_light == 0 and res.rows_heavy == 0, what


def _wid(w):
    if w > 64 and w & (w - 1) == 0:
        return "2^%d" % (w.bit_length() - 1)
    if w > 65 and (w - 1) & (w - 2) == 0:
        return "2^%d+1" % ((w - 1).bit_length() - 1)
    return str(w)


WIDTH_IDS = [_wid(w) for w in er.WIDTHS]


@pytest.mark.parametrize("few_max", [0, -1], ids=["few_default", "few_off"])
@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("ncol", er.WIDTHS, ids=WIDTH_IDS)
def test_coo_sink(ctx, capfd, ncol, path, few_max):
    """The COO sink, count and store pass: the oracle's tuples in the oracle's order under every setting of emit_path (a
    forced ordering gives the tuples of the natural one) and with every mid row on k_hash."""
    c = er.width_case(ncol)
    what = "%d columns, emit_path %d, few_max %d" % (ncol, path, few_max)
    gi, gj, gv, res, few = _traced(ctx, capfd, c, {"emit_path": path, "few_max": few_max}, _capi().SINK_COO)
    _check_routing(c, res, few, few_max, what)
    check_tuples((gi, gj, gv), er.oracle_tuples(c), what + ": COO sink")
    assert res.nnz == sum(r.outputs for r in c.rec)


def _capi():
    from spsparse_amd import capi
    return capi


@pytest.mark.parametrize("few_max", [0, -1], ids=["few_default", "few_off"])
@pytest.mark.parametrize("ncol", er.WIDTHS, ids=WIDTH_IDS)
def test_digest_sink(ctx, capfd, ncol, few_max):
    """The digest sink with and without ROWSTATS: nnz, hash and sum exact, row_nnz and row_hash exact."""
    capi = _capi()
    c = er.width_case(ncol)
    want = er.oracle_tuples(c)
    nrow = c.A.shape[0]
    what = "%d columns, few_max %d" % (ncol, few_max)
    *_, d, few = _traced(ctx, capfd, c, {"few_max": few_max}, capi.SINK_DIGEST)
    _check_routing(c, d, few, few_max, what)
    check_digest(d, want, what)
    *_, d, few = _traced(ctx, capfd, c, {"few_max": few_max}, capi.SINK_DIGEST, capi.SINK_ROWSTATS)
    _check_routing(c, d, few, few_max, what + ", ROWSTATS")
    check_digest(d, want, what + ", ROWSTATS")
    nnz, h = er.row_stats(want, nrow)
    assert np.array_equal(ctx.to_host(d.row_nnz, nrow, np.int64), nnz), what
    assert np.array_equal(ctx.to_host(d.row_hash, nrow, np.uint64), h), what
    assert np.array_equal(nnz, [r.outputs for r in c.rec])


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("ncol", [w for w in er.WIDTHS if w < er.SCALE_BELOW], ids=WIDTH_IDS[:-1])
def test_scale_vectors(ctx, capfd, ncol, path):
    """C != 1, scalei (a row absent, a row scaled by 0: neither is a mid row then) and scalek with a fifth of the columns
    absent: a dropped column shifts every later rank.  Powers of two: still exact."""
    capi = _capi()
    c = er.width_case(ncol)
    kw = er.scales(c)
    want = er.oracle_tuples(c, scaled=True)
    on = np.zeros(c.A.shape[0], bool)
    on[kw["scalei"].idx[kw["scalei"].val != 0]] = True
    what = "%d columns, scaled, emit_path %d" % (ncol, path)
    gi, gj, gv, res, few = _traced(ctx, capfd, c, {"emit_path": path}, capi.SINK_COO, **kw)
    _check_routing(c, res, few, 0, what, on)
    check_tuples((gi, gj, gv), want, what + ": COO sink")
    if path == 0:
        *_, d, few = _traced(ctx, capfd, c, {}, capi.SINK_DIGEST, **kw)
        check_digest(d, want, what)


@pytest.mark.parametrize("mode", ["ordered", "exact_pattern"])
def test_widest_matrix_ordered_and_exact_pattern(ctx, capfd, mode):
    """2^31 columns under SINK_ORDERED (hash_products_ordered feeds the same emission) and SINK_EXACT_PATTERN (pat_fix_wave
    takes the column): every mid row on k_hash, the oracle's tuples bit for bit, column 2^31 - 1 among them."""
    capi = _capi()
    c = er.width_case(er.TOP)
    want = er.oracle_tuples(c)
    flags = capi.SINK_ORDERED if mode == "ordered" else capi.SINK_EXACT_PATTERN
    gi, gj, gv, res, few = _traced(ctx, capfd, c, {}, capi.SINK_COO, flags)
    _check_routing(c, res, few, -1, mode)
    check_tuples((gi, gj, gv), want, mode + ": COO sink")
    assert gj.max() == (1 << 31) - 1
    *_, d, few = _traced(ctx, capfd, c, {}, capi.SINK_DIGEST, flags)
    _check_routing(c, d, few, -1, mode)
    check_digest(d, want, mode)


# ---- the heavy rows' hash cells

@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("T,W,where", er.WINDOW_CASES, ids=["%s-%d-%s" % x for x in er.WINDOW_CASES])
def test_window_cells(ctx, capfd, T, W, where, path):
    """Cells of 1 .. 5 (9) windows at the bottom and at the top of 2048 windows: colbits on a table's last bitmap width
    and its first radix width, colbase + rel up to the last column, under every setting of emit_path; the table of 3072
    with more than 1024 outputs (the bitonic network pads them to 2048 keys)."""
    p = er.window_case(T, W, where)
    for scheme in p.schemes:
        coo, dig = shapes.run_plan(ctx, capfd, p, scheme, extra={"emit_path": path})
        n = len(er.spans_of(T, W))
        assert coo.rows_heavy == n and coo.cells_hash == n and coo.window == W
        assert (coo.products_tiles > 0) == (T == "tiles")
