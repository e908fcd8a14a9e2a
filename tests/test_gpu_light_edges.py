"""The light-row kernels (k_light.hip: k_light_direct<S, MODE, K64> for products in which every row is light, the binned
k_light<S> otherwise) at their class, key-width and round edges.  GPU only.

Inputs: tests/light_ref.py (tests/test_light_host.py pins what each must reach without a GPU).  Comparator: the row-wise
oracle, orc.multiply(..., rowwise=True).  The light kernels sum in ascending k, so the bars are exact:
  COO sink: index arrays and order identical, values bit for bit (random normal values);
  digest sink: nnz and hash exact, and the sum exact on the integer twin of the case (sums exact in any order);
  ROWSTATS: per-row count and hash exact, per-row sum exact on the integer twin.
Every case runs through the direct kernel with the COO sink in one pass and in two (light_two_pass), with the digest sink
with and without ROWSTATS, and through the binned kernels (light_path) with both sinks, and asserts from the result's
counters which of the two it ran: the direct kernel reports every row of op(A) as light, empty and skipped rows included;
the binned kernels only rows that have products.

Which variant of the direct kernel a column count takes is not in the counters; by the documented rule (spgemm_all_light)
it is the narrow one -- 32-bit keys (column << log2 S | A position), 32-bit addressing -- while bits(ncol - 1) + 6 <= 32,
except at S = 64 and exactly 2^26 columns, where the key of (column 2^26 - 1, A position 63) would be 0xFFFFFFFF, the
narrow "no product" mark: so 2^26 - 1 columns run narrow at every S, 2^26 narrow for S <= 32 and wide for S = 64,
2^26 + 1 and 2^31 wide.  (Before that exception the S = 64 case at 2^26 columns lost the last term of the top column's
sum: test_key_width[67108864-64] failed with one value differing.)"""
import numpy as np
import pytest

from oracle import binding as orc
from tests import light_ref as lr
from tests.gpu_util import Knobs, check_digest, check_tuples, ctx  # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu

DIRECT, TWO_PASS, BINNED = {}, {"light_two_pass": 1}, {"light_path": 1}


def _call(ctx, A, B, kw, sink, flags=0):
    from spsparse_amd import capi
    keep = []

    def vec(v):
        if v is None:
            return None
        s, k = capi.host_vec(v.idx, v.val, v.shape0, v.sort0)
        keep.append(k)
        return s
    a, ka = capi.host_coo(A.idx0, A.idx1, A.val, A.shape, A.sort0)
    b, kb = capi.host_coo(B.idx0, B.idx1, B.val, B.shape, B.sort0)
    res = ctx.multiply(a, b, kw.get("C_", 1.0), vec(kw.get("scalei")), kw.get("tA", "."), vec(kw.get("scalej")), kw.get("tB", "."),
                       vec(kw.get("scalek")), sink=sink, flags=flags)
    del ka, kb
    return res


def _row_stats(want, nrow):
    wi, wj, wv = want[:3]
    h = np.zeros(nrow, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(h, wi, orc.mix64(wi, wj))
    return np.bincount(wi, minlength=nrow), h, np.bincount(wi, weights=wv, minlength=nrow)


def _counters(res, eff, nrow, binned, what):
    print("%s: rows l/m/h = %d/%d/%d products = %d" % (what, res.rows_light, res.rows_mid, res.rows_heavy, res.products))
    assert res.products == eff.sum(), what
    want = int(np.sum(eff > 0)) if binned else nrow
    assert (res.rows_light, res.rows_mid, res.rows_heavy) == (want, 0, 0), what


def _all_ways(ctx, case, kw, what):
    """One case under kw through every way the light kernels take it; the normals and the integer twin."""
    from spsparse_amd import capi
    nrow, eff = case.rec["nrow"], lr.rowprod(case, kw)
    for ints in (False, True):
        A, B = case.operands(ints)
        want = orc.multiply(A, B, rowwise=True, **kw)
        rn, rh, rs = _row_stats(want, nrow)
        for knobs in (DIRECT, TWO_PASS, BINNED):
            w = "%s %s %s" % (what, "ints" if ints else "normals", knobs or "direct")
            binned = knobs is BINNED
            with Knobs(ctx, knobs):
                res = _call(ctx, A, B, kw, capi.SINK_COO)
                check_tuples(ctx.fetch(res), want[:3], w + " COO")
                assert res.nnz == len(want[0])
                _counters(res, eff, nrow, binned, w + " COO")
                if knobs is TWO_PASS:                                   # (the knob is about the COO sink only)
                    continue
                for rowstats in (0, capi.SINK_ROWSTATS):
                    d = _call(ctx, A, B, kw, capi.SINK_DIGEST, rowstats)
                    if ints:
                        check_digest(d, want, w + " digest")
                    else:
                        cnt, _, h = orc.digest(*want[:3])
                        assert (d.nnz, d.hash) == (cnt, h), w + " digest"
                    _counters(d, eff, nrow, binned, w + " digest")
                    if rowstats:
                        assert np.array_equal(ctx.to_host(d.row_nnz, nrow, np.int64), rn), w + " row_nnz"
                        assert np.array_equal(ctx.to_host(d.row_hash, nrow, np.uint64), rh), w + " row_hash"
                        if ints:
                            assert np.array_equal(ctx.to_host(d.row_sum, nrow, np.float64), rs), w + " row_sum"


# ------------------------------------------------------------------------------------------------ class edges

@pytest.mark.parametrize("la,lb", lr.CLASS_SHAPES)
@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_class_edges(ctx, la, lb, layout):
    """Rows of exactly la * lb = 8, 9, 16, 17, 32, 33 and 64 products, of one product less, empty rows, rows over empty B
    rows; plain (C = 1, no scale vector: the kernel's short emit) and with scalei skipping two full rows."""
    c = lr.class_case(la, lb, layout)
    assert c.rec["S"] == lr.s_class(la * lb) and c.rec["rowprod"].max() == la * lb
    _all_ways(ctx, c, {}, "%dx%d %s plain" % (la, lb, layout))
    _all_ways(ctx, c, c.kw, "%dx%d %s scalei" % (la, lb, layout))


@pytest.mark.parametrize("la,lb", lr.EXTRA_SHAPES)
@pytest.mark.parametrize("tA,tB", [("T", "."), (".", "T"), ("T", "T")])
def test_class_edges_scaled_and_transposed(ctx, la, lb, tA, tB):
    """C != 1, scalei, scalej and scalek with absent entries, 'T' on either side (op() keeps the intended row lengths)."""
    c = lr.class_case(la, lb, "mixed", tA, tB, extra=True)
    assert c.rec["rowprod"].max() == la * lb
    _all_ways(ctx, c, c.kw, "%dx%d %s%s extra" % (la, lb, tA, tB))


@pytest.mark.parametrize("la,lb", lr.STEP_OUT)
def test_step_out_of_the_direct_kernel(ctx, la, lb):
    """65 products: not all-light.  The full rows are mid rows (ascending-k sums there under SINK_ORDERED: bit for bit on the
    normals; the integer twin is exact in any order), the others stay with the binned light kernels."""
    from spsparse_amd import capi
    for layout in lr.LAYOUTS:
        c = lr.class_case(la, lb, layout)
        eff = lr.rowprod(c, {})
        assert eff.max() == 65
        for ints, flags in ((False, capi.SINK_ORDERED), (True, 0)):
            A, B = c.operands(ints)
            want = orc.multiply(A, B, rowwise=True)
            what = "%dx%d %s ints=%d" % (la, lb, layout, ints)
            res = _call(ctx, A, B, {}, capi.SINK_COO, flags)
            check_tuples(ctx.fetch(res), want[:3], what)
            assert (res.rows_light, res.rows_mid, res.rows_heavy) == (np.sum((eff > 0) & (eff <= 64)), np.sum(eff == 65), 0), what
            assert res.rows_mid >= 3 and res.products == eff.sum()
            d = _call(ctx, A, B, {}, capi.SINK_DIGEST, flags)
            if ints:
                check_digest(d, want, what)
            assert (d.nnz, d.rows_mid) == (len(want[0]), res.rows_mid), what


def test_maxlen_over_64_rows_under_65(ctx):
    """maxlen(A) * maxlen(B) = 66 with no row above 64 products: the binned light kernels by themselves, no knob set."""
    from spsparse_amd import capi
    c = lr.undershoot_case()
    eff = lr.rowprod(c, {})
    assert c.rec["maxp"] == 66 and eff.max() <= 64
    for ints in (False, True):
        A, B = c.operands(ints)
        want = orc.multiply(A, B, rowwise=True)
        res = _call(ctx, A, B, {}, capi.SINK_COO)
        check_tuples(ctx.fetch(res), want[:3], "undershoot ints=%d" % ints)
        _counters(res, eff, c.rec["nrow"], True, "undershoot COO")
        assert res.rows_light < c.rec["nrow"]
        d = _call(ctx, A, B, {}, capi.SINK_DIGEST)
        _counters(d, eff, c.rec["nrow"], True, "undershoot digest")
        if ints:
            check_digest(d, want, "undershoot")


# ------------------------------------------------------------------------------------------------ key width

@pytest.mark.parametrize("S", lr.KEY_S)
@pytest.mark.parametrize("ncol", lr.KEY_NCOLS)
def test_key_width(ctx, S, ncol):
    """Columns 0 and ncol - 1 from the first and the last A tuple of rows that fill class S, either side of the narrow key's
    limit and at the widest shape the multiply accepts.  Variant by the documented rule (module docstring): narrow for
    ncol <= 2^26 except (S = 64, 2^26), wide beyond."""
    assert lr.wide_variant(ncol, S) == (ncol > (1 << 26) or (S == 64 and ncol == 1 << 26))
    for tall in (True, False):
        c = lr.key_case(S, ncol, tall)
        assert c.rec["S"] == S and c.B.shape[1] == ncol
        _all_ways(ctx, c, {}, "S=%d ncol=%d %s" % (S, ncol, "tall" if tall else "flat"))


# ------------------------------------------------------------------------------------------------ pipeline rounds

def _cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("S", lr.KEY_S)
def test_pipeline_one_round(ctx, S):
    """1, 4G - 1, 4G and 4G + 1 rows: one round, whole and ragged groups, a second workgroup of one row."""
    for nrow in lr.pipe_nrows(S, _cu())[0]:
        c = lr.pipe_case(S, nrow)
        assert lr.rounds(nrow, S, _cu())[:2] == (1, 1)
        _all_ways(ctx, c, {}, "S=%d nrow=%d plain" % (S, nrow))
        _all_ways(ctx, c, c.kw, "S=%d nrow=%d scalei" % (S, nrow))


@pytest.mark.parametrize("S", lr.KEY_S)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_pipeline_rounds(ctx, S, which):
    """R - 1, R + 1 and 2R + 4G + 1 rows for the R = compute units * 32 * 4 * (64 / S) rows of one round of this device:
    one full round, a second round in one workgroup, three rounds beside two with a ragged last group.  No row looks like
    the row R below it (lengths, inner indices, columns and values are random, 5 % of the rows are skipped by scalei), so
    a round that used the next round's A tuple, B bounds or row pointer differs bit for bit.  The binned kernels' grid-stride
    loop takes the same row counts."""
    cu = _cu()
    nrow = lr.pipe_nrows(S, cu)[1][which]
    assert lr.rounds(nrow, S, cu) == [(1, 1, 4 * (64 // S) - 1), (1, 2, 1), (2, 3, 1)][which]
    c = lr.pipe_case(S, nrow)
    _all_ways(ctx, c, c.kw, "S=%d nrow=%d (%d CUs)" % (S, nrow, cu))
