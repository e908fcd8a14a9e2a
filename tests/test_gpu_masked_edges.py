"""spsamd_multiply_masked's evaluation kernels (k_masked.hip: k_masked_entry with its register join and its gallop walk,
k_masked_row, k_masked_wave) at their class, step and grid edges.  GPU only.

Inputs and reference: tests/masked_edges.py (tests/test_masked_edges_host.py pins join_ref / dense_ref to the oracle and
asserts what every input claims, without a GPU).  Every value is one serial chain in ascending k, so every comparison is
exact: keys equal, values as int64 bit patterns (check_tuples), res.products equal to the reference's count on both
sinks, the digest's count and hash exact.  Only the fuzz, whose values hold NaNs, counts two NaNs as equal
(masked_ref.same_tuples).  Unless a test says otherwise a case runs under all four masked_path
values, each against the same reference.

Which class the auto path (0) gives a key is not in the result; what 31 / 32 / 33 assert is that all four paths give the
reference's bits."""
import numpy as np
import pytest

from oracle import binding as orc
from tests import add_ref as ar
from tests import masked_edges as me
from tests import masked_ref as mr
from tests.gpu_util import check_digest, check_tuples, coo as _coo, ctx, forced  # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu

PATHS = me.PATHS
CS = (1.0, -0.75, np.inf)


def _vec(s, dim, keep):
    from spsparse_amd import capi
    if s is None:
        return None
    v, k = capi.host_vec(s[0], s[1], dim)
    keep.append(k)
    return v


def _call(ctx, case, path, scalej=True, tA='.', tB='.', sink=None, flags=0):
    """The case through one path; 'T': the operand is handed over transposed, so op() is the case's own."""
    from spsparse_amd import capi
    keep = []
    A, ash = (case.A, case.ashape) if tA == '.' else ((case.A[1], case.A[0], case.A[2]), case.ashape[::-1])
    B, bsh = (case.B, case.bshape) if tB == '.' else ((case.B[1], case.B[0], case.B[2]), case.bshape[::-1])
    a, b = _coo(A, ash, -1, True, keep), _coo(B, bsh, -1, True, keep)
    m = _coo((case.M[0], case.M[1], np.ones(len(case.M[0]))), (case.ashape[0], case.bshape[1]), -1, True, keep)
    sc = [_vec(s, d, keep) for s, d in ((case.scalei, case.ashape[0]), (case.scalej if scalej else None, case.ashape[1]),
                                        (case.scalek, case.bshape[1]))]
    with forced(ctx, "masked_path", path):
        return ctx.multiply_masked(a, b, m, case.C, sc[0], tA, sc[1], tB, sc[2], sink=capi.SINK_COO if sink is None else sink, flags=flags)


def _count_hash(want):
    """Count and index hash of the digest sink (the sum is left out: a value may be NaN or Inf)."""
    with np.errstate(over="ignore"):
        return len(want[0]), int(np.sum(orc.mix64(want[0], want[1]), dtype=np.uint64))


def _both_sinks(ctx, case, want, path, what, **kw):
    from spsparse_amd import capi
    res = _call(ctx, case, path, **kw)
    check_tuples(ctx.fetch(res), want[:3], what + " COO")
    assert res.products == want[3], "%s COO: %d products, want %d" % (what, res.products, want[3])
    d = _call(ctx, case, path, sink=capi.SINK_DIGEST, **kw)
    assert (d.nnz, d.hash, d.products) == _count_hash(want) + (want[3],), what + " digest"


# ------------------------------------------------------------------------------------------------ a. semantics, every path

def test_semantic_fuzz_every_path(ctx):
    """tests/test_gpu_masked.py::test_argument_grid's recipe with masked_path as a digit of the trial number: both
    transposes, the three scales present or absent (with missing and zero entries), C in {1, -0.75, Inf}, the three
    policies, zero_nan, NaN / +-Inf / +-0 values, operands host or device, M host, sorted with duplicates, or device.
    Every third trial has an inner dimension of 64..300 and up to 4000 tuples per operand: lists of several wave steps.
    The reference is masked_ref; both sinks report the same number of products."""
    from spsparse_amd import capi
    rng = np.random.default_rng(31)
    seen_t, seen_s = set(), set()
    for trial in range(256):
        path, tA, tB = trial % 4, ('.', 'T')[(trial // 4) % 2], ('.', 'T')[(trial // 8) % 2]
        present = (trial // 16) % 8
        big = trial % 3 == 0
        nrow, ncol = (int(x) for x in rng.integers(1, 30, 2))
        ninner = int(rng.integers(64, 301)) if big else int(rng.integers(1, 30))
        ash = (ninner, nrow) if tA == 'T' else (nrow, ninner)
        bsh = (ncol, ninner) if tB == 'T' else (ninner, ncol)
        pol = (trial // 3) % 3
        junk = bool(rng.integers(2))
        zn = junk or bool(trial % 5 == 0)
        top = 4000 if big else 300
        A = mr.sanitize_duplicates(ar.random_operand(rng, ash, int(rng.integers(0, top)), 0.3, lead_junk=junk))
        B = mr.sanitize_duplicates(ar.random_operand(rng, bsh, int(rng.integers(0, top)), 0.3, lead_junk=junk))
        sc = [mr.random_scale(rng, d, bool(present >> n & 1)) for n, d in enumerate((nrow, ninner, ncol))]
        keep = []
        dv = [_vec(s, d, keep) for s, d in zip(sc, (nrow, ninner, ncol))]
        ov = [None if s is None else orc.Vec(s[0], s[1], d) for s, d in zip(sc, (nrow, ninner, ncol))]
        C_ = CS[trial % 3] if trial % 7 else 1.0
        a = _coo(A, ash, -1, bool(trial // 2 % 2), keep)
        b = _coo(B, bsh, -1, bool(trial // 32 % 2), keep)
        M = mr.random_mask(rng, (nrow, ncol), int(rng.integers(1, 400)))
        mform = trial // 5 % 3
        if mform == 0:
            m = _coo((M[0], M[1], np.zeros(len(M[0]))), (nrow, ncol), -1, False, keep)
        elif mform == 1:
            o = np.lexsort((M[1], M[0]))
            m = _coo((M[0][o], M[1][o], np.ones(len(o))), (nrow, ncol), 0, False, keep, no_val=True)
        else:
            m = _coo((M[0], M[1], np.ones(len(M[0]))), (nrow, ncol), -1, True, keep)
        want = mr.masked_ref(orc.Mat(*A, ash), orc.Mat(*B, bsh), M, C_, ov[0], tA, ov[1], tB, ov[2], pol, zn)
        what = "trial %d path %d %s%s scales %d pol %d zn %d C %r" % (trial, path, tA, tB, present, pol, zn, C_)
        with forced(ctx, "masked_path", path):
            res = ctx.multiply_masked(a, b, m, C_, dv[0], tA, dv[1], tB, dv[2], duplicate_policy=pol, zero_nan=zn)
            got = ctx.fetch(res)
            d = ctx.multiply_masked(a, b, m, C_, dv[0], tA, dv[1], tB, dv[2], duplicate_policy=pol, zero_nan=zn, sink=capi.SINK_DIGEST)
        assert (res.shape0, res.shape1) == (nrow, ncol)
        check_tuples(got, want, what, mr.same_tuples,
                     lambda g, w: (g.view(np.int64) != w.view(np.int64)) & ~(np.isnan(g) & np.isnan(w)))
        assert (d.nnz, d.hash, d.products) == _count_hash(want) + (res.products,), what
        seen_t.add((path, tA, tB))
        seen_s.add((path, present))
    assert seen_t == {(p, x, y) for p in PATHS for x in ".T" for y in ".T"}
    assert seen_s == {(p, s) for p in PATHS for s in range(8)}


# ------------------------------------------------------------------------------------------------ b. c. the entry kernel

@pytest.mark.parametrize("path", PATHS)
def test_short_join_edges(ctx, path):
    """MASK_SHORT = 8: la, lb over {1, 7, 8, 9}^2 with no match, all of the shorter list, only the first, only the last
    and every other k; scalej skips one matched k per key; the cancelling keys (a*b then -a*b, exact) are absent."""
    case = me.short_case()
    for sj in (True, False):
        _both_sinks(ctx, case, me.reference("short", sj), path, "short path %d scalej %d" % (path, sj), scalej=sj)


@pytest.mark.parametrize("path", PATHS)
def test_gallop_positions(ctx, path):
    """A short list of 12..40 against a long one of 3000 with the matches 1, 2, 3, 4, 5, 7, 8, 9, 15 ... 257 apart in the
    long list (around every doubling of gallop's step), ending on the long list's final element, running past its end,
    starting below its start; A long and B long; scalej present."""
    case = me.gallop_case()
    _both_sinks(ctx, case, me.reference("gallop"), path, "gallop path %d" % path)
    _both_sinks(ctx, case, me.reference("gallop"), path, "gallop path %d TT" % path, tA='T', tB='T')


# ------------------------------------------------------------------------------------------------ d. the wave kernel

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sj", (False, True))
def test_wave_step_edges(ctx, path, sj):
    """Short lengths 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200 against s, s + 1 and 5000: matches in lane 63, in lane
    0 of the next step, in the last element of a partial step, a long list that ends between two steps; A short and B
    short; without scalej, and with a scalej of values that are no powers of two that misses matched k's ((a * sj) * b
    tells a swap of aval and bval apart)."""
    _both_sinks(ctx, me.wave_case(), me.reference("wave", sj), path, "wave path %d scalej %d" % (path, sj), scalej=sj)


@pytest.mark.parametrize("path", PATHS)
def test_wave_largest_inner_dimension(ctx, path):
    """Inner dimension 2^31 (the largest the operand check accepts; consolidating op(B) takes no memory in proportion to
    it), matches at k = 0 and k = 2^31 - 1."""
    case = me.big_inner_case()
    _both_sinks(ctx, case, me.reference("big_inner", False), path, "inner 2^31 path %d" % path, scalej=False)


# ------------------------------------------------------------------------------------------------ e. the row kernel

@pytest.mark.parametrize("path", PATHS)
def test_row_cap_and_row_widths(ctx, path):
    """A rows of 4095, 4096 and 4097 tuples (MASK_ROW_CAP; under path 2 the 4097 rows' keys come from the entry kernel),
    mask rows of 1, 255, 256, 257 and 600 keys, empty B columns inside the rows, scalei with rows missing and zero."""
    case = me.row_case()
    for sj in (True, False):
        _both_sinks(ctx, case, me.reference("row", sj), path, "row path %d scalej %d" % (path, sj), scalej=sj)


# ------------------------------------------------------------------------------------------------ f. grid strides

def test_every_stride_takes_a_second_pass(ctx):
    """Inputs sized from the device's CU count, 10 % over the launches' caps of num_cu * 32 workgroups: a complete mask
    for the entry and wave kernels (paths 0, 1, 3) and the digest kernel (2048 workgroups), and num_cu * 32 + 300 mask
    rows for the row kernel, whose second row is staged over the first one's LDS copy."""
    import torch
    from spsparse_amd import capi
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    case = me.stride_dense_case(num_cu)
    nkeys = len(case.M[0])
    assert nkeys > num_cu * 32 * 256 and nkeys > num_cu * 32 * 4 and nkeys > 2048 * 256
    want = me.reference("stride_dense", True, num_cu)
    for path in (0, 1, 3):
        res = _call(ctx, case, path)
        check_tuples(ctx.fetch(res), want[:3], "stride path %d" % path)
        assert res.products == want[3]
    n = case.ashape[0]
    d = _call(ctx, case, 0, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
    check_digest(d, want, "stride digest")
    assert d.products == want[3]
    rh = np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(rh, want[0], orc.mix64(want[0], want[1]))
    assert np.array_equal(ctx.to_host(d.row_nnz, n, np.int64), np.bincount(want[0], minlength=n))
    assert np.array_equal(ctx.to_host(d.row_hash, n, np.uint64), rh)
    rows = me.stride_row_case(num_cu)
    assert rows.ashape[0] > num_cu * 32 and rows.claims["shorter_second"] > 0
    _both_sinks(ctx, rows, me.reference("stride_row", True, num_cu), 2, "row stride")
