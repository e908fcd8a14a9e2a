"""spsamd_select on the device against tests/select_ref.py (pinned on the host by tests/test_select_host.py): indices equal
and values as int64 bit patterns, zero tolerance -- the call computes no value, so there is nothing to tolerate.  ROW_TOPK
runs under every setting of the select_path knob, so that every row meets every kernel that can hold it."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as orc
from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests.gpu_util import check_tuples as _check, coo as _coo, ctx, forced  # noqa: F401
from tests import select_ref as sr

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2, 3)


def _select(ctx, A, pred, path=0, **kw):
    with forced(ctx, "select_path", path):
        return ctx.select(A, pred, **kw)


def _params(rng, pred, S):
    if pred <= sr.OFFDIAG:
        return int(rng.integers(-4, 5)), 0.0
    if pred == sr.ROW_TOPK:
        return int(rng.choice([0, 1, 2, 3, 7, 50])), 0.0
    finite = np.abs(S[2][np.isfinite(S[2])])
    pick = [0.0, 0.25, 1.0, np.inf] + ([float(rng.choice(finite))] if finite.size else [])
    return 0, float(pick[int(rng.integers(len(pick)))])


def test_semantic_cases(ctx):
    """All seven predicates and their complements, both transposes, the three policies, zero_nan, host and device operands,
    raw (unique keys with NaN / Inf / +-0; duplicate keys) and trusted (sorted by the leading index only: duplicate keys and
    columns out of order inside a row, special values anywhere), every select_path."""
    rng = np.random.default_rng(21)
    for trial in range(280):
        shape = (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        nnz = int(rng.integers(0, 3000 if trial % 7 == 0 else 250))
        t = '.' if trial % 4 < 2 else 'T'
        lead = 1 if t == 'T' else 0
        nrow = shape[lead]
        pol, zn = trial % 3, bool(trial % 5 == 0)
        kind = trial % 3
        ties = trial % 2 == 0
        sort0 = -1
        if kind == 0:
            A = sr.unique_key_operand(rng, shape, nnz, ties=ties)
        elif kind == 1:
            A = sr.duplicate_key_operand(rng, shape, nnz, ties=ties)
        else:
            i0 = rng.integers(0, shape[0], nnz).astype(np.int32)
            i1 = rng.integers(0, shape[1], nnz).astype(np.int32)
            v = sr.special_values(rng, nnz, 0.3, ties)
            o = np.argsort(i1 if lead else i0, kind="stable")
            A, sort0 = (i0[o], i1[o], v[o]), lead
        S = sr.operand_S(A, t, pol, zn, sort0)
        keep = []
        a = _coo(A, shape, sort0, device=trial % 2 == 1, keep=keep)
        for pred in sr.PREDICATES:
            ip, dp = _params(rng, pred, S)
            for comp in (False, True):
                res = _select(ctx, a, pred, trial % 4, iparam=ip, dparam=dp, complement=comp, transpose=t,
                              duplicate_policy=pol, zero_nan=zn)
                what = "trial %d pred %d ip %d dp %r comp %d %s pol %d zn %d kind %d" % (trial, pred, ip, dp, comp, t, pol, zn, kind)
                assert (res.shape0, res.shape1) == ((shape[1], shape[0]) if lead else shape), what
                assert res.nnz_a == len(S[2]), what
                _check(ctx.fetch(res), sr.select_ref(S, nrow, pred, ip, dp, comp), what)


def test_lying_sort0_is_rejected(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(22)
    A = sr.unique_key_operand(rng, (30, 20), 400)
    assert np.any(np.diff(A[0]) < 0) and np.any(np.diff(A[1]) < 0)
    for device in (False, True):
        keep = []
        for t, s0 in (('.', 0), ('T', 1)):
            for pred in sr.PREDICATES:
                with pytest.raises(capi.SpsamdError) as e:
                    ctx.select(_coo(A, (30, 20), s0, device, keep), pred, iparam=1, dparam=0.5, transpose=t)
                assert e.value.code == -2
        # the other order's claim is no claim about this one: the operand is consolidated
        res = ctx.select(_coo(A, (30, 20), 1, device, keep), sr.TRIL, iparam=0)
        _check(ctx.fetch(res), sr.select_ref(sr.operand_S(A), 30, sr.TRIL, 0), "sort0 of the other order")


_ROWS = {}


def _row_classes():
    """One matrix with rows of exactly 0, 1, light_max, light_max + 1, mid_max, mid_max + 1 and 200 000 tuples (twice each:
    mixed values, and one magnitude with both signs -- every decision a tie)."""
    from spsparse_amd import capi
    if not _ROWS:
        rng = np.random.default_rng(23)
        base = [0, 1, capi.select_light_max, capi.select_light_max + 1, capi.select_mid_max, capi.select_mid_max + 1, 200_000]
        lengths = base + base[1:] + [0, 3]
        equal = set(range(len(base), len(base) + len(base) - 1))
        ncol = 1 << 18
        _ROWS["X"] = sr.rows_of_lengths(rng, lengths, ncol, equal_rows=equal)
        _ROWS["shape"] = (len(lengths), ncol)
    return _ROWS["X"], _ROWS["shape"]


@pytest.mark.parametrize("path", PATHS)
def test_topk_row_classes(ctx, path):
    from spsparse_amd import capi
    X, shape = _row_classes()
    lens = np.bincount(X[0], minlength=shape[0])
    keep = []
    a = _coo(X, shape, 0, True, keep)
    for k in (0, 1, 2, 63, 64, 65, 4096, 10 ** 6):
        for comp in (False, True):
            res = _select(ctx, a, sr.ROW_TOPK, path, iparam=k, complement=comp)
            _check(ctx.fetch(res), sr.select_ref(X, shape[0], sr.ROW_TOPK, k, complement=comp), "path %d k %d comp %d" % (path, k, comp))
            served = lens[lens > k]
            assert res.rows_light + res.rows_mid + res.rows_heavy == served.size
            assert res.tuples_light + res.tuples_mid + res.tuples_heavy == served.sum()
            if path == 0 and k == 1:                     # the input has rows for every class
                assert res.rows_light > 0 and res.rows_mid > 0 and res.rows_heavy > 0
                assert res.rows_light == np.sum((lens > 1) & (lens <= capi.select_light_max))
                assert res.rows_mid == np.sum((lens > capi.select_light_max) & (lens <= capi.select_mid_max))
                assert res.rows_heavy == np.sum(lens > capi.select_mid_max)
            if path == 2:
                assert res.rows_light == 0 and res.rows_heavy == np.sum((lens > k) & (lens > capi.select_mid_max))
            if path == 3:
                assert res.rows_light == 0 and res.rows_mid == 0


@pytest.mark.parametrize("path", PATHS)
def test_value_predicates_on_long_rows(ctx, path):
    X, shape = _row_classes()
    keep = []
    a = _coo(X, shape, 0, True, keep)
    for pred, dp in ((sr.ABS_GE, 1.0), (sr.ABS_GE, 2.0), (sr.ROW_REL, 0.25), (sr.ROW_REL, 1.0), (sr.ROW_REL, 0.0)):
        for comp in (False, True):
            res = _select(ctx, a, pred, path, dparam=dp, complement=comp)
            _check(ctx.fetch(res), sr.select_ref(X, shape[0], pred, 0, dp, comp), "pred %d theta %r comp %d" % (pred, dp, comp))
    for d in (-1, 0, 70000):
        res = _select(ctx, a, sr.TRIU, path, iparam=d)
        _check(ctx.fetch(res), sr.select_ref(X, shape[0], sr.TRIU, d), "triu %d" % d)


def test_chain_product_topk_product(ctx):
    """A*A -> select(ROW_TOPK, 16) reading the output set in place -> multiply again, against the same chain through
    ctx.fetch and select_ref on the host."""
    from spsparse_amd import capi
    i0, i1, v, shape = wl.rmat(12, seed=7)
    keep = []
    a = _coo((i0, i1, v), shape, -1, True, keep)
    for path in PATHS:
        r1 = ctx.multiply(a, a, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
        S = ctx.fetch(r1)
        T_h = sr.select_ref(S, shape[0], sr.ROW_TOPK, 16)
        r2 = _select(ctx, capi.result_operand(r1), sr.ROW_TOPK, path, iparam=16)
        assert r2.nnz_a == r1.nnz
        _check(ctx.fetch(r2), T_h, "top-16 of A*A, path %d" % path)
        r3 = ctx.multiply(capi.result_operand(r2), a, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
        got = ctx.fetch(r3)
        r4 = ctx.multiply(_coo(T_h, shape, 0, False, keep), a, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
        _check(got, ctx.fetch(r4), "top16(A*A) * A, path %d" % path)
        assert len(got[2]) > 0


def test_prepared_operand_both_transposes(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(24)
    shape = (35, 25)
    B = ar.random_operand(rng, shape, 900, special=0.0)
    keep = []
    for tprep in ('.', 'T'):
        lead = 1 if tprep == 'T' else 0
        op = capi.Operand(ctx, _coo(B, shape, -1, False, keep), tprep, capi.AS_A, capi.ADD, False)
        try:
            P = orc.consolidate(B[0], B[1], B[2], lead, ar.ADD, False)
            for t in ('.', 'T'):
                S = sr.operand_S(P, t, sort0=lead)
                nrow = shape[1] if t == 'T' else shape[0]
                for pred, ip, dp in ((sr.ROW_TOPK, 3, 0.0), (sr.TRIL, -1, 0.0), (sr.ROW_REL, 0, 0.5)):
                    res = ctx.select(op.coo, pred, iparam=ip, dparam=dp, transpose=t)
                    _check(ctx.fetch(res), sr.select_ref(S, nrow, pred, ip, dp), "prepared %s used %s pred %d" % (tprep, t, pred))
        finally:
            op.close()


def test_permute_sink_and_column_topk(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(25)
    shape = (40, 30)
    A = sr.unique_key_operand(rng, shape, 700)
    keep = []
    res = ctx.select(_coo(A, shape, -1, True, keep), sr.ROW_TOPK, iparam=3, transpose='T', flags=capi.SINK_PERMUTE)
    S = sr.operand_S(A, 'T')
    wi, wj, wv = sr.select_ref(S, shape[1], sr.ROW_TOPK, 3)
    assert (res.shape0, res.shape1) == shape                    # the top 3 of every column, in A's own orientation
    gi, gj, gv = ctx.fetch(res)
    _check((gj, gi, gv), (wi, wj, wv), "permute")
    # chained back as the column-major operand it is
    P = capi.Coo(res.idx0, res.idx1, res.val, int(res.nnz), shape[0], shape[1], 1, capi.MEM_DEVICE)
    r2 = ctx.select(P, sr.TRIL, iparam=0, transpose='T', complement=True)
    _check(ctx.fetch(r2), sr.select_ref((wi, wj, wv), shape[1], sr.TRIL, 0, complement=True), "permuted result chained")


def test_digest_sink(ctx):
    import torch
    from spsparse_amd import capi
    from tests import projection as pj
    rng = np.random.default_rng(26)
    shape = (500, 400)
    A = ar.random_operand(rng, shape, 60_000, special=0.0)
    keep = []
    a = _coo(A, shape, -1, True, keep)
    S = sr.operand_S(A)
    for pred, ip, dp in ((sr.ROW_TOPK, 20, 0.0), (sr.ABS_GE, 0, 0.7), (sr.OFFDIAG, 0, 0.0)):
        wi, wj, wv = sr.select_ref(S, shape[0], pred, ip, dp)
        d = ctx.select(a, pred, iparam=ip, dparam=dp, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
        assert d.nnz == len(wv) and d.nnz_a == len(S[2])
        rn = ctx.to_host(d.row_nnz, shape[0], np.int64)
        assert np.array_equal(rn, np.bincount(wi, minlength=shape[0]))
        assert abs(d.sum - wv.sum()) <= 1e-9 * np.abs(wv).sum()
        c = ctx.select(a, pred, iparam=ip, dparam=dp)
        gi, gj, gv = ctx.fetch(c)
        _check((gi, gj, gv), (wi, wj, wv), "coo run")
        mix = pj.mix64_t(torch.from_numpy(gi.astype(np.int64)), torch.from_numpy(gj.astype(np.int64)))
        assert d.hash == int(mix.sum().item()) & (2 ** 64 - 1)
        for flags in (capi.SINK_ORDERED, capi.SINK_EXACT_PATTERN):      # accepted, change nothing
            _check(ctx.fetch(ctx.select(a, pred, iparam=ip, dparam=dp, flags=flags)), (wi, wj, wv), "flags %d" % flags)


def test_scatter_dense_of_a_tril_result(ctx):
    import torch
    rng = np.random.default_rng(27)
    shape = (60, 50)
    A = ar.random_operand(rng, shape, 2500, special=0.0)
    keep = []
    res = ctx.select(_coo(A, shape, -1, False, keep), sr.TRIL, iparam=-1)
    dense = torch.zeros(shape, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.scatter_dense(res, dense.data_ptr(), shape[1])
    wi, wj, wv = sr.select_ref(sr.operand_S(A), shape[0], sr.TRIL, -1)
    want = np.zeros(shape)
    want[wi, wj] = wv
    assert np.array_equal(dense.cpu().numpy(), want) and np.all(np.triu(want) == 0)


def test_triangle_count(ctx):
    """The advertised use: L = tril(A, -1) of a symmetric 0/1 pattern, then (L*L) o L sums to the number of triangles."""
    from spsparse_amd import capi
    i0, i1, _v, shape = wl.rmat(12, seed=3)
    n = shape[0]
    key = np.unique(np.concatenate([i0.astype(np.int64) * n + i1, i1.astype(np.int64) * n + i0]))
    si, sj = (key // n).astype(np.int32), (key % n).astype(np.int32)
    keep = []
    a = _coo((si, sj, np.ones(len(key))), shape, 0, True, keep)
    L = ctx.select(a, sr.TRIL, iparam=-1)
    assert L.nnz == np.sum(sj < si)
    Lop = capi.result_operand(L)
    tri = ctx.multiply_masked(Lop, Lop, Lop, flags=capi.SINK_ORDERED)
    got = ctx.fetch(tri)[2].sum()
    Ld = np.zeros((n, n), np.float32)
    Ld[si[sj < si], sj[sj < si]] = 1.0
    want = float(((Ld @ Ld) * Ld).sum(dtype=np.float64))
    assert want > 0 and got == want


def _raw(ctx, A, res, pred=1, ip=0, dp=0.0, sflags=0, pol=1, zn=0, sink=1, flags=0):
    return ctx.L.spsamd_select(ctx.h, None if A is None else C.byref(A), b'.', pred, ip, dp, sflags, pol, zn, sink, flags,
                               None if res is None else C.byref(res))


def test_errors_leave_the_context_usable(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(28)
    A = sr.unique_key_operand(rng, (6, 8), 30)
    keep = []
    a = _coo(A, (6, 8), -1, False, keep)
    res = capi.Result()
    assert _raw(ctx, None, res) == -2 and _raw(ctx, a, None) == -2
    assert _raw(ctx, a, res, pred=0) == -2 and _raw(ctx, a, res, pred=8) == -2
    assert _raw(ctx, a, res, sflags=2) == -2
    assert _raw(ctx, a, res, sink=3) == -2 and _raw(ctx, a, res, sink=0) == -2
    assert _raw(ctx, a, res, pol=3) == -2 and _raw(ctx, a, res, pol=-1) == -2
    for pred in (sr.ABS_GE, sr.ROW_REL):
        assert _raw(ctx, a, res, pred=pred, dp=-1.0) == -2 and _raw(ctx, a, res, pred=pred, dp=float("nan")) == -2
        assert _raw(ctx, a, res, pred=pred, dp=float("inf")) == 0
    assert _raw(ctx, a, res, pred=sr.ROW_TOPK, ip=-1) == -2
    assert _raw(ctx, a, res, pred=sr.TRIL, ip=-2 ** 63) == 0 and res.nnz == 0
    assert _raw(ctx, a, res, pred=sr.TRIL, ip=2 ** 63 - 1) == 0 and res.nnz == len(sr.operand_S(A)[2])
    for device in (False, True):
        bad = (A[0].copy(), A[1].copy(), A[2])
        bad[1][5] = 8
        assert _raw(ctx, _coo(bad, (6, 8), -1, device, keep), res) == -2
        bad[1][5] = -1
        assert _raw(ctx, _coo(bad, (6, 8), 0 if device else -1, device, keep), res) == -2
    huge = capi.Coo(a.idx0, a.idx1, a.val, 2 ** 31, 6, 8, -1, capi.MEM_HOST)
    assert _raw(ctx, huge, res) == -2
    # an empty A: an empty result of op(A)'s shape
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    r = ctx.select(_coo(E, (6, 8), -1, False, keep), sr.ROW_TOPK, iparam=2, transpose='T')
    assert r.nnz == 0 and (r.shape0, r.shape1) == (8, 6)
    # and the context still works
    r = ctx.select(a, sr.ROW_TOPK, iparam=2)
    _check(ctx.fetch(r), sr.select_ref(sr.operand_S(A), 6, sr.ROW_TOPK, 2), "after the errors")
