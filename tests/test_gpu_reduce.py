"""spsamd_reduce on the device against tests/reduce_ref.py (pinned on the host by tests/test_reduce_host.py): indices equal and
values as int64 bit patterns, zero tolerance -- every value is defined by a serial loop, so there is nothing to tolerate.
Every setting of the reduce_path knob runs, so that every row meets both row kernels."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as orc
from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests import dense_ref as dr
from tests import reduce_ref as rr
from tests import select_ref as sr
from tests.gpu_util import check_tuples, coo as _coo, ctx, forced  # noqa: F401

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2)


def _same(got, want, what):
    gi, gv = got
    wi, wv = want
    assert np.array_equal(gi, wi), "%s: rows %r, want %r" % (what, gi[:10], wi[:10])
    bad = np.flatnonzero(gv.view(np.int64) != wv.view(np.int64))
    assert bad.size == 0, "%s: %d values differ, first at row %d: %r (%#x) vs %r (%#x)" % (
        what, bad.size, gi[bad[0]], gv[bad[0]], gv.view(np.uint64)[bad[0]], wv[bad[0]], wv.view(np.uint64)[bad[0]])


def _dense_same(got, want, what):
    _same((np.arange(len(want)), got), (np.arange(len(want)), want), what)


def _device_reduce(ctx, a, nrow, op, post, t, pol, zn, dense):
    """Through torch device tensors (sentinel-filled); returns what the host forms return."""
    import torch
    val = torch.full((nrow,), -7.5, dtype=torch.float64, device="cuda")
    if dense:
        ctx.reduce(a, op, post, t, pol, zn, dense=True, out=val)
        return val.cpu().numpy()
    idx = torch.full((nrow,), -3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = ctx.reduce(a, op, post, t, pol, zn, out=(idx, val))
    gi, gv = idx.cpu().numpy(), val.cpu().numpy()
    assert np.all(gi[n:] == -3) and np.all(gv[n:] == -7.5)
    return gi[:n], gv[:n]


def test_semantic_cases(ctx):
    """All six ops x four posts, both transposes, the three policies, zero_nan, host and device operands, raw (unique keys
    with NaN / Inf / +-0; duplicate keys) and trusted operands (sorted by the leading index only, special values anywhere),
    sparse and dense form, host and device outputs, every reduce_path.  The kind of operand, the policy and the path are the
    three base-3 digits of the trial and the transpose, the operand's and the outputs' memory three bits of it, so that over
    the 200 trials every kind meets every policy under every path, with both transposes and either memory."""
    rng = np.random.default_rng(41)
    for trial in range(200):
        shape = (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        nnz = int(rng.integers(0, 3000 if trial % 7 == 0 else 250))
        t = '.' if trial % 2 == 0 else 'T'
        lead = 1 if t == 'T' else 0
        nrow = shape[lead]
        kind, pol, path = trial % 3, (trial // 3) % 3, (trial // 9) % 3
        zn = bool(trial % 5 == 0)
        sort0 = -1
        if kind == 0:
            A = sr.unique_key_operand(rng, shape, nnz)
        elif kind == 1:
            A = sr.duplicate_key_operand(rng, shape, nnz)
        else:
            i0 = rng.integers(0, shape[0], nnz).astype(np.int32)
            i1 = rng.integers(0, shape[1], nnz).astype(np.int32)
            v = sr.special_values(rng, nnz, 0.3)
            o = np.argsort(i1 if lead else i0, kind="stable")
            A, sort0 = (i0[o], i1[o], v[o]), lead
        S = sr.operand_S(A, t, pol, zn, sort0)
        keep = []
        a = _coo(A, shape, sort0, device=(trial // 2) % 2 == 1, keep=keep)
        dev_out = (trial // 4) % 2 == 1
        with forced(ctx, "reduce_path", path):
            for op in rr.OPS:
                # every post for a third of the (trial, op) pairs, one post in turn for the others
                for post in (rr.POSTS if (trial + op) % 3 == 0 else (rr.POSTS[(trial + op) % 4],)):
                    what = "trial %d op %d post %d %s pol %d zn %d kind %d path %d" % (trial, op, post, t, pol, zn, kind, path)
                    wi, wv, wd = rr.reduce_fast(S, nrow, op, post)
                    if dev_out:
                        _same(_device_reduce(ctx, a, nrow, op, post, t, pol, zn, False), (wi, wv), what + " sparse dev")
                        _dense_same(_device_reduce(ctx, a, nrow, op, post, t, pol, zn, True), wd, what + " dense dev")
                    else:
                        _same(ctx.reduce(a, op, post, t, pol, zn), (wi, wv), what + " sparse host")
                        _dense_same(ctx.reduce(a, op, post, t, pol, zn, dense=True), wd, what + " dense host")


def test_prepared_operand_both_transposes(ctx):
    """A handle prepared for '.' and one for 'T', each reduced under both transposes: with the handle's own transpose its
    tuples and its row pointer (which carries a trailing sentinel row) are read in place, with the other one the handle is
    a device operand sorted the other way.  All ops, sparse and dense form, every reduce_path, against reduce_ref on the
    oracle's consolidation.  12 x 300 with 3000 tuples: the rows are long (about 250 tuples), the columns short."""
    from spsparse_amd import capi
    rng = np.random.default_rng(46)
    shape = (12, 300)
    B = ar.random_operand(rng, shape, 3000, special=0.0)
    keep = []
    for tprep in ('.', 'T'):
        lead = 1 if tprep == 'T' else 0
        h = capi.Operand(ctx, _coo(B, shape, -1, False, keep), tprep, capi.AS_A, capi.ADD, False)
        try:
            P = orc.consolidate(B[0], B[1], B[2], lead, ar.ADD, False)
            for t in ('.', 'T'):
                S = sr.operand_S(P, t, sort0=lead)
                nrow = shape[1] if t == 'T' else shape[0]
                for op in rr.OPS:
                    wi, wv, wd = rr.reduce_ref(S, nrow, op)
                    assert len(wi) > 0
                    for path in PATHS:
                        what = "prepared %s used %s op %d path %d" % (tprep, t, op, path)
                        with forced(ctx, "reduce_path", path):
                            res = capi.Result()
                            _same(ctx.reduce(h.coo, op, transpose=t, result=res), (wi, wv), what)
                            assert (res.shape0, res.nnz, res.nnz_a) == (nrow, len(wi), len(S[2])), what
                            _dense_same(ctx.reduce(h.coo, op, transpose=t, dense=True), wd, what + " dense")
                    _same(ctx.reduce(h.coo, op, rr.RSQRT, transpose=t), (wi, rr.post_apply(wv, rr.RSQRT)), "post, " + what)
                    _same(_device_reduce(ctx, h.coo, nrow, op, rr.NONE, t, ar.ADD, False, False), (wi, wv), what + " dev")
                    _dense_same(_device_reduce(ctx, h.coo, nrow, op, rr.NONE, t, ar.ADD, False, True), wd, what + " dense dev")
        finally:
            h.close()


_ROWS = {}


def _row_classes():
    """A trusted operand with rows of exactly 0, 1, 63, 64, 65, 4096, 4097 and 20 000 tuples, the chunk edges of the long
    rows' tile, and a run of 70 empty rows (it crosses a wave's block of 64 rows).  Values of mixed magnitude: every order of
    summation gives other bits.  Rows in turn hold their diagonal tuple first, last and not at all.  Shared by the tests."""
    from spsparse_amd import capi
    if not _ROWS:
        rng = np.random.default_rng(42)
        ch = capi.reduce_chunk
        lengths = [0, 1, 63, 64, 65, 4096, 4097, 20_000, ch - 1, ch, ch + 1, 2 * ch + 1] + [0] * 70 + [3, 64, 65, 1]
        ncol = 1 << 15
        rows, cols, vals = [], [], []
        for r, n in enumerate(lengths):
            if n == 0:
                continue
            c = rng.choice(np.setdiff1d(np.arange(ncol), [r]), n, replace=False).astype(np.int32)
            if r % 3 == 0:
                c[0] = r
            elif r % 3 == 1:
                c[-1] = r
            v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
            rows.append(np.full(n, r, np.int32)); cols.append(c); vals.append(v)
        _ROWS["X"] = (np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))
        _ROWS["shape"] = (len(lengths), ncol)
        _ROWS["lens"] = np.array(lengths)
        _ROWS["want"] = {op: rr.reduce_fast(_ROWS["X"], len(lengths), op) for op in rr.OPS}
    return _ROWS


def test_row_class_reference_depends_on_the_order():
    """The shared input does what it is for: the sum of a long row in reverse order has other bits."""
    R = _row_classes()
    X, lens = R["X"], R["lens"]
    r = int(np.argmax(lens))
    v = X[2][X[0] == r]
    fwd = rr.fold_row(rr.SUM, r, np.zeros(len(v)), v)[1]
    back = rr.fold_row(rr.SUM, r, np.zeros(len(v)), v[::-1])[1]
    assert fwd != back and fwd != np.sum(v)
    assert fwd == R["want"][rr.SUM][2][r]


@pytest.mark.parametrize("path", PATHS)
def test_row_classes(ctx, path):
    from spsparse_amd import capi
    R = _row_classes()
    X, shape, lens = R["X"], R["shape"], R["lens"]
    keep = []
    a = _coo(X, shape, 0, True, keep)
    with forced(ctx, "reduce_path", path):
        for op in rr.OPS:
            wi, wv, wd = R["want"][op]
            res = capi.Result()
            gi, gv = ctx.reduce(a, op, result=res)
            _same((gi, gv), (wi, wv), "path %d op %d" % (path, op))
            _dense_same(ctx.reduce(a, op, dense=True), wd, "path %d op %d dense" % (path, op))
            assert (res.shape0, res.shape1, res.nnz, res.nnz_a) == (shape[0], 0, len(wi), len(X[2]))
            if op == rr.COUNT:
                continue
            short = (lens > 0) & (lens <= capi.reduce_light_max) if path == 0 else (lens > 0) if path == 1 else lens < 0
            long_ = (lens > 0) & ~short
            assert (res.rows_light, res.rows_mid, res.rows_heavy) == (short.sum(), 0, long_.sum()), (path, op)
            assert (res.tuples_light, res.tuples_mid, res.tuples_heavy) == (lens[short].sum(), 0, lens[long_].sum()), (path, op)
        for post in rr.POSTS[1:]:
            wi, wv = R["want"][rr.SUM_SQ][0], rr.post_apply(R["want"][rr.SUM_SQ][1], post)
            _same(ctx.reduce(a, rr.SUM_SQ, post), (wi, wv), "path %d post %d" % (path, post))


def test_post_operations_on_the_device(ctx):
    """The device's 1.0 / r and sqrt(r) against numpy's SSE results on the probe values of the host test: each probe
    value is a row of one tuple under SUM (0 + v = v, except that -0.0 becomes +0.0 and a NaN is quieted, as in the
    reference)."""
    rng = np.random.default_rng(43)
    x = rr.post_probe_values(rng)
    n = len(x)
    X = (np.arange(n, dtype=np.int32), np.zeros(n, np.int32), x)
    keep = []
    a = _coo(X, (n, 1), 0, True, keep)
    base = dr.add(np.zeros(n), x)
    for post in rr.POSTS:
        gi, gv = ctx.reduce(a, rr.SUM, post)
        _same((gi, gv), (np.arange(n, dtype=np.int32), rr.post_apply(base, post)), "post %d" % post)


def test_chain_scale_a_product_without_leaving_the_device(ctx):
    """T = A*A chained in place; d = reduce(T, SUM, RECIP) into torch tensors; multiply(scalei = device_vec(d), T, B) equals
    the product with the host-computed vector; T is still fetchable and unchanged after the reduce."""
    import torch
    from spsparse_amd import capi
    i0, i1, v, shape = wl.poisson2d(32)
    n = shape[0]
    keep = []
    a = _coo((i0, i1, v), shape, 0, True, keep)
    T = ctx.multiply(a, a, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
    Th = ctx.fetch(T)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    val = torch.empty(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    cnt = ctx.reduce(capi.result_operand(T), rr.SUM, rr.RECIP, out=(idx, val))
    wi, wv, _ = rr.reduce_fast(Th, n, rr.SUM, rr.RECIP)
    _same((idx.cpu().numpy()[:cnt], val.cpu().numpy()[:cnt]), (wi, wv), "row sums of A*A")
    check_tuples(ctx.fetch(T), Th, "T after the reduce")
    d = capi.device_vec(idx.data_ptr(), val.data_ptr(), cnt, n)
    got = ctx.fetch(ctx.multiply(capi.result_operand(T), a, scalei=d, sink=capi.SINK_COO, flags=capi.SINK_ORDERED))
    # the oracle's product with the vector computed on the host
    oi, oj, ov, _shape = orc.multiply(orc.Mat(Th[0], Th[1], Th[2], shape, 0), orc.Mat(i0, i1, v, shape, 0),
                                      scalei=orc.Vec(wi, wv, n), rowwise=True)
    check_tuples(got, (oi, oj, ov), "diag(1 / rowsum(T)) * T * A")
    assert len(got[2]) > 0


def test_cross_checks_on_the_device(ctx):
    import torch
    rng = np.random.default_rng(44)
    shape = (300, 200)
    nnz = 9000
    i0 = np.sort(rng.integers(0, shape[0], nnz)).astype(np.int32)
    A = (i0, rng.integers(0, shape[1], nnz).astype(np.int32), sr.special_values(rng, nnz, 0.05))
    keep = []
    a = _coo(A, shape, 0, True, keep)
    # SUM dense equals multiply_dense with ones into zeros
    ones = torch.ones(shape[1], dtype=torch.float64, device="cuda")
    Y = torch.zeros(shape[0], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.multiply_dense(a, ones, Y)
    _dense_same(ctx.reduce(a, rr.SUM, dense=True), Y.cpu().numpy(), "SUM against multiply_dense")
    # select(ROW_REL, theta) equals the tuples at or above mag(theta * reduce(MAX_ABS)[row])
    m = ctx.reduce(a, rr.MAX_ABS, dense=True)
    for theta in (0.0, 0.25, 1.0):
        with np.errstate(all="ignore"):
            thr = sr.mag(np.float64(theta) * m)
        k = sr.mag(A[2]) >= thr[A[0]]
        check_tuples(ctx.fetch(ctx.select(a, sr.ROW_REL, dparam=theta)), tuple(x[k] for x in A), "ROW_REL theta %r" % theta)


def _raw(ctx, A, op=1, post=0, pol=1, pi=None, pv=None, cap=0, mem=0, cnt=None, t=b'.'):
    return ctx.L.spsamd_reduce(ctx.h, None if A is None else C.byref(A), t, op, post, pol, 0, pi, pv, cap, mem,
                               None if cnt is None else C.byref(cnt), None)


def test_errors_leave_the_context_usable(ctx):
    import torch
    from spsparse_amd import capi
    rng = np.random.default_rng(45)
    A = sr.unique_key_operand(rng, (6, 8), 30, special=0.0)
    S = sr.operand_S(A)
    wi, wv, wd = rr.reduce_ref(S, 6, rr.SUM)
    keep = []
    a = _coo(A, (6, 8), -1, False, keep)
    idx, val = np.full(8, -3, np.int32), np.full(8, -7.5)
    cnt = C.c_size_t(99)
    pi, pv = idx.ctypes.data, val.ctypes.data
    # the size query: ECAPACITY, the count, nothing written
    assert _raw(ctx, a, pi=pi, pv=pv, cap=0, cnt=cnt) == -5 and cnt.value == len(wi)
    assert _raw(ctx, a, pi=pi, pv=pv, cap=len(wi) - 1, cnt=cnt) == -5 and cnt.value == len(wi)
    assert _raw(ctx, a, op=rr.DIAG, pi=pi, pv=pv, cap=0, cnt=cnt) == -5 and cnt.value == len(rr.reduce_ref(S, 6, rr.DIAG)[0])
    assert np.all(idx == -3) and np.all(val == -7.5)
    assert _raw(ctx, a, pi=None, pv=pv, cap=5, cnt=cnt) == -5            # dense: one entry per row
    assert np.all(val == -7.5)
    assert _raw(ctx, a, pi=pi, pv=pv, cap=8, cnt=cnt) == 0 and cnt.value == len(wi)
    _same((idx[:len(wi)], val[:len(wi)]), (wi, wv), "exact capacity")
    assert np.all(idx[len(wi):] == -3)
    # null pointers, unknown op / post / policy / mem
    assert _raw(ctx, None, pi=pi, pv=pv, cap=8, cnt=cnt) == -2
    assert _raw(ctx, a, pi=pi, pv=None, cap=8, cnt=cnt) == -2 and _raw(ctx, a, pi=pi, pv=pv, cap=8, cnt=None) == -2
    assert _raw(ctx, a, op=0, pi=pi, pv=pv, cap=8, cnt=cnt) == -2 and _raw(ctx, a, op=7, pi=pi, pv=pv, cap=8, cnt=cnt) == -2
    assert _raw(ctx, a, post=-1, pi=pi, pv=pv, cap=8, cnt=cnt) == -2 and _raw(ctx, a, post=4, pi=pi, pv=pv, cap=8, cnt=cnt) == -2
    assert _raw(ctx, a, pol=3, pi=pi, pv=pv, cap=8, cnt=cnt) == -2
    assert _raw(ctx, a, pi=pi, pv=pv, cap=8, mem=2, cnt=cnt) == -2
    # a false sort0, an index out of bounds, too many tuples
    assert np.any(np.diff(A[0]) < 0)
    for device in (False, True):
        assert _raw(ctx, _coo(A, (6, 8), 0, device, keep), pi=pi, pv=pv, cap=8, cnt=cnt) == -2
        bad = (A[0].copy(), A[1].copy(), A[2])
        bad[1][5] = 8
        assert _raw(ctx, _coo(bad, (6, 8), -1, device, keep), pi=pi, pv=pv, cap=8, cnt=cnt) == -2
    huge = capi.Coo(a.idx0, a.idx1, a.val, 2 ** 31, 6, 8, -1, capi.MEM_HOST)
    assert _raw(ctx, huge, pi=pi, pv=pv, cap=8, cnt=cnt) == -2
    # overlapping buffers: idx over val, an output over A's values
    both = np.zeros(16)
    assert _raw(ctx, a, pi=both.ctypes.data + 8, pv=both.ctypes.data, cap=8, cnt=cnt) == -2
    assert _raw(ctx, a, pi=pi, pv=a.val, cap=8, cnt=cnt) == -2
    assert _raw(ctx, a, pi=a.idx1, pv=pv, cap=8, cnt=cnt) == -2
    # a device output inside the context's output set
    r = ctx.multiply(a, _coo((A[1], A[0], A[2]), (8, 6), -1, False, keep))
    assert r.nnz >= 6
    assert _raw(ctx, a, pi=None, pv=r.val, cap=6, mem=1, cnt=cnt) == -2
    assert _raw(ctx, a, pi=r.idx0, pv=torch.zeros(8, dtype=torch.float64, device="cuda").data_ptr(), cap=6, mem=1, cnt=cnt) == -2
    # an empty operand, both forms
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    e = _coo(E, (6, 8), -1, False, keep)
    gi, gv = ctx.reduce(e, rr.SUM, transpose='T')
    assert len(gi) == 0 and len(gv) == 0
    d = ctx.reduce(e, rr.COUNT, rr.RECIP, transpose='T', dense=True)
    assert d.shape == (8,) and dr.same_bits(d, np.zeros(8))
    dv = torch.full((6,), -7.5, dtype=torch.float64, device="cuda")
    assert ctx.reduce(e, rr.SUM, dense=True, out=dv) == 0 and dr.same_bits(dv.cpu().numpy(), np.zeros(6))
    # and the context still works
    _same(ctx.reduce(a, rr.SUM), (wi, wv), "after the errors")
    _dense_same(ctx.reduce(a, rr.SUM, dense=True), wd, "after the errors, dense")
