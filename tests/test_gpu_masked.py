"""spsamd_multiply_masked on the device against tests/masked_ref.py (the oracle's product filtered by M's keys, pinned to
the inner-product loop by tests/test_masked_host.py).  Indices compare exactly, values as int64 bit patterns (NaNs as
NaNs where the oracle's own two loops may differ, masked_ref.same_tuples); NaN-free cases compare every bit."""
import ctypes
import math

import numpy as np
import pytest

from oracle import binding as orc
from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests import masked_ref as mr
from tests.gpu_util import check_tuples, coo as _coo, ctx, forced  # noqa: F401

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2, 3)
CS = (1.0, -0.75, np.inf)


def _vec(s, dim, keep):
    from spsparse_amd import capi
    if s is None:
        return None, None
    v, k = capi.host_vec(s[0], s[1], dim)
    keep.append(k)
    return v, orc.Vec(s[0], s[1], dim)


def _masked(ctx, *args, path=0, **kw):
    with forced(ctx, "masked_path", path):
        return ctx.multiply_masked(*args, **kw)


def _nan_aware(gv, wv):
    return (gv.view(np.int64) != wv.view(np.int64)) & ~(np.isnan(gv) & np.isnan(wv))


def _check(got, want, what, payloads=False):
    # its own: masked_ref.same_tuples (two NaNs agree unless payloads), and a mismatch mask that knows it
    check_tuples(got, want, what, lambda g, w: mr.same_tuples(g, w, payloads), _nan_aware)


def _operand(ctx, X, shape, form, t, role, pol, zn, keep, ops):
    """X as the call's operand in one of four forms; returns (Coo, the tuples the reference multiplies)."""
    from spsparse_amd import capi
    if form == "host":
        return _coo(X, shape, -1, False, keep), X
    if form == "device":
        return _coo(X, shape, -1, True, keep), X
    if form == "prepared":                   # stands for its consolidated tuples; the same policy and zero_nan
        op = capi.Operand(ctx, _coo(X, shape, -1, True, keep), t, role, pol, zn)
        ops.append(op)
        return op.coo, X
    # chained: a SINK_COO result of this context (spsamd_consolidate, row-major), NaN-free values
    r = ctx.consolidate(_coo(X, shape, -1, True, keep), 0, pol, zn)
    i, j, v = ctx.fetch(r)
    return capi.result_operand(r), (i, j, v)


def _mask_form(ctx, M, shape, form, keep, ops):
    """M in one of its forms; returns (Coo, keys the reference filters by)."""
    from spsparse_amd import capi
    ones = np.ones(len(M[0]))
    if form == "host":
        return _coo((M[0], M[1], np.zeros(len(M[0]))), shape, -1, False, keep), M           # explicit zeros
    if form == "host_sorted":
        o = np.lexsort((M[1], M[0]))
        return _coo((M[0][o], M[1][o], ones), shape, 0, False, keep, no_val=True), M      # sort0 = 0 with duplicates, val NULL
    if form == "device":
        return _coo((M[0], M[1], ones), shape, -1, True, keep), M
    if form in ("prepared", "prepared_T"):     # prepared for 'T': read as a device operand sorted the other way
        op = capi.Operand(ctx, _coo((M[0], M[1], ones), shape, -1, True, keep), 'T' if form == "prepared_T" else '.', capi.AS_A)
        ops.append(op)
        return op.coo, M
    r = ctx.consolidate(_coo((M[0], M[1], ones), shape, -1, True, keep), 0)            # chained, current output set
    return capi.result_operand(r), M


def test_argument_grid(ctx):
    """Random operands of tests/add_ref.py (NaN payloads, +-Inf, +-0, duplicates, junk leading entries) over both
    transposes, scales present or absent with missing and zero entries, C in {1, -0.75, Inf}, all policies, zero_nan,
    operands host / device / prepared / chained, and M host (explicit zeros), sorted with sort0 = 0 and duplicates, device,
    prepared, chained, with keys outside the product's pattern, or empty."""
    rng = np.random.default_rng(21)
    forms = ("host", "device", "prepared", "chained")
    mforms = ("host", "host_sorted", "device", "prepared", "prepared_T", "chained")
    for trial in range(240):
        nrow, ninner, ncol = (int(x) for x in rng.integers(1, 30, 3))
        tA, tB = ('.', 'T')[trial % 2], ('.', 'T')[(trial // 2) % 2]
        ash = (ninner, nrow) if tA == 'T' else (nrow, ninner)
        bsh = (ncol, ninner) if tB == 'T' else (ninner, ncol)
        fa, fb = forms[trial % 4], forms[(trial // 4) % 4]
        pol = trial % 3
        junk = bool(rng.integers(2))
        zn = junk or bool(trial % 5 == 0)
        special = 0.0 if "chained" in (fa, fb) else 0.3
        A = mr.sanitize_duplicates(ar.random_operand(rng, ash, int(rng.integers(0, 300)), special, lead_junk=junk and special > 0))
        B = mr.sanitize_duplicates(ar.random_operand(rng, bsh, int(rng.integers(0, 300)), special, lead_junk=junk and special > 0))
        keep, ops = [], []
        try:
            sc = [mr.random_scale(rng, d, rng.random() < 0.35) for d in (nrow, ninner, ncol)]
            dv = [_vec(s, d, keep) for s, d in zip(sc, (nrow, ninner, ncol))]
            C_ = CS[trial % 3] if trial % 7 else 1.0
            if fa == fb == "chained":                               # one chained result per call: a SINK_COO call overwrites
                fb = "device"                                       # the output set the previous one is not read from
            a, Aref = _operand(ctx, A, ash, fa, tA, capi_role("A"), pol, zn, keep, ops)
            b, Bref = _operand(ctx, B, bsh, fb, tB, capi_role("B"), pol, zn, keep, ops)
            nm = 0 if trial % 23 == 0 else int(rng.integers(1, 400))
            M = mr.random_mask(rng, (nrow, ncol), nm)
            mform = mforms[(trial // 3) % 6] if nm else "host"
            if mform == "chained" and "chained" in (fa, fb):
                mform = "device"
            m, Mkeys = _mask_form(ctx, M, (nrow, ncol), mform, keep, ops)
            # a chained operand is the consolidated tuples (NaN-free: consolidating them again changes nothing)
            Ao, Bo = orc.Mat(*Aref, ash), orc.Mat(*Bref, bsh)
            want = mr.masked_ref(Ao, Bo, Mkeys, C_, dv[0][1], tA, dv[1][1], tB, dv[2][1], pol, zn)
            res = ctx.multiply_masked(a, b, m, C_, dv[0][0], tA, dv[1][0], tB, dv[2][0], duplicate_policy=pol, zero_nan=zn)
            assert (res.shape0, res.shape1) == (nrow, ncol)
            _check(ctx.fetch(res), want, "trial %d %s%s A %s B %s M %s pol %d zn %d C %r" % (trial, tA, tB, fa, fb, mform, pol, zn, C_))
        finally:
            for op in ops:
                op.close()


def capi_role(side):
    from spsparse_amd import capi
    return capi.AS_A if side == "A" else capi.AS_B


def _skewed():
    """6000 x 6000: ~6 random tuples per row, two hub rows and two hub columns of 5000 tuples (above the row kernel's LDS
    cap of 4096), NaN-free."""
    rng = np.random.default_rng(8)
    n = 6000
    r = [rng.integers(0, n, 6 * n)]
    c = [rng.integers(0, n, 6 * n)]
    for h in (3, 17):
        r.append(np.full(5000, h)); c.append(rng.choice(n, 5000, replace=False))
    for h in (5, 11):
        c.append(np.full(5000, h)); r.append(rng.choice(n, 5000, replace=False))
    r, c = np.concatenate(r).astype(np.int32), np.concatenate(c).astype(np.int32)
    v = rng.standard_normal(r.size)
    mi = np.concatenate([rng.integers(0, n, 40000), np.repeat([3, 17, 5, 11], 3000), rng.integers(0, n, 12000)]).astype(np.int32)
    mj = np.concatenate([rng.integers(0, n, 40000), rng.integers(0, n, 12000), np.tile([5, 11, 3, 17], 3000)]).astype(np.int32)
    return (r, c, v), (n, n), (mi, mj)


@pytest.mark.parametrize("path", PATHS)
def test_every_path_skewed(ctx, path):
    X, shape, M = _skewed()
    keep = []
    a = _coo(X, shape, -1, True, keep)
    m = _coo((M[0], M[1], np.ones(M[0].size)), shape, -1, True, keep)
    A = orc.Mat(*X, shape)
    for tB in ('.', 'T'):
        want = mr.masked_ref(A, A, M, tB=tB, nthreads=orc.host_threads(16))
        res = _masked(ctx, a, a, m, tB=tB, path=path)
        _check(ctx.fetch(res), want, "skewed path %d tB %s" % (path, tB), payloads=True)
        assert res.products > 0 and res.nnz_a == res.nnz_b == len(set(zip(X[0].tolist(), X[1].tolist())))


@pytest.mark.parametrize("path", PATHS)
def test_every_path_rmat14(ctx, path):
    """R-MAT scale 14, A * A on A's own pattern (the graph case), and with a scalej that skips part of k."""
    i0, i1, v, shape = wl.rmat(14, seed=3)
    keep = []
    a = _coo((i0, i1, v), shape, -1, True, keep)
    A = orc.Mat(i0, i1, v, shape)
    want = mr.masked_ref(A, A, (i0, i1), nthreads=orc.host_threads(16))
    res = _masked(ctx, a, a, a, path=path)
    _check(ctx.fetch(res), want, "rmat14 path %d" % path, payloads=True)
    rng = np.random.default_rng(4)
    sj = mr.random_scale(rng, shape[0])
    sv, so = _vec(sj, shape[0], keep)
    want = mr.masked_ref(A, A, (i0, i1), scalej=so, zero_nan=True, nthreads=orc.host_threads(16))
    res = _masked(ctx, a, a, a, scalej=sv, path=path, zero_nan=True)
    _check(ctx.fetch(res), want, "rmat14 scalej path %d" % path, payloads=True)

def test_mask_is_the_whole_product(ctx):
    """M = the product's own pattern (the multiply's result, chained as it is in the current output set): the masked
    product equals spsamd_multiply(..., SINK_COO, SINK_ORDERED) tuple for tuple."""
    from spsparse_amd import capi
    rng = np.random.default_rng(5)
    keep = []
    for tA, tB in (('.', '.'), ('T', '.'), ('.', 'T')):
        A = ar.random_operand(rng, (300, 200), 6000, special=0.0)
        B = ar.random_operand(rng, (200, 300) if tA == tB else (300, 200), 6000, special=0.0)
        ash = (300, 200)
        bsh = (200, 300) if tA == tB else (300, 200)
        a, b = _coo(A, ash, -1, True, keep), _coo(B, bsh, -1, True, keep)
        r = ctx.multiply(a, b, tA=tA, tB=tB, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
        full = ctx.fetch(r)
        res = ctx.multiply_masked(a, b, capi.result_operand(r), tA=tA, tB=tB)
        _check(ctx.fetch(res), full, "whole pattern %s%s" % (tA, tB), payloads=True)


def _lower(pairs, n):
    u, v = pairs
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    k = np.unique(hi.astype(np.int64) * n + lo)
    k = k[(k // n) != (k % n)]
    return (k // n).astype(np.int32), (k % n).astype(np.int32)


def _triangles(ctx, L, n, path=0):
    from spsparse_amd import capi
    keep = []
    l = _coo((L[0], L[1], np.ones(L[0].size)), (n, n), 0, True, keep)
    d = _masked(ctx, l, l, l, path=path, sink=capi.SINK_DIGEST)
    return d


def test_closed_form_complete_graph(ctx):
    n = 2048
    iu = np.tril_indices(n, -1)
    L = (iu[0].astype(np.int32), iu[1].astype(np.int32))
    d = _triangles(ctx, L, n)
    assert d.sum == math.comb(n, 3)
    assert d.nnz == (n - 1) * (n - 2) // 2          # every key (i, j) with a k strictly between
    assert d.products == math.comb(n, 3)


def test_closed_form_grids(ctx):
    N = 512
    idx = np.arange(N * N).reshape(N, N)
    right = (idx[:, :-1].ravel(), idx[:, 1:].ravel())
    down = (idx[:-1, :].ravel(), idx[1:, :].ravel())
    diag = (idx[:-1, :-1].ravel(), idx[1:, 1:].ravel())
    n = N * N
    tri = _lower((np.concatenate([right[0], down[0], diag[0]]), np.concatenate([right[1], down[1], diag[1]])), n)
    for path in PATHS:
        d = _triangles(ctx, tri, n, path)
        # two triangles per grid square, both found at the key of its diagonal edge
        assert d.sum == 2 * (N - 1) ** 2 and d.nnz == (N - 1) ** 2, path
    plain = _lower((np.concatenate([right[0], down[0]]), np.concatenate([right[1], down[1]])), n)
    d = _triangles(ctx, plain, n)
    assert d.sum == 0 and d.nnz == 0


def test_sinks(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(13)
    shape = (500, 400)
    A = ar.random_operand(rng, (500, 300), 20000, special=0.0)
    B = ar.random_operand(rng, (300, 400), 20000, special=0.0)
    M = mr.random_mask(rng, shape, 60000)
    keep = []
    a, b = _coo(A, (500, 300), -1, True, keep), _coo(B, (300, 400), -1, True, keep)
    m = _coo((M[0], M[1], np.ones(M[0].size)), shape, -1, True, keep)
    want = mr.masked_ref(orc.Mat(*A, (500, 300)), orc.Mat(*B, (300, 400)), M, C_=-0.5)
    wi, wj, wv = want
    d = ctx.multiply_masked(a, b, m, -0.5, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
    cnt, s, h = orc.digest(wi, wj, wv)
    assert d.nnz == cnt and d.hash == h
    assert abs(d.sum - s) <= 1e-9 * np.sum(np.abs(wv))
    rn = ctx.to_host(d.row_nnz, shape[0], np.int64)
    rh = ctx.to_host(d.row_hash, shape[0], np.uint64)
    assert np.array_equal(rn, np.bincount(wi, minlength=shape[0]))
    want_h = np.zeros(shape[0], np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(want_h, wi, orc.mix64(wi, wj))
    assert np.array_equal(rh, want_h)
    for flags in (capi.SINK_ORDERED, capi.SINK_EXACT_PATTERN):      # accepted, change nothing
        _check(ctx.fetch(ctx.multiply_masked(a, b, m, -0.5, flags=flags)), want, "flags %d" % flags, payloads=True)
    # PERMUTE: swapped tuples, chained back as the column-major operand it is
    p = ctx.multiply_masked(a, b, m, -0.5, flags=capi.SINK_PERMUTE)
    assert (p.shape0, p.shape1) == (400, 500)
    gi, gj, gv = ctx.fetch(p)
    _check((gj, gi, gv), want, "permute", payloads=True)
    P = capi.Coo(p.idx0, p.idx1, p.val, int(p.nnz), 400, 500, 1, capi.MEM_DEVICE)
    E = ar.random_operand(rng, (400, 50), 3000, special=0.0)
    r2 = ctx.multiply(P, _coo(E, (400, 50), -1, False, keep), tA='T', sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
    qi, qj, qv, _ = orc.multiply(orc.Mat(wj, wi, wv, (400, 500)), orc.Mat(*E, (400, 50)), tA='T')
    _check(ctx.fetch(r2), ar.sort_storage((qi, qj, qv), 0), "permuted result into multiply", payloads=True)
    # COO: chained into the next multiply
    r = ctx.multiply_masked(a, b, m, -0.5)
    _check(ctx.fetch(r), want, "coo", payloads=True)
    F = ar.random_operand(rng, (400, 70), 3000, special=0.0)
    r3 = ctx.multiply(capi.result_operand(r), _coo(F, (400, 70), -1, False, keep), sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
    qi, qj, qv, _ = orc.multiply(orc.Mat(wi, wj, wv, shape, 0), orc.Mat(*F, (400, 70)))
    _check(ctx.fetch(r3), ar.sort_storage((qi, qj, qv), 0), "masked result into multiply", payloads=True)


def test_errors(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(4)
    A = ar.random_operand(rng, (6, 8), 100, special=0.0)
    B = ar.random_operand(rng, (8, 5), 100, special=0.0)
    M = mr.random_mask(rng, (6, 5), 20)
    keep = []
    a, b = _coo(A, (6, 8), -1, False, keep), _coo(B, (8, 5), -1, True, keep)
    good = _coo((M[0], M[1], np.ones(M[0].size)), (6, 5), -1, False, keep)
    want = mr.masked_ref(orc.Mat(*A, (6, 8)), orc.Mat(*B, (8, 5)), M)

    def still_usable():
        _check(ctx.fetch(ctx.multiply_masked(a, b, good)), want, "after an error", payloads=True)

    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_masked(a, b, _coo((M[0], M[1], np.ones(M[0].size)), (5, 6), -1, False, keep))
    assert e.value.code == -1 and "5 x 6" in e.value.msg and "6 x 5" in e.value.msg
    still_usable()
    bad = (M[0].copy(), M[1].copy())
    bad[1][3] = 5
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_masked(a, b, _coo((bad[0], bad[1], np.ones(bad[0].size)), (6, 5), -1, True, keep))
    assert e.value.code == -2
    still_usable()
    o = np.lexsort((M[1], M[0]))[::-1]                              # descending, claimed ascending
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_masked(a, b, _coo((M[0][o], M[1][o], np.ones(M[0].size)), (6, 5), 0, False, keep))
    assert e.value.code == -2
    still_usable()
    # the same keys without the claim are sorted by the call
    _check(ctx.fetch(ctx.multiply_masked(a, b, _coo((M[0][o], M[1][o], np.ones(M[0].size)), (6, 5), -1, False, keep))), want, "unsorted", True)
    rc = ctx.L.spsamd_multiply_masked(ctx.h, 1.0, None, ctypes.byref(a), b'.', None, ctypes.byref(b), b'.', None, None,
                                      1, 0, capi.SINK_COO, 0, ctypes.byref(capi.Result()))
    assert rc == -2 and "mask" in ctx.L.spsamd_last_error(ctx.h).decode()
    still_usable()
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_masked(a, b, good, duplicate_policy=3)
    assert e.value.code == -2
    still_usable()
    # both output sets as operands: a masked result, then one masked by it (written to the other set), then both at once
    r1 = ctx.multiply_masked(a, b, good)
    P1 = capi.result_operand(r1)
    r2 = ctx.multiply_masked(a, b, P1)
    _check(ctx.fetch(r2), want, "masked by its own result", payloads=True)
    P2 = capi.result_operand(r2)
    eye = _coo((np.arange(5), np.arange(5), np.ones(5)), (5, 5), -1, False, keep)
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_masked(P1, eye, P2)
    assert e.value.code == -2 and "both result buffers" in e.value.msg
    still_usable()
    # empty M, C == 0: empty results of the product's shape
    E = _coo((np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)), (6, 5), -1, False, keep)
    r = ctx.multiply_masked(a, b, E)
    assert r.nnz == 0 and (r.shape0, r.shape1) == (6, 5)
    r = ctx.multiply_masked(a, b, good, 0.0)
    assert r.nnz == 0 and (r.shape0, r.shape1) == (6, 5)
