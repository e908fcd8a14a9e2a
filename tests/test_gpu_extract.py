"""spsamd_extract on the device against tests/extract_ref.py (pinned on the host by tests/test_extract_host.py): indices equal
and values as int64 bit patterns, zero tolerance -- the call computes no value, so there is nothing to tolerate.  Every
setting of the extract_path knob runs, so that every row meets every ordering kernel that can hold it."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as orc
from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests.gpu_util import check_tuples as _check, coo as _coo, ctx, forced  # noqa: F401
from tests import extract_ref as er
from tests import select_ref as sr

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2, 3, 4)


def _lst(L, device):
    """An index list as Context.extract takes it: numpy int32 (host) or a torch CUDA int32 tensor (device)."""
    if L is None:
        return None
    a = np.ascontiguousarray(L, dtype=np.int32)
    if not device:
        return a
    import torch
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t


def _extract(ctx, A, I, J, path=0, device_lists=False, **kw):
    with forced(ctx, "extract_path", path):
        return ctx.extract(A, _lst(I, device_lists), _lst(J, device_lists), **kw)


def test_semantic_cases(ctx):
    """Both transposes, the three policies, zero_nan, host and device operands and lists, raw (unique keys with NaN / Inf /
    +-0; duplicate keys) and trusted (sorted by the leading index only: duplicate keys and columns out of order inside a row,
    special values anywhere) operands, the six list shapes on either side, every extract_path."""
    rng = np.random.default_rng(41)
    kinds = er.LIST_KINDS
    for trial in range(288):
        shape = (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
        nnz = int(rng.integers(0, 3000 if trial % 7 == 0 else 250))
        t = '.' if trial % 4 < 2 else 'T'
        lead = 1 if t == 'T' else 0
        nrow, ncol = (shape[1], shape[0]) if lead else shape
        pol, zn = trial % 3, bool(trial % 5 == 0)
        kind = (trial // 2) % 3
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
        a = _coo(A, shape, sort0, device=trial % 2 == 1, keep=keep)
        for sub in range(3):
            ki, kj = kinds[(trial + sub) % 6], kinds[(trial // 6 + 2 * sub) % 6]
            I, J = er.index_list(rng, ki, nrow), er.index_list(rng, kj, ncol)
            path = (trial + sub) % 5
            res = _extract(ctx, a, I, J, path, device_lists=(trial // 3 + sub) % 2 == 1, transpose=t, duplicate_policy=pol, zero_nan=zn)
            what = "trial %d I %s J %s path %d %s pol %d zn %d kind %d" % (trial, ki, kj, path, t, pol, zn, kind)
            nR, nC = (nrow if I is None else len(I)), (ncol if J is None else len(J))
            assert (res.shape0, res.shape1) == (nR, nC), what
            assert res.nnz_a == len(S[2]), what
            want = er.extract_ref(S, I, J, nrow, ncol)
            assert res.nnz == len(want[2]), what
            _check(ctx.fetch(res), want, what)


_ROWS = {}
LENGTHS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 200_000, 0, 3]


def _row_classes():
    if not _ROWS:
        rng = np.random.default_rng(42)
        ncol = 1 << 18
        _ROWS["X"] = sr.rows_of_lengths(rng, LENGTHS, ncol)
        _ROWS["shape"] = (len(LENGTHS), ncol)
    return _ROWS["X"], _ROWS["shape"]


def _served(n, path):
    """(rows_light, rows_mid, rows_heavy, tuples_light, tuples_mid, tuples_heavy) the forced class must have served: every
    output row of two or more tuples, in the forced class if it can hold the row, else in the next one."""
    from spsparse_amd import capi
    n = np.asarray(n)
    lm, mm = capi.extract_light_max, capi.extract_mid_max
    light = (n >= 2) & (n <= lm) if path <= 2 else np.zeros(n.shape, bool)
    mid = (n >= 2) & (n <= mm) & ~light if path <= 3 else np.zeros(n.shape, bool)
    heavy = (n >= 2) & ~light & ~mid
    return tuple(int(m.sum()) for m in (light, mid, heavy)) + tuple(int(n[m].sum()) for m in (light, mid, heavy))


@pytest.mark.parametrize("path", (2, 3, 4))
@pytest.mark.parametrize("twice", (False, True))
def test_row_lengths_on_every_kernel(ctx, path, twice):
    """Rows of 0, 1, 63, 64, 65, 4095, 4096, 4097 and 200 000 tuples; J a random permutation of all columns, or every column
    twice in random order (the CSR map: every row doubles); each ordering class forced in turn."""
    X, shape = _row_classes()
    rng = np.random.default_rng(43 + path)
    J = rng.permutation(shape[1]).astype(np.int32)
    if twice:
        J = rng.permutation(np.repeat(np.arange(shape[1], dtype=np.int32), 2))
    keep = []
    a = _coo(X, shape, 0, True, keep)
    for I in (None, np.array([8, 3, 8, 0, 5, 7, 10, 2, 6, 4, 1], np.int32)):
        res = _extract(ctx, a, I, J, path, device_lists=True)
        want = er.extract_ref(X, I, J, shape[0], shape[1])
        _check(ctx.fetch(res), want, "path %d twice %d I %s" % (path, twice, "all" if I is None else "list"))
        n_r = np.bincount(want[0], minlength=res.shape0)
        got = (res.rows_light, res.rows_mid, res.rows_heavy, res.tuples_light, res.tuples_mid, res.tuples_heavy)
        assert got == _served(n_r, path), (path, twice)
        if path == 2 and not twice:                                  # the input has rows for every class
            assert res.rows_light > 0 and res.rows_mid > 0 and res.rows_heavy > 0


def test_in_order_path(ctx):
    """J ALL or strictly ascending over a column-ordered S: nothing is ordered (the counters stay 0), and the tuples are those
    of the permuted path."""
    X, shape = _row_classes()
    rng = np.random.default_rng(44)
    keep = []
    a = _coo(X, shape, 0, True, keep)
    Jasc = np.flatnonzero(rng.random(shape[1]) < 0.5).astype(np.int32)
    for I in (None, np.array([8, 8, 2, 7, 4], np.int32)):
        for J in (None, Jasc):
            r0 = _extract(ctx, a, I, J, 0)
            assert r0.rows_light + r0.rows_mid + r0.rows_heavy == 0 and r0.tuples_light + r0.tuples_mid + r0.tuples_heavy == 0
            g0 = ctx.fetch(r0)
            r1 = _extract(ctx, a, I, J, 1)
            assert r1.rows_light + r1.rows_mid + r1.rows_heavy > 0
            _check(ctx.fetch(r1), g0, "path 1 against path 0")
            _check(g0, er.extract_ref(X, I, J, shape[0], shape[1]), "in order")
    # a trusted operand whose columns descend inside a row is not in order: it is sorted even under path 0
    U = (np.array([0, 0, 0, 1], np.int32), np.array([5, 2, 9, 1], np.int32), np.array([1.0, 2.0, 3.0, 4.0]))
    r = _extract(ctx, _coo(U, (2, 10), 0, False, keep), None, None, 0)
    assert r.rows_light == 1 and r.tuples_light == 3
    _check(ctx.fetch(r), er.extract_ref(U, None, None, 2, 10), "unordered trusted rows")


def _selection(ctx, L, dim, keep):
    m = er.selection_matrix(L, dim)
    return _coo(m[:3], m[3], 0, True, keep)


@pytest.mark.parametrize("name", ("rmat14", "poisson256"))
def test_equals_the_selection_products_on_the_device(ctx, name):
    """extract(A, I, J) == multiply(multiply(S_I, A), S_J, tB='T') bit for bit: the composition the call replaces."""
    from spsparse_amd import capi
    i0, i1, v, shape = wl.rmat(14, seed=5) if name == "rmat14" else wl.poisson2d(256)
    assert np.all(np.isfinite(v)) and np.all(v != 0)
    rng = np.random.default_rng(45)
    n = shape[0]
    keep = []
    a = _coo((i0, i1, v), shape, -1, True, keep)
    cases = [(rng.permutation(n)[: n // 2].astype(np.int32), rng.integers(0, n, n // 3).astype(np.int32)),
             (np.arange(n // 4, n // 2, dtype=np.int32), None),
             (np.sort(rng.permutation(n)[: n // 2]).astype(np.int32),) * 2]
    for k, (I, J) in enumerate(cases):
        got = ctx.fetch(_extract(ctx, a, I, J, 0, device_lists=True))
        T = ctx.multiply(_selection(ctx, I, n, keep), a, flags=capi.SINK_ORDERED)
        G = ctx.multiply(capi.result_operand(T), _selection(ctx, J, n, keep), tB='T', flags=capi.SINK_ORDERED)
        assert (G.shape0, G.shape1) == (len(I), n if J is None else len(J))
        _check(got, ctx.fetch(G), "%s case %d" % (name, k))
        assert len(got[2]) > 0


def test_permutation_round_trip(ctx):
    from spsparse_amd import capi
    i0, i1, v, shape = wl.rmat(16, seed=6)
    n = shape[0]
    rng = np.random.default_rng(46)
    p = rng.permutation(n).astype(np.int32)
    q = np.empty(n, np.int32)
    q[p] = np.arange(n, dtype=np.int32)
    keep = []
    a = _coo((i0, i1, v), shape, -1, True, keep)
    want = ctx.fetch(ctx.consolidate(a, 0))
    for path in (0, 3):
        P = _extract(ctx, a, p, p, path, device_lists=True)
        assert P.nnz == len(want[2])
        B = _extract(ctx, capi.result_operand(P), q, q, path, device_lists=True)
        _check(ctx.fetch(B), want, "round trip, path %d" % path)


def test_chained_product_as_operand(ctx):
    from spsparse_amd import capi
    i0, i1, v, shape = wl.rmat(12, seed=7)
    n = shape[0]
    rng = np.random.default_rng(47)
    keep = []
    a = _coo((i0, i1, v), shape, -1, True, keep)
    I = np.sort(rng.permutation(n)[: n // 2]).astype(np.int32)
    J = rng.permutation(n)[: n // 2].astype(np.int32)
    T = ctx.multiply(a, a, flags=capi.SINK_ORDERED)
    Th = ctx.fetch(T)
    for path in PATHS:
        r = _extract(ctx, capi.result_operand(T), I, J, path)
        assert r.nnz_a == T.nnz
        _check(ctx.fetch(r), er.extract_ref(Th, I, J, n, n), "extract of a chained product, path %d" % path)
        _check(ctx.fetch(T), Th, "the product stays fetchable")     # the result went to the other set
        r2 = _extract(ctx, _coo(Th, shape, 0, False, keep), I, J, path)
        _check(ctx.fetch(r2), er.extract_ref(Th, I, J, n, n), "extract of the fetched product")


def test_chain_extract_select_masked(ctx):
    """An induced subgraph, its strict lower triangle, then (L*L) o L: every step reads the previous result in place."""
    from spsparse_amd import capi
    i0, i1, _v, shape = wl.rmat(12, seed=3)
    n = shape[0]
    key = np.unique(np.concatenate([i0.astype(np.int64) * n + i1, i1.astype(np.int64) * n + i0]))
    si, sj = (key // n).astype(np.int32), (key % n).astype(np.int32)
    rng = np.random.default_rng(48)
    V = np.sort(rng.permutation(n)[: n // 2]).astype(np.int32)
    keep = []
    a = _coo((si, sj, np.ones(len(key))), shape, 0, True, keep)
    G = _extract(ctx, a, V, V, 0, device_lists=True)
    L = ctx.select(capi.result_operand(G), sr.TRIL, iparam=-1)
    Lop = capi.result_operand(L)
    tri = ctx.multiply_masked(Lop, Lop, Lop, flags=capi.SINK_ORDERED)
    got = ctx.fetch(tri)[2].sum()
    D = np.zeros((n, n), np.float32)
    D[si, sj] = 1.0
    Ld = np.tril(D[np.ix_(V, V)], -1)
    want = float(((Ld @ Ld) * Ld).sum(dtype=np.float64))
    assert want > 0 and got == want


def test_prepared_operand_both_transposes(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(49)
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
                nrow, ncol = (shape[1], shape[0]) if t == 'T' else shape
                for ki, kj in (("permutation", "repeats"), ("ascending", "all"), ("repeats", "ascending")):
                    I, J = er.index_list(rng, ki, nrow), er.index_list(rng, kj, ncol)
                    res = ctx.extract(op.coo, I, J, transpose=t)
                    _check(ctx.fetch(res), er.extract_ref(S, I, J, nrow, ncol), "prepared %s used %s" % (tprep, t))
        finally:
            op.close()


def test_sinks(ctx):
    import torch
    from spsparse_amd import capi
    rng = np.random.default_rng(50)
    shape = (500, 400)
    A = ar.random_operand(rng, shape, 60_000, special=0.0)
    keep = []
    a = _coo(A, shape, -1, True, keep)
    S = sr.operand_S(A)
    I = rng.integers(0, shape[0], 300).astype(np.int32)
    for J in (rng.permutation(shape[1])[:250].astype(np.int32), None, rng.integers(0, shape[1], 700).astype(np.int32)):
        wi, wj, wv = er.extract_ref(S, I, J, shape[0], shape[1])
        d = ctx.extract(a, I, J, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
        cnt, _sum, h = orc.digest(wi, wj, wv)
        assert d.nnz == cnt == len(wv) and d.nnz_a == len(S[2]) and d.hash == h
        assert abs(d.sum - wv.sum()) <= 1e-9 * np.abs(wv).sum()
        assert np.array_equal(ctx.to_host(d.row_nnz, len(I), np.int64), np.bincount(wi, minlength=len(I)))
        for flags in (0, capi.SINK_ORDERED, capi.SINK_EXACT_PATTERN):      # accepted, change nothing
            _check(ctx.fetch(ctx.extract(a, I, J, flags=flags)), (wi, wj, wv), "flags %d" % flags)
        # PERMUTE: the index arrays and the shape swap; chained back as the column-major operand it is
        nC = shape[1] if J is None else len(J)
        p = ctx.extract(a, I, J, flags=capi.SINK_PERMUTE)
        assert (p.shape0, p.shape1) == (nC, len(I))
        gi, gj, gv = ctx.fetch(p)
        _check((gj, gi, gv), (wi, wj, wv), "permute")
        Pop = capi.Coo(p.idx0, p.idx1, p.val, int(p.nnz), nC, len(I), 1, capi.MEM_DEVICE)
        back = ctx.extract(Pop, None, None, transpose='T')
        _check(ctx.fetch(back), (wi, wj, wv), "permuted result chained with sort0 = 1")
    # scatter_dense of a result
    res = ctx.extract(a, I, None)
    dense = torch.zeros((len(I), shape[1]), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.scatter_dense(res, dense.data_ptr(), shape[1])
    D = np.zeros(shape)
    D[S[0], S[1]] = S[2]
    assert np.array_equal(dense.cpu().numpy(), D[I, :])


def _raw(ctx, A, res, rows=None, nrows=0, cols=None, ncols=0, mem=0, t=b'.', pol=1, zn=0, sink=1, flags=0):
    return ctx.L.spsamd_extract(ctx.h, None if A is None else C.byref(A), t, rows, nrows, cols, ncols, mem, pol, zn, sink, flags,
                                None if res is None else C.byref(res))


def _msg(ctx):
    return ctx.L.spsamd_last_error(ctx.h).decode()


def test_errors_leave_the_context_usable(ctx):
    import torch
    from spsparse_amd import capi
    rng = np.random.default_rng(51)
    A = sr.unique_key_operand(rng, (6, 8), 30)
    S = sr.operand_S(A)
    keep = []
    a = _coo(A, (6, 8), -1, False, keep)
    prev = ctx.extract(a, np.array([5, 0, 5], np.int32), None)
    prev_want = er.extract_ref(S, [5, 0, 5], None, 6, 8)
    res = capi.Result()
    ok = np.array([1, 2], np.int32)
    assert _raw(ctx, None, res) == -2 and _raw(ctx, a, None) == -2
    assert _raw(ctx, a, res, sink=3) == -2 and _raw(ctx, a, res, sink=0) == -2
    assert _raw(ctx, a, res, pol=3) == -2 and _raw(ctx, a, res, pol=-1) == -2
    assert _raw(ctx, a, res, rows=ok.ctypes.data, nrows=2, mem=5) == -2
    assert _raw(ctx, a, res, rows=ok.ctypes.data, nrows=2, mem=capi.MEM_DEVICE) == -2          # a host pointer named a device list
    dev_ok = torch.from_numpy(ok).cuda()
    torch.cuda.synchronize()
    assert _raw(ctx, a, res, cols=dev_ok.data_ptr(), ncols=2, mem=capi.MEM_HOST) == -2          # and the reverse
    assert _raw(ctx, a, res, rows=ok.ctypes.data, nrows=2 ** 31) == -2 and _raw(ctx, a, res, cols=ok.ctypes.data, ncols=2 ** 31) == -2
    # an entry out of range, in I and in J, host and device lists: the message names the first such position
    for device in (False, True):
        for bad in (6, -1):
            with pytest.raises(capi.SpsamdError) as e:
                ctx.extract(a, _lst([0, 3, bad, 1, 9], device), None)
            assert e.value.code == -2 and "rows[2]" in e.value.msg
        for bad in (8, -5):
            with pytest.raises(capi.SpsamdError) as e:
                ctx.extract(a, None, _lst([7, bad, 0, 99], device))
            assert e.value.code == -2 and "cols[1]" in e.value.msg
        with pytest.raises(capi.SpsamdError) as e:                   # under 'T' the bounds swap
            ctx.extract(a, _lst([7], device), _lst([6], device), transpose='T')
        assert "cols[0]" in e.value.msg
    # an index of A out of bounds, a lying sort0
    for device in (False, True):
        badA = (A[0].copy(), A[1].copy(), A[2])
        badA[1][5] = 8
        assert _raw(ctx, _coo(badA, (6, 8), -1, device, keep), res) == -2
        assert np.any(np.diff(A[0]) < 0)
        assert _raw(ctx, _coo(A, (6, 8), 0, device, keep), res) == -2
    huge = capi.Coo(a.idx0, a.idx1, a.val, 2 ** 31, 6, 8, -1, capi.MEM_HOST)
    assert _raw(ctx, huge, res) == -2
    # a device list that lies in the output set about to be written
    assert _raw(ctx, a, res, cols=prev.idx1, ncols=int(prev.nnz), mem=capi.MEM_DEVICE) == -2 and "output set" in _msg(ctx)
    # 2^31 tuples or more, refused before the output is grown: one row of 2^16 tuples on one key named 2^15 times as a
    # column; the same row named 2^15 times with all columns; and a count that does not fit 32 bits
    L = 1 << 16
    one_key = (np.zeros(L, np.int32), np.zeros(L, np.int32), np.ones(L))
    long_row = (np.zeros(L, np.int32), np.arange(L, dtype=np.int32), np.ones(L))
    for X, I, J in ((one_key, None, np.zeros(1 << 15, np.int32)), (long_row, np.zeros(1 << 15, np.int32), None),
                    (one_key, None, np.zeros(1 << 17, np.int32))):
        with pytest.raises(capi.SpsamdError) as e:
            ctx.extract(_coo(X, (1, L), 0, True, keep), I, J)
        assert e.value.code == -2 and "2^31" in e.value.msg
        if len(J if J is not None else I) == 1 << 15:
            assert str(2 ** 31) in e.value.msg
    # one short of it is no error for the count (one tuple fewer in the row): not run, it would need 32 GiB of output
    # the previous result is intact
    _check(ctx.fetch(prev), prev_want, "previous result after the errors")
    # the empty cases: empty results of the right shape
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    e0 = np.zeros(0, np.int32)
    r = ctx.extract(_coo(E, (6, 8), -1, False, keep), np.array([1, 1, 1], np.int32), None, transpose='T')
    assert r.nnz == 0 and (r.shape0, r.shape1) == (3, 6)
    for device in (False, True):
        r = ctx.extract(a, _lst(e0, device), None)
        assert r.nnz == 0 and (r.shape0, r.shape1) == (0, 8)
        r = ctx.extract(a, _lst([1, 2], device), _lst(e0, device))
        assert r.nnz == 0 and (r.shape0, r.shape1) == (2, 0)
    r = ctx.extract(a, np.array([3], np.int32), np.array([0], np.int32)) if not np.any((S[0] == 3) & (S[1] == 0)) else None
    assert r is None or (r.nnz == 0 and (r.shape0, r.shape1) == (1, 1))
    # and the context still works
    r = ctx.extract(a, np.array([2, 1], np.int32), np.array([7, 0, 7], np.int32))
    _check(ctx.fetch(r), er.extract_ref(S, [2, 1], [7, 0, 7], 6, 8), "after the errors")
