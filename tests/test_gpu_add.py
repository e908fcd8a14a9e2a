"""spsamd_add on the device, bit for bit against the test oracle's consolidate() of the concatenated, pre-scaled tuples
(the restatement in tests/add_ref.py is pinned to it by tests/test_add_host.py).  Values compare as int64 bit patterns,
for both settings of the add_path knob (0: operands already in order are read in place, 1: every operand is sorted)."""
import numpy as np
import pytest

from oracle import binding as orc
from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests.gpu_util import check_tuples as _check, coo as _coo, ctx, forced  # noqa: F401

pytestmark = pytest.mark.gpu

PATHS = (0, 1)
SCALES = (1.0, -0.75, 0.0, np.inf)


def _add(ctx, A, B, path=0, **kw):
    with forced(ctx, "add_path", path):
        return ctx.add(A, B, **kw)


def _want(A, B, alpha=1.0, beta=1.0, tA='.', tB='.', pol=ar.ADD, zn=False):
    r, c, v = ar.scaled_cat(A, B, alpha, beta, tA, tB)
    i, j, w = orc.consolidate(r, c, v, 0, pol, zn)
    return i, j, w


def _case(rng, big=False):
    shape = (int(rng.integers(1, 40)), int(rng.integers(1, 40)))
    tA, tB = str(rng.choice(['.', 'T'])), str(rng.choice(['.', 'T']))
    bshape = shape[::-1] if (tA == 'T') != (tB == 'T') else shape
    junk = bool(rng.integers(2))
    hi = 3000 if big else 200
    A = ar.random_operand(rng, shape, int(rng.integers(0, hi)), lead_junk=junk)
    B = ar.random_operand(rng, bshape, int(rng.integers(0, hi)), lead_junk=junk)
    return A, B, shape, bshape, tA, tB, junk


@pytest.mark.parametrize("path", PATHS)
def test_semantic_cases(ctx, path):
    """Duplicates within and across operands, +-0, NaN payloads, +-Inf, both transposes, every policy, zero_nan with the
    leading run over both operands, host and device operands, sort0 absent or trusted, every pair of scales."""
    rng = np.random.default_rng(11 + path)
    for trial in range(160):
        A, B, shape, bshape, tA, tB, junk = _case(rng, big=trial % 4 == 0)
        alpha, beta = SCALES[trial % 4], SCALES[(trial // 4) % 4]
        pol, zn = trial % 3, junk or bool(trial % 5 == 0)
        sa = sb = -1
        if trial % 3 == 1:                              # stored in op()'s row order and saying so
            la, lb = (1 if tA == 'T' else 0), (1 if tB == 'T' else 0)
            A, B, sa, sb = ar.sort_storage(A, la), ar.sort_storage(B, lb), la, lb
        keep = []
        a = _coo(A, shape, sa, device=trial % 2 == 0, keep=keep)
        b = _coo(B, bshape, sb, device=trial % 4 < 2, keep=keep)
        res = _add(ctx, a, b, path, alpha=alpha, beta=beta, tA=tA, tB=tB, duplicate_policy=pol, zero_nan=zn)
        want = _want(A, B, alpha, beta, tA, tB, pol, zn)
        assert (res.shape0, res.shape1) == ((shape[1], shape[0]) if tA == 'T' else shape)
        assert res.nnz_a == len(A[2]) and res.nnz_b == len(B[2])
        _check(ctx.fetch(res), want,
               "trial %d path %d %s%s pol %d zn %d" % (trial, path, tA, tB, pol, zn))


@pytest.mark.parametrize("path", PATHS)
def test_sort0_trusted_lying_absent(ctx, path):
    from spsparse_amd import capi
    rng = np.random.default_rng(5)
    A = ar.random_operand(rng, (30, 20), 500, special=0.1)
    B = ar.random_operand(rng, (30, 20), 500, special=0.1)
    As = ar.sort_storage(A, 0)
    for device in (False, True):
        keep = []
        got = ctx.fetch(_add(ctx, _coo(As, (30, 20), 0, device, keep), _coo(B, (30, 20), -1, device, keep), path))
        _check(got, _want(As, B), "trusted")
        got = ctx.fetch(_add(ctx, _coo(As, (30, 20), -1, device, keep), _coo(B, (30, 20), -1, device, keep), path))
        _check(got, _want(As, B), "absent")
        with pytest.raises(capi.SpsamdError) as e:                    # claims row order, is not in it
            _add(ctx, _coo(A, (30, 20), 0, device, keep), _coo(B, (30, 20), -1, device, keep), path)
        assert e.value.code == -2
        with pytest.raises(capi.SpsamdError) as e:                    # claims column order, used with 'T'
            _add(ctx, _coo(A, (30, 20), 1, device, keep), _coo(ar.sort_storage(B, 1), (30, 20), 1, device, keep), path, tA='T', tB='T')
        assert e.value.code == -2


@pytest.mark.parametrize("path", PATHS)
def test_prepared_operands(ctx, path):
    """A prepared operand stands for its consolidated tuples, used with its own transpose or the other one."""
    from spsparse_amd import capi
    rng = np.random.default_rng(7)
    A = ar.random_operand(rng, (25, 35), 800)
    B = ar.random_operand(rng, (35, 25), 800, special=0.0)      # (preparing sums duplicates with the device's own NaN bits)
    keep = []
    for tprep in ('.', 'T'):
        lead = 1 if tprep == 'T' else 0
        op = capi.Operand(ctx, _coo(B, (35, 25), -1, False, keep), tprep, capi.AS_A, capi.ADD, False)
        try:
            pi, pj, pv = orc.consolidate(B[0], B[1], B[2], lead, ar.ADD, False)
            for tB in ('.', 'T'):
                tA = '.' if tB == 'T' else 'T'
                res = _add(ctx, _coo(A, (25, 35), -1, True, keep), op.coo, path, alpha=-0.75, beta=2.0, tA=tA, tB=tB, duplicate_policy=ar.ADD)
                _check(ctx.fetch(res), _want(A, (pi, pj, pv), -0.75, 2.0, tA, tB), "prepared %s used %s" % (tprep, tB))
        finally:
            op.close()


def test_scales(ctx):
    rng = np.random.default_rng(3)
    A = ar.random_operand(rng, (9, 9), 300)
    B = ar.random_operand(rng, (9, 9), 300)
    keep = []
    a, b = _coo(A, (9, 9), -1, True, keep), _coo(B, (9, 9), -1, True, keep)
    for path in PATHS:
        for alpha in SCALES:
            for beta in SCALES:
                for zn in (False, True):
                    got = ctx.fetch(_add(ctx, a, b, path, alpha=alpha, beta=beta, zero_nan=zn))
                    _check(got, _want(A, B, alpha, beta, zn=zn), "alpha %r beta %r zn %d" % (alpha, beta, zn))


def test_empty_and_errors(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(4)
    A = ar.random_operand(rng, (6, 8), 100)
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    keep = []
    for path in PATHS:
        r = _add(ctx, _coo(A, (6, 8), -1, True, keep), _coo(E, (6, 8), -1, False, keep), path, alpha=-0.75)
        _check(ctx.fetch(r), _want(A, E, -0.75), "B empty")
        r = _add(ctx, _coo(E, (8, 6), -1, False, keep), _coo(A, (6, 8), -1, False, keep), path, beta=3.0, tA='T')
        _check(ctx.fetch(r), _want(E, A, 1.0, 3.0, 'T'), "A empty")
        r = _add(ctx, _coo(E, (6, 8), -1, False, keep), _coo(E, (6, 8), -1, False, keep), path)
        assert r.nnz == 0 and (r.shape0, r.shape1) == (6, 8)
    with pytest.raises(capi.SpsamdError) as e:
        ctx.add(_coo(A, (6, 8), -1, False, keep), _coo(A, (6, 8), -1, False, keep), tB='T')
    assert e.value.code == -1 and "op(A)" in e.value.msg
    bad = (A[0].copy(), A[1].copy(), A[2])
    bad[1][5] = 8
    with pytest.raises(capi.SpsamdError) as e:
        ctx.add(_coo(A, (6, 8), -1, False, keep), _coo(bad, (6, 8), -1, True, keep))
    assert e.value.code == -2
    with pytest.raises(capi.SpsamdError) as e:
        ctx.add(_coo(A, (6, 8), -1, False, keep), _coo(A, (6, 8), -1, False, keep), duplicate_policy=3)
    assert e.value.code == -2
    # both output buffers of the context as operands
    r1 = ctx.add(_coo(A, (6, 8), -1, False, keep), _coo(A, (6, 8), -1, False, keep))
    P1 = capi.result_operand(r1)
    r2 = ctx.add(P1, _coo(A, (6, 8), -1, False, keep))
    _check(ctx.fetch(r2), _want(_want(A, A), A), "chained add")
    P2 = capi.result_operand(r2)
    with pytest.raises(capi.SpsamdError) as e:
        ctx.add(P1, P2)
    assert e.value.code == -2 and "both result buffers" in e.value.msg


@pytest.mark.parametrize("path", PATHS)
def test_many_tiles_and_a_long_run(ctx, path):
    """Sizes past many tiles of 2048 merged items, key groups across tile boundaries, one key 10^5 times in each operand."""
    rng = np.random.default_rng(9)
    shape = (300, 50)
    A = ar.random_operand(rng, shape, 200_000, special=0.05)
    B = ar.random_operand(rng, shape, 150_000, special=0.05)
    for X in (A, B):
        X[0][:100_000] = 123
        X[1][:100_000] = 17
    keep = []
    for pol in (ar.ADD, ar.REPLACE, ar.LEAVE_ALONE):
        res = _add(ctx, _coo(A, shape, -1, True, keep), _coo(B, shape, -1, True, keep), path, alpha=0.5, beta=-1.25, duplicate_policy=pol, zero_nan=True)
        _check(ctx.fetch(res), _want(A, B, 0.5, -1.25, pol=pol, zn=True), "tiles pol %d" % pol)
    As, Bs = ar.sort_storage(A, 0), ar.sort_storage(B, 0)
    res = _add(ctx, _coo(As, shape, 0, True, keep), _coo(Bs, shape, 0, True, keep), path, beta=-1.0)
    _check(ctx.fetch(res), _want(As, Bs, 1.0, -1.0), "tiles sorted")


_BIG = {}


def _big(name):
    """(operands, shape, expected) of the two whole-matrix cases, built once for both paths."""
    if name not in _BIG:
        if name == "rmat":
            i0, i1, v, shape = wl.rmat(18, seed=5)
            X = (i0, i1, v)
            _BIG[name] = (X, X), shape, _want(X, X, tB='T')
        else:
            i0, i1, v, shape = wl.poisson2d(2048)
            n = shape[0]
            eye = (np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
            _BIG[name] = ((i0, i1, v), eye), shape, _want((i0, i1, v), eye, 1.0, 0.3)
    return _BIG[name]


@pytest.mark.parametrize("path", PATHS)
def test_rmat18_plus_transpose(ctx, path):
    (X, _), shape, want = _big("rmat")
    keep = []
    A = _coo(X, shape, -1, True, keep)
    res = _add(ctx, A, A, path, tB='T')
    _check(ctx.fetch(res), want, "rmat18 A + A^T")


@pytest.mark.parametrize("path", PATHS)
def test_poisson2048_plus_shift(ctx, path):
    (X, eye), shape, want = _big("poisson")
    keep = []
    res = _add(ctx, _coo(X, shape, 0, True, keep), _coo(eye, shape, 0, True, keep), path, beta=0.3)
    _check(ctx.fetch(res), want, "poisson2048 A + 0.3 I")


def test_permute_sink(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(12)
    A = ar.random_operand(rng, (40, 30), 2000)
    B = ar.random_operand(rng, (30, 40), 2000)
    keep = []
    res = ctx.add(_coo(A, (40, 30), -1, True, keep), _coo(B, (30, 40), -1, True, keep), tB='T', flags=capi.SINK_PERMUTE)
    wi, wj, wv = _want(A, B, tB='T')
    assert (res.shape0, res.shape1) == (30, 40)
    gi, gj, gv = ctx.fetch(res)
    _check((gj, gi, gv), (wi, wj, wv), "permute")
    # chained back as the column-major operand it is
    P = capi.Coo(res.idx0, res.idx1, res.val, int(res.nnz), 30, 40, 1, capi.MEM_DEVICE)
    r2 = ctx.add(P, _coo(A, (40, 30), -1, False, keep), tA='T', beta=-1.0)
    _check(ctx.fetch(r2), _want((wj, wi, wv), A, 1.0, -1.0, 'T', '.'), "permuted result chained")


def test_digest_sink(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(13)
    shape = (500, 400)
    A = ar.random_operand(rng, shape, 50_000, special=0.0)
    B = ar.random_operand(rng, shape, 50_000, special=0.0)
    keep = []
    a, b = _coo(A, shape, -1, True, keep), _coo(B, shape, -1, True, keep)
    wi, wj, wv = _want(A, B, 1.0, -0.5)
    d = ctx.add(a, b, beta=-0.5, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
    cnt, s, h = orc.digest(wi, wj, wv)
    assert d.nnz == cnt and d.hash == h
    assert abs(d.sum - s) <= 1e-9 * np.sum(np.abs(wv))
    rn = ctx.to_host(d.row_nnz, shape[0], np.int64)
    rh = ctx.to_host(d.row_hash, shape[0], np.uint64)
    c = ctx.add(a, b, beta=-0.5)
    gi, gj, gv = ctx.fetch(c)
    assert np.array_equal(rn, np.bincount(gi, minlength=shape[0]))
    want_h = np.zeros(shape[0], np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(want_h, gi, orc.mix64(gi, gj))
    assert np.array_equal(rh, want_h)
    for flags in (capi.SINK_ORDERED, capi.SINK_EXACT_PATTERN):      # accepted, change nothing
        _check(ctx.fetch(ctx.add(a, b, beta=-0.5, flags=flags)), (wi, wj, wv), "flags %d" % flags)


def test_chaining_with_multiply(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(14)
    n = 60
    M = ar.random_operand(rng, (n, n), 1500, special=0.0)
    S = ar.random_operand(rng, (n, n), 700, special=0.0)
    keep = []
    m = _coo(M, (n, n), -1, True, keep)
    # a multiply result as an operand
    r = ctx.multiply(m, m, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
    pi, pj, pv, _ = orc.multiply(orc.Mat(M[0], M[1], M[2], (n, n)), orc.Mat(M[0], M[1], M[2], (n, n)))
    prod = ar.sort_storage((pi, pj, pv), 0)
    s = _coo(S, (n, n), -1, True, keep)
    r2 = ctx.add(capi.result_operand(r), s, beta=-2.0)
    wi, wj, wv = _want(prod, S, 1.0, -2.0)
    _check(ctx.fetch(r2), (wi, wj, wv), "product + S")
    # the sum fed back into multiply
    r3 = ctx.multiply(capi.result_operand(r2), m, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
    qi, qj, qv, _ = orc.multiply(orc.Mat(wi, wj, wv, (n, n), 0), orc.Mat(M[0], M[1], M[2], (n, n)))
    _check(ctx.fetch(r3), ar.sort_storage((qi, qj, qv), 0), "(product + S) * M")


def test_smoothed_aggregation_chain(ctx):
    """P = R^T - w D^-1 A R^T, then P^T A P, at 32^3: bit-identical to the oracle's pipeline."""
    import torch
    from spsparse_amd import capi
    N, w = 32, 2.0 / 3.0
    A = wl.laplace3d(N)
    R = wl.aggregation3d(N)
    nA = A[3][0]
    dinv = (np.arange(nA, dtype=np.int32), np.full(nA, 1.0 / 6.0))
    keep = []
    a = _coo(A[:3], A[3], 0, True, keep)
    rr = _coo(R[:3], R[3], 0, True, keep)
    sdinv, kd = capi.host_vec(dinv[0], dinv[1], nA)
    T = ctx.multiply(a, rr, -w, scalei=sdinv, tB='T', sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
    T_got = ctx.fetch(T)
    P = ctx.add(rr, capi.result_operand(T), tA='T')
    # copy P out of the output set: the last product reads P and P^T A at once
    nP = int(P.nnz)
    pt = [torch.empty(nP, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.float64)]
    for t, src, sz in zip(pt, (P.idx0, P.idx1, P.val), (4, 4, 8)):
        ctx.memcpy(t.data_ptr(), src, nP * sz)
    Pc = capi.device_coo(pt[0].data_ptr(), pt[1].data_ptr(), pt[2].data_ptr(), nP, (P.shape0, P.shape1), 0)
    X = ctx.multiply(Pc, a, tA='T', sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
    G = ctx.multiply(capi.result_operand(X), Pc, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
    got = ctx.fetch(G)
    # the oracle's pipeline
    oA, oR = orc.Mat(*A), orc.Mat(*R)
    ti, tj, tv, _ = orc.multiply(oA, oR, -w, scalei=orc.Vec(dinv[0], dinv[1], nA), tB='T')
    T_h = ar.sort_storage((ti, tj, tv), 0)
    _check(T_got, T_h, "T")
    pi, pj, pv = _want(R[:3], T_h, tA='T')
    _check((pt[0].cpu().numpy(), pt[1].cpu().numpy(), pt[2].cpu().numpy()), (pi, pj, pv), "P")
    oP = orc.Mat(pi, pj, pv, (P.shape0, P.shape1), 0)
    xi, xj, xv, _ = orc.multiply(oP, oA, tA='T')
    X_h = ar.sort_storage((xi, xj, xv), 0)
    gi, gj, gv, _ = orc.multiply(orc.Mat(*X_h, (X.shape0, X.shape1), 0), oP)
    _check(got, ar.sort_storage((gi, gj, gv), 0), "P^T A P")
