"""spsamd_multiply_dense on the device, bit for bit against the reference loop restated in tests/dense_ref.py: every
entry of Y (NaN payloads and signed zeros included) equals the loop over M's tuples in storage order."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_ref as dr
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

NAN, INF = np.nan, np.inf
PATHS = (0, 1, 2, 3)          # spmm_path: auto | serial | lanes | fold


def _sprinkle(rng, A, frac=0.03):
    flat = A.reshape(-1)
    k = rng.random(flat.size)
    flat[k < frac] = NAN
    flat[(k >= frac) & (k < 2 * frac)] = INF
    flat[(k >= 2 * frac) & (k < 3 * frac)] = -INF


def _apply(ctx, i0, i1, v, shape, X, Y, t='.', pol=dr.ADD, hn=False, sort0=-1, path=0, device=False):
    from spsparse_amd import capi
    ctx.set_tuning("spmm_path", path)
    try:
        if device:
            import torch
            ti = torch.from_numpy(np.ascontiguousarray(i0, np.int32)).cuda()
            tj = torch.from_numpy(np.ascontiguousarray(i1, np.int32)).cuda()
            tv = torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()
            M = capi.device_coo(ti.data_ptr(), tj.data_ptr(), tv.data_ptr(), len(v), shape, sort0)
            tX = torch.from_numpy(np.ascontiguousarray(X)).cuda()
            tY = torch.from_numpy(np.ascontiguousarray(Y)).cuda()
            torch.cuda.synchronize()
            ctx.multiply_dense(M, tX, tY, t, pol, hn)
            return tY.cpu().numpy()
        M, _keep = capi.host_coo(i0, i1, v, shape, sort0)
        out = np.array(Y, copy=True)
        ctx.multiply_dense(M, np.ascontiguousarray(X), out, t, pol, hn)
        return out
    finally:
        ctx.set_tuning("spmm_path", 0)


# (its own: compares dense Y arrays entry by entry, not tuple sets as gpu_util.check_tuples does)
def _check(got, i0, i1, v, X, Y, t, pol, hn, what="", want=None):
    if want is None:
        want = dr.apply_fast(i0, i1, v, X, Y, t, pol, hn)
    if not dr.same_bits(got, want):
        bad = np.flatnonzero(np.asarray(got).view(np.int64).reshape(-1) != np.asarray(want).view(np.int64).reshape(-1))
        raise AssertionError("%s: %d entries differ, first at %d: %r vs %r" % (what, bad.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


# (its own: test_gpu_sampled.py's maker of the same name draws a different random stream for the same seed)
def _random_matrix(rng, nrow, ncol, nnz, storage):
    """Duplicates, explicit zeros, empty rows and columns; storage: 'raw', 'row' (sort0 0) or 'col' (sort0 1)."""
    rows = rng.choice(nrow, max(1, nrow * 2 // 3), replace=False)
    cols = rng.choice(ncol, max(1, ncol * 2 // 3), replace=False)
    i0 = rng.choice(rows, nnz).astype(np.int32)
    i1 = rng.choice(cols, nnz).astype(np.int32)
    i0[nnz // 2:nnz // 2 + 5] = i0[0]
    i1[nnz // 2:nnz // 2 + 5] = i1[0]                  # duplicates of tuple 0
    v = rng.standard_normal(nnz)
    v[rng.random(nnz) < 0.08] = 0.0
    sort0 = -1
    if storage == 'row':
        o = np.lexsort((i1, i0)); sort0 = 0
    elif storage == 'col':
        o = np.lexsort((i0, i1)); sort0 = 1
    else:
        o = np.arange(nnz)
    return i0[o], i1[o], v[o], sort0


@pytest.mark.parametrize("storage", ["raw", "row", "col"])
def test_random_every_policy_transpose_and_path(ctx, storage):
    rng = np.random.default_rng({"raw": 1, "row": 2, "col": 3}[storage])
    shape = (41, 29)
    i0, i1, v, sort0 = _random_matrix(rng, shape[0], shape[1], 400, storage)
    specials = v.copy()
    _sprinkle(rng, specials)
    for t in ('.', 'T'):
        nrow, ncol = (shape[1], shape[0]) if t == 'T' else shape
        for nrhs in (1, 3, 16):
            X = rng.standard_normal((ncol, nrhs))
            Y = rng.standard_normal((nrow, nrhs))
            _sprinkle(rng, X)
            _sprinkle(rng, Y)
            for vals in (v, specials):
                for pol in (dr.LEAVE_ALONE, dr.ADD, dr.REPLACE):
                    for hn in (False, True):
                        want = dr.apply_fast(i0, i1, vals, X, Y, t, pol, hn)
                        for path in PATHS:
                            got = _apply(ctx, i0, i1, vals, shape, X, Y, t, pol, hn, sort0, path, device=path == 3)
                            _check(got, i0, i1, vals, X, Y, t, pol, hn, "%s t=%s nrhs=%d pol=%d hn=%d path=%d" % (storage, t, nrhs, pol, hn, path), want)


@pytest.mark.parametrize("nrhs", [1, 3, 16, 64, 200])
def test_nrhs_and_leading_dimensions(ctx, nrhs):
    import torch
    rng = np.random.default_rng(nrhs)
    shape = (70, 50)
    i0, i1, v, _ = _random_matrix(rng, shape[0], shape[1], 900, "raw")
    for t in ('.', 'T'):
        nrow, ncol = (shape[1], shape[0]) if t == 'T' else shape
        Xw = rng.standard_normal((ncol, nrhs + 5))
        Yw = rng.standard_normal((nrow, nrhs + 3))
        for path in PATHS:
            for device in (False, True):
                if device:
                    tX, tY = torch.from_numpy(Xw).cuda(), torch.from_numpy(Yw).cuda()
                    torch.cuda.synchronize()
                    ctx.set_tuning("spmm_path", path)
                    ctx.multiply_dense(_coo(ctx, i0, i1, v, shape)[0], tX[:, :nrhs], tY[:, :nrhs], t)
                    ctx.set_tuning("spmm_path", 0)
                    out = tY.cpu().numpy()
                else:
                    out = Yw.copy()
                    M, _keep = _coo(ctx, i0, i1, v, shape)
                    ctx.set_tuning("spmm_path", path)
                    ctx.multiply_dense(M, Xw[:, :nrhs], out[:, :nrhs], t)
                    ctx.set_tuning("spmm_path", 0)
                _check(out[:, :nrhs].copy(), i0, i1, v, Xw[:, :nrhs], Yw[:, :nrhs], t, dr.ADD, False, "nrhs=%d path=%d dev=%d" % (nrhs, path, device))
                assert dr.same_bits(out[:, nrhs:], Yw[:, nrhs:]), "padding after the nrhs values was written"


# (its own: host only, returns capi.host_coo's (struct, keepalive) pair; gpu_util.coo appends to a keep list)
def _coo(ctx, i0, i1, v, shape, sort0=-1):
    from spsparse_amd import capi
    return capi.host_coo(i0, i1, v, shape, sort0)


def test_one_dimensional_x_and_y(ctx):
    rng = np.random.default_rng(5)
    i0, i1, v, _ = _random_matrix(rng, 20, 30, 100, "raw")
    x, y = rng.standard_normal(30), rng.standard_normal(20)
    got = _apply(ctx, i0, i1, v, (20, 30), x, y)
    assert got.shape == (20,)
    _check(got, i0, i1, v, x, y, '.', dr.ADD, False, "1-D")


@pytest.mark.parametrize("device", [False, True])
def test_long_rows_every_kernel(ctx, device):
    """Rows of 100 and of 5000 tuples (beyond 64 and 4096) among short ones, unsorted, with NaN / Inf."""
    rng = np.random.default_rng(11)
    nrow, ncol = 300, 6000
    parts_r, parts_c = [rng.integers(0, nrow, 3000)], [rng.integers(0, ncol, 3000)]
    for r, n in ((7, 100), (150, 5000), (299, 4097)):
        parts_r.append(np.full(n, r)); parts_c.append(rng.integers(0, ncol, n))
    for c, n in ((33, 3000), (4000, 200)):                # long rows of op(M) = M^T
        parts_r.append(rng.integers(0, nrow, n)); parts_c.append(np.full(n, c))
    i0 = np.concatenate(parts_r).astype(np.int32)
    i1 = np.concatenate(parts_c).astype(np.int32)
    perm = rng.permutation(i0.size)
    i0, i1 = i0[perm], i1[perm]
    v = rng.standard_normal(i0.size) * np.exp(rng.standard_normal(i0.size) * 8)
    _sprinkle(rng, v, 0.0005)
    for t in ('.', 'T'):
        nr, nc = (ncol, nrow) if t == 'T' else (nrow, ncol)
        for nrhs in (1, 8, 20):
            X = rng.standard_normal((nc, nrhs)); _sprinkle(rng, X, 0.0005)
            Y = rng.standard_normal((nr, nrhs)); _sprinkle(rng, Y, 0.01)
            for pol in (dr.ADD, dr.LEAVE_ALONE):
                for hn in (False, True):
                    want = dr.apply_fast(i0, i1, v, X, Y, t, pol, hn)
                    for path in PATHS:
                        got = _apply(ctx, i0, i1, v, (nrow, ncol), X, Y, t, pol, hn, -1, path, device)
                        _check(got, i0, i1, v, X, Y, t, pol, hn, "t=%s nrhs=%d pol=%d hn=%d path=%d" % (t, nrhs, pol, hn, path), want)


@pytest.mark.parametrize("nrhs", [1, 8])
def test_rmat14_and_poisson512_whole(ctx, nrhs):
    from spsparse_amd import workloads as wl
    rng = np.random.default_rng(nrhs)
    for name, (i0, i1, v, shape), sort0 in (("rmat14", wl.rmat(14, seed=3), -1), ("poisson512", wl.poisson2d(512), 0)):
        for t in ('.', 'T'):
            X = rng.standard_normal((shape[0], nrhs))
            Y = rng.standard_normal((shape[0], nrhs))
            want = dr.apply_fast(i0, i1, v, X, Y, t, dr.ADD, False)
            for path in PATHS if name == "rmat14" else (0,):
                got = _apply(ctx, i0, i1, v, shape, X, Y, t, dr.ADD, False, sort0, path, device=True)
                _check(got, i0, i1, v, X, Y, t, dr.ADD, False, "%s t=%s path=%d" % (name, t, path), want)


@pytest.mark.parametrize("t", ['.', 'T'])
def test_prepared_operand_is_its_consolidated_tuples(ctx, t):
    from spsparse_amd import capi
    rng = np.random.default_rng(21)
    shape = (60, 45)
    i0, i1, v, _ = _random_matrix(rng, shape[0], shape[1], 700, "raw")
    M, _keep = capi.host_coo(i0, i1, v, shape)
    op = capi.Operand(ctx, M, t, capi.AS_A)
    try:
        lead = 1 if t == 'T' else 0
        res = ctx.consolidate(op.coo, lead)
        c0, c1, cv = ctx.fetch(res)
        plain, _k2 = capi.host_coo(c0, c1, cv, shape, lead)
        for tt in ('.', 'T'):                       # the same transpose (its own tuples) and the other one
            nrow, ncol = (shape[1], shape[0]) if tt == 'T' else shape
            for nrhs in (1, 16):
                X, Y = rng.standard_normal((ncol, nrhs)), rng.standard_normal((nrow, nrhs))
                for path in PATHS:
                    ctx.set_tuning("spmm_path", path)
                    a, b = Y.copy(), Y.copy()
                    ctx.multiply_dense(op.coo, X, a, tt)
                    ctx.multiply_dense(plain, X, b, tt)
                    ctx.set_tuning("spmm_path", 0)
                    assert dr.same_bits(a, b), (tt, nrhs, path)
                    _check(a, c0, c1, cv, X, Y, tt, dr.ADD, False, "prepared %s/%s" % (t, tt))
    finally:
        op.close()


def test_chained_result_as_m(ctx):
    """T = R*A, C = T*R^T (cfg5's Galerkin product, small): the SINK_COO result C applied in place, both ways; C stays
    fetchable and unchanged."""
    from spsparse_amd import capi, workloads as wl
    R, A = wl.aggregation3d(8), wl.laplace3d(8)
    r, _kr = capi.host_coo(*R[:3], R[3], 0)
    a, _ka = capi.host_coo(*A[:3], A[3], 0)
    T = ctx.multiply(r, a)
    Cres = ctx.multiply(capi.result_operand(T), r, tB='T')
    before = ctx.fetch(Cres)
    Cm = capi.result_operand(Cres)
    rng = np.random.default_rng(4)
    n = int(Cres.shape0)
    for t in ('.', 'T'):
        for nrhs in (1, 5, 32):
            X, Y = rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs))
            for path in PATHS:
                ctx.set_tuning("spmm_path", path)
                got = Y.copy()
                ctx.multiply_dense(Cm, X, got, t)
                ctx.set_tuning("spmm_path", 0)
                _check(got, before[0], before[1], before[2], X, Y, t, dr.ADD, False, "chained t=%s path=%d" % (t, path))
    after = ctx.fetch(Cres)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert dr.same_bits(before[2], after[2])


def test_errors(ctx):
    from spsparse_amd import capi
    L = ctx.L
    i0, i1, v = np.array([0, 1], np.int32), np.array([1, 2], np.int32), np.array([1.0, 2.0])
    M, _k = capi.host_coo(i0, i1, v, (2, 3))
    X = np.ones((3, 4)); Y = np.zeros((2, 4))
    px, py = X.ctypes.data, Y.ctypes.data

    def call(m, x, ldx, y, ldy, nrhs, mem=capi.MEM_HOST, pol=capi.ADD, t=b'.'):
        return L.spsamd_multiply_dense(ctx.h, None if m is None else C.byref(m), t, x, ldx, y, ldy, nrhs, mem, pol, 0)

    EINVAL = -2
    assert call(None, px, 4, py, 4, 4) == EINVAL
    assert call(M, None, 4, py, 4, 4) == EINVAL
    assert call(M, px, 4, None, 4, 4) == EINVAL
    assert call(M, px, 3, py, 4, 4) == EINVAL                    # ldx < nrhs
    assert call(M, px, 4, py, 2, 4) == EINVAL                    # ldy < nrhs
    assert call(M, px, 4, py, 4, 4, pol=3) == EINVAL
    assert call(M, px, 4, py, 4, 4, pol=-1) == EINVAL
    assert call(M, px, 4, py, 4, 4, mem=2) == EINVAL
    assert call(M, px, 4, px + 8, 4, 3) == EINVAL               # Y inside X
    assert call(M, py + 16, 4, py, 4, 4) == EINVAL              # X starting inside Y
    bad, _kb = capi.host_coo(np.array([0, 2], np.int32), i1, v, (2, 3))
    assert call(bad, px, 4, py, 4, 4) == EINVAL                  # row index out of bounds
    bad2, _kb2 = capi.host_coo(i0, np.array([1, -1], np.int32), v, (2, 3))
    assert call(bad2, px, 4, py, 4, 4) == EINVAL
    assert b"out of bounds" in L.spsamd_last_error(ctx.h)
    assert np.all(Y == 0)
    # nothing to do: 0, Y untouched -- even with NULL arrays
    assert call(M, None, 0, None, 0, 0) == 0
    empty, _ke = capi.host_coo(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), (2, 3))
    Y[:] = 7.0
    assert call(empty, px, 4, py, 4, 4) == 0 and np.all(Y == 7.0)
    assert L.spsamd_multiply_dense(None, C.byref(M), b'.', px, 4, py, 4, 4, 0, 1, 0) == EINVAL
    # the Python binding checks shapes and types before the call
    with pytest.raises(ValueError):
        ctx.multiply_dense(M, np.ones((2, 4)), Y)
    with pytest.raises(TypeError):
        ctx.multiply_dense(M, np.ones((3, 4), np.float32), Y)
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_dense(bad, X, Y)
    assert e.value.code == EINVAL


def test_more_pairs_than_the_serial_grid(ctx):
    """256 rows per CU and one more, 64 right-hand sides, rows of 0 to 3 tuples: 64 (row, rhs) pairs more than
    k_spmm_serial's capped grid of 64 workgroups per CU has threads, so its stride loop takes a second trip."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nrow, ncol, nrhs = cus * 256 + 1, 3000, 64
    assert nrow * nrhs > cus * 64 * 256
    rng = np.random.default_rng(21)
    i0 = np.repeat(np.arange(nrow), rng.integers(0, 4, nrow)).astype(np.int32)
    i0[-1] = nrow - 1                                      # the last row, the one past the grid, has a tuple
    i1 = rng.integers(0, ncol, i0.size).astype(np.int32)
    v = rng.standard_normal(i0.size)
    X = rng.standard_normal((ncol, nrhs))
    Y = rng.standard_normal((nrow, nrhs))
    got = _apply(ctx, i0, i1, v, (nrow, ncol), X, Y, sort0=0, device=True)
    _check(got, i0, i1, v, X, Y, '.', dr.ADD, False, "%d rows x %d" % (nrow, nrhs))


@pytest.mark.parametrize("large", ["X", "Y"])
def test_offsets_beyond_2_to_the_32(ctx, large):
    """rows * ld > 2^32 values in X (the columns of M name its last rows) or in Y (the rows of M are its last rows): about
    34 GB on the device, col * ldx and row * ldy in 64 bits in the serial, lanes and fold kernels.  Rows of 1 to 150 tuples."""
    import torch
    from spsparse_amd import capi
    dev = torch.device("cuda", 0)
    big, small, ld, nrhs = (1 << 22) + 8, 64, 1025, 3
    assert big * ld > 1 << 32
    rng = np.random.default_rng({"X": 31, "Y": 32}[large])
    named = np.r_[0, 1, np.arange(big - 40, big)]
    m = 600
    far = rng.choice(named, m)
    far[:150] = big - 1                                    # 150 tuples on the last row of the large array: a long row / column
    near = rng.integers(0, small, m)
    near[150:300] = 7                                      # ... and a long row or column on the small side
    o = rng.permutation(m)
    far, near = far[o].astype(np.int32), near[o].astype(np.int32)
    v = rng.standard_normal(m)
    i0, i1, shape = (near, far, (small, big)) if large == "X" else (far, near, (big, small))
    M, _keep = capi.host_coo(i0, i1, v, shape)
    Lh = np.zeros((big, nrhs))
    Lh[named] = rng.standard_normal((named.size, nrhs))
    Sh = rng.standard_normal((small, nrhs))
    Xh, Yh = (Lh, Sh) if large == "X" else (Sh, Lh)
    want = dr.apply_fast(i0, i1, v, Xh, Yh)
    assert np.count_nonzero(np.any(want != Yh, axis=1)) >= (40 if large == "Y" else 60)
    idx = torch.from_numpy(named).to(dev)
    L = torch.zeros((big, ld), dtype=torch.float64, device=dev)
    S = torch.empty((small, nrhs), dtype=torch.float64, device=dev)
    try:
        for path in (1, 2, 3):
            L[idx, :nrhs] = torch.from_numpy(Lh[named]).to(dev)
            S.copy_(torch.from_numpy(Sh))
            torch.cuda.synchronize()
            tX, tY = (L[:, :nrhs], S) if large == "X" else (S, L[:, :nrhs])
            ctx.set_tuning("spmm_path", path)
            try:
                ctx.multiply_dense(M, tX, tY)
            finally:
                ctx.set_tuning("spmm_path", 0)
            _check(tY.cpu().numpy(), i0, i1, v, Xh, Yh, '.', dr.ADD, False, "64-bit %s path=%d" % (large, path), want)
            assert dr.same_bits(tX.cpu().numpy(), Xh), "X was written"
        assert int(torch.count_nonzero(L[:, nrhs:])) == 0, "the padding of the large array was written"
    finally:
        del L
        torch.cuda.empty_cache()
