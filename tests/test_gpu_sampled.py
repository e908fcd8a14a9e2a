"""spsamd_multiply_sampled on the device, bit for bit against the loop restated in tests/sampled_ref.py: every out[t] (NaN
payloads and signed zeros included) equals the serial, ascending-r dot product of the tuple's P and Q rows, scaled."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import dense_ref as dr
from tests import sampled_ref as sr
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

NAN, INF = np.nan, np.inf
PATHS = (0, 1, 2)             # sampled_path: auto | lane | slab
KS = (0, 1, 2, 3, 7, 8, 15, 16, 17, 64, 65, 256, 1000)
SCALES = ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (2.5, -1.0), (NAN, 0.0), (1.0, NAN))
EINVAL = -2


def nan_with(payload):
    x = np.array([0.0])
    x.view(np.uint64)[0] = payload
    return x[0]


def _sprinkle(rng, A, frac=0.02):
    """NaNs with distinct payloads (quiet and signalling, both signs) and infinities."""
    flat = A.reshape(-1)
    u = rng.random(flat.size)
    nan = u < frac
    pay = rng.integers(1, 1 << 50, flat.size).astype(np.uint64)
    sign = (rng.random(flat.size) < 0.5).astype(np.uint64) << np.uint64(63)
    quiet = (rng.random(flat.size) < 0.5).astype(np.uint64) << np.uint64(51)
    flat.view(np.uint64)[nan] = (np.uint64(0x7FF0000000000000) | sign | quiet | pay)[nan]
    flat[(u >= frac) & (u < 2 * frac)] = INF
    flat[(u >= 2 * frac) & (u < 3 * frac)] = -INF


# (its own: compares the out[] value arrays, not tuple sets as gpu_util.check_tuples does)
def _check(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if not dr.same_bits(got, want):
        bad = np.flatnonzero(got.view(np.int64).reshape(-1) != want.view(np.int64).reshape(-1))
        raise AssertionError("%s: %d of %d values differ, first at %d: %r vs %r" % (
            what, bad.size, want.size, bad[0], got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]]))


# (its own: test_gpu_dense.py's maker of the same name draws a different random stream for the same seed)
def _random_matrix(rng, nrow, ncol, nnz, storage):
    """Duplicates and explicit zeros; storage: 'raw', 'row' (sort0 0) or 'col' (sort0 1)."""
    i0 = rng.integers(0, nrow, nnz).astype(np.int32)
    i1 = rng.integers(0, ncol, nnz).astype(np.int32)
    if nnz > 8:
        i0[nnz // 2:nnz // 2 + 4] = i0[0]
        i1[nnz // 2:nnz // 2 + 4] = i1[0]
    v = rng.standard_normal(nnz)
    v[rng.random(nnz) < 0.1] = 0.0
    sort0 = -1
    if storage == 'row':
        o = np.lexsort((i1, i0)); sort0 = 0
    elif storage == 'col':
        o = np.lexsort((i0, i1)); sort0 = 1
    else:
        o = np.arange(nnz)
    return i0[o], i1[o], v[o], sort0


def _padded(rng, rows, k, pad):
    """rows x k values inside a rows x (k + pad) array (ld = k + pad)."""
    W = rng.standard_normal((rows, k + pad))
    return W, W[:, :k]


def _run(ctx, M, P, Q, t, alpha, beta, path, device):
    ctx.set_tuning("sampled_path", path)
    try:
        if device:
            import torch
            tP = torch.from_numpy(np.ascontiguousarray(P.base if P.base is not None else P)).cuda()
            tQ = torch.from_numpy(np.ascontiguousarray(Q.base if Q.base is not None else Q)).cuda()
            k = P.shape[1]
            torch.cuda.synchronize()
            out = ctx.multiply_sampled(M, tP[:, :k], tQ[:, :k], transpose=t, alpha=alpha, beta=beta)
            return out.cpu().numpy()
        return ctx.multiply_sampled(M, P, Q, transpose=t, alpha=alpha, beta=beta)
    finally:
        ctx.set_tuning("sampled_path", 0)


@pytest.mark.parametrize("storage", ["raw", "row", "col"])
@pytest.mark.parametrize("shape", [(1, 1), (97, 13), (13, 97)])
def test_seeded_grid(ctx, storage, shape):
    from spsparse_amd import capi
    rng = np.random.default_rng(zlib.crc32(repr((storage, shape)).encode()))
    nnz = 1 if shape == (1, 1) else 700
    i0, i1, v, sort0 = _random_matrix(rng, shape[0], shape[1], nnz, storage)
    _sprinkle(rng, v)
    M, _keep = capi.host_coo(i0, i1, v, shape, sort0)
    for t in ('.', 'T'):
        nrow, ncol = (shape[1], shape[0]) if t == 'T' else shape
        for k in KS:
            (Pw, P), (Qw, Q) = _padded(rng, nrow, k, 1 + k % 3), _padded(rng, ncol, k, 2)
            _sprinkle(rng, Pw, 0.002)
            _sprinkle(rng, Qw, 0.002)
            for alpha, beta in (SCALES if k in (0, 3, 17, 65) else SCALES[:1] + SCALES[3:4]):
                want = sr.sample_ref(i0, i1, v, P, Q, t, alpha, beta)
                for path in PATHS:
                    for device in (False, True):
                        got = _run(ctx, M, P, Q, t, alpha, beta, path, device)
                        _check(got, want, "%s %s t=%s k=%d a=%r b=%r path=%d dev=%d" % (storage, shape, t, k, alpha, beta, path, device))


@pytest.mark.parametrize("t", ['.', 'T'])
def test_odd_k_with_even_leading_dimensions(ctx, t):
    """Odd k with ldp and ldq both even on the device: the rows stay 16-byte aligned, so both kernels take their 16-byte
    loads and then the single-value tail (the lane kernel's last r, the slab loader's last value of a partial slab)."""
    from spsparse_amd import capi
    rng = np.random.default_rng(31 if t == '.' else 32)
    shape = (90, 70)
    i0, i1, v, _ = _random_matrix(rng, shape[0], shape[1], 2000, "raw")
    _sprinkle(rng, v)
    M, _keep = capi.host_coo(i0, i1, v, shape)
    nrow, ncol = (shape[1], shape[0]) if t == 'T' else shape
    for k in (1, 3, 15, 17, 33, 47, 65):
        for pad in (1, 3):                            # ld = k + 1 and k + 3: both even
            (Pw, P), (Qw, Q) = _padded(rng, nrow, k, pad), _padded(rng, ncol, k, pad)
            _sprinkle(rng, Pw, 0.002)
            _sprinkle(rng, Qw, 0.002)
            want = sr.sample_ref(i0, i1, v, P, Q, t, -1.5, 0.5)
            for path in PATHS:
                got = _run(ctx, M, P, Q, t, -1.5, 0.5, path, device=True)
                _check(got, want, "t=%s k=%d ld=%d path=%d" % (t, k, k + pad, path))


def test_empty_m(ctx):
    from spsparse_amd import capi
    for shape in ((0, 0), (5, 3)):
        M, _k = capi.host_coo(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), shape)
        if shape[0]:
            out = ctx.multiply_sampled(M, np.ones((shape[0], 4)), np.ones((shape[1], 4)))
            assert out.shape == (0,)
        assert ctx.L.spsamd_multiply_sampled(ctx.h, C.byref(M), b'.', None, 4, None, 4, 4, 1.0, 1.0, None, 0) == 0


def test_device_m_and_in_place(ctx):
    """M on the device, out == M.val: each tuple's v is read before its slot is written."""
    import torch
    from spsparse_amd import capi
    rng = np.random.default_rng(8)
    shape = (300, 200)
    i0, i1, v, _ = _random_matrix(rng, shape[0], shape[1], 5000, "raw")
    _sprinkle(rng, v)
    for k in (3, 8, 64, 65):
        for path in PATHS:
            P, Q = rng.standard_normal((shape[0], k)), rng.standard_normal((shape[1], k))
            ti, tj = torch.from_numpy(i0).cuda(), torch.from_numpy(i1).cuda()
            tv = torch.from_numpy(v.copy()).cuda()
            tP, tQ = torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda()
            M = capi.device_coo(ti.data_ptr(), tj.data_ptr(), tv.data_ptr(), len(v), shape)
            torch.cuda.synchronize()
            ctx.set_tuning("sampled_path", path)
            got = ctx.multiply_sampled(M, tP, tQ, out=tv, alpha=-1.0, beta=1.0)
            ctx.set_tuning("sampled_path", 0)
            assert got is tv
            _check(tv.cpu().numpy(), sr.sample_ref(i0, i1, v, P, Q, '.', -1.0, 1.0), "in place k=%d path=%d" % (k, path))
    # host M and host out == M.val
    M, keep = capi.host_coo(i0, i1, v.copy(), shape)
    P, Q = rng.standard_normal((shape[0], 5)), rng.standard_normal((shape[1], 5))
    got = ctx.multiply_sampled(M, P, Q, out=keep[2], alpha=2.0, beta=-1.0)
    _check(got, sr.sample_ref(i0, i1, v, P, Q, '.', 2.0, -1.0), "host in place")


def test_one_dimensional_p_and_q(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(5)
    i0, i1, v, _ = _random_matrix(rng, 20, 30, 100, "raw")
    M, _k = capi.host_coo(i0, i1, v, (20, 30))
    p, q = rng.standard_normal(20), rng.standard_normal(30)
    _check(ctx.multiply_sampled(M, p, q, beta=0.5), sr.sample_ref(i0, i1, v, p, q, '.', 1.0, 0.5), "1-D")


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
        c0, c1, cv = ctx.fetch(ctx.consolidate(op.coo, lead))
        assert int(op.coo.nnz) == len(cv)
        for tt in ('.', 'T'):                         # the transpose it was prepared for and the other one
            nrow, ncol = (shape[1], shape[0]) if tt == 'T' else shape
            for k in (1, 8, 17, 64):
                P, Q = rng.standard_normal((nrow, k)), rng.standard_normal((ncol, k))
                want = sr.sample_ref(c0, c1, cv, P, Q, tt, 1.5, -2.0)
                for path in PATHS:
                    for device in (False, True):
                        got = _run(ctx, op.coo, P, Q, tt, 1.5, -2.0, path, device)
                        _check(got, want, "prepared %s/%s k=%d path=%d dev=%d" % (t, tt, k, path, device))
    finally:
        op.close()


def test_chained_result_as_m(ctx):
    """T = R*A, C = T*R^T (cfg5's Galerkin product, small): the SINK_COO result C sampled in place, both ways; C stays
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
        for k in (1, 8, 33):
            P, Q = rng.standard_normal((n, k)), rng.standard_normal((n, k))
            want = sr.sample_ref(before[0], before[1], before[2], P, Q, t, 1.0, 3.0)
            for path in PATHS:
                got = _run(ctx, Cm, P, Q, t, 1.0, 3.0, path, device=True)
                _check(got, want, "chained t=%s k=%d path=%d" % (t, k, path))
    after = ctx.fetch(Cres)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert dr.same_bits(before[2], after[2])


def test_full_size_poisson_and_rmat(ctx):
    """Poisson 4096^2 at k = 8 (row-sorted, 83.9 M tuples) and R-MAT 20 at k = 64 (unsorted, duplicates): every value."""
    import torch
    from spsparse_amd import capi
    dev = torch.device("cuda", 0)
    for name, k in (("poisson", 8), ("rmat", 64)):
        if name == "poisson":
            N = 4096
            nnz, shape = 5 * N * N - 4 * N, (N * N, N * N)
        else:
            nnz, shape = 16 << 20, (1 << 20, 1 << 20)
        ti = torch.empty(nnz, dtype=torch.int32, device=dev)
        tj = torch.empty(nnz, dtype=torch.int32, device=dev)
        tv = torch.empty(nnz, dtype=torch.float64, device=dev)
        if name == "poisson":
            ctx.gen_poisson2d(N, ti.data_ptr(), tj.data_ptr(), tv.data_ptr())
        else:
            ctx.gen_rmat(20, 1, 0, nnz, ti.data_ptr(), tj.data_ptr(), tv.data_ptr())
        M = capi.device_coo(ti.data_ptr(), tj.data_ptr(), tv.data_ptr(), nnz, shape)
        g = torch.Generator(device=dev).manual_seed(k)
        P = torch.rand((shape[0], k), dtype=torch.float64, device=dev, generator=g) - 0.5
        Q = torch.rand((shape[1], k), dtype=torch.float64, device=dev, generator=g) - 0.5
        torch.cuda.synchronize()
        got = ctx.multiply_sampled(M, P, Q, alpha=1.0, beta=-0.5).cpu().numpy()
        want = sr.sample_ref(ti.cpu().numpy(), tj.cpu().numpy(), tv.cpu().numpy(), P.cpu().numpy(), Q.cpu().numpy(),
                             '.', 1.0, -0.5)
        _check(got, want, name)
        del ti, tj, tv, P, Q
        torch.cuda.empty_cache()


def test_offsets_beyond_2_to_the_32(ctx):
    """rows * ldp > 2^32 values (P about 34 GB on the device), tuples in the last rows: 64-bit index arithmetic."""
    import torch
    from spsparse_amd import capi
    dev = torch.device("cuda", 0)
    nrow, ncol, ldp, k = (1 << 22) + 8, 64, 1025, 3
    assert nrow * ldp > 1 << 32
    P = torch.empty((nrow, ldp), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(9)
    i0 = np.concatenate([np.arange(nrow - 40, nrow), [0, 1, nrow - 1]]).astype(np.int32)
    i1 = rng.integers(0, ncol, i0.size).astype(np.int32)
    v = rng.standard_normal(i0.size)
    Ph = np.zeros((nrow, k))
    used = np.unique(i0)
    Ph[used] = rng.standard_normal((used.size, k))
    P[torch.from_numpy(used.astype(np.int64)).to(dev), :k] = torch.from_numpy(Ph[used]).to(dev)
    Q = torch.from_numpy(rng.standard_normal((ncol, k))).to(dev)
    M, _keep = capi.host_coo(i0, i1, v, (nrow, ncol))
    want = sr.sample_ref(i0, i1, v, Ph, Q.cpu().numpy(), '.', 1.0, 1.0)
    for path in PATHS:
        ctx.set_tuning("sampled_path", path)
        got = ctx.multiply_sampled(M, P[:, :k], Q, beta=1.0).cpu().numpy()
        ctx.set_tuning("sampled_path", 0)
        _check(got, want, "64-bit path=%d" % path)
    del P
    torch.cuda.empty_cache()


def test_errors(ctx):
    from spsparse_amd import capi
    L = ctx.L
    i0, i1, v = np.array([0, 1], np.int32), np.array([1, 2], np.int32), np.array([1.0, 2.0])
    M, keep = capi.host_coo(i0, i1, v, (2, 3))
    P, Q = np.ones((2, 4)), np.ones((3, 4))
    out = np.full(2, 7.0)
    pp, pq, po = P.ctypes.data, Q.ctypes.data, out.ctypes.data

    def call(m, p, ldp, q, ldq, k, o, beta=1.0, mem=capi.MEM_HOST, t=b'.'):
        return L.spsamd_multiply_sampled(ctx.h, None if m is None else C.byref(m), t, p, ldp, q, ldq, k, 1.0, beta, o, mem)

    assert call(None, pp, 4, pq, 4, 4, po) == EINVAL                      # M NULL
    assert call(M, None, 4, pq, 4, 4, po) == EINVAL                       # P NULL
    assert call(M, pp, 4, None, 4, 4, po) == EINVAL                       # Q NULL
    assert call(M, pp, 4, pq, 4, 4, None) == EINVAL                       # out NULL
    novals = capi.Coo(keep[0].ctypes.data, keep[1].ctypes.data, None, 2, 2, 3, -1, capi.MEM_HOST)
    assert call(novals, pp, 4, pq, 4, 4, po, beta=1.0) == EINVAL          # M->val NULL, beta != 0
    assert call(M, pp, 3, pq, 4, 4, po) == EINVAL                         # ldp < k
    assert call(M, pp, 4, pq, 3, 4, po) == EINVAL                         # ldq < k
    assert call(M, pp, 4, pq, 4, 4, po, mem=2) == EINVAL                  # bad mem
    assert call(M, pp, 4, pq, 4, 4, po, mem=-1) == EINVAL
    bad, _kb = capi.host_coo(np.array([0, 2], np.int32), i1, v, (2, 3))
    assert call(bad, pp, 4, pq, 4, 4, po) == EINVAL                       # row index out of bounds
    bad2, _kb2 = capi.host_coo(i0, np.array([1, -1], np.int32), v, (2, 3))
    assert call(bad2, pp, 4, pq, 4, 4, po) == EINVAL
    assert b"out of bounds" in L.spsamd_last_error(ctx.h)
    bad3, _kb3 = capi.host_coo(i0, np.array([1, 3], np.int32), v, (2, 3))
    assert call(bad3, pp, 4, pq, 4, 4, po, t=b'T') == EINVAL              # column index 3 of 3 columns, read under 'T'
    assert call(M, pp, 4, pq, 4, 4, pp + 8) == EINVAL                     # out inside P
    assert call(M, pp, 4, pq, 4, 4, pq + 80) == EINVAL                    # out over Q's last row
    assert call(M, pp, 4, pq, 4, 4, keep[0].ctypes.data) == EINVAL        # out over M's row indices
    assert call(M, pp, 4, pq, 4, 4, keep[1].ctypes.data - 4) == EINVAL    # ... and its column indices
    assert call(M, pp, 4, pq, 4, 4, keep[2].ctypes.data + 8) == EINVAL    # overlapping M->val without being it
    assert np.all(out == 7.0) and np.array_equal(keep[2], v)
    # beta == 0: M->val may be NULL; k == 0: P and Q may be NULL
    assert call(novals, pp, 4, pq, 4, 4, po, beta=0.0) == 0 and np.all(out == 4.0)
    assert call(M, None, 0, None, 0, 0, po, beta=2.0) == 0 and out.tolist() == [2.0, 4.0]
    assert L.spsamd_multiply_sampled(None, C.byref(M), b'.', pp, 4, pq, 4, 4, 1.0, 0.0, po, 0) == EINVAL
    # the Python binding checks shapes and types before the call
    with pytest.raises(ValueError):
        ctx.multiply_sampled(M, np.ones((3, 4)), Q)
    with pytest.raises(ValueError):
        ctx.multiply_sampled(M, P, np.ones((3, 5)))
    with pytest.raises(TypeError):
        ctx.multiply_sampled(M, P.astype(np.float32), Q)
    with pytest.raises(ValueError):
        ctx.multiply_sampled(M, P, Q, out=np.empty(3))
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_sampled(bad, P, Q)
    assert e.value.code == EINVAL


def test_busy_context_is_refused(ctx):
    """A call from inside a streamed multiply's callback (the context is delivering) is refused, out untouched."""
    from spsparse_amd import capi
    A, _ka = capi.host_coo(np.array([0, 1], np.int32), np.array([1, 0], np.int32), np.array([1.0, 2.0]), (2, 2))
    M, _km = capi.host_coo(np.array([0], np.int32), np.array([1], np.int32), np.array([1.0]), (2, 2))
    P, Q, out = np.ones((2, 2)), np.ones((2, 2)), np.full(1, 5.0)
    codes = []

    def on_chunk(i, j, v):
        codes.append(ctx.L.spsamd_multiply_sampled(ctx.h, C.byref(M), b'.', P.ctypes.data, 2, Q.ctypes.data, 2, 2,
                                                    1.0, 0.0, out.ctypes.data, capi.MEM_HOST))
    ctx.multiply_stream(A, A, on_chunk=on_chunk)
    assert codes and all(c == EINVAL for c in codes)
    assert out.tolist() == [5.0]
    assert ctx.multiply_sampled(M, P, Q).tolist() == [2.0]
