"""Every value of the full-size products (BASELINE cfg2-cfg5), not only their row sums: row and column projections by
linearity (tests/projection.py) against rigorous bounds, bit for bit for the integer stencils.  GPU only.

Coverage caveat.  A digest call with scalek = w leaves the kernels' `plain` emit branch (C == 1, no scalei, no scalek)
for emit_value: the accumulation, the column arithmetic and the store are the same in both branches, but at these sizes
the plain branch's values are covered only by the unweighted row sums (test_gpu_parity) and by the whole-COO checks here
and in test_gpu_parity's R-MAT 18 tests, which apply the weights after the multiply."""
import time

import numpy as np
import pytest

import projection as pj
from oracle import binding as orc
from tests.gpu_util import PeakMemory as _PeakMemory, device_operand as _device_operand, threads as _threads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from spsparse_amd import capi
    c = capi.Context()
    yield c
    c.close()


def _host(keep, shape):
    return keep[0].cpu().numpy(), keep[1].cpu().numpy(), keep[2].cpu().numpy(), shape


def _full_vec(x):
    """A scale vector with every index present."""
    from spsparse_amd import capi
    return capi.host_vec(np.arange(x.size), x, x.size, sort0=0)


def _reduce(ctx, res, shape, w=None, u=None):
    return pj.reduce_coo(pj.device_source(ctx, res, 1 << 27), int(res.nnz), shape, w=w, u=u, device="cuda:0")


def _report(name, got, proj):
    ok, ratio = pj.within(got, *proj)
    print("%s: largest error/bound %.3g" % (name, ratio))
    assert ok, (name, ratio)
    return ratio


def test_cfg2_rmat20_digest_weighted_rows(ctx):
    """cfg2, R-MAT scale-20 A*A, digest with scalek = w: row_sum is (A A w)_i for every one of the 1M rows, each within
    its bound of A (A w).  Once more with scalej = w2, scalei = u and C = -0.75 (every index present and non-zero: no row,
    term or column is skipped).  The index set (count, hash, per-row counts and hashes) stays the unscaled digest's,
    which test_cfg2_rmat20_full_size_properties pins to the oracle."""
    from spsparse_amd import capi
    t0 = time.time()
    scale, seed = 20, 1
    n, ne = 1 << scale, 16 << scale
    A, keep = _device_operand(ctx, lambda *p: ctx.gen_rmat(scale, seed, 0, ne, *p), ne, (n, n))
    d0 = ctx.multiply(A, A, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
    rn0, rh0 = ctx.to_host(d0.row_nnz, n, np.int64), ctx.to_host(d0.row_hash, n, np.uint64)
    a = _host(keep, (n, n))
    w, w2, u = pj.weights(n, 1), pj.weights(n, 2), pj.weights(n, 3)
    (sk, k1), (sj, k2), (si, k3) = _full_vec(w), _full_vec(w2), _full_vec(u)
    for C_, kw, ref in ((1.0, {}, pj.Reference(a, a)),
                        (-0.75, dict(scalei=si, scalej=sj), pj.Reference(a, a, C_=-0.75, si=u, sj=w2))):
        d = ctx.multiply(A, A, C_=C_, scalek=sk, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS, **kw)
        assert (d.nnz, d.hash, d.products) == (d0.nnz, d0.hash, d0.products)
        assert np.array_equal(ctx.to_host(d.row_nnz, n, np.int64), rn0)
        assert np.array_equal(ctx.to_host(d.row_hash, n, np.uint64), rh0)
        _report("cfg2 C=%g rows (A A w)" % C_, ctx.to_host(d.row_sum, n, np.float64), ref.rows(w))
    print("wall %.1f s" % (time.time() - t0))
    del keep


def test_cfg2_coo_sink_whole():
    """cfg2's COO sink, all 9.7e9 tuples (155 GB, offsets past 2^32), walked on the device in chunks: count, per-row
    counts and index hash equal the oracle's streaming digest; strict (i, j) order over the whole result; the row
    projections with 1 and w and the column projection with u inside their bounds; every value positive.  A context of its
    own, closed at the end, so no later test inherits the result."""
    import torch
    from spsparse_amd import capi
    t0 = time.time()
    scale, seed = 20, 1
    n, ne = 1 << scale, 16 << scale
    torch.cuda.empty_cache()
    c = capi.Context()
    try:
        with _PeakMemory() as mem:
            A, keep = _device_operand(c, lambda *p: c.gen_rmat(scale, seed, 0, ne, *p), ne, (n, n))
            r = c.multiply(A, A, sink=capi.SINK_COO)
            assert r.nnz > 1 << 33
            w, u = pj.weights(n, 1), pj.weights(n, 2)
            s = _reduce(c, r, (n, n), w, u)
        t1 = time.time()
        a = _host(keep, (n, n))
        o = orc.multiply_digest(orc.Mat(*a[:3], (n, n)), orc.Mat(*a[:3], (n, n)), nthreads=_threads(), rowstats=True)
        assert o.nnz == r.nnz
        ref = pj.Reference(a, a)
        assert pj.failures(s, ref, w, u, want=(o.nnz, o.row_nnz, o.hash)) == []
        assert s.vmin > 0
        for name, got, proj in (("rows 1", s.row_sum, ref.rows(np.ones(n))), ("rows w", s.row_w, ref.rows(w)),
                                ("cols u", s.col_u, ref.cols(u))):
            _report("cfg2 COO " + name, got, proj)
        print("device memory peak %.1f GB; device part %.1f s, host part %.1f s"
              % (mem.peak / 1e9, t1 - t0, time.time() - t1))
    finally:
        c.close()
        keep = None
        torch.cuda.empty_cache()


def test_cfg4_rmat23_digest_weighted_rows(ctx):
    """cfg4 on one GPU, R-MAT scale-23 A*A, digest with scalek = w: every one of the 8.4M rows value-checked against
    A (A w) within its bound (the host side from the device-generated tuples, copied out)."""
    import torch
    from spsparse_amd import capi
    t0 = time.time()
    scale, seed = 23, 1
    n, ne = 1 << scale, 16 << scale
    A, keep = _device_operand(ctx, lambda *p: ctx.gen_rmat(scale, seed, 0, ne, *p), ne, (n, n))
    w = pj.weights(n, 1)
    sk, k1 = _full_vec(w)
    d = ctx.multiply(A, A, scalek=sk, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
    assert d.window == 16384 and d.rows_heavy > 0 and d.cells_dense > 0
    got = ctx.to_host(d.row_sum, n, np.float64)
    a = _host(keep, (n, n))
    del keep
    torch.cuda.empty_cache()
    _report("cfg4 rows (A A w)", got, pj.Reference(a, a).rows(w))
    print("wall %.1f s" % (time.time() - t0))


def _poisson_row_counts(N):
    """nnz per row of A*A for the 5-point stencil: the 13-point diamond |dy| + |dx| <= 2 clipped to the grid."""
    i = np.arange(N * N)
    y, x = i // N, i % N
    cnt = np.zeros(N * N, np.int64)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if abs(dy) + abs(dx) <= 2:
                cnt += ((y + dy >= 0) & (y + dy < N) & (x + dx >= 0) & (x + dx < N))
    return cnt


def test_cfg3_poisson4096_every_value_exact(ctx):
    """cfg3, 5-point Poisson 4096^2, A*A with integer weights (every projection exact in fp64): the digest with
    scalek = w gives A (A w) bit for bit; the whole COO result has the closed-form count and per-row counts, strict
    order, and row (1, w) and column (u) projections equal to the host's bit for bit."""
    from spsparse_amd import capi
    t0 = time.time()
    N = 4096
    n = N * N
    na = 5 * N * N - 4 * N
    A, keep = _device_operand(ctx, lambda *p: ctx.gen_poisson2d(N, *p), na, (n, n), sort0=0)
    a = _host(keep, (n, n))
    w, u = pj.weights(n, 1, "int"), pj.weights(n, 2, "int")
    sk, k1 = _full_vec(w)
    d = ctx.multiply(A, A, scalek=sk, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
    ref = pj.Reference(a, a)
    assert np.array_equal(ctx.to_host(d.row_sum, n, np.float64), ref.rows(w)[0])
    r = ctx.multiply(A, A, sink=capi.SINK_COO)
    assert r.nnz == 13 * N * N - 20 * N + 4
    rc = _poisson_row_counts(N)
    assert int(rc.sum()) == r.nnz
    s = _reduce(ctx, r, (n, n), w, u)
    assert pj.failures(s, ref, w, u, want=(int(r.nnz), rc, None), exact=True) == []
    print("wall %.1f s" % (time.time() - t0))
    del keep


def test_cfg5_galerkin256_every_value_exact(ctx):
    """cfg5, R A R^T on the 256^3 Laplacian with integer weights: T = R A and C = T R^T (T chained in place) each whole:
    closed-form count and per-row counts, strict order, row (1, w) and column (u) projections bit for bit --
    C w = R (A (R^T w)) and u^T C = ((u^T R) A) R^T on the host."""
    from spsparse_amd import capi
    t0 = time.time()
    N, nc = 256, 128
    nf, ncc = N ** 3, nc ** 3
    A, k1 = _device_operand(ctx, lambda *p: ctx.gen_laplace3d(N, *p), 7 * N ** 3 - 6 * N ** 2, (nf, nf), sort0=0)
    R, k2 = _device_operand(ctx, lambda *p: ctx.gen_aggregation3d(N, *p), nf, (ncc, nf), sort0=0)
    a, rr = _host(k1, (nf, nf)), _host(k2, (ncc, nf))
    c = np.arange(ncc)
    x, y, z = c % nc, (c // nc) % nc, c // (nc * nc)
    faces = sum(((q > 0).astype(np.int64) + (q < nc - 1)) for q in (x, y, z))
    # T = R A
    rt = ctx.multiply(R, A, sink=capi.SINK_COO)
    assert rt.nnz == 32 * nc ** 3 - 24 * nc ** 2
    w, u = pj.weights(nf, 1, "int"), pj.weights(ncc, 2, "int")
    s = _reduce(ctx, rt, (ncc, nf), w, u)
    assert pj.failures(s, pj.Reference(rr, a), w, u, want=(int(rt.nnz), 8 + 4 * faces, None), exact=True) == []
    # C = T R^T, T read in place
    T = capi.result_operand(rt)
    rc = ctx.multiply(T, R, tB="T", sink=capi.SINK_COO)
    assert rc.nnz == 7 * nc ** 3 - 6 * nc ** 2
    w, u = pj.weights(ncc, 3, "int"), pj.weights(ncc, 4, "int")
    s = _reduce(ctx, rc, (ncc, ncc), w, u)
    assert pj.failures(s, want=(int(rc.nnz), 1 + faces, None)) == []
    assert s.vmin == -4.0 and s.vmax == 24.0
    for got, vec in ((s.row_sum, np.ones(ncc)), (s.row_w, w)):
        assert np.array_equal(got, pj.mv(rr, pj.mv(a, pj.mv(rr, vec, 'T'))))
    assert np.array_equal(s.col_u, pj.mv(rr, pj.vm(pj.vm(u, rr), a)))
    print("wall %.1f s" % (time.time() - t0))
    del k1, k2
