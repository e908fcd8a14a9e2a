"""spsamd_multiply_stream on the device: the streamed tuples are those of spsamd_multiply + spsamd_result_fetch (bit for
bit under SINK_ORDERED, to the same rules otherwise), the partition is the numpy model's (tests/stream_ref.py), errors come
before the first chunk, chained and prepared operands work, and the block outputs stay within two budgets."""
import os
import subprocess
import time

import numpy as np
import pytest

import projection as pj

from oracle import binding as orc
from spsparse_amd import workloads as wl
from tests import stream_ref as sr
from tests.gpu_util import PeakMemory as _PeakMemory, build_cpp_test, ctx, threads as _threads  # noqa: F401

pytestmark = pytest.mark.gpu

UNLIMITED = 1 << 62


class Keep:
    """Host operands and scale vectors as C structs, kept alive for the test."""

    def __init__(self):
        self.keep = []

    def coo(self, M, sort0=-1):
        from spsparse_amd import capi
        s, k = capi.host_coo(M[0], M[1], M[2], M[3], sort0)
        self.keep.append(k)
        return s

    def vec(self, V):
        from spsparse_amd import capi
        if V is None:
            return None
        s, k = capi.host_vec(V[0], V[1], V[2])
        self.keep.append(k)
        return s


class Collect:
    """on_chunk that keeps every tuple and checks that no chunk is empty."""

    def __init__(self):
        self.parts, self.chunks = [], 0

    def __call__(self, i, j, v):
        assert i.size >= 1
        self.parts.append((i.copy(), j.copy(), v.copy()))
        self.chunks += 1

    def tuples(self):
        if not self.parts:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
        return tuple(np.concatenate([p[q] for p in self.parts]) for q in range(3))


def _plain(ctx, A, B, **kw):
    res = ctx.multiply(A, B, **kw)
    return ctx.fetch(res), res


def _stream(ctx, A, B, budget, **kw):
    col = Collect()
    res, st = ctx.multiply_stream(A, B, block_tuples=budget, on_chunk=col, **kw)
    return col.tuples(), res, st


def _bits_equal(got, want):
    return (got[0].size == want[0].size and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            and np.array_equal(got[2].view(np.int64), want[2].view(np.int64)))


def _model_bounds(ctx, A, B, tA, tB, pol, zn):
    """Bounds of op(A)'s rows from the consolidated operands (spsamd_consolidate in the orders the product uses)."""
    a0, bk = (1 if tA == "T" else 0), (1 if tB == "T" else 0)
    bj = 1 - bk
    ra = ctx.consolidate(A, a0, pol, zn)
    ia, ja, _ = ctx.fetch(ra)
    rb = ctx.consolidate(B, bj, pol, zn)                 # (the reference's order for B: its zero_nan drops these NaNs)
    ib, jb, _ = ctx.fetch(rb)
    arows, ainner = (ja, ia) if a0 else (ia, ja)
    brows = jb if bk else ib
    shapeA, shapeB = (A.shape0, A.shape1), (B.shape0, B.shape1)
    nrow, nrowb, ncol = shapeA[a0], shapeB[bk], shapeB[bj]
    blen = np.bincount(brows, minlength=nrowb)
    return arows, ainner, nrow, blen, ncol


def _nan_mat(rng, shape, nnz, nan):
    i0 = rng.integers(0, shape[0], nnz)
    i1 = rng.integers(0, shape[1], nnz)
    v = rng.uniform(-1, 1, nnz)
    v[rng.integers(0, nnz, max(1, nnz // 12))] = 0.0
    if nan:
        v[rng.integers(0, nnz, max(1, nnz // 15))] = np.nan
        v[rng.integers(0, nnz, max(1, nnz // 30))] = np.inf
    if nnz > 4:                                          # duplicates
        i0[:3], i1[:3] = i0[3], i1[3]
    return (i0.astype(np.int32), i1.astype(np.int32), v, shape)


# (its own: test_gpu_parity.py's _rand_vec zeroes an entry and returns an orc.Vec)
def _rand_vec(rng, n):
    idx = np.flatnonzero(rng.uniform(size=n) < 0.7)
    if idx.size == 0:
        idx = np.array([0])
    return (idx.astype(np.int32), rng.uniform(0.5, 2, idx.size), n)


def test_fuzzed_shapes_bit_identical_at_three_budgets(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(2026)
    shapes = [(1, 1, 1), (5, 1, 7), (60, 60, 60), (200, 17, 20000), (17, 400, 12000), (2, 3000, 9000), (64, 64, 70000),
              (90, 30, 200)]
    seen = dict(blocks_many=0, heavy=0, mid=0, permute=0, zero_nan=0)
    for case in range(48):
        m, k, n = shapes[case % len(shapes)]
        tA, tB = ("T" if case % 2 else "."), ("T" if case % 4 >= 2 else ".")
        nnz_a = max(1, int(m * k * rng.choice([0.05, 0.3, 0.9])))
        nnz_b = max(1, min(int(k * n * rng.choice([0.01, 0.1, 0.5])), 300000))
        A = _nan_mat(rng, (k, m) if tA == "T" else (m, k), nnz_a, nan=case % 3 == 0)
        B = _nan_mat(rng, (n, k) if tB == "T" else (k, n), nnz_b, nan=case % 5 == 0)
        pol = [capi.ADD, capi.LEAVE_ALONE, capi.REPLACE][case % 3]
        zn = case % 6 in (0, 3)
        flags = capi.SINK_ORDERED | (capi.SINK_PERMUTE if case % 4 == 1 else 0)
        kp = Keep()
        a, b = kp.coo(A), kp.coo(B)
        kw = dict(C_=float(rng.choice([1.0, -0.5, 3.0])), tA=tA, tB=tB, duplicate_policy=pol, zero_nan=zn, flags=flags,
                  scalei=kp.vec(_rand_vec(rng, m) if case % 2 else None),
                  scalej=kp.vec(_rand_vec(rng, k) if case % 3 == 1 else None),
                  scalek=kp.vec(_rand_vec(rng, n) if case % 4 == 2 else None))
        want, pres = _plain(ctx, a, b, **kw)
        model = _model_bounds(ctx, a, b, tA, tB, pol, zn)
        bound = sr.row_bounds(*model)
        lo = max(1, int(bound.max()) if bound.size else 1)
        for budget in (lo, 3 * lo, UNLIMITED):
            got, res, st = _stream(ctx, a, b, budget, **kw)
            assert _bits_equal(got, want), "case %d budget %d" % (case, budget)
            assert (res.shape0, res.shape1, res.nnz) == (pres.shape0, pres.shape1, pres.nnz)
            assert res.products == pres.products and not res.idx0 and not res.val
            assert st.blocks == sr.block_count(*model, budget), "case %d budget %d" % (case, budget)
            assert st.block_tuples == budget
            seen["blocks_many"] += st.blocks >= 5
        seen["heavy"] += pres.rows_heavy > 0
        seen["mid"] += pres.rows_mid > 0
        seen["permute"] += bool(flags & capi.SINK_PERMUTE)
        seen["zero_nan"] += zn
    print("stream fuzz coverage:", seen)
    assert seen["blocks_many"] >= 10 and seen["heavy"] >= 3 and seen["mid"] >= 5


def test_rmat14_against_the_oracle_in_ten_blocks_or_more(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(14)
    a = wl.rmat(14, seed=4)
    vals = rng.uniform(-1, 1, a[2].size)
    A = orc.Mat(a[0], a[1], vals, a[3])
    want = orc.multiply(A, A, rowwise=True, nthreads=8)
    kp = Keep()
    s = kp.coo((a[0], a[1], vals, a[3]))
    model = _model_bounds(ctx, s, s, ".", ".", capi.ADD, False)
    bound = sr.row_bounds(*model)
    budget = max(int(bound.max()), int(bound.sum()) // 12)
    got, res, st = _stream(ctx, s, s, budget, flags=capi.SINK_ORDERED)
    assert st.blocks >= 10 and st.blocks == sr.block_count(*model, budget)
    assert res.rows_heavy > 0 and res.rows_mid > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.int64), np.asarray(want[2]).view(np.int64))


def _rel_close(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.all(np.abs(got[2] - want[2]) <= 1e-12 * np.abs(want[2]))


def _wide_16k():
    rng = np.random.default_rng(8)
    m, k, ncol = 6, 96, 1 << 22
    ai0 = np.repeat(np.arange(m), k)
    ai1 = np.tile(np.arange(k), m)
    keep = rng.uniform(size=ai0.size) < 0.8
    A = (ai0[keep].astype(np.int32), ai1[keep].astype(np.int32), rng.uniform(0.1, 1, int(keep.sum())), (m, k))
    rows, cols = [], []
    for r in range(k):
        c = np.unique(np.concatenate([rng.integers(0, 90000, 1500), rng.integers(0, ncol, 400)]))
        rows.append(np.full(c.size, r))
        cols.append(c)
    bi0, bi1 = np.concatenate(rows), np.concatenate(cols)
    B = (bi0.astype(np.int32), bi1.astype(np.int32), rng.uniform(0.1, 1, bi0.size), (k, ncol))
    return A, B


@pytest.mark.parametrize("flags", [0, 8])
def test_default_flags_and_exact_pattern(ctx, flags):
    kp = Keep()
    r = wl.rmat(16, seed=3)
    s = kp.coo(r)
    want, pres = _plain(ctx, s, s, flags=flags)
    assert pres.rows_light > 0 and pres.rows_mid > 0 and pres.rows_heavy > 0
    got, res, st = _stream(ctx, s, s, max(1 << 20, pres.nnz // 6), flags=flags)
    assert st.blocks >= 3
    _rel_close(got, want)
    A, B = _wide_16k()
    a, b = kp.coo(A), kp.coo(B)
    want, pres = _plain(ctx, a, b, flags=flags)
    assert pres.cells_dense > 0 and pres.cells_hash > 0
    got, res, st = _stream(ctx, a, b, 1 << 18, flags=flags)
    assert st.blocks >= 2 and res.shape1 == 1 << 22
    _rel_close(got, want)
    p = wl.poisson2d(512)
    s = kp.coo(p)
    want, pres = _plain(ctx, s, s, flags=flags)
    got, res, st = _stream(ctx, s, s, pres.nnz // 5, flags=flags)
    assert st.blocks >= 5
    _rel_close(got, want)


def test_chained_and_prepared_operands(ctx):
    from spsparse_amd import capi
    kp = Keep()
    rng = np.random.default_rng(3)
    a = wl.rmat(12, seed=5)
    n = a[3][0]
    R = (rng.integers(0, n // 4, 3000).astype(np.int32), rng.integers(0, n, 3000).astype(np.int32), rng.uniform(-1, 1, 3000), (n // 4, n))
    r, s = kp.coo(R), kp.coo(a)
    T = ctx.multiply(r, s, flags=capi.SINK_ORDERED)
    t_before = ctx.fetch(T)
    t = capi.result_operand(T)
    want, _ = _plain(ctx, t, r, tB="T", flags=capi.SINK_ORDERED)          # (plain T * R^T writes the other set)
    T2 = ctx.multiply(r, s, flags=capi.SINK_ORDERED)                        # T again, in place for the streamed call
    t = capi.result_operand(T2)
    got, res, st = _stream(ctx, t, r, 1 << 12, tB="T", flags=capi.SINK_ORDERED)
    assert st.blocks >= 2 and _bits_equal(got, want)
    assert _bits_equal(ctx.fetch(T2), t_before)                             # T untouched, still fetchable
    # a prepared B used by two streamed calls
    pb = capi.Operand(ctx, s, role=capi.AS_B)
    try:
        want, _ = _plain(ctx, s, s, flags=capi.SINK_ORDERED)
        for budget in (1 << 14, UNLIMITED):
            got, res, st = _stream(ctx, s, pb.coo, budget, flags=capi.SINK_ORDERED)
            assert _bits_equal(got, want)
    finally:
        pb.close()


def test_errors_before_the_first_chunk(ctx):
    from spsparse_amd import capi
    kp = Keep()
    a = wl.rmat(10, seed=1)
    s = kp.coo(a)
    calls = []
    on_chunk = lambda i, j, v: calls.append(i.size)                         # noqa: E731
    model = _model_bounds(ctx, s, s, ".", ".", capi.ADD, False)
    mx = int(sr.row_bounds(*model).max())
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_stream(s, s, block_tuples=mx - 1, on_chunk=on_chunk)
    assert e.value.code == -5 and ("smallest budget that works is %d" % mx) in e.value.msg
    bad = kp.coo((a[0][:10], a[1][:10], a[2][:10], (a[3][0] + 3, a[3][1])))
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_stream(s, bad, on_chunk=on_chunk)
    assert e.value.code == -1
    oob = kp.coo((np.array([0, 5000], np.int32), np.array([0, 1], np.int32), np.array([1.0, 2.0]), a[3]))
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_stream(oob, s, on_chunk=on_chunk)
    assert e.value.code == -2
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_stream(s, s, flags=capi.SINK_ROWSTATS, on_chunk=on_chunk)
    assert e.value.code == -2
    assert calls == []
    # a callback that stops at its third chunk: the call returns 7, the context stays usable
    n = [0]

    def stop_third(i, j, v):
        n[0] += 1
        return 7 if n[0] == 3 else 0
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_stream(s, s, block_tuples=mx, on_chunk=stop_third)
    assert e.value.code == 7 and n[0] == 3
    want = orc.multiply(orc.Mat(*a), orc.Mat(*a), rowwise=True)
    res = ctx.multiply(s, s)
    got = ctx.fetch(res)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # re-entrant: any call on the context from inside the callback is refused
    codes = []

    def reenter(i, j, v):
        if not codes:
            try:
                ctx.multiply(s, s)
                codes.append(0)
            except capi.SpsamdError as ee:
                codes.append((ee.code, ee.msg))
    ctx.multiply_stream(s, s, on_chunk=reenter)
    assert codes and codes[0][0] == -2 and "busy" in codes[0][1]


def test_column_block_products_are_refused_before_delivery(ctx):
    """A heavy row and more than 2^25 columns (spsamd_multiply goes by column blocks): SPSAMD_EINVAL, no chunk."""
    from spsparse_amd import capi
    kp = Keep()
    rng = np.random.default_rng(5)
    ncol, k = 3 * (1 << 25) - 12345, 6000
    brow = np.repeat(np.arange(k, dtype=np.int32), 3)
    B = (brow, rng.integers(0, ncol, k * 3).astype(np.int32), rng.standard_normal(k * 3), (k, ncol))
    A = (np.ones(k, np.int32), np.arange(k, dtype=np.int32), rng.standard_normal(k), (3, k))
    calls = []
    with pytest.raises(capi.SpsamdError) as e:
        ctx.multiply_stream(kp.coo(A), kp.coo(B), on_chunk=lambda i, j, v: calls.append(1))
    assert e.value.code == -2 and "column blocks" in e.value.msg and calls == []
    # the window indices over the budget (index_budget_mb): refused too
    a = wl.rmat(15, seed=9)
    s = kp.coo(a)
    ctx.set_tuning("index_budget_mb", 1)
    try:
        with pytest.raises(capi.SpsamdError) as e:
            ctx.multiply_stream(s, s, on_chunk=lambda i, j, v: calls.append(1))
    finally:
        ctx.set_tuning("index_budget_mb", 0)
    assert e.value.code == -2 and calls == []
    # light rows at that width need no windows: streamed like any other product
    A2 = (np.array([0, 0, 2], np.int32), np.array([1, 2, 3], np.int32), np.array([1.0, 2.0, 3.0]), (3, k))
    want, _ = _plain(ctx, kp.coo(A2), kp.coo(B), flags=capi.SINK_ORDERED)
    got, res, st = _stream(ctx, kp.coo(A2), kp.coo(B), 6, flags=capi.SINK_ORDERED)
    assert _bits_equal(got, want) and st.blocks >= 2


def test_block_outputs_stay_within_two_budgets():
    """R-MAT 18 at a budget of 2^22: device memory sampled during the call grows by the two block output sets, the
    workspace and op(B)'s structures -- far less than the 16 B per tuple the plain path's output set takes."""
    from spsparse_amd import capi
    import torch
    kp = Keep()
    a = wl.rmat(18, seed=2)
    s = kp.coo(a)
    budget = 1 << 22
    count = [0, -1]                                      # tuples, last (i, j) seen as one key

    def consume(i, j, v):
        key = i.astype(np.int64) * (1 << 31) + j
        assert np.all(np.diff(key) > 0) and key[0] > count[1]
        count[1] = int(key[-1])
        count[0] += i.size
    torch.cuda.empty_cache()
    c = capi.Context(0)
    try:
        with _PeakMemory() as mem:
            res, st = c.multiply_stream(s, s, block_tuples=budget, on_chunk=consume)
        d = c.multiply(s, s, sink=capi.SINK_DIGEST)
    finally:
        c.close()
    grew = mem.peak - mem.base
    assert count[0] == res.nnz == d.nnz
    assert st.blocks >= 4 and st.max_block_nnz <= budget
    assert st.device_output_bytes <= 2 * 16 * budget + 6 * 256
    b_structures = 16 * a[2].size * 4                    # op(B)'s tuples, packed copy, window index and window-major copy
    assert grew <= st.device_output_bytes + res.workspace_bytes + b_structures + (256 << 20)
    assert grew < 16 * res.nnz // 4
    print("rmat18: nnz %d in %d blocks, device memory +%.2f GB (plain output %.1f GB), device %.1f ms, callback %.1f ms, wall %.1f ms"
          % (res.nnz, st.blocks, grew / 1e9, 16 * res.nnz / 1e9, st.ms_device, st.ms_callback, st.ms_wall))


# ---- full size: the C++ consumer of tests/cpp/test_stream.cpp through the template with stream_block_tuples

def _consumer(tmp_path):
    return build_cpp_test("stream", tmp_path, "-O2")


def _write_square(path, a, n):
    with open(path, "wb") as f:
        f.write(np.array([n, a[2].size], np.uint64).tobytes())
        for x, t in ((a[0], np.int32), (a[1], np.int32), (a[2], np.float64)):
            f.write(np.ascontiguousarray(x, t).tobytes())


def _run(cmd, timeout):
    t0 = time.time()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    print(out.stdout[-1000:], out.stderr[-1000:])
    assert out.returncode == 0, out.stdout[-1000:]
    w = out.stdout.split()
    return dict(count=int(w[w.index("count") + 1]), hash=int(w[w.index("hash") + 1]), ordered=w[w.index("ordered") + 1] == "1",
                wall=time.time() - t0)


def _rows(prefix, n):
    return (np.fromfile(prefix + ".nnz", np.int64, n), np.fromfile(prefix + ".hash", np.uint64, n),
            np.fromfile(prefix + ".sum", np.float64, n))


def _check_row_sums(got, a, n):
    want = pj.row_sums_by_linearity(a, a, n, n)
    nz = want != 0
    assert np.array_equal(got != 0, nz)                  # values are positive: a row is empty iff its sum is 0
    assert np.max(np.abs(got[nz] - want[nz]) / want[nz]) <= 1e-10


def test_cfg2_streamed_into_the_cpp_consumer(tmp_path):
    """cfg2 (R-MAT scale-20 A*A, 9.7e9 tuples) streamed at a budget of 2^28 into a C++ accumulator through the template:
    count, index hash and per-row counts and hashes equal the oracle's streaming digest, the order is strictly ascending
    across all chunks, per-row value sums within 1e-10 of linearity, and the device memory in use stays far below the
    155 GB the plain path's output set takes."""
    import torch
    exe = _consumer(tmp_path)
    n = 1 << 20
    a = wl.rmat(20, seed=1)
    path = os.path.join(str(tmp_path), "a.bin")
    _write_square(path, a, n)
    torch.cuda.empty_cache()
    with _PeakMemory() as mem:
        got = _run([exe, "--stream", path, str(1 << 28), os.path.join(str(tmp_path), "s")], timeout=1200)
    assert got["ordered"]
    rn, rh, rs = _rows(os.path.join(str(tmp_path), "s"), n)
    o = orc.multiply_digest(orc.Mat(*a[:3], (n, n)), orc.Mat(*a[:3], (n, n)), nthreads=_threads(), rowstats=True)
    assert got["count"] == o.nnz and got["hash"] == o.hash
    assert np.array_equal(rn, o.row_nnz) and np.array_equal(rh, o.row_hash)
    _check_row_sums(rs, a, n)
    assert mem.peak - mem.base < 155e9 / 4
    print("cfg2 streamed: %d tuples, %.1f s, device memory peak +%.1f GB" % (got["count"], got["wall"], (mem.peak - mem.base) / 1e9))


def test_product_larger_than_the_device(tmp_path):
    """The smallest R-MAT scale whose COO output (16 B per tuple) exceeds the device: 21.  Streamed into the C++
    consumer; count, index hash, row_nnz and row_hash equal the digest sink with ROWSTATS on the same product, and the
    per-row sums match linearity.  Both GPU steps run as processes of their own under a time limit."""
    import torch
    exe = _consumer(tmp_path)
    scale = 21
    n = 1 << scale
    a = wl.rmat(scale, seed=1)
    path = os.path.join(str(tmp_path), "a.bin")
    _write_square(path, a, n)
    total = torch.cuda.mem_get_info(0)[1]
    d = _run([exe, "--digest", path, os.path.join(str(tmp_path), "d")], timeout=600)
    assert d["count"] * 16 > total                      # nnz(C) x 16 B does not fit the device
    s = _run([exe, "--stream", path, str(1 << 28), os.path.join(str(tmp_path), "s")], timeout=1800)
    assert s["ordered"] and (s["count"], s["hash"]) == (d["count"], d["hash"])
    dn, dh, _ = _rows(os.path.join(str(tmp_path), "d"), n)
    sn, sh, ss = _rows(os.path.join(str(tmp_path), "s"), n)
    assert np.array_equal(sn, dn) and np.array_equal(sh, dh)
    _check_row_sums(ss, a, n)
    print("R-MAT %d: nnz(C) %d = %.0f GB of tuples on a %.0f GB device; streamed in %.1f s (digest %.1f s)"
          % (scale, s["count"], 16 * s["count"] / 1e9, total / 1e9, s["wall"], d["wall"]))
