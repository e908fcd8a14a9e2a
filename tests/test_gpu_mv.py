"""spsamd_multiply_mv, and spsamd_multiply with a narrow op(B), on mid, heavy and dense-cell rows.  GPU only.

An MV product has no kernel of its own: V becomes a k x 1 device matrix and the light / mid / heavy machinery of the matrix
product runs with ONE output column.  A row of op(A) yields at most one scalar product per tuple, so the two older MV
tests (5 x 5 and m, k < 80) stay in the light class.  The inputs here (tests/mv_ref.py; tests/test_mv_host.py pins them
without a GPU) hold rows of every class and exactly at the class boundaries, and every test asserts the class and cell
counters it is meant to reach.

Comparator: the CPU oracle, orc.multiply_mv for MV and the row-wise checker for MM.  Bars:
  index sets identical in every mode (default-mode inputs are random reals: no sum cancels to rounding);
  SINK_ORDERED: values bit-identical (NaN counts as NaN: MV promises no payloads);
  default and EXACT_PATTERN: |got - want| <= 1e-12 * sum|terms| per entry, the bound from the oracle run on the absolute
    values of every operand (REL is BASELINE.json's north star, as in tests/test_gpu_parity.py);
  digest: nnz and hash equal, |sum - sum(want)| <= 2e-12 * sum(bound) (the per-entry bar summed, plus the summation's
    own rounding); with ROWSTATS row_nnz is 0 or 1 and row_hash mix64(i, 0) for MV.

What the counters report (MI355X): a heavy MV row has more than 4096 tuples of A, so it is a long row with one window
of P_r > 4096 products, above every dense_min the library allows: one dense cell per heavy row, no hash cell, under every
knob.  The same holds for MM with cols(op(B)) <= 8192: one window per row, so a heavy TILE row (<= 256 tuples of A
against full rows of B) is a dense cell too and products_tiles stays 0; only 8193 columns open a second window, whose
single column the tile kernels then serve (products_tiles > 0).
"""
import functools

import numpy as np
import pytest

from oracle import binding as orc
from tests import mv_ref as mr

pytestmark = pytest.mark.gpu

REL = 1e-12
K = 200000                      # inner dimension of the long-row cases (the two very long rows need k >= 150000)
K_CANCEL = 20000


@pytest.fixture(scope="module")
def ctx():
    from spsparse_amd import capi
    c = capi.Context()
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ inputs (seeded)

@functools.lru_cache(maxsize=None)
def long_a(signed=False, dups=0, zeros=0, tile_rows=0, k=K):
    rng = np.random.default_rng(1)
    return mr.long_row_matrix(rng, k, mr.row_lengths(rng, k), signed=signed, dups=dups, zeros=zeros, tile_rows=tile_rows)


@functools.lru_cache(maxsize=None)
def mv_cases():
    """name -> (A, V, arguments): the MV inputs whose rows must reach all three classes."""
    rng = np.random.default_rng(7)
    A, As, Ad = long_a(), long_a(signed=True), long_a(signed=True, dups=20000, zeros=5000)
    nrow = A.shape[0]
    cases = {
        "dense": (A, mr.dense_vec(rng, K), {}),
        "dense_T": (mr.transposed(A), mr.dense_vec(rng, K), {"tA": "T"}),
        "dense_signed": (As, mr.dense_vec(rng, K, signed=True), {}),
        "sparse": (Ad, mr.sparse_vec(rng, K, 0.3, signed=True),
                   {"C_": -2.5, "scalei": mr.scale_vec(rng, nrow), "scalej": mr.scale_vec(rng, K)}),
    }
    for name, pol in (("add", orc.ADD), ("leave_alone", orc.LEAVE_ALONE), ("replace", orc.REPLACE)):
        cases["messy_" + name] = (Ad, mr.messy_vec(rng, K, 2 * K),
                                  {"C_": -2.5, "duplicate_policy": pol, "scalei": mr.scale_vec(rng, nrow), "scalej": mr.scale_vec(rng, K, 0.9)})
    An = orc.Mat(As.idx0, As.idx1, As.val.copy(), As.shape)
    An.val[rng.integers(0, An.nnz, 30)] = np.nan
    Vn = mr.sparse_vec(rng, K, 0.9, signed=True)
    Vn.val[rng.integers(0, Vn.nnz, 3)] = np.nan
    Vn.val[rng.integers(0, Vn.nnz, 2000)] = 0.0
    for zn in (False, True):
        cases["nan_zero_nan_%d" % zn] = (An, Vn, {"zero_nan": zn})
    return cases


@functools.lru_cache(maxsize=None)
def narrow_a():
    return long_a(signed=True, tile_rows=6)


@functools.lru_cache(maxsize=None)
def narrow_case(n):
    """(B, arguments) of the narrow right operand with n columns; every other n is stored transposed and used with 'T'."""
    rng = np.random.default_rng(100 + n)
    B = mr.narrow_b(rng, K, n, 150000 if n <= 3 else 3000000, signed=True)
    kw = {"tB": "T" if mr.NARROW_N.index(n) % 2 else "."}
    if kw["tB"] == "T":
        B = mr.transposed(B)
    if n in (64, 257):
        kw["scalek"] = mr.scale_vec(rng, n)
    return B, kw


# ------------------------------------------------------------------------------------------------ calls and checks

def _vec(keep, V, sort0=None):
    from spsparse_amd import capi
    if V is None:
        return None
    s, k = capi.host_vec(V.idx, V.val, V.shape0, V.sort0 if sort0 is None else sort0)
    keep.append(k)
    return s


def _mv(ctx, A, V, sink=None, flags=0, **kw):
    """spsamd_multiply_mv on host operands (A: an orc.Mat or a ready Coo struct; V: an orc.Vec or a ready Vec struct).
    Returns (i, v, res); i and v are None for the digest sink."""
    from spsparse_amd import capi
    keep = []
    if isinstance(A, orc.Mat):
        a, k1 = capi.host_coo(A.idx0, A.idx1, A.val, A.shape, A.sort0)
        keep.append(k1)
    else:
        a = A
    v = _vec(keep, V) if isinstance(V, orc.Vec) else V
    sink = capi.SINK_COO if sink is None else sink
    res = ctx.multiply_mv(a, v, kw.get("C_", 1.0), _vec(keep, kw.get("scalei")), kw.get("tA", "."), _vec(keep, kw.get("scalej")),
                          kw.get("duplicate_policy", capi.ADD), kw.get("zero_nan", False), sink, flags)
    nrow = a.shape1 if kw.get("tA", ".") == "T" else a.shape0
    assert (res.shape0, res.shape1) == (nrow, 0)               # rank-1 result: ret.set_shape({rows})
    assert not res.idx1                                        # ... with one index array
    if sink != capi.SINK_COO:
        return None, None, res
    i, j, val = ctx.fetch(res)
    assert not j.any()
    assert np.all(np.diff(i) > 0)                              # ascending, every row once
    return i, val, res


def _mm(ctx, A, B, sink=None, flags=0, **kw):
    from spsparse_amd import capi
    keep = []
    a, k1 = capi.host_coo(A.idx0, A.idx1, A.val, A.shape, A.sort0)
    b, k2 = capi.host_coo(B.idx0, B.idx1, B.val, B.shape, B.sort0)
    sink = capi.SINK_COO if sink is None else sink
    res = ctx.multiply(a, b, kw.get("C_", 1.0), _vec(keep, kw.get("scalei")), kw.get("tA", "."), _vec(keep, kw.get("scalej")),
                       kw.get("tB", "."), _vec(keep, kw.get("scalek")), kw.get("duplicate_policy", capi.ADD),
                       kw.get("zero_nan", False), sink, flags)
    del k1, k2
    if sink != capi.SINK_COO:
        return None, None, None, res
    return ctx.fetch(res) + (res,)


def _abs_kw(kw):
    out = dict(kw)
    for s in ("scalei", "scalej", "scalek"):
        if out.get(s) is not None:
            out[s] = mr.absolute(out[s])
    if "C_" in out:
        out["C_"] = abs(out["C_"])
    return out


@functools.lru_cache(maxsize=None)
def _mv_want(name):
    """(want, bound) of an MV case: the oracle's tuples, and per wanted tuple the sum of |terms| (the oracle run on the
    absolute values; its pattern holds the wanted one: positive terms never cancel)."""
    A, V, kw = mv_cases()[name]
    wi, _, wv, _ = orc.multiply_mv(A, V, **kw)
    bi, _, bv, _ = orc.multiply_mv(mr.absolute(A), mr.absolute(V), **_abs_kw(kw))
    if np.isnan(bv).any():                                     # (NaN inputs: no bound there; those cases compare exactly)
        return (wi, wv), None
    assert np.all(np.isin(wi, bi))
    return (wi, wv), bv[np.searchsorted(bi, wi)]


def _assert_tuples(got, want, bound=None, exact=False):
    gi, gv = got[:2]
    wi, wv = want
    assert len(gi) == len(wi) and np.array_equal(gi, wi)
    if exact:
        assert np.array_equal(gv, wv, equal_nan=True)
    else:
        err = np.abs(gv - wv)
        print("max |got - want| / bound = %.3g" % (np.max(err / bound) if len(wv) else 0.0))
        assert np.all(err <= REL * bound)


def _assert_classes(res, rc, nrow):
    """The counters of the result against the numpy count (a test that silently stayed light fails here)."""
    print("rows l/m/h = %d/%d/%d cells dense/hash = %d/%d products = %d tiles = %d" % (
        res.rows_light, res.rows_mid, res.rows_heavy, res.cells_dense, res.cells_hash, res.products, res.products_tiles))
    assert res.products == rc.total
    if rc.all_light:                                           # the direct kernel: every row of op(A) is reported light
        assert (res.rows_light, res.rows_mid, res.rows_heavy) == (nrow, 0, 0)
        return
    assert (res.rows_light, res.rows_mid, res.rows_heavy) == (rc.rows_light, rc.rows_mid, rc.rows_heavy)
    assert (res.products_light, res.products_mid, res.products_heavy) == (rc.products_light, rc.products_mid, rc.products_heavy)


def _assert_mv_cells(res):
    """One window of more than 4096 products per heavy row, above every dense_min: one dense cell each, no hash cell."""
    assert res.rows_heavy > 0 and res.rows_mid > 0 and res.rows_light > 0
    assert res.cells_dense == res.rows_heavy and res.cells_hash == 0
    assert res.products_dense == res.products_heavy and res.products_tiles == 0


def _classes(name):
    A, V, kw = mv_cases()[name]
    rc = mr.row_classes(A, V, tA=kw.get("tA", "."), scalei=kw.get("scalei"), scalej=kw.get("scalej"),
                        duplicate_policy=kw.get("duplicate_policy", orc.ADD), zero_nan=kw.get("zero_nan", False))
    return rc, (A.shape[1] if kw.get("tA") == "T" else A.shape[0])


def _assert_digest(d, want, bound):
    cnt, _, h = orc.digest(want[0], None, want[1])
    assert d.nnz == cnt and d.hash == h
    if bound is not None:
        assert abs(d.sum - float(np.sum(want[1]))) <= 2e-12 * float(np.sum(bound))


# ------------------------------------------------------------------------------------------------ MV

@pytest.mark.parametrize("name", ["dense", "dense_T"])
def test_mv_dense_v_all_classes(ctx, name):
    """Case 1: every index of V present, so P_r is the row's length: rows exactly at 64 / 65 and 4096 / 4097 products, the
    150000- and 200000-tuple rows; default flags; stored plain and transposed ('T')."""
    A, V, kw = mv_cases()[name]
    want, bound = _mv_want(name)
    got = _mv(ctx, A, V, **kw)
    _assert_tuples(got, want, bound)
    rc, nrow = _classes(name)
    assert all(rc.at(p) >= 1 for p in (64, 65, 4096, 4097))
    _assert_classes(got[2], rc, nrow)
    _assert_mv_cells(got[2])
    assert got[2].nnz_a == A.nnz and got[2].nnz_b == K
    print("ms_total %.3f ms_dense %.3f" % (got[2].ms_total, got[2].ms_dense))


def test_mv_ordered_is_bit_exact_on_signed_values(ctx):
    """Case 2: SINK_ORDERED sums in ascending k like the reference: bit-identical on every row, the 150000- and
    200000-tuple rows included.  EXACT_PATTERN and the default mode on the same signed input: same rows, values to the bound."""
    from spsparse_amd import capi
    A, V, kw = mv_cases()["dense_signed"]
    want, bound = _mv_want("dense_signed")
    got = _mv(ctx, A, V, flags=capi.SINK_ORDERED, **kw)
    _assert_tuples(got, want, exact=True)
    rc, nrow = _classes("dense_signed")
    _assert_classes(got[2], rc, nrow)
    _assert_mv_cells(got[2])
    for flags in (0, capi.SINK_EXACT_PATTERN):
        g = _mv(ctx, A, V, flags=flags, **kw)
        _assert_tuples(g, want, bound)
        _assert_mv_cells(g[2])
    d = _mv(ctx, A, V, sink=capi.SINK_DIGEST, flags=capi.SINK_ORDERED, **kw)[2]
    _assert_digest(d, want, bound)


def test_mv_exact_cancellation(ctx):
    """Case 3: against an all-ones V, rows of (+x, -x) pairs (0 in every order), rows of (1e16, 1, -1e16) triples (0 only in
    ascending k) and rows of (1e16, -1e16, 1) triples (1 in ascending k) -- in light, mid and heavy rows.  Under ORDERED
    and under EXACT_PATTERN the rows the reference drops are dropped and the kept rows carry the reference's value."""
    from spsparse_amd import capi
    C, kinds = mr.cancel_matrix(K_CANCEL)
    V = mr.ones_vec(K_CANCEL)
    wi, _, wv, _ = orc.multiply_mv(C, V)
    assert wi.tolist() == [r for r, kind in enumerate(kinds) if kind == "kept"] and np.all(wv == 1.0)
    rc = mr.row_classes(C, V)
    for flags in (capi.SINK_ORDERED, capi.SINK_EXACT_PATTERN):
        gi, gv, res = _mv(ctx, C, V, flags=flags)
        assert (res.rows_light, res.rows_mid, res.rows_heavy) == (6, 6, 6) and res.products == rc.total
        assert res.cells_dense == 6 and res.cells_hash == 0
        assert np.array_equal(gi, wi), flags
        assert np.array_equal(gv, wv), flags                   # ORDERED: by definition; EXACT_PATTERN: a re-evaluated sum is the reference's
        d = _mv(ctx, C, V, sink=capi.SINK_DIGEST, flags=flags)[2]
        assert (d.nnz, d.hash, d.sum) == (len(wi), orc.digest(wi, None, wv)[2], float(len(wi)))


@pytest.mark.parametrize("name", ["sparse", "messy_add", "messy_leave_alone", "messy_replace"])
def test_mv_sparse_and_messy_v_with_scales(ctx, name):
    """Case 4: a V of 30 % of the indices, and a V with duplicates and explicit zeros under the three duplicate policies;
    A with duplicates and zeros; scalei / scalej with absent and zero entries; C = -2.5.  Rows whose matches are all
    removed vanish; the product count is the numpy count on the consolidated operands."""
    from spsparse_amd import capi
    A, V, kw = mv_cases()[name]
    want, bound = _mv_want(name)
    rc, nrow = _classes(name)
    assert 0 < len(want[0]) < (rc.a_len > 0).sum()             # some rows vanish: absent or zero scalei, no match left
    got = _mv(ctx, A, V, **kw)
    _assert_tuples(got, want, bound)
    _assert_classes(got[2], rc, nrow)
    _assert_mv_cells(got[2])
    ca = orc.consolidate(A.idx0, A.idx1, A.val, 0, kw.get("duplicate_policy", orc.ADD))
    cv = orc.consolidate(V.idx, None, V.val, 0, kw.get("duplicate_policy", orc.ADD))
    assert got[2].nnz_a == len(ca[0]) and got[2].nnz_b == len(cv[0])
    g = _mv(ctx, A, V, flags=capi.SINK_ORDERED, **kw)          # duplicates are merged in storage order like the reference's: bit for bit
    _assert_tuples(g, want, exact=True)


@pytest.mark.parametrize("zero_nan", [False, True])
def test_mv_nan_values_and_zero_nan(ctx, zero_nan):
    """Case 5: NaNs in A and in an unsorted V that also holds explicit zeros, zero_nan on and off: the same rows, NaN in
    the same places, every other value bit-identical (ORDERED)."""
    from spsparse_amd import capi
    name = "nan_zero_nan_%d" % zero_nan
    A, V, kw = mv_cases()[name]
    want, _ = _mv_want(name)
    assert np.isnan(want[1]).any() and not np.isnan(want[1]).all()
    got = _mv(ctx, A, V, flags=capi.SINK_ORDERED, **kw)
    _assert_tuples(got, want, exact=True)
    rc, nrow = _classes(name)
    _assert_classes(got[2], rc, nrow)
    _assert_mv_cells(got[2])
    g = _mv(ctx, A, V, **kw)                                  # arrival order: NaN stays NaN
    assert np.array_equal(g[0], want[0]) and np.array_equal(np.isnan(g[1]), np.isnan(want[1]))


def test_mv_sorted_v_is_taken_as_stored_under_zero_nan(ctx):
    """Case 5, the sort0 == 0 vectors: the reference consolidates V by its own order {0} (multiply_sparse.hpp:313), and
    Consolidate<> takes a V that carries it as stored (algorithm.hpp:360) -- a leading NaN or an explicit zero stays,
    also under zero_nan.  The expected values are the oracle's, pinned in tests/test_mv_host.py: NaN against 2.0.
    (The device once consolidated the k x 1 stand-in for V as if it were a matrix B, whose reference order is the other
    dimension, re-filtered it under zero_nan and returned 2.0 for the sorted V as well.)"""
    from spsparse_amd import capi
    A = orc.Mat([0, 0], [0, 1], [1., 1.], (1, 2))
    Ai = orc.Mat([0, 0], [0, 1], [np.inf, 1.], (1, 2))
    for zn in (False, True):
        for X, vals in ((A, [np.nan, 2.0]), (Ai, [0.0, 2.0])):
            for sort0 in (0, -1):
                V = orc.Vec([0, 1], vals, 2, sort0)
                wi, _, wv, _ = orc.multiply_mv(X, V, zero_nan=zn)
                gi, gv, _ = _mv(ctx, X, V, zero_nan=zn, flags=capi.SINK_ORDERED)
                assert np.array_equal(gi, wi) and np.array_equal(gv, wv, equal_nan=True), (zn, vals, sort0, gv, wv)
    g = _mv(ctx, A, orc.Vec([0, 1], [np.nan, 2.0], 2, 0), zero_nan=True)
    assert g[0].tolist() == [0] and np.isnan(g[1][0])
    g = _mv(ctx, A, orc.Vec([0, 1], [np.nan, 2.0], 2, -1), zero_nan=True)
    assert g[0].tolist() == [0] and g[1].tolist() == [2.0]
    # the same on long rows: a sorted dense V with a leading NaN run and zeros; rows that miss the NaNs stay finite
    rng = np.random.default_rng(3)
    Al = long_a(signed=True)
    val = rng.uniform(0.5, 2.0, K)
    val[:2] = np.nan
    val[rng.integers(2, K, 500)] = 0.0
    V = orc.Vec(np.arange(K), val, K, 0)
    for zn in (False, True):
        wi, _, wv, _ = orc.multiply_mv(Al, V, zero_nan=zn)
        assert np.isnan(wv).any() and not np.isnan(wv).all()
        gi, gv, res = _mv(ctx, Al, V, zero_nan=zn, flags=capi.SINK_ORDERED)
        assert np.array_equal(gi, wi) and np.array_equal(gv, wv, equal_nan=True)
        assert res.nnz_b == K and res.rows_heavy > 0 and res.cells_dense == res.rows_heavy


def test_mv_device_resident_operands(ctx):
    """Case 6: V in device memory (SPSAMD_MEM_DEVICE), A in device memory, both: the tuples of the host-operand call."""
    import torch
    from spsparse_amd import capi
    A, V, kw = mv_cases()["dense_signed"]
    want, bound = _mv_want("dense_signed")
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(x).to(dev) for x in (A.idx0, A.idx1, A.val, V.idx, V.val)]
    torch.cuda.synchronize()
    Ad = capi.device_coo(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), A.nnz, A.shape)
    Vd = capi.Vec(t[3].data_ptr(), t[4].data_ptr(), V.nnz, K, -1, capi.MEM_DEVICE)
    host = _mv(ctx, A, V, flags=capi.SINK_ORDERED)
    _assert_tuples(host, want, exact=True)
    for a, v in ((A, Vd), (Ad, V), (Ad, Vd)):
        g = _mv(ctx, a, v, flags=capi.SINK_ORDERED)
        assert np.array_equal(g[0], host[0]) and np.array_equal(g[1], host[1])
        _assert_mv_cells(g[2])
        g = _mv(ctx, a, v)
        _assert_tuples(g, want, bound)
    # the operands are read, never written
    torch.cuda.synchronize()
    assert np.array_equal(t[3].cpu().numpy(), V.idx) and np.array_equal(t[4].cpu().numpy(), V.val)
    assert np.array_equal(t[1].cpu().numpy(), A.idx1) and np.array_equal(t[2].cpu().numpy(), A.val)


def test_mv_sinks_and_flags(ctx):
    """Case 7: the digest sink, with and without row statistics; SINK_PERMUTE changes nothing (a rank-1 result has nothing
    to permute); a prepared A gives the same tuples; the MM product after an MV call is still right, and so is one chained
    from its result (the rank-1 result is not taken for an operand of the context's own)."""
    from spsparse_amd import capi
    A, V, kw = mv_cases()["dense"]
    want, bound = _mv_want("dense")
    nrow = A.shape[0]
    for flags in (0, capi.SINK_ROWSTATS):
        d = _mv(ctx, A, V, sink=capi.SINK_DIGEST, flags=flags)[2]
        _assert_digest(d, want, bound)
        _assert_mv_cells(d)
        if flags:
            rn = ctx.to_host(d.row_nnz, nrow, np.int64)
            rh = ctx.to_host(d.row_hash, nrow, np.uint64)
            rs = ctx.to_host(d.row_sum, nrow, np.float64)
            present = np.zeros(nrow, bool)
            present[want[0]] = True
            assert np.array_equal(rn, present.astype(np.int64))
            assert np.array_equal(rh, np.where(present, orc.mix64(np.arange(nrow), np.zeros(nrow, np.int64)), np.uint64(0)))
            assert np.all(np.abs(rs[want[0]] - want[1]) <= REL * bound) and not rs[~present].any()
    As, Vs, _ = mv_cases()["dense_signed"]
    ws, _ = _mv_want("dense_signed")
    g = _mv(ctx, As, Vs, flags=capi.SINK_PERMUTE | capi.SINK_ORDERED)
    _assert_tuples(g, ws, exact=True)
    g = _mv(ctx, A, V, flags=capi.SINK_PERMUTE)
    _assert_tuples(g, want, bound)
    d = _mv(ctx, A, V, sink=capi.SINK_DIGEST, flags=capi.SINK_PERMUTE)[2]
    _assert_digest(d, want, bound)
    # a prepared A
    s, keep = capi.host_coo(As.idx0, As.idx1, As.val, As.shape)
    op = capi.Operand(ctx, s, '.', capi.AS_A)
    try:
        g = _mv(ctx, op.coo, Vs, flags=capi.SINK_ORDERED)
        _assert_tuples(g, ws, exact=True)
        _assert_mv_cells(g[2])
        assert g[2].nnz_a == As.nnz
    finally:
        op.close()
    # MV, then MM on the same context, then a product chained from that result
    rng = np.random.default_rng(4)
    X = orc.Mat(rng.integers(0, 60, 900), rng.integers(0, 70, 900), rng.uniform(0.1, 1, 900), (60, 70))
    Y = orc.Mat(rng.integers(0, 70, 900), rng.integers(0, 50, 900), rng.uniform(0.1, 1, 900), (70, 50))
    Z = orc.Mat(rng.integers(0, 50, 400), rng.integers(0, 8, 400), rng.uniform(0.1, 1, 400), (50, 8))
    w1 = orc.multiply(X, Y, rowwise=True)
    w2 = orc.multiply(orc.Mat(w1[0], w1[1], w1[2], (60, 50)), Z, rowwise=True)
    _mv(ctx, A, V)
    x, kx = capi.host_coo(X.idx0, X.idx1, X.val, X.shape)
    y, ky = capi.host_coo(Y.idx0, Y.idx1, Y.val, Y.shape)
    z, kz = capi.host_coo(Z.idx0, Z.idx1, Z.val, Z.shape)
    r1 = ctx.multiply(x, y, flags=capi.SINK_ORDERED)
    f1 = ctx.fetch(r1)
    assert all(np.array_equal(a, b) for a, b in zip(f1, w1[:3]))
    r2 = ctx.multiply(capi.result_operand(r1), z, flags=capi.SINK_ORDERED)
    f2 = ctx.fetch(r2)
    assert all(np.array_equal(a, b) for a, b in zip(f2, w2[:3]))
    mvres = _mv(ctx, As, Vs, flags=capi.SINK_ORDERED)          # ... and an MV call after a chained product
    _assert_tuples(mvres, ws, exact=True)
    r3 = ctx.multiply(x, y, flags=capi.SINK_ORDERED)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.fetch(r3), w1[:3]))


@pytest.mark.parametrize("knobs", [{"window": 16384}, {"xcd": 0}, {"xcd": 1}, {"long_dense_min": 4096, "long_cap": 4096}, {"no_wmajor": 1}],
                         ids=lambda k: ",".join("%s=%d" % kv for kv in k.items()))
def test_mv_under_tuning_knobs(ctx, knobs):
    """Case 8: the dense-V product under the knobs that choose between equivalent kernels: the same tuples every time
    (ORDERED: bit for bit; default: to the bound), and still one dense cell per heavy row."""
    from spsparse_amd import capi
    A, V, kw = mv_cases()["dense_signed"]
    want, bound = _mv_want("dense_signed")
    for k, v in knobs.items():
        ctx.set_tuning(k, v)
    try:
        g0 = _mv(ctx, A, V)
        g1 = _mv(ctx, A, V, flags=capi.SINK_ORDERED)
        d = _mv(ctx, A, V, sink=capi.SINK_DIGEST)[2]
    finally:
        for k in knobs:
            ctx.set_tuning(k, 2 if k == "xcd" else 0)
    _assert_tuples(g0, want, bound)
    _assert_tuples(g1, want, exact=True)
    _assert_digest(d, want, bound)
    rc, nrow = _classes("dense_signed")
    for res in (g0[2], g1[2], d):
        _assert_classes(res, rc, nrow)
        _assert_mv_cells(res)
    if "window" in knobs:
        assert g0[2].window == 16384


def test_mv_all_light_both_paths(ctx):
    """Case 8, light_path: rows of at most 64 tuples take the direct kernel (every row reported light); light_path = 1
    sends them through the symbolic phase and the binned light kernels instead.  Both sum in ascending k: bit-identical."""
    from spsparse_amd import capi
    rng = np.random.default_rng(6)
    k = 5000
    lens = np.concatenate([[0, 1, 2, 63, 64], rng.integers(1, 65, 200)])
    A = mr.long_row_matrix(rng, k, lens, signed=True)
    V = mr.dense_vec(rng, k, signed=True)
    wi, _, wv, _ = orc.multiply_mv(A, V)
    rc = mr.row_classes(A, V)
    assert rc.all_light and rc.rows_light == len(lens) - 1
    g = _mv(ctx, A, V)
    _assert_tuples(g, (wi, wv), exact=True)
    _assert_classes(g[2], rc, len(lens))
    ctx.set_tuning("light_path", 1)
    try:
        g = _mv(ctx, A, V)
        d = _mv(ctx, A, V, sink=capi.SINK_DIGEST)[2]
    finally:
        ctx.set_tuning("light_path", 0)
    _assert_tuples(g, (wi, wv), exact=True)
    assert (g[2].rows_light, g[2].rows_mid, g[2].rows_heavy) == (rc.rows_light, 0, 0) and g[2].products == rc.total
    assert (d.nnz, d.hash) == (len(wi), orc.digest(wi, None, wv)[2])


def test_mv_errors_leave_the_context_usable(ctx):
    """Case 10: a V index out of bounds, a V with nnz > 0 and a NULL array, the inner-dimension text under 'T' -- each
    followed by a good call."""
    from spsparse_amd import capi
    A = orc.Mat([0, 0, 1], [0, 2, 1], [1., 2., 3.], (2, 3))
    V = orc.Vec([0, 1, 2], [1., 1., 1.], 3)

    def good():
        gi, gv, _ = _mv(ctx, A, V)
        assert gi.tolist() == [0, 1] and gv.tolist() == [3., 3.]

    good()
    for bad in ([0, 3], [-1, 1]):
        with pytest.raises(capi.SpsamdError, match="out of bounds") as e:
            _mv(ctx, A, orc.Vec(bad, [1., 1.], 3))
        assert e.value.code == -2
        good()
    with pytest.raises(capi.SpsamdError, match="null array") as e:
        _mv(ctx, A, capi.Vec(None, None, 2, 3, -1, capi.MEM_HOST))
    assert e.value.code == -2
    good()
    with pytest.raises(capi.SpsamdError, match=r"Inner dimensions for A \(2\) and V \(3\) must match!") as e:
        _mv(ctx, A, V, tA="T")
    assert e.value.code == -1
    good()
    gi, gv, _ = _mv(ctx, A, orc.Vec([0, 1], [1., 1.], 2), tA="T")
    assert gi.tolist() == [0, 1, 2] and gv.tolist() == [1., 3., 2.]


# ------------------------------------------------------------------------------------------------ MM, narrow op(B)

def _key(i, j):
    return i.astype(np.int64) * (1 << 32) + j


@pytest.mark.parametrize("n", mr.NARROW_N)
def test_mm_narrow_right_operand(ctx, n):
    """Case 9: the long-row A (plus six rows of 200 ... 256 tuples on the full rows of B) times a B of n columns: the
    output bound per row is n, far below P_r, and the one window is partial.  Default mode to the bound, ORDERED bit
    for bit, ORDERED | PERMUTE the same tuples with the indices swapped, the digest.  n = 1 equals the MV result."""
    from spsparse_amd import capi
    A = narrow_a()
    B, kw = narrow_case(n)
    wi, wj, wv, wshape = orc.multiply(A, B, rowwise=True, nthreads=8, **kw)
    assert tuple(wshape) == (A.shape[0], n) and len(wi) > 0
    bi, bj, bv, _ = orc.multiply(mr.absolute(A), mr.absolute(B), rowwise=True, nthreads=8, **_abs_kw(kw))
    assert np.all(np.isin(_key(wi, wj), _key(bi, bj)))
    bound = bv[np.searchsorted(_key(bi, bj), _key(wi, wj))]

    rc = mr.row_classes(A, B, tB=kw["tB"])
    gi, gj, gv, res = _mm(ctx, A, B, **kw)
    assert (res.shape0, res.shape1) == (A.shape[0], n)
    assert np.array_equal(gi, wi) and np.array_equal(gj, wj)
    err = np.abs(gv - wv)
    print("n = %d: max |got - want| / bound = %.3g" % (n, np.max(err / bound)))
    assert np.all(err <= REL * bound)
    _assert_classes(res, rc, A.shape[0])
    assert res.rows_heavy > 0 and res.cells_dense > 0
    if n <= 8192:
        # one window per row: every heavy row's window holds P_r > 4096 products, above every dense_min -- a dense cell,
        # also for the heavy TILE rows (<= 256 tuples of A; 200 x 63 products and more from n = 63 on)
        assert res.cells_dense == res.rows_heavy and res.cells_hash == 0 and res.products_tiles == 0
    else:
        # 8193 columns: a second window of one column, which the tile rows' few products there reach through the tile kernels
        assert res.cells_dense >= res.rows_heavy and res.products_tiles > 0
    if n >= 63:
        assert rc.tile_rows_heavy >= 6

    oi, oj, ov, ores = _mm(ctx, A, B, flags=capi.SINK_ORDERED, **kw)
    assert np.array_equal(oi, wi) and np.array_equal(oj, wj) and np.array_equal(ov, wv)
    assert ores.rows_heavy == rc.rows_heavy and ores.cells_dense > 0
    pi, pj, pv, pres = _mm(ctx, A, B, flags=capi.SINK_ORDERED | capi.SINK_PERMUTE, **kw)
    assert (pres.shape0, pres.shape1) == (n, A.shape[0])
    assert np.array_equal(pi, wj) and np.array_equal(pj, wi) and np.array_equal(pv, wv)
    d = _mm(ctx, A, B, sink=capi.SINK_DIGEST, **kw)[3]
    cnt, _, h = orc.digest(wi, wj, wv)
    assert d.nnz == cnt and d.hash == h
    assert abs(d.sum - float(np.sum(wv))) <= 2e-12 * float(np.sum(bound))
    assert d.rows_heavy == rc.rows_heavy and d.cells_dense > 0

    if n == 1:
        b0 = B.idx1 if kw["tB"] == "T" else B.idx0
        V = orc.Vec(b0, B.val, K)
        mi, mv_, mres = _mv(ctx, A, V, flags=capi.SINK_ORDERED)
        assert np.array_equal(mi, oi) and np.array_equal(mv_, ov) and not oj.any()
        assert (mres.rows_light, mres.rows_mid, mres.rows_heavy, mres.cells_dense, mres.products) == \
            (ores.rows_light, ores.rows_mid, ores.rows_heavy, ores.cells_dense, ores.products)
