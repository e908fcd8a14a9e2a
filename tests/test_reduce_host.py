"""Pins tests/reduce_ref.py, the host restatement of spsamd_reduce, without a GPU: against dense numpy where the order of
summation is immaterial, SUM against dense_ref's multiply_dense with a vector of ones, MAX_ABS against the m_i inside
select_ref's ROW_REL, the post-operations against numpy's SSE division and square root on 10^5 doubles, the fast (rounds)
form against the loop -- and that the entry point is declared in every layer and exported by the cross-compiled library."""
import ctypes
import os

import numpy as np

from tests import add_ref as ar
from tests import dense_ref as dr
from tests import reduce_ref as rr
from tests import select_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(rng, trial, special=0.3):
    shape = (int(rng.integers(1, 12)), int(rng.integers(1, 12)))
    nnz = int(rng.integers(0, 90))
    kind = trial % 3
    sort0 = -1
    t = '.' if trial % 4 < 2 else 'T'
    lead = 1 if t == 'T' else 0
    if kind == 0:
        A = sr.unique_key_operand(rng, shape, nnz, special=special)
    elif kind == 1:
        A = sr.duplicate_key_operand(rng, shape, nnz)
    else:
        i0 = rng.integers(0, shape[0], nnz).astype(np.int32)
        i1 = rng.integers(0, shape[1], nnz).astype(np.int32)
        v = sr.special_values(rng, nnz, special)
        o = np.argsort(i1 if lead else i0, kind="stable")
        A, sort0 = (i0[o], i1[o], v[o]), lead
    return A, shape, t, sort0


def test_exact_values_equal_dense_numpy():
    """Unique keys and small integers scaled by a power of two: every partial sum is exact, so any order gives the same
    bits and dense numpy is a reference."""
    rng = np.random.default_rng(31)
    for trial in range(120):
        shape = (int(rng.integers(1, 14)), int(rng.integers(1, 14)))
        nnz = int(rng.integers(0, 120))
        i0, i1, _ = sr.unique_key_operand(rng, shape, nnz, special=0.0)
        v = rng.integers(-50, 51, len(i0)).astype(np.float64) * 0.25
        v[v == 0] = 3.0
        t = 'T' if trial % 2 else '.'
        D = np.zeros(shape)
        D[i0, i1] = v
        if t == 'T':
            D = D.T
        nrow = D.shape[0]
        S = sr.operand_S((i0, i1, v), t)
        present = (D != 0).sum(axis=1) > 0
        n = min(D.shape)
        diag = np.zeros(nrow)
        diag[:n] = np.diag(D)[:n]
        want = {rr.SUM: D.sum(axis=1), rr.SUM_ABS: np.abs(D).sum(axis=1), rr.SUM_SQ: (D * D).sum(axis=1),
                rr.MAX_ABS: np.abs(D).max(axis=1), rr.COUNT: (D != 0).sum(axis=1).astype(np.float64), rr.DIAG: diag}
        for op in rr.OPS:
            idx, val, dense = rr.reduce_ref(S, nrow, op)
            rows = np.flatnonzero(diag != 0) if op == rr.DIAG else np.flatnonzero(present)
            assert np.array_equal(idx, rows), (trial, op)
            assert np.array_equal(val, want[op][rows]), (trial, op)
            assert np.array_equal(dense, np.where(np.isin(np.arange(nrow), rows), want[op], 0.0)), (trial, op)
            with np.errstate(all="ignore"):
                assert dr.same_bits(rr.reduce_ref(S, nrow, op, rr.RSQRT)[1], 1.0 / np.sqrt(val)), (trial, op)


def test_sum_equals_multiply_dense_with_ones():
    rng = np.random.default_rng(32)
    for trial in range(150):
        A, shape, t, sort0 = _case(rng, trial)
        nrow, ncol = (shape[1], shape[0]) if t == 'T' else shape
        S = sr.operand_S(A, t, trial % 3, bool(trial % 5 == 0), sort0)
        Y = dr.apply_ref(S[0], S[1], S[2], np.ones(ncol), np.zeros(nrow))
        idx, val, dense = rr.reduce_ref(S, nrow, rr.SUM)
        assert dr.same_bits(dense[idx], Y[idx]), trial
        assert np.array_equal(idx, np.unique(S[0])), trial
        # rows without a tuple: +0.0 in both
        assert dr.same_bits(np.delete(dense, idx), np.delete(Y, idx))


def test_max_abs_equals_row_rels_m():
    rng = np.random.default_rng(33)
    for trial in range(150):
        A, shape, t, sort0 = _case(rng, trial)
        nrow = shape[1] if t == 'T' else shape[0]
        S = sr.operand_S(A, t, trial % 3, False, sort0)
        idx, val, dense = rr.reduce_ref(S, nrow, rr.MAX_ABS)
        assert dr.same_bits(dense, sr.row_max(S[0], S[2], nrow)), trial


def test_fast_form_equals_the_loop():
    rng = np.random.default_rng(34)
    for trial in range(150):
        A, shape, t, sort0 = _case(rng, trial)
        nrow = shape[1] if t == 'T' else shape[0]
        S = sr.operand_S(A, t, trial % 3, bool(trial % 2), sort0)
        for op in rr.OPS:
            for post in rr.POSTS:
                a, b = rr.reduce_ref(S, nrow, op, post), rr.reduce_fast(S, nrow, op, post)
                assert np.array_equal(a[0], b[0]) and dr.same_bits(a[1], b[1]) and dr.same_bits(a[2], b[2]), (trial, op, post)


def test_by_hand():
    snan = np.array([0xFFF4000000000123], np.uint64).view(np.float64)[0]
    rows = np.array([0, 0, 0, 1, 1, 3, 3, 3], np.int32)
    cols = np.array([2, 0, 1, 0, 1, 3, 0, 3], np.int32)
    vals = np.array([1e16, 1.0, -1e16, snan, 2.0, -0.0, 5.0, np.inf])
    S = (rows, cols, vals)
    idx, val, dense = rr.reduce_ref(S, 4, rr.SUM)
    assert idx.tolist() == [0, 1, 3]
    assert val[0] == 0.0                                    # (0 + 1e16) + 1 = 1e16; - 1e16 = 0: the order shows
    assert val[1:2].view(np.uint64)[0] == 0xFFFC000000000123        # 0 + sNaN: the right operand's NaN, quieted
    assert val[2] == np.inf and dense[2] == 0.0 and not np.signbit(dense[2])
    idx, val, _ = rr.reduce_ref(S, 4, rr.DIAG)
    assert idx.tolist() == [0, 1, 3] and val.tolist() == [1.0, 2.0, np.inf]
    idx, val, _ = rr.reduce_ref(S, 4, rr.MAX_ABS)
    assert val.tolist() == [1e16, 2.0, np.inf]              # the NaN of row 1 does not count
    idx, val, _ = rr.reduce_ref(S, 4, rr.COUNT, rr.RECIP)
    assert val.tolist() == [1.0 / 3.0, 0.5, 1.0 / 3.0]
    idx, val, _ = rr.reduce_ref(S, 4, rr.SUM_ABS, rr.SQRT)
    assert val[0] == np.sqrt(2e16) and val[1:2].view(np.uint64)[0] == 0x7FFC000000000123      # |sNaN|: sign cleared, then quieted
    # a row whose only tuples are off the diagonal does not appear under DIAG
    idx, val, dense = rr.reduce_ref((np.array([0, 1], np.int32), np.array([1, 1], np.int32), np.array([4.0, 9.0])), 2, rr.DIAG, rr.RSQRT)
    assert idx.tolist() == [1] and val.tolist() == [1.0 / 3.0] and dense.tolist() == [0.0, 1.0 / 3.0]


def test_post_operations_are_numpys_sse_results():
    """recip / sqrt of reduce_ref state their NaN rules themselves; on x86-64 numpy's own results carry the same bits, for
    10^5 doubles of every kind (so the device, held to reduce_ref, is held to divsd / sqrtsd)."""
    rng = np.random.default_rng(35)
    x = rr.post_probe_values(rng)
    assert x.size >= 100_000
    assert np.isnan(x).sum() > 1000 and (x < 0).sum() > 1000 and ((x != 0) & (np.abs(x) < 2.3e-308)).sum() > 1000
    with np.errstate(all="ignore"):
        d, s = 1.0 / x, np.sqrt(x)
    assert dr.same_bits(rr.recip(x), d)
    assert dr.same_bits(rr.sqrt(x), s)
    with np.errstate(all="ignore"):
        assert dr.same_bits(rr.post_apply(x, rr.RSQRT), 1.0 / np.sqrt(x))
    one = np.array([-0.0, -1.0, np.inf, -np.inf])
    assert dr.same_bits(rr.sqrt(one), np.array([-0.0, np.array([0xFFF8000000000000], np.uint64).view(np.float64)[0], np.inf,
                                                np.array([0xFFF8000000000000], np.uint64).view(np.float64)[0]]))
    assert dr.same_bits(rr.recip(one), np.array([-np.inf, -1.0, 0.0, -0.0]))


def test_reduce_is_declared_in_every_layer():
    from spsparse_amd import build, capi
    assert "k_reduce.hip" in build.SOURCES
    assert "spsamd_reduce" in capi.SYMBOLS
    assert callable(getattr(capi.Context, "reduce", None)) and callable(getattr(capi, "device_vec", None))
    assert capi.reduce_light_max == 64 and capi.reduce_chunk > 1
    assert (capi.REDUCE_SUM, capi.REDUCE_SUM_ABS, capi.REDUCE_SUM_SQ, capi.REDUCE_MAX_ABS, capi.REDUCE_COUNT, capi.REDUCE_DIAG) == rr.OPS
    assert (capi.POST_NONE, capi.POST_RECIP, capi.POST_SQRT, capi.POST_RSQRT) == rr.POSTS
    with open(os.path.join(ROOT, "include", "spsparse_amd.h")) as f:
        header = f.read()
    assert "int spsamd_reduce(" in header and "SPSAMD_REDUCE_DIAG" in header and "SPSAMD_POST_RSQRT" in header and "reduce_path" in header
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "spsamd_reduce")
