"""Pins tests/select_ref.py, the host restatement of spsamd_select, without a GPU: top-k against a brute-force sorted() per
row, select and its complement as a partition of S, the identities between the predicates, S against the test oracle's
consolidate() -- and that the entry point is declared in every layer and exported by the cross-compiled library."""
import ctypes
import os

import numpy as np

from oracle import binding as orc
from tests import add_ref as ar
from tests import dense_ref as dr
from tests import select_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(rng, trial):
    shape = (int(rng.integers(1, 12)), int(rng.integers(1, 12)))
    nnz = int(rng.integers(0, 90))
    A = sr.unique_key_operand(rng, shape, nnz, ties=trial % 2 == 0) if trial % 3 else sr.duplicate_key_operand(rng, shape, nnz, ties=trial % 2 == 0)
    t = '.' if trial % 4 < 2 else 'T'
    return A, shape, t


def test_topk_equals_sorted_per_row():
    rng = np.random.default_rng(1)
    for trial in range(300):
        A, shape, t = _case(rng, trial)
        S = sr.operand_S(A, t, trial % 3, bool(trial % 5 == 0))
        for k in (0, 1, 2, 3, 5, 100):
            assert np.array_equal(sr.topk_mask(S[0], S[2], k), sr.topk_mask_loop(S[0], S[2], k)), (trial, k)


def test_select_and_complement_partition_S():
    rng = np.random.default_rng(2)
    for trial in range(200):
        A, shape, t = _case(rng, trial)
        nrow = shape[1] if t == 'T' else shape[0]
        S = sr.operand_S(A, t)
        for pred in sr.PREDICATES:
            ip = int(rng.integers(-3, 4)) if pred <= sr.OFFDIAG else int(rng.integers(0, 5))
            dp = float(rng.choice([0.0, 0.25, 1.0, np.inf]))
            a = sr.select_mask(S, nrow, pred, ip, dp, False)
            b = sr.select_mask(S, nrow, pred, ip, dp, True)
            assert a.shape == b.shape == S[2].shape and np.all(a ^ b), (trial, pred)


def test_topk_with_k_at_least_the_longest_row_keeps_S():
    rng = np.random.default_rng(3)
    for trial in range(100):
        A, shape, t = _case(rng, trial)
        S = sr.operand_S(A, t)
        longest = int(np.bincount(S[0]).max()) if len(S[0]) else 0
        assert sr.select_mask(S, max(shape), sr.ROW_TOPK, longest).all()
        assert sr.select_mask(S, max(shape), sr.ROW_TOPK, 10 ** 6).all()
        if longest:
            assert not sr.select_mask(S, max(shape), sr.ROW_TOPK, longest - 1).all()


def test_tril_and_triu_meet_in_diag():
    rng = np.random.default_rng(4)
    for trial in range(100):
        A, shape, t = _case(rng, trial)
        S = sr.operand_S(A, t)
        for d in (-2, -1, 0, 1, 3, 2 ** 40, -2 ** 40):
            lo, hi = sr.select_mask(S, 0, sr.TRIL, d), sr.select_mask(S, 0, sr.TRIU, d)
            assert np.array_equal(lo & hi, sr.select_mask(S, 0, sr.DIAG, d))
            assert np.array_equal(~(lo & hi), sr.select_mask(S, 0, sr.OFFDIAG, d))


def test_value_predicates_by_hand():
    nan = np.array([0x7FF0000000000001], np.uint64).view(np.float64)[0]           # the smallest NaN pattern
    rows = np.array([0, 0, 0, 0, 1, 1, 2], np.int32)
    cols = np.arange(7, dtype=np.int32)
    vals = np.array([1.0, -4.0, nan, 0.5, np.inf, 3.0, -0.0])
    S = (rows, cols, vals)
    assert sr.select_mask(S, 3, sr.ABS_GE, dparam=1.0).tolist() == [True, True, True, False, True, True, False]
    assert sr.select_mask(S, 3, sr.ABS_GE, dparam=np.inf).tolist() == [False, False, True, False, True, False, False]
    # row 0: m = 4 (the NaN does not count), t = 1; row 1: m = Inf, t = Inf; row 2: m = 0, t = 0
    assert sr.select_mask(S, 3, sr.ROW_REL, dparam=0.25).tolist() == [True, True, True, False, True, False, True]
    # theta = 0: row 1's threshold is 0 * Inf = NaN, above every non-NaN entry
    assert sr.select_mask(S, 3, sr.ROW_REL, dparam=0.0).tolist() == [True, True, True, True, False, False, True]
    # a NaN is the largest of its row; ties go to the lower position
    assert sr.select_mask(S, 3, sr.ROW_TOPK, 1).tolist() == [False, False, True, False, True, False, True]
    tie = (np.zeros(4, np.int32), np.arange(4, dtype=np.int32), np.array([2.0, -2.0, 2.0, -2.0]))
    assert sr.select_mask(tie, 1, sr.ROW_TOPK, 2).tolist() == [True, True, False, False]
    got = sr.select_ref(S, 3, sr.ROW_TOPK, 1)
    assert dr.same_bits(got[2], vals[[2, 4, 6]])                                   # values as stored, -0.0 and the NaN included


def test_S_equals_the_oracles_consolidate():
    rng = np.random.default_rng(5)
    for trial in range(120):
        A, shape, t = _case(rng, trial)
        pol, zn = trial % 3, bool(trial % 2)
        lead = 1 if t == 'T' else 0
        S = sr.operand_S(A, t, pol, zn)
        o0, o1, ov = orc.consolidate(A[0], A[1], A[2], lead, pol, zn)
        want = (o1, o0, ov) if lead else (o0, o1, ov)
        assert ar.same_tuples(S, want), trial
        # an operand that carries op()'s row order is S as stored
        As = ar.sort_storage(A, lead)
        S2 = sr.operand_S(As, t, pol, zn, sort0=lead)
        assert ar.same_tuples(S2, (As[1], As[0], As[2]) if lead else As)


def test_select_is_declared_in_every_layer():
    from spsparse_amd import build, capi
    assert "k_select.hip" in build.SOURCES
    assert "spsamd_select" in capi.SYMBOLS
    assert callable(getattr(capi.Context, "select", None))
    assert capi.select_light_max < capi.select_mid_max
    with open(os.path.join(ROOT, "include", "spsparse_amd.h")) as f:
        header = f.read()
    assert "int spsamd_select(" in header and "SPSAMD_SELECT_ROW_TOPK" in header and "select_path" in header
    with open(os.path.join(ROOT, "include", "spsparse_amd", "multiply.hpp")) as f:
        assert "void select(" in f.read()
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "spsamd_select")
