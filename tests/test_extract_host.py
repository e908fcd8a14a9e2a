"""Pins tests/extract_ref.py, the host restatement of spsamd_extract, without a GPU: against dense slicing, against the
composition S_I * A * S_J^T through the test oracle (the only way to extract before this call existed), against a brute-force
loop for the (r, c, p) order -- and that the entry point is declared in every layer and exported by the cross-compiled
library."""
import ctypes
import os

import numpy as np

from oracle import binding as orc
from tests import add_ref as ar
from tests import extract_ref as er
from tests import select_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lists(rng, trial, nrow, ncol):
    kinds = er.LIST_KINDS
    return er.index_list(rng, kinds[trial % 6], nrow), er.index_list(rng, kinds[(trial // 6) % 6], ncol)


def test_unique_keys_equal_dense_slicing():
    rng = np.random.default_rng(31)
    for trial in range(216):
        shape = (int(rng.integers(1, 14)), int(rng.integers(1, 14)))
        t = '.' if trial % 4 < 2 else 'T'
        nrow, ncol = (shape[1], shape[0]) if t == 'T' else shape
        A = sr.unique_key_operand(rng, shape, int(rng.integers(0, 120)), special=0.0)
        S = sr.operand_S(A, t)
        I, J = _lists(rng, trial, nrow, ncol)
        D = np.zeros((nrow, ncol))
        D[S[0], S[1]] = S[2]
        Ii = np.arange(nrow) if I is None else I
        Jj = np.arange(ncol) if J is None else J
        want = D[np.ix_(Ii, Jj)]
        gi, gj, gv = er.extract_ref(S, I, J, nrow, ncol)
        got = np.zeros((len(Ii), len(Jj)))
        got[gi, gj] = gv
        assert np.array_equal(got, want), trial
        assert len(gv) == np.count_nonzero(want), trial             # every key once
        key = gi.astype(np.int64) * max(len(Jj), 1) + gj
        assert np.all(np.diff(key) > 0), trial                      # row-major


def test_equals_the_oracles_selection_products():
    """extract(A, I, J) == S_I * A * S_J^T through the restated reference algorithm, bit for bit: every sum has one term and
    0 + 1.0 * a, 0 + a * 1.0 are exact."""
    rng = np.random.default_rng(32)
    for trial in range(72):
        shape = (int(rng.integers(1, 12)), int(rng.integers(1, 12)))
        t = '.' if trial % 4 < 2 else 'T'
        nrow, ncol = (shape[1], shape[0]) if t == 'T' else shape
        A = ar.random_operand(rng, shape, int(rng.integers(1, 90)), special=0.0)
        A = (A[0], A[1], np.where(A[2] == 0, 1.5, A[2]))
        pol = trial % 3
        S = sr.operand_S(A, t, pol)
        I, J = _lists(rng, trial, nrow, ncol)
        want = er.extract_ref(S, I, J, nrow, ncol)
        si, sj = er.selection_matrix(I, nrow), er.selection_matrix(J, ncol)
        T = orc.multiply(orc.Mat(si[0], si[1], si[2], si[3]), orc.Mat(A[0], A[1], A[2], shape), tB=t, duplicate_policy=pol)
        G = orc.multiply(orc.Mat(T[0], T[1], T[2], T[3]), orc.Mat(sj[0], sj[1], sj[2], sj[3]), tB='T', duplicate_policy=pol)
        assert tuple(G[3]) == (len(si[0]), len(sj[0])), trial
        got = ar.consolidate(G[0], G[1], G[2])                      # the oracle appends in its loop order: row-major already
        assert ar.same_tuples(got, want), trial


def test_trusted_duplicates_and_unordered_rows_follow_r_c_p():
    rng = np.random.default_rng(33)
    for trial in range(60):
        shape = (int(rng.integers(1, 7)), int(rng.integers(1, 7)))
        t = '.' if trial % 2 else 'T'
        lead = 1 if t == 'T' else 0
        nrow, ncol = (shape[1], shape[0]) if lead else shape
        nnz = int(rng.integers(0, 40))
        i0 = rng.integers(0, shape[0], nnz).astype(np.int32)
        i1 = rng.integers(0, shape[1], nnz).astype(np.int32)
        v = sr.special_values(rng, nnz, 0.3)
        o = np.argsort(i1 if lead else i0, kind="stable")
        S = sr.operand_S((i0[o], i1[o], v[o]), t, sort0=lead)
        I, J = _lists(rng, trial, nrow, ncol)
        assert ar.same_tuples(er.extract_ref(S, I, J, nrow, ncol), er.extract_ref_loop(S, I, J, nrow, ncol)), trial


def test_by_hand():
    #      c0   c1   c2
    # r0   1    .    2
    # r1   .    3    .
    S = (np.array([0, 0, 1], np.int32), np.array([0, 2, 1], np.int32), np.array([1.0, 2.0, 3.0]))
    gi, gj, gv = er.extract_ref(S, [1, 0, 1], [2, 2, 0], 2, 3)
    assert gi.tolist() == [1, 1, 1] and gj.tolist() == [0, 1, 2] and gv.tolist() == [2.0, 2.0, 1.0]
    gi, gj, gv = er.extract_ref(S, None, [1], 2, 3)
    assert gi.tolist() == [1] and gj.tolist() == [0] and gv.tolist() == [3.0]
    assert all(len(x) == 0 for x in er.extract_ref(S, [], None, 2, 3))


def test_extract_is_declared_in_every_layer():
    from spsparse_amd import build, capi
    assert "k_extract.hip" in build.SOURCES
    assert "spsamd_extract" in capi.SYMBOLS
    assert callable(getattr(capi.Context, "extract", None))
    assert capi.extract_light_max < capi.extract_mid_max
    with open(os.path.join(ROOT, "include", "spsparse_amd.h")) as f:
        header = f.read()
    assert "int spsamd_extract(" in header and "SPSAMD_EXTRACT_ALL" in header and "extract_path" in header
    with open(os.path.join(ROOT, "include", "spsparse_amd", "multiply.hpp")) as f:
        assert "void extract(" in f.read()
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "spsamd_extract")
