"""multiply_sampled without a GPU: the host restatement (tests/sampled_ref.py) pinned to hand-worked cases, the vectorised
form equal to the tuple-by-tuple loop, and the entry point present in the library, the header and the Python binding."""
import ctypes
import os

import numpy as np

from tests import dense_ref as dr
from tests import sampled_ref as sr

NAN, INF = np.nan, np.inf
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def nan_with(payload):
    x = np.array([0.0])
    x.view(np.uint64)[0] = payload
    return x[0]


def both(*args, **kw):
    a, b = sr.sample_loop(*args, **kw), sr.sample_ref(*args, **kw)
    assert dr.same_bits(a, b)
    return a


def test_dot_products_in_storage_order():
    P = [[1.0, 2.0], [3.0, 4.0]]
    Q = [[10.0, 100.0], [-1.0, 0.5], [0.0, 0.0]]
    out = both([1, 0, 1], [0, 1, 2], [9.0, 9.0, 9.0], P, Q)
    assert out.tolist() == [430.0, 0.0, 0.0]
    out = both([1, 0, 1], [0, 1, 2], [2.0, 3.0, 4.0], P, Q, alpha=2.0, beta=-1.0)
    assert out.tolist() == [858.0, -3.0, -4.0]


def test_serial_ascending_r():
    # 1e16 + 1 + 1 - 1e16 = 0 in ascending r (a tree or another order would give 2)
    P = [[1e16, 1.0, 1.0, -1e16]]
    Q = [[1.0, 1.0, 1.0, 1.0]]
    assert both([0], [0], [0.0], P, Q).tolist() == [0.0]


def test_transpose_swaps_the_roles():
    P = [[1.0], [2.0], [3.0]]                        # rows(op(M)) = cols(M) = 3
    Q = [[10.0], [20.0]]                             # cols(op(M)) = rows(M) = 2
    out = both([1, 0], [2, 0], [0.0, 0.0], P, Q, transpose='T')
    assert out.tolist() == [60.0, 10.0]


def test_k_zero():
    P, Q = np.zeros((2, 0)), np.zeros((2, 0))
    assert bits(both([0, 1], [1, 0], [5.0, -2.0], P, Q)).tolist() == [0, 0]
    assert both([0, 1], [1, 0], [5.0, -2.0], P, Q, alpha=3.0, beta=2.0).tolist() == [10.0, -4.0]
    # alpha * +0 with a negative alpha is -0
    assert bits(both([0], [0], [1.0], np.zeros((1, 0)), np.zeros((1, 0)), alpha=-1.0)).tolist() == [0x8000000000000000]


def test_beta_zero_never_reads_v():
    v = np.array([nan_with(0x7FF8000000000ABC), INF])
    out = both([0, 0], [0, 0], v, [[2.0]], [[3.0]], beta=0.0)
    assert out.tolist() == [6.0, 6.0]
    # beta = NaN is not zero: v is read, and the NaN of the left operand (beta * v: beta) wins
    out = both([0], [0], [1.0], [[2.0]], [[3.0]], beta=nan_with(0x7FF8000000000DEF))
    assert bits(out)[0] == 0x7FF8000000000DEF


def test_nan_payloads_left_operand_first():
    p = nan_with(0x7FF8000000000111)
    q = nan_with(0xFFF8000000000222)
    assert bits(both([0], [0], [0.0], [[p]], [[q]]))[0] == 0x7FF8000000000111
    assert bits(both([0], [0], [0.0], [[1.0]], [[q]]))[0] == 0xFFF8000000000222
    # a signalling NaN comes out quiet
    assert bits(both([0], [0], [0.0], [[nan_with(0x7FF0000000000001)]], [[1.0]]))[0] == 0x7FF8000000000001
    # the running sum's NaN (left operand of the add) wins over a later product's NaN
    out = both([0], [0], [0.0], [[p, 1.0]], [[1.0, q]])
    assert bits(out)[0] == 0x7FF8000000000111
    # v's NaN reaches out through beta * v when alpha * d is not a NaN
    out = both([0], [0], [nan_with(0x7FF8000000000333)], [[1.0]], [[1.0]], beta=1.0)
    assert bits(out)[0] == 0x7FF8000000000333


def test_zero_times_inf_and_inf_minus_inf_are_the_default_nan():
    assert bits(both([0], [0], [0.0], [[0.0]], [[INF]]))[0] == 0xFFF8000000000000
    assert bits(both([0], [0], [0.0], [[1.0, 1.0]], [[INF, -INF]]))[0] == 0xFFF8000000000000
    # alpha = 0 times an infinite dot product
    assert bits(both([0], [0], [0.0], [[1.0]], [[INF]], alpha=0.0))[0] == 0xFFF8000000000000


def test_signed_zeros():
    # d starts at +0: +0 + (-0) = +0, and a single -0 product does not make the sum -0
    assert bits(both([0], [0], [0.0], [[-0.0]], [[1.0]]))[0] == 0
    # alpha * d: -1 * +0 = -0; then + beta * v = -0 + (+0) = +0
    assert bits(both([0], [0], [0.0], [[0.0]], [[1.0]], alpha=-1.0))[0] == 0x8000000000000000
    assert bits(both([0], [0], [0.0], [[0.0]], [[1.0]], alpha=-1.0, beta=1.0))[0] == 0


def test_duplicates_each_get_an_output():
    out = both([0, 0, 0], [1, 1, 1], [1.0, 2.0, 0.0], [[2.0]], [[0.0], [5.0]], beta=1.0)
    assert out.tolist() == [11.0, 12.0, 10.0]


def test_vectorised_equals_the_loop_on_seeded_cases():
    rng = np.random.default_rng(3)
    for case in range(30):
        nrow, ncol = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        nnz, k = int(rng.integers(0, 40)), int(rng.integers(0, 6))
        i0 = rng.integers(0, nrow, nnz).astype(np.int32)
        i1 = rng.integers(0, ncol, nnz).astype(np.int32)
        v = rng.standard_normal(nnz)
        v[rng.random(nnz) < 0.1] = 0.0
        P = rng.standard_normal((nrow, k))
        Q = rng.standard_normal((ncol, k))
        if case % 2:
            for A in (v, P.reshape(-1), Q.reshape(-1)):
                u = rng.random(A.size)
                A[u < 0.05] = NAN
                A[(u >= 0.05) & (u < 0.1)] = INF
                A[(u >= 0.1) & (u < 0.15)] = -INF
        for t in ('.', 'T'):
            PP, QQ = (P, Q) if t == '.' else (rng.standard_normal((ncol, k)), rng.standard_normal((nrow, k)))
            for alpha, beta in ((1.0, 0.0), (-1.0, 2.0), (0.0, -1.0), (NAN, 1.0), (2.0, NAN)):
                a = sr.sample_loop(i0, i1, v, PP, QQ, t, alpha, beta)
                b = sr.sample_ref(i0, i1, v, PP, QQ, t, alpha, beta, chunk=7)
                assert dr.same_bits(a, b), (case, t, alpha, beta)


def test_library_exports_multiply_sampled():
    from spsparse_amd import build, capi
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "spsamd_multiply_sampled")
    assert "spsamd_multiply_sampled" in capi.SYMBOLS
    assert callable(getattr(capi.Context, "multiply_sampled", None))
    with open(os.path.join(ROOT, "include", "spsparse_amd.h")) as f:
        header = f.read()
    assert "int spsamd_multiply_sampled(" in header and "sampled_path" in header
