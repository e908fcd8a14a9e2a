"""multiply_dense without a GPU: the host restatement of the reference loop (tests/dense_ref.py) pinned to hand-written
cases, the fast restatement equal to it, and the entry point present in the library and the Python binding."""
import ctypes

import numpy as np

from tests import dense_ref as dr

NAN, INF = np.nan, np.inf


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_add_in_storage_order():
    # Y0 = 5 + 2*10 + (-1)*100; row 1 = 7 + 3*1
    y = dr.apply_ref([0, 1, 0], [1, 0, 2], [2.0, 3.0, -1.0], [[1.0], [10.0], [100.0]], [[5.0], [7.0]])
    assert y.tolist() == [[-75.0], [10.0]]


def test_duplicates_each_contribute():
    i0, i1, v, X = [0, 0], [0, 0], [2.0, 3.0], [[4.0]]
    assert dr.apply_ref(i0, i1, v, X, [[1.0]], policy=dr.ADD).tolist() == [[21.0]]
    assert dr.apply_ref(i0, i1, v, X, [[1.0]], policy=dr.REPLACE).tolist() == [[12.0]]
    assert dr.apply_ref(i0, i1, v, X, [[1.0]], policy=dr.LEAVE_ALONE).tolist() == [[12.0]]


def test_y_never_zeroed():
    y = dr.apply_ref([0], [0], [2.0], [[3.0, 4.0]], [[1.0, 1.0], [-7.5, 9.0]])
    assert y.tolist() == [[7.0, 9.0], [-7.5, 9.0]]


def test_leave_alone_quirk():
    # accum.hpp:128-130: the entry is overwritten UNLESS it holds a NaN
    y = dr.apply_ref([0, 1], [0, 0], [2.0, 3.0], [[1.0]], [[NAN], [1.0]], policy=dr.LEAVE_ALONE)
    assert np.isnan(y[0, 0]) and y[1, 0] == 3.0
    # a NaN product written once makes the entry stick: the later 5.0 leaves it alone
    y = dr.apply_ref([0, 0], [0, 1], [1.0, 5.0], [[NAN], [1.0]], [[4.0]], policy=dr.LEAVE_ALONE)
    assert np.isnan(y[0, 0])


def test_handle_nan_skips_nan_and_inf_products():
    X = [[1.0], [NAN], [2.0]]
    i0, i1, v = [0, 0, 0, 0], [0, 1, 2, 0], [INF, 1.0, 3.0, 1.0]
    assert dr.apply_ref(i0, i1, v, X, [[1.0]], handle_nan=True).tolist() == [[8.0]]
    assert np.isnan(dr.apply_ref(i0, i1, v, X, [[1.0]], handle_nan=False)[0, 0])
    y = dr.apply_ref(i0, i1, v, X, [[1.0]], policy=dr.REPLACE, handle_nan=True)
    assert y.tolist() == [[1.0]]                      # the last finite product


def test_zero_times_inf_is_the_x86_default_nan():
    # an explicit zero in M is not dropped: 0 * Inf = NaN, with the bits x86-64 gives it
    y = dr.apply_ref([0], [0], [0.0], [[INF]], [[1.0]])
    assert bits(y)[0, 0] == 0xFFF8000000000000
    # the NaN of the left operand wins: the entry's own payload survives the add
    y0 = np.array([[1.0]]); y0.view(np.uint64)[0, 0] = 0x7FF8000000000123
    y = dr.apply_ref([0], [0], [0.0], [[INF]], y0)
    assert bits(y)[0, 0] == 0x7FF8000000000123
    # a signalling NaN comes out quiet
    x = np.array([[1.0]]); x.view(np.uint64)[0, 0] = 0x7FF0000000000001
    assert bits(dr.mul(np.float64(2.0), x))[0, 0] == 0x7FF8000000000001
    # signed zeros: -0 * 1 = -0, and -0 + -0 stays -0
    y = dr.apply_ref([0], [0], [-0.0], [[1.0]], [[-0.0]])
    assert bits(y)[0, 0] == 0x8000000000000000


def test_transpose_on_unsorted_storage():
    # op(M) = M^T: output row = idx1.  Storage order 1e16, 1, 1, -1e16 gives 0; in column order it would give 2.
    i0 = [0, 1, 2, 3, 0]
    i1 = [0, 0, 0, 0, 1]
    v = [1.0, 1.0, 1.0, 1.0, 4.0]
    X = [[1e16], [1.0], [1.0], [-1e16]]
    y = dr.apply_ref(i0, i1, v, X, [[0.0], [0.5]], transpose='T')
    assert y.tolist() == [[0.0], [4e16 + 0.5]]
    i0s = [1, 2, 0, 3]                                # the same tuples in another storage order: another sum
    y2 = dr.apply_ref(i0s, [0, 0, 0, 0], [1.0] * 4, X, [[0.0]], transpose='T')
    assert y2.tolist() == [[2.0]]


def _random_case(rng, nrow, ncol, nnz, nrhs, specials):
    i0 = rng.integers(0, nrow, nnz).astype(np.int32)
    i1 = rng.integers(0, ncol, nnz).astype(np.int32)
    v = rng.standard_normal(nnz)
    v[rng.random(nnz) < 0.1] = 0.0
    X = rng.standard_normal((ncol, nrhs))
    Y = rng.standard_normal((nrow, nrhs))
    if specials:
        for A in (v, X.reshape(-1), Y.reshape(-1)):
            k = rng.random(A.size)
            A[k < 0.03] = NAN
            A[(k >= 0.03) & (k < 0.05)] = INF
            A[(k >= 0.05) & (k < 0.07)] = -INF
    return i0, i1, v, X, Y


def test_fast_restatement_equals_the_loop():
    rng = np.random.default_rng(7)
    for case in range(24):
        nrow, ncol = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        i0, i1, v, X, Y = _random_case(rng, nrow, ncol, int(rng.integers(0, 60)), int(rng.integers(1, 4)), case % 2 == 1)
        for t in ('.', 'T'):
            XX = X if t == '.' else rng.standard_normal((nrow, X.shape[1]))
            YY = Y if t == '.' else rng.standard_normal((ncol, Y.shape[1]))
            for pol in (dr.LEAVE_ALONE, dr.ADD, dr.REPLACE):
                for hn in (False, True):
                    a = dr.apply_ref(i0, i1, v, XX, YY, t, pol, hn)
                    b = dr.apply_fast(i0, i1, v, XX, YY, t, pol, hn)
                    assert dr.same_bits(a, b), (case, t, pol, hn)


def test_library_exports_multiply_dense():
    from spsparse_amd import build, capi
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "spsamd_multiply_dense")
    assert "spsamd_multiply_dense" in capi.SYMBOLS
    assert callable(getattr(capi.Context, "multiply_dense", None))
