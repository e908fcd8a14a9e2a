"""tests/krylov_ref.py pinned on the host: the fold against values worked out by hand where its shape shows, its two forms
against each other at the chunk edges, the loop on systems small enough to follow with a pencil and every stop reason, the
solution it returns against plain numpy, and the resource pin of the device kernels (no GPU needed for any of it)."""
import numpy as np
import pytest

from tests import krylov_ref as kr

P53 = 2.0 ** 53


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def test_fold_by_hand():
    # four lanes: (2^53 + 1) + (1 + 1); left to right every + 1 is lost
    t = np.array([P53, 1.0, 1.0, 1.0])
    assert kr.fold_ref(t) == P53 + 2 and kr.fold(t) == P53 + 2 and float(np.cumsum(t)[-1]) == P53
    # the same three values, all in lane 0 (elements 0, 64, 128): added one by one, both ones are lost
    t = np.zeros(130)
    t[[0, 64, 128]] = P53, 1.0, 1.0
    assert kr.fold_ref(t) == P53 and kr.fold(t) == P53
    # ... and with the ones in lane 1 (elements 1 and 65) they meet first
    t = np.zeros(130)
    t[[0, 1, 65]] = P53, 1.0, 1.0
    assert kr.fold_ref(t) == P53 + 2 and kr.fold(t) == P53 + 2
    # lanes 0 and 32 meet in the first butterfly step, lanes 0 and 1 in the last:
    # ((2^53 + 1) + ...) + 1 loses both ones, (2^53 + ...) + (1 + 1) keeps them
    t = np.zeros(64)
    t[[0, 32, 1]] = P53, 1.0, 1.0
    assert kr.fold_ref(t) == P53 and kr.fold(t) == P53
    t = np.zeros(64)
    t[[0, 1, 33]] = P53, 1.0, 1.0
    assert kr.fold_ref(t) == P53 + 2 and kr.fold(t) == P53 + 2
    # two chunks: the partials 2^53 + 2 and 1 are the two lanes of the second level
    t = np.zeros(1025)
    t[[0, 1, 65, 1024]] = P53, 1.0, 1.0, 3.0
    assert kr.fold_ref(t) == P53 + 4 and kr.fold(t) == P53 + 4        # (2^53 + 2) + 3 = 2^53 + 5 -> ties to even: 2^53 + 4
    # one element: +0.0 + x, so -0.0 comes back as +0.0; nothing: +0.0
    for f in (kr.fold_ref, kr.fold):
        assert _bits(f(np.array([-0.0]))) == 0 and _bits(f(np.zeros(0))) == 0 and f(np.array([-2.5])) == -2.5
    # a NaN keeps its payload through the adds (quieted)
    q = np.array([0x7FF0000000000123], np.uint64).view(np.float64)[0]
    want = np.array([0x7FF8000000000123], np.uint64).view(np.int64)[0]
    t = np.array([1.0, q, 2.0])
    assert _bits(kr.fold_ref(t)) == want and _bits(kr.fold(t)) == want


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_fold_forms_agree(m):
    rng = np.random.default_rng(2300 + m)
    t = rng.standard_normal(m) * 10.0 ** rng.integers(-8, 9, m)
    a, b = kr.fold_ref(t), kr.fold(t)
    assert _bits(a) == _bits(b)
    if m > 2:
        assert abs(a - np.sum(t)) <= 4 * m * 2.0 ** -53 * np.abs(t).sum()


def test_fold_forms_agree_on_three_levels():
    m = 1024 * 1024 + 1
    rng = np.random.default_rng(2399)
    t = rng.standard_normal(m) * 10.0 ** rng.integers(-8, 9, m)
    assert _bits(kr.fold_ref(t)) == _bits(kr.fold(t))


def _dense(rows):
    a = np.array(rows, np.float64)
    i, j = np.nonzero(a)
    return (i.astype(np.int32), j.astype(np.int32), a[i, j]), a.shape[0]


def test_loop_by_hand_2x2():
    # A = [2 2; 2 6], b = (-3, 3), x0 = 0:
    #   k = 0: r = (-3, 3), rr = 18, p = r, q = (0, 12), pq = 36, alpha = 1/2, x = (-3/2, 3/2), r = (-3, -3), rr = 18
    #   k = 1: beta = 1, p = (-6, 0), q = (-12, -12), pq = 72, alpha = 1/4, x = (-3, 3/2), r = 0
    S, n = _dense([[2, 2], [2, 6]])
    b = np.array([-3.0, 3.0])
    for fold in (kr.fold, kr.fold_ref):
        got = kr.pcg(S, n, b, np.zeros(2), 0.0, 10, fold_fn=fold)
        assert list(got["x"]) == [-3.0, 1.5] and list(got["hist"]) == [18.0, 18.0, 0.0]
        assert (got["iterations"], got["reason"], got["bb"], got["rr0"], got["rr"]) == (2, kr.CONVERGED, 18.0, 18.0, 0.0)
    one = kr.pcg(S, n, b, np.zeros(2), 0.0, 1)
    assert list(one["x"]) == [-1.5, 1.5] and (one["iterations"], one["reason"], one["rr"]) == (1, kr.MAXITER, 18.0)
    # Jacobi, d = (2, 6): z = (-3/2, 1/2), rz = 6, p = z, q = (-2, 0), pq = 3, alpha = 2, x = (-3, 1), r = (1, 3), rr = 10
    jac = kr.pcg(S, n, b, np.zeros(2), 0.0, 1, kr.JACOBI)
    assert list(jac["x"]) == [-3.0, 1.0] and list(jac["hist"]) == [18.0, 10.0]
    # a start that is the solution: converged before the first iteration, x untouched
    at = kr.pcg(S, n, b, np.array([-3.0, 1.5]), 0.0, 10)
    assert (at["iterations"], at["reason"], list(at["x"]), list(at["hist"])) == (0, kr.CONVERGED, [-3.0, 1.5], [0.0])


def test_loop_by_hand_3x3():
    # A = [3 2 1; 2 6 2; 1 2 1], b = (-1, 0, 1), x0 = 0:
    #   k = 0: rr = 2, q = (-2, 0, 0), pq = 2, alpha = 1, x = (-1, 0, 1), r = (1, 0, 1), rr = 2
    #   k = 1: beta = 1, p = (0, 0, 2), q = (2, 4, 2), pq = 4, alpha = 1/2, x = (-1, 0, 2), r = (0, -2, 0), rr = 4
    #   k = 2: beta = 2, p = (0, -2, 4), q = (0, -4, 0), pq = 8, alpha = 1/2, x = (-1, -1, 4), r = 0
    S, n = _dense([[3, 2, 1], [2, 6, 2], [1, 2, 1]])
    b = np.array([-1.0, 0.0, 1.0])
    want_x = {0: [0, 0, 0], 1: [-1, 0, 1], 2: [-1, 0, 2], 3: [-1, -1, 4]}
    for k in range(4):
        got = kr.pcg(S, n, b, np.zeros(3), 0.0, k)
        assert list(got["x"]) == want_x[k] and list(got["hist"]) == [2.0, 2.0, 4.0, 0.0][:k + 1]
        assert (got["iterations"], got["reason"]) == (k, kr.CONVERGED if k == 3 else kr.MAXITER)
    # with the exact factor as M the first iterate is the solution: L = [1; 2/3 1; 1/3 2/7 1] is not dyadic, so take
    # M = diag(4, 8, 2) stored as a factor (no lower part): z = r / diag, as Jacobi with that diagonal
    F = (np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int32), np.array([4.0, 8.0, 2.0]))
    lu = kr.pcg(S, n, b, np.zeros(3), 0.0, 1, kr.LU, F)
    # z = (-1/4, 0, 1/2), rz = 3/4, q = (-1/4, 1/2, 1/4), pq = 3/16, alpha = 4, x = (-1, 0, 2), r = (0, -2, 0)
    assert list(lu["x"]) == [-1.0, 0.0, 2.0] and list(lu["hist"]) == [2.0, 4.0]


def test_stop_reasons():
    S, n = _dense([[2, 2], [2, 6]])
    x0 = np.array([0.5, -0.25])
    zero = kr.pcg(S, n, np.zeros(2), np.zeros(2), 1e-6, 10)                 # b = 0: 0 <= 0
    assert (zero["iterations"], zero["reason"], zero["bb"], list(zero["hist"])) == (0, kr.CONVERGED, 0.0, [0.0])
    none = kr.pcg(S, n, np.array([1.0, 1.0]), x0, 1e-6, 0)                  # max_iter = 0
    assert (none["iterations"], none["reason"], list(none["x"])) == (0, kr.MAXITER, list(x0)) and len(none["hist"]) == 1
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))          # A = 0: q = 0, pq = 0
    sing = kr.pcg(E, 2, np.array([1.0, 1.0]), x0, 1e-6, 10)
    assert (sing["iterations"], sing["reason"], list(sing["x"]), list(sing["hist"])) == (0, kr.BREAKDOWN, list(x0), [2.0])
    S1, _ = _dense([[1, 0], [0, 0]])                                         # singular, reached after one iteration
    late = kr.pcg(S1, 2, np.array([1.0, 1.0]), np.zeros(2), 0.0, 10)
    # k = 0: p = (1, 1), q = (1, 0), pq = 1, alpha = 2, x = (2, 2), r = (-1, 1); k = 1: beta = 1, p = (0, 2), q = 0
    assert (late["iterations"], late["reason"], list(late["x"]), list(late["hist"])) == (1, kr.BREAKDOWN, [2.0, 2.0], [2.0, 2.0])
    nan = kr.pcg(S, n, np.array([np.nan, 1.0]), np.zeros(2), 1e-6, 10)       # a NaN compares false, then rz is not usable
    assert (nan["iterations"], nan["reason"]) == (0, kr.BREAKDOWN) and np.isnan(nan["rr"])
    assert kr.pcg(E, 0, np.zeros(0), np.zeros(0), 1e-6, 10)["reason"] == kr.CONVERGED


@pytest.mark.parametrize("precond", [kr.NONE, kr.JACOBI, kr.LU])
def test_the_reference_solves_poisson(precond):
    """Poisson 16^2, tol = 1e-6: ||b - A x|| <= 2 tol ||b|| in plain numpy.  The recursive residual the stop test reads
    drifts from the true one by the order of k eps ||A|| ||x|| ~ 1e-13, far below tol ||b||; the factor 2 only keeps the
    check from being an equality."""
    from tests import factor_ref as fr
    S, n = kr.poisson2d(16)
    A = np.zeros((n, n))
    A[S[0], S[1]] = S[2]
    rng = np.random.default_rng(2301)
    b = rng.standard_normal(n)
    tol = 1e-6
    F = None
    if precond == kr.LU:
        f, _ = fr.ilu0_ref(S, n)
        F = (S[0], S[1], f)
    got = kr.pcg(S, n, b, np.zeros(n), tol, 500, precond, F)
    assert got["reason"] == kr.CONVERGED and 0 < got["iterations"] < 100
    assert np.linalg.norm(b - A @ got["x"]) <= 2 * tol * np.linalg.norm(b)
    assert len(got["hist"]) == got["iterations"] + 1 and got["hist"][-1] == got["rr"] <= tol * tol * got["bb"]


def test_no_krylov_kernel_uses_scratch():
    """Every kernel of k_krylov.hip in the built library -- the loop's own and the vector kernels every Krylov loop launches
    through the frame, k_pcg_spmv in its three forms: no scratch, no spill (resource figures only, no GPU)."""
    from scripts import kernel_resources
    from spsparse_amd import build
    every = kernel_resources.library_kernels(build.build())
    found = {name: f for name, f in every.items() if "k_pcg_" in name}
    want = ("dot", "residual", "jacobi", "spmvILi0", "spmvILi1", "spmvILi2", "direction", "update", "dot_rows", "init", "finish")
    assert all(any("k_pcg_" + k in name for name in found) for k in want), sorted(found)
    twins = [name for name in every for k in ("dot", "residual", "jacobi", "spmv", "init") if "k_bicg_" + k in name]
    assert not twins, twins                                                # the shared kernels exist once
    for name, f in found.items():
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, (name, f)
