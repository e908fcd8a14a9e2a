"""tests/factor_ref.py pinned on the host: hand-computed factorisations, exact recovery of L0 and U0 from A = L0 * U0 on
patterns that do not fill, ilu0_fast against ilu0_ref bit for bit, and the level vector of a symmetrised by_levels operand."""
import numpy as np

from tests import factor_ref as fr
from tests import select_ref as sel
from tests import solve_ref as sr


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _S(rows, cols, vals):
    return np.array(rows, np.int32), np.array(cols, np.int32), np.array(vals, np.float64)


def test_hand_3x3_dense():
    """A = [[2,1,1],[4,3,3],[8,7,9]] = [[1,0,0],[2,1,0],[4,3,1]] * [[2,1,1],[0,1,1],[0,0,2]]."""
    S = _S([0, 0, 0, 1, 1, 1, 2, 2, 2], [0, 1, 2, 0, 1, 2, 0, 1, 2], [2, 1, 1, 4, 3, 3, 8, 7, 9])
    f, st = fr.ilu0_ref(S, 3)
    assert np.array_equal(f, [2, 1, 1, 2, 1, 1, 4, 3, 2])
    assert st == dict(updates=5, lookups=5, zero_pivot=-1, missing_diag=-1)


def test_hand_3x3_zero_pivot():
    """Row 1's pivot becomes 1 - 1 * 1 = 0: row 2 divides by it (Inf) and its diagonal is 1 - Inf * 1 = -Inf."""
    S = _S([0, 0, 1, 1, 1, 2, 2], [0, 1, 0, 1, 2, 1, 2], [1, 1, 1, 1, 1, 1, 1])
    f, st = fr.ilu0_ref(S, 3)
    assert np.array_equal(_bits(f), _bits([1, 1, 1, 0.0, 1, np.inf, -np.inf]))
    assert st == dict(updates=2, lookups=2, zero_pivot=1, missing_diag=-1)


def test_hand_4x4_missing_diagonal():
    """Row 1 stores no diagonal: p_1 = +0.0.  (1,0) = 4 / 2 = 2, (1,2) = 3 - 2 * 1 = 1; (2,0) = 1, (2,2) = 1 - 1 * 1 = 0,
    (2,1) = 5 / +0.0 = Inf, (2,2) = 0 - Inf * 1 = -Inf; (3,2) = 7 / -Inf = -0.0 and row 2 has nothing right of its diagonal."""
    S = _S([0, 0, 1, 1, 2, 2, 2, 3, 3], [0, 2, 0, 2, 0, 1, 2, 2, 3], [2, 1, 4, 3, 2, 5, 1, 7, 1])
    f, st = fr.ilu0_ref(S, 4)
    assert np.array_equal(_bits(f), _bits([2, 1, 2, 1, 1, np.inf, -np.inf, -0.0, 1]))
    assert st == dict(updates=3, lookups=3, zero_pivot=1, missing_diag=1)
    g, st2 = fr.ilu0_fast(S, 4)
    assert np.array_equal(_bits(g), _bits(f)) and st2 == st


def test_nan_takes_the_left_operand():
    """f_t * f_s with both NaN keeps f_t's payload (quieted); the subtraction then keeps f_u's if it is one."""
    a = np.array([0x7FF0000000000123], np.uint64).view(np.float64)[0]        # signalling, payload 0x123
    b = np.array([0xFFF8000000000456], np.uint64).view(np.float64)[0]
    S = _S([0, 0, 1, 1], [0, 1, 0, 1], [1.0, b, a, 2.0])
    f, _ = fr.ilu0_ref(S, 2)
    assert f.view(np.uint64)[2] == 0x7FF8000000000123                        # a / 1: a, quieted
    assert f.view(np.uint64)[3] == 0x7FF8000000000123                        # 2 - (a' * b): the product is a', the right operand of the subtraction


def test_exact_recovery():
    """A = L0 * U0 with small integers and power-of-two pivots on patterns without fill: every operation is exact, so the
    factorisation returns tril(L0, -1) + U0 exactly, and every lookup inside the pattern is an update."""
    rng = np.random.default_rng(2101)
    cases = [("full %d" % n, n, np.ones((n, n), bool)) for n in range(1, 9)]
    cases += [("band 2/3", 40, fr.band(40, 2, 3)), ("band 3/2", 40, fr.band(40, 3, 2)), ("arrow", 23, fr.arrow(23))]
    for what, n, pattern in cases:
        S, want = fr.product_lu(rng, n, pattern)
        for fn in (fr.ilu0_ref, fr.ilu0_fast):
            f, st = fn(S, n)
            assert np.array_equal(f, want), what                    # (as numbers: a zero of L0 comes back as 0 / p, -0.0 under a negative pivot)
            assert st["zero_pivot"] == -1 and st["missing_diag"] == -1, what
            if what.startswith("full"):
                assert st["updates"] == st["lookups"] == (n - 1) * n * (2 * n - 1) // 6, what
    S, _ = fr.product_lu(rng, 40, fr.band(40, 2, 3))
    _, st = fr.ilu0_ref(S, 40)
    assert st["updates"] == st["lookups"] == 227


def test_fast_equals_ref_on_the_fuzz_operands():
    rng = np.random.default_rng(2102)
    for trial in range(150):
        n = int(rng.integers(1, 41))
        t = '.' if rng.integers(2) == 0 else 'T'
        kind = trial % 3
        pol, zn = int(rng.integers(3)), bool(rng.integers(5) == 0)
        A, sort0 = fr.fuzz_operand(rng, n, kind, t)
        S = sel.operand_S(A, t, pol, zn, sort0)
        assert fr.strictly_ascending(S), trial
        f, st = fr.ilu0_ref(S, n)
        g, st2 = fr.ilu0_fast(S, n)
        assert np.array_equal(_bits(f), _bits(g)), "trial %d kind %d" % (trial, kind)
        assert st == st2, trial
        assert st["lookups"] == int(fr.row_work(S, n).sum())


def test_symmetrised_by_levels_keeps_its_levels():
    rng = np.random.default_rng(2103)
    for scatter in (False, True):
        A, n, lev = sr.by_levels(rng, [1, 5, 9, 40, 3, 1, 1, 17], scatter=scatter)
        S = fr.symmetrised(A, n, rng)
        assert fr.strictly_ascending(S)
        assert np.array_equal(sr.levels(S, n), lev)
        f, st = fr.ilu0_ref(S, n)
        g, st2 = fr.ilu0_fast(S, n, lev)
        assert np.array_equal(_bits(f), _bits(g)) and st == st2
        low = int(np.count_nonzero(S[1] < S[0]))
        assert st["updates"] >= low                                 # every lower tuple (i, k) updates (i, i) through (k, i)


def test_classes_and_plan():
    """Rows by class under the thresholds, and the launch plan of a schedule."""
    S = _S([0, 0, 0, 1, 1, 1, 2, 2, 2], [0, 1, 2, 0, 1, 2, 0, 1, 2], np.ones(9))
    assert list(fr.row_work(S, 3)) == [0, 2, 3]
    assert list(fr.classes(S, 3, 2, 1024)) == [0, 1, 2]
    assert list(fr.classes(S, 3, 2, 2)) == [0, 1, 3]
    assert list(fr.classes(S, 3, 64, 2, 2)) == [0, 3, 3] and list(fr.classes(S, 3, 0, 2, 1)) == [0, 1, 1]
    sizes, work, length = [5, 300, 10, 10, 7], [0, 3, 3, 100, 3], [1, 3, 3, 2000, 3]
    assert fr.plan(sizes, work, length, 256, 64, 1024) == (6, 2)     # serial; fused 2; serial + wave + block; fused 4
    assert fr.plan(sizes, work, length, 256, 64, 4096) == (5, 2)
    assert fr.plan(sizes, work, length, 256, 64, 1024, factor_path=1) == (6, 0)
    assert fr.plan(sizes, work, length, 256, 64, 1024, factor_path=2) == (5, 3)
    assert fr.plan(sizes, work, length, 256, 64, 1024, factor_row=1) == (2, 3)
    assert fr.plan(sizes, work, length, 256, 64, 1024, factor_row=2) == (5, 0)
    assert fr.plan(sizes, work, length, 256, 64, 1024, factor_row=3) == (4, 0)
