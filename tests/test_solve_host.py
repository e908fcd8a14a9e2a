"""tests/solve_ref.py pinned without a GPU: hand-computed cases, solve_fast against solve_ref bit for bit, scipy's
spsolve_triangular where every operation is exact, the level structure of three known matrices, and the other triangle
ignored."""
import numpy as np

from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests import select_ref as sel
from tests import solve_ref as sr


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def with_bits(b):
    return np.array([b], np.uint64).view(np.float64)[0]


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


QNAN_A, QNAN_B = 0x7FF80000DEADBEEF, 0xFFF8000000000123
SNAN = 0x7FF0000000000001
DEFAULT = 0xFFF8000000000000


def test_sub_and_div_nan_rules():
    a, b, s = with_bits(QNAN_A), with_bits(QNAN_B), with_bits(SNAN)
    for f in (sr.sub, sr.div):
        assert bits(f(a, 1.0)) == QNAN_A and bits(f(1.0, a)) == QNAN_A           # either position: that NaN
        assert bits(f(a, b)) == QNAN_A and bits(f(b, a)) == QNAN_B               # both: the left one
        assert bits(f(s, b)) == SNAN | (1 << 51) and bits(f(2.0, s)) == SNAN | (1 << 51)   # a signalling one: quieted
    assert bits(sr.sub(1.0, b)) == QNAN_B                                       # not 1.0 + (-b): b's sign stays
    assert bits(sr.sub(np.inf, np.inf)) == DEFAULT and bits(sr.sub(-np.inf, -np.inf)) == DEFAULT
    assert bits(sr.div(0.0, 0.0)) == DEFAULT and bits(sr.div(np.inf, -np.inf)) == DEFAULT and bits(sr.div(-0.0, 0.0)) == DEFAULT
    assert sr.div(1.0, 0.0) == np.inf and sr.div(-1.0, 0.0) == -np.inf and sr.div(1.0, -0.0) == -np.inf
    assert bits(sr.sub(0.0, 0.0)) == 0 and bits(sr.sub(-0.0, 0.0)) == 1 << 63
    assert sr.div(1.0, 3.0) == 1.0 / 3.0 and sr.sub(0.1, 0.3) == 0.1 - 0.3


def test_hand_2x2():
    # [[2, 9], [3, 4]]: LOWER reads 2, 3, 4; UPPER reads 2, 9, 4
    S = (np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1]), np.array([2.0, 9.0, 3.0, 4.0]))
    B = np.array([[4.0, 1.0], [10.0, 0.0]])
    assert same(sr.solve_ref(S, 2, B), [[2.0, 0.5], [(10.0 - 3.0 * 2.0) / 4.0, (0.0 - 3.0 * 0.5) / 4.0]])
    assert same(sr.solve_ref(S, 2, B, sr.LOWER, sr.UNIT), [[4.0, 1.0], [10.0 - 12.0, -3.0]])
    assert same(sr.solve_ref(S, 2, B, sr.UPPER), [[(4.0 - 9.0 * 2.5) / 2.0, 0.5], [2.5, 0.0]])
    assert same(sr.solve_ref(S, 2, B, sr.UPPER, sr.UNIT), [[4.0 - 90.0, 1.0], [10.0, 0.0]])
    # 'T': op(A) = [[2, 3], [9, 4]], so LOWER reads 2, 9, 4
    St = sel.operand_S((S[0], S[1], S[2]), 'T')
    assert same(sr.solve_ref(St, 2, B[:, 0]), [2.0, (10.0 - 9.0 * 2.0) / 4.0])


def test_hand_3x3_order_missing_and_negative_zero_diagonal():
    # row 1 has no diagonal; row 2 is stored (2,2) -0.0, (2,0) 1, (2,2) 0.5, (2,1) 2: a trusted operand keeps that order
    S = (np.array([0, 1, 2, 2, 2, 2]), np.array([0, 0, 2, 0, 2, 1]), np.array([4.0, 1.0, -0.0, 1.0, 0.5, 2.0]))
    B = np.array([8.0, 3.0, 1.0])
    x0 = 2.0
    x1 = np.inf                                                   # (3 - 1 * 2) / +0.0: a missing diagonal leaves d at +0.0
    X = sr.solve_ref(S, 3, B)
    assert same(X[:2], [x0, x1])
    assert X[2] == -np.inf                                        # (1 - 2 - Inf) / (+0 + -0 + 0.5)
    assert sr.zero_pivot(S, 3) == 1 and sr.zero_pivot(S, 3, diag=sr.UNIT) == -1
    assert same(sr.diag_fold(S, 3), [4.0, 0.0, 0.5])
    # a diagonal of one -0.0 folds to +0.0 (+0.0 + -0.0), a zero pivot; so do two of them
    for dv in ([-0.0], [-0.0, -0.0]):
        Z = (np.array([0] * len(dv)), np.array([0] * len(dv)), np.array(dv))
        assert bits(sr.diag_fold(Z, 1))[0] == 0 and sr.zero_pivot(Z, 1) == 0
        assert sr.solve_ref(Z, 1, np.array([-3.0]))[0] == -np.inf
    # a NaN diagonal is no zero pivot
    Z = (np.array([0]), np.array([0]), np.array([np.nan]))
    assert sr.zero_pivot(Z, 1) == -1
    # a row without a used tuple: B / +0.0, or B under UNIT
    E = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    assert same(sr.solve_ref(E, 2, np.array([1.0, -0.0])), [np.inf, with_bits(DEFAULT)])
    assert same(sr.solve_ref(E, 2, np.array([1.0, -0.0]), diag=sr.UNIT), [1.0, -0.0])


def test_nan_in_each_operand_position():
    a, b = with_bits(QNAN_A), with_bits(QNAN_B)
    # x1 = (B1 - v * x0) / d with x0 = B0 / 1
    def x1(B0, B1, v, d):
        S = (np.array([0, 1, 1]), np.array([0, 0, 1]), np.array([1.0, v, d]))
        return bits(sr.solve_ref(S, 2, np.array([B0, B1])))[1]
    assert x1(1.0, a, 2.0, 4.0) == QNAN_A                         # acc NaN: left of the sub, left of the div
    assert x1(1.0, a, b, 4.0) == QNAN_A                           # acc and v NaN: acc is the left operand of the sub
    assert x1(b, 1.0, 2.0, 4.0) == QNAN_B                         # x NaN: right of the mul, then right of the sub
    assert x1(b, 1.0, a, 4.0) == QNAN_A                           # v and x NaN: v is the left operand of the mul
    assert x1(1.0, 1.0, 2.0, b) == QNAN_B                         # d NaN: right of the div
    assert x1(1.0, a, 2.0, b) == QNAN_A                           # acc and d NaN: acc is the left operand of the div
    assert x1(np.inf, np.inf, 1.0, 4.0) == DEFAULT                # Inf - Inf
    assert x1(np.inf, 1.0, 0.0, 4.0) == DEFAULT                   # 0 * Inf


def test_fast_equals_ref_on_random_operands_with_special_values():
    rng = np.random.default_rng(5)
    for trial in range(120):
        n = int(rng.integers(1, 30))
        nnz = int(rng.integers(0, 5 * n))
        t = '.' if trial % 2 else 'T'
        lead = 1 if t == 'T' else 0
        if trial % 3 == 0:
            A, sort0 = sel.unique_key_operand(rng, (n, n), nnz), -1
        elif trial % 3 == 1:
            A, sort0 = sel.duplicate_key_operand(rng, (n, n), nnz), -1
        else:
            i0, i1 = rng.integers(0, n, nnz).astype(np.int32), rng.integers(0, n, nnz).astype(np.int32)
            o = np.argsort(i1 if lead else i0, kind="stable")
            A, sort0 = (i0[o], i1[o], sel.special_values(rng, nnz, 0.3)[o]), lead
        S = sel.operand_S(A, t, trial % 3, trial % 5 == 0, sort0)
        B = ar._values(rng, n * 3, 0.1).reshape(n, 3)
        for uplo in (sr.LOWER, sr.UPPER):
            for diag in (sr.NONUNIT, sr.UNIT):
                assert same(sr.solve_fast(S, n, B, uplo, diag), sr.solve_ref(S, n, B, uplo, diag)), (trial, uplo, diag)


def test_equals_scipy_where_every_operation_is_exact():
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve_triangular
    rng = np.random.default_rng(6)
    for trial in range(60):
        n = int(rng.integers(1, 13))
        lower = trial % 2 == 0
        rows, cols, vals = [], [], []
        for i in range(n):
            rows.append(i); cols.append(i); vals.append(float(rng.choice([1.0, 2.0, -1.0, 0.5])))
            cand = np.arange(i) if lower else np.arange(i + 1, n)
            for j in rng.choice(cand, min(len(cand), int(rng.integers(0, 3))), replace=False):
                rows.append(i); cols.append(int(j)); vals.append(float(rng.choice([-1.0, 1.0])))
        o = np.lexsort((cols, rows))
        S = (np.array(rows)[o], np.array(cols)[o], np.array(vals)[o])
        B = rng.integers(-8, 9, (n, 2)).astype(np.float64)
        M = sp.csr_matrix((S[2], (S[0], S[1])), shape=(n, n))
        want = spsolve_triangular(M, B, lower=lower)
        got = sr.solve_ref(S, n, B, sr.LOWER if lower else sr.UPPER)
        assert np.array_equal(got, want), trial                    # small dyadic rationals: exact in any order


def test_levels_of_known_structures():
    n = 9
    i = np.arange(n)
    D = (i, i, np.ones(n))
    assert sr.schedule_stats(D, n) == (1, n) and not sr.levels(D, n).any()
    Bi = (np.r_[i, i[1:]], np.r_[i, i[1:] - 1], np.ones(2 * n - 1))
    Bi = tuple(x[np.lexsort((Bi[1], Bi[0]))] for x in Bi)
    assert sr.schedule_stats(Bi, n) == (n, 1) and np.array_equal(sr.levels(Bi, n), i)
    assert np.array_equal(sr.levels(Bi, n, sr.UPPER), np.zeros(n))              # no tuple above the diagonal
    N = 7
    P = wl.poisson2d(N)[:3]
    lev = sr.levels(P, N * N)
    assert np.array_equal(lev, np.arange(N * N) // N + np.arange(N * N) % N) and lev.max() + 1 == 2 * N - 1
    assert np.array_equal(sr.levels(P, N * N, sr.UPPER), lev[::-1])
    # by pattern: an explicit zero is a dependency
    Z = (np.array([0, 1, 1]), np.array([0, 0, 1]), np.array([1.0, 0.0, 1.0]))
    assert np.array_equal(sr.levels(Z, 2), [0, 1])
    assert np.array_equal(sr.levels(Z, 2, sr.LOWER, sr.UNIT), [0, 1]) and sr.tuples_used(Z, sr.LOWER, sr.UNIT) == 1


def test_the_other_triangle_is_ignored():
    rng = np.random.default_rng(7)
    n = 25
    A = sel.unique_key_operand(rng, (n, n), 200, special=0.1)
    S = sel.operand_S(A)
    B = rng.standard_normal((n, 2))
    lo = S[1] <= S[0]
    up = S[1] >= S[0]
    assert same(sr.solve_ref(S, n, B), sr.solve_ref(tuple(x[lo] for x in S), n, B))
    assert same(sr.solve_ref(S, n, B, sr.UPPER), sr.solve_ref(tuple(x[up] for x in S), n, B, sr.UPPER))
    poison = (S[0], S[1], np.where(lo, S[2], np.nan))
    assert same(sr.solve_ref(poison, n, B), sr.solve_ref(S, n, B))


def test_peel_plan_by_hand():
    T, K = 8, 4
    pp = lambda sizes: sr.peel_plan(sizes, T, K)
    assert pp([]) == (0, 0) and pp([100]) == (0, 0) and pp([3]) == (0, 0)      # one level: no off-diagonal tuple, no peel
    assert pp([3, 2]) == (1, 0) and pp([1] * 50) == (1, 0)                     # thin to the end: one launch, no batch
    assert pp([8, 8, 8]) == (1, 0)                                             # thin_max itself is thin
    assert pp([9, 1]) == (0, 4) and pp([9, 9]) == (0, 4)                       # wide first: a batch, whatever follows in it
    assert pp([9] * 4) == (0, 4) and pp([9] * 5) == (0, 8)                     # a batch is `batch` levels; the fifth needs another
    assert pp([9] * 8) == (0, 8) and pp([9] * 9) == (0, 12)
    assert pp([9] * 4 + [5]) == (1, 4)                                         # thin after a full batch: no batch after it
    assert pp([9] * 4 + [5, 1, 9]) == (1, 8)                                   # ... unless it widens again
    assert pp([2, 9]) == (1, 4)                                                # thin hands over at the first wide level
    assert pp([2, 9, 1, 1, 1, 8, 2]) == (2, 4)                                 # the batch swallows thin levels; the host sees the 8
    assert pp([2, 9, 1, 1, 1, 9, 2]) == (1, 8)                                 # ... or a 9: wide again, no thin launch between
    assert pp([1, 9, 9, 9, 9, 8, 1, 1, 1, 1, 1, 9]) == (2, 8)
    assert sr.peel_plan([2049] * 17, 2048, 16) == (0, 32) and sr.peel_plan([2048] * 17, 2048, 16) == (1, 0)


def _lower_levels_ok(A, n, lev, sizes):
    assert np.array_equal(sr.levels(A, n), lev) and np.array_equal(np.bincount(lev), sizes)
    assert np.all(np.diff(A[0]) >= 0)


def test_builders_have_the_levels_they_claim():
    rng = np.random.default_rng(21)
    sizes = [5, 3, 4]
    for scatter in (False, True):
        A, n, lev = sr.by_levels(rng, sizes, scatter=scatter)
        _lower_levels_ok(A, n, lev, sizes)
        B = rng.standard_normal((n, 2))
        assert same(sr.solve_fast(A, n, B, lev=lev), sr.solve_ref(A, n, B))
    A, n, lev = sr.by_levels(rng, [60, 50, 70, 9], scatter=True)
    assert np.any(np.diff(lev) < 0)                                            # scattered: the levels are not in row order
    # hubs: a fan of 7 from a lone row, a fan of 6 among 5 rows, a row gathering 9 of 11
    for sizes, fan, gather, hub_deg in (([1, 7, 3], {0: 7}, None, 7), ([5, 12, 4], {0: 6}, None, 6), ([4, 11, 6, 2], None, {2: 9}, 9)):
        A, n, lev = sr.by_levels(rng, sizes, fan=fan, gather=gather)
        _lower_levels_ok(A, n, lev, sizes)
        off = A[1] < A[0]
        if fan:
            dependants = np.bincount(A[1][off], minlength=n)
            hub = int(np.argmax(dependants))
            assert dependants[hub] == hub_deg and lev[hub] == 0
            others = dependants[(lev == 0) & (np.arange(n) != hub)]
            assert others.size == sizes[0] - 1 and np.all((others >= 1) & (others <= 2))
        else:
            indeg = np.bincount(A[0][off], minlength=n)
            hub = int(np.argmax(indeg))
            assert indeg[hub] == hub_deg and lev[hub] == 2 and np.unique(A[1][off & (A[0] == hub)]).size == hub_deg
            assert np.all(lev[A[1][off & (A[0] == hub)]] == 1)
        B = rng.standard_normal((n, 3))
        want = sr.solve_ref(A, n, B)
        assert same(sr.solve_fast(A, n, B, lev=lev), want)
        U, ulev = sr.mirrored(A, n, lev)
        assert np.array_equal(sr.levels(U, n, sr.UPPER), ulev) and np.all(U[1] >= U[0]) and np.all(np.diff(U[0]) >= 0)
        assert same(sr.solve_fast(U, n, B[::-1], sr.UPPER, lev=ulev), want[::-1])       # the same chains, renumbered
        assert same(sr.solve_ref(U, n, B[::-1], sr.UPPER), want[::-1])


def test_pattern_noise_moves_no_level():
    rng = np.random.default_rng(22)
    sizes = [9, 9, 9]
    A, n, lev = sr.by_levels(rng, sizes)
    drop, nz = (int(x) for x in np.flatnonzero(lev == 1)[:2])
    N = sr.pattern_noise(rng, A, n, lev, drop, nz)
    assert np.all(np.diff(N[0]) >= 0) and len(N[2]) > len(A[2]) + n // 2
    keys = N[0].astype(np.int64) * n + N[1]
    low = N[1] < N[0]
    assert np.unique(keys[low]).size < np.count_nonzero(low) and np.any(N[2][low] == 0.0)      # duplicates and explicit zeros
    assert np.any(N[1] > N[0]) and np.any(np.isnan(N[2][N[1] > N[0]]))
    assert sr.zero_pivot(N, n) == min(drop, nz) and sr.zero_pivot(N, n, diag=sr.UNIT) == -1
    B = rng.standard_normal((n, 2))
    for diag in (sr.NONUNIT, sr.UNIT):
        assert np.array_equal(sr.levels(N, n, sr.LOWER, diag), lev)                # trusted: by pattern
        assert same(sr.solve_fast(N, n, B, sr.LOWER, diag, lev=lev), sr.solve_ref(N, n, B, sr.LOWER, diag))
    assert not np.all(np.isfinite(sr.solve_ref(N, n, B)))
    U, ulev = sr.mirrored(N, n, lev)
    assert np.array_equal(sr.levels(U, n, sr.UPPER), ulev)
    for pol in (ar.LEAVE_ALONE, ar.ADD, ar.REPLACE):                                # raw: merged, zeros dropped, the levels stay
        o = rng.permutation(len(N[2]))
        S = sel.operand_S(tuple(x[o] for x in N), '.', pol, False, -1)
        assert np.array_equal(sr.levels(S, n), lev), pol
        St = sel.operand_S((N[1][o], N[0][o], N[2][o]), 'T', pol, False, -1)
        assert all(np.array_equal(x, y) for x, y in zip(S[:2], St[:2]))


def test_far_rows():
    rng = np.random.default_rng(23)
    A, lev, named = sr.far_rows(rng, 100, 12)
    assert np.array_equal(sr.levels(A, 100), lev) and lev.max() == 13 and np.array_equal(named, np.r_[0, 1, np.arange(88, 100)])
    assert np.count_nonzero(A[0] == 99) == 12 and np.all(A[2][A[0] == A[1]] > 0)
    off = A[0] != A[1]
    assert np.all(np.isin(A[0][off], named)) and np.all(np.isin(A[1][off], named))
    B = np.zeros((100, 3))
    B[named] = rng.standard_normal((named.size, 3))
    X = sr.solve_ref(A, 100, B)
    assert same(sr.solve_fast(A, 100, B, lev=lev), X)
    rest = np.setdiff1d(np.arange(100), named)
    assert not X[rest].view(np.int64).any() and np.all(X[named] != 0)            # an unnamed row is +0.0 / d = +0.0
