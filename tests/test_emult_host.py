"""tests/emult_ref.py pinned without a device: against dense numpy, against its own plain loop, against select_ref and
add_ref where the operations meet, and the NaN bits of its products against numpy's own multiply (wherever at most one operand is a
NaN) and the written-out x86 rule of tests/dense_ref.py."""
import numpy as np

from tests import add_ref as ar
from tests import dense_ref as dr
from tests import emult_ref as er
from tests import select_ref as sr

FORMS = ((er.TIMES, False), (er.FIRST, False), (er.FIRST, True))


def _plain(rng, shape, nnz):
    """Unique keys, non-special values, shuffled storage order."""
    return sr.unique_key_operand(rng, shape, nnz, special=0.0)


def _dense(X, shape):
    d = np.zeros(shape)
    d[X[0], X[1]] = X[2]
    return d


def _bits(v):
    return np.ascontiguousarray(v, np.float64).view(np.int64)


def test_against_dense_numpy():
    rng = np.random.default_rng(1)
    for trial in range(40):
        opshape = (int(rng.integers(1, 12)), int(rng.integers(1, 12)))
        tA, tB = ('.', 'T')[trial % 2], ('.', 'T')[(trial // 2) % 2]
        shA, shB = (opshape[::-1] if tA == 'T' else opshape), (opshape[::-1] if tB == 'T' else opshape)
        A, B = _plain(rng, shA, int(rng.integers(0, 80))), _plain(rng, shB, int(rng.integers(0, 80)))
        dA, dB = _dense(A, shA), _dense(B, shB)
        dA, dB = (dA.T if tA == 'T' else dA), (dB.T if tB == 'T' else dB)
        pa, pb = dA != 0, dB != 0                               # no stored zeros: the pattern is where the values are
        alpha = float(rng.choice([1.0, -0.5, 3.0]))
        for op, comp in FORMS:
            S = er.operands(A, B, op, tA, tB)
            i, j, v = er.emult_ref(S[0], S[1], op, alpha, comp)
            on = pa & (~pb if comp else pb)
            want = (alpha * dA) * dB if op == er.TIMES else dA
            wi, wj = np.nonzero(on)                             # row-major, like S_A
            assert np.array_equal(i, wi) and np.array_equal(j, wj)
            assert np.array_equal(_bits(v), _bits(want[on]))


def test_vectorised_and_loop_forms_agree():
    rng = np.random.default_rng(2)
    for trial in range(60):
        shape = (int(rng.integers(1, 15)), int(rng.integers(1, 15)))
        A = ar.random_operand(rng, shape, int(rng.integers(0, 150)))             # duplicates, NaN payloads, +-0, +-Inf
        B = ar.random_operand(rng, shape, int(rng.integers(0, 150)))
        sA = sB = -1
        if trial % 2:
            A, B, sA, sB = ar.sort_storage(A, 0), ar.sort_storage(B, 0), 0, 0     # trusted: duplicates stay
        alpha = float(rng.choice([1.0, 0.0, -2.0, np.inf]))
        for op, comp in FORMS:
            S = er.operands(A, B, op, policy=trial % 3, zero_nan=trial % 4 == 0, sortA=sA, sortB=sB)
            assert ar.same_tuples(er.emult_ref(S[0], S[1], op, alpha, comp), er.emult_ref_loop(S[0], S[1], op, alpha, comp))


def test_first_and_complement_partition_SA():
    rng = np.random.default_rng(3)
    for trial in range(30):
        shape = (9, 11)
        A = ar.sort_storage(ar.random_operand(rng, shape, 120), 0)
        B = ar.random_operand(rng, shape, 60)
        SA, SB = er.operands(A, B, er.FIRST, sortA=0)
        on, off = er.emult_ref(SA, SB, er.FIRST), er.emult_ref(SA, SB, er.FIRST, complement=True)
        assert len(on[2]) + len(off[2]) == len(SA[2])
        # merged back by position in S_A: the two subsequences interleave to S_A itself
        kb = set(zip(SB[0].tolist(), SB[1].tolist()))
        mask = np.array([k in kb for k in zip(SA[0].tolist(), SA[1].tolist())], bool)
        for got, m in ((on, mask), (off, ~mask)):
            assert ar.same_tuples(got, tuple(x[m] for x in SA))


def test_restriction_to_a_selection_is_the_selection():
    rng = np.random.default_rng(4)
    shape = (14, 10)
    A = ar.sort_storage(ar.random_operand(rng, shape, 200), 0)                   # trusted, duplicate keys
    SA = sr.operand_S(A, sort0=0)
    for pred in (sr.TRIL, sr.TRIU, sr.DIAG, sr.OFFDIAG):
        for d in (-3, 0, 2):
            sel = sr.select_ref(SA, shape[0], pred, d)
            assert ar.same_tuples(er.emult_ref(SA, (sel[0], sel[1], None), er.FIRST), sel)
            rest = sr.select_ref(SA, shape[0], pred, d, complement=True)
            assert ar.same_tuples(er.emult_ref(SA, (sel[0], sel[1], None), er.FIRST, complement=True), rest)


def test_intersection_size_against_the_union():
    """|FIRST(A, B)| = |A| + |B| - |pattern of add_ref(A, B)| for unique-key operands whose values cannot cancel (all positive)."""
    rng = np.random.default_rng(5)
    for trial in range(20):
        shape = (12, 9)
        A, B = _plain(rng, shape, int(rng.integers(0, 90))), _plain(rng, shape, int(rng.integers(0, 90)))
        A, B = (A[0], A[1], np.abs(A[2]) + 1.0), (B[0], B[1], np.abs(B[2]) + 1.0)
        union = ar.add_ref(A, B)
        S = er.operands(A, B, er.FIRST)
        assert len(er.emult_ref(S[0], S[1], er.FIRST)[2]) == len(A[2]) + len(B[2]) - len(union[2])


def test_times_pattern_is_the_first_pattern_when_B_holds_no_zeros():
    rng = np.random.default_rng(6)
    shape = (10, 10)
    A = sr.unique_key_operand(rng, shape, 70)                                    # special values in A are fair game
    B = _plain(rng, shape, 60)
    St, Sf = er.operands(A, B, er.TIMES), er.operands(A, B, er.FIRST)
    t, f = er.emult_ref(St[0], St[1], er.TIMES, 0.0), er.emult_ref(Sf[0], Sf[1], er.FIRST)
    assert np.array_equal(t[0], f[0]) and np.array_equal(t[1], f[1])            # alpha = 0: zero and NaN products are emitted


def test_nan_payloads():
    """NaN * x, x * NaN, Inf * 0 and a signalling NaN under alpha = 1, as int64 against numpy's own multiply and against the
    x86 rule written out in dense_ref.mul (the left operand's NaN quieted, else the right one's, else the default NaN)."""
    q, s, neg = 0x7FF80000DEADBEEF, 0x7FF0000000000001, 0xFFF4000000000123
    def f(b):
        return np.array([b], np.uint64).view(np.float64)[0]
    a = np.array([f(q), 2.0, np.inf, f(s), f(neg), 0.0, f(s), -0.0])
    b = np.array([3.0, f(q), 0.0, 1.5, f(q), -np.inf, f(neg), 5.0])
    n = len(a)
    idx = np.arange(n, dtype=np.int32)
    SA, SB = (idx, idx, a), (idx, idx, b)
    for alpha in (1.0, 0.0, -2.0, np.inf):
        got = er.emult_ref(SA, SB, er.TIMES, alpha)[2]
        with np.errstate(all="ignore"):
            scaled = np.float64(alpha) * a
            own = scaled * b
        one_nan = ~(np.isnan(scaled) & np.isnan(b))                             # (two NaNs: numpy's loops may return either)
        assert one_nan.sum() >= 5 and np.array_equal(_bits(got)[one_nan], _bits(own)[one_nan])
        assert np.array_equal(_bits(got), _bits(dr.mul(dr.mul(np.float64(alpha), a), b)))
        assert np.array_equal(_bits(got), _bits(er.emult_ref_loop(SA, SB, er.TIMES, alpha)[2]))
    one = er.emult_ref(SA, SB, er.TIMES, 1.0)[2]
    assert _bits(one)[3] == np.int64(s | (1 << 51))                              # the signalling NaN comes out quieted, payload kept
    assert _bits(one)[2] == np.array([0xFFF8000000000000], np.uint64).view(np.int64)[0]      # Inf * 0: the default NaN
    assert np.array_equal(_bits(er.emult_ref(SA, SB, er.FIRST)[2]), _bits(a))    # FIRST: bits untouched, signalling NaN included


def test_first_of_key_rule_for_a_trusted_B_with_duplicates():
    ra, ca = np.array([0, 1, 1, 2], np.int32), np.array([3, 0, 0, 2], np.int32)
    A = (ra, ca, np.array([2.0, 3.0, 5.0, 7.0]))
    B = (np.array([0, 0, 1, 1, 1, 2], np.int32), np.array([1, 3, 0, 0, 0, 2], np.int32), np.array([9.0, 10.0, 11.0, 12.0, 13.0, 14.0]))
    SA, SB = er.operands(A, B, er.TIMES, sortA=0, sortB=0)
    for fn in (er.emult_ref, er.emult_ref_loop):
        i, j, v = fn(SA, SB, er.TIMES, 1.0)
        assert i.tolist() == [0, 1, 1, 2] and j.tolist() == [3, 0, 0, 2]
        assert v.tolist() == [20.0, 33.0, 55.0, 98.0]                           # both tuples of (1, 0) meet B's first (1, 0): 11
    # raw, the same B is consolidated first: its (1, 0) is 11 + 12 + 13
    SA, SB = er.operands(A, B, er.TIMES, sortA=0)
    assert er.emult_ref(SA, SB, er.TIMES)[2].tolist() == [20.0, 108.0, 180.0, 98.0]
