"""The inputs of tests/test_gpu_light_edges.py have the properties their records claim (tests/light_ref.py).  No GPU: an
edit to a builder cannot quietly make a GPU test vacuous."""
import numpy as np
import pytest

from oracle import binding as orc
from tests import light_ref as lr
from tests.light_ref import CLASS_SHAPES, EXTRA_SHAPES, KEY_S, STEP_OUT


def _lens(M, t, n):
    return np.bincount(lr.op_rows(M, t)[0], minlength=n)


def _sorted_unique(M, t):
    r, k, _ = lr.op_rows(M, t)
    key = r.astype(np.int64) * (1 << 32) + k
    return np.all(np.diff(key) > 0)


def _check_record(c):
    """maxlen, class and per-row products of the record against the stored operands, for both value sets."""
    rec, tA, tB = c.rec, c.kw.get("tA", "."), c.kw.get("tB", ".")
    for A, B in (c.operands(False), c.operands(True)):
        assert _sorted_unique(A, tA) and _sorted_unique(B, tB)
        alen, blen = _lens(A, tA, rec["nrow"]), _lens(B, tB, rec["K"])
        assert (alen.max(), blen.max()) == (rec["la"], rec["lb"]) == (rec["maxlen_a"], rec["maxlen_b"])
        r, k, _ = lr.op_rows(A, tA)
        assert np.array_equal(np.bincount(r, weights=blen[k], minlength=rec["nrow"]).astype(np.int64), rec["rowprod"])
        shape_a = A.shape[::-1] if tA == "T" else A.shape
        shape_b = B.shape[::-1] if tB == "T" else B.shape
        assert shape_a == (rec["nrow"], rec["K"]) and shape_b == (rec["K"], rec["ncol"])
    assert rec["maxp"] == rec["la"] * rec["lb"] and rec["S"] == lr.s_class(rec["maxp"])


def test_class_and_variant_rules():
    assert [lr.s_class(p) for p in (1, 8, 9, 16, 17, 32, 33, 64, 65)] == [8, 8, 16, 16, 32, 32, 64, 64, None]
    n = 1 << 26
    # narrow while bits(ncol - 1) + 6 <= 32; the one narrow key that would equal NOKEY (S = 64, column 2^26 - 1, position 63) goes wide
    assert [lr.wide_variant(n - 1, S) for S in (8, 16, 32, 64)] == [False] * 4
    assert [lr.wide_variant(n, S) for S in (8, 16, 32, 64)] == [False, False, False, True]
    assert [lr.wide_variant(n + 1, S) for S in (8, 16, 32, 64)] == [True] * 4
    assert not lr.wide_variant(1 << 24, 64) and not lr.wide_variant(1 << 24, 32)       # BASELINE cfg3 and cfg5 stay narrow
    assert lr.KEY_NCOLS == (n - 1, n, n + 1, 1 << 31)
    # the shapes cover each side of every class limit
    assert sorted({a * b for a, b in CLASS_SHAPES}) == [1, 8, 9, 16, 17, 32, 33, 64]
    assert sorted({a * b for a, b in STEP_OUT}) == [65]


@pytest.mark.parametrize("la,lb", CLASS_SHAPES + STEP_OUT)
@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_class_case(la, lb, layout):
    c = lr.class_case(la, lb, layout)
    _check_record(c)
    rec, P = c.rec, la * lb
    rows, rp = rec["rows"], rec["rowprod"]
    assert 30 <= rec["nrow"] <= 60
    assert rp[rows["full"]] == rp[rows["full_last"]] == rp[rows["absent"]] == rp[rows["zero"]] == P == rp.max()
    assert rp[rows["short"]] == rp[rows["short_first"]] == P - 1
    assert rp[rows["empty"]] == rp[rows["empty2"]] == rp[-1] == rp[-2] == 0
    r, k, av = lr.op_rows(c.A, ".")
    blen = rec["blen"]
    # alt: the A tuples alternate between empty and non-empty B rows; ends: the first and last ones hit empty rows
    alt = blen[k[r == rows["alt"]]]
    assert alt.size == la and np.all(alt[0::2] == 0) and np.all(alt[1::2] == lb)
    ends = blen[k[r == rows["ends"]]]
    assert ends.size == la and ends[0] == 0 and ends[-1] == 0 and np.all(ends[1:-1] == lb)
    # scalei: no entry for `absent`, a zero for `zero`, both rows would otherwise emit
    si = c.kw["scalei"]
    assert rows["absent"] not in si.idx and si.val[np.searchsorted(si.idx, rows["zero"])] == 0
    plain = orc.multiply(c.A, c.B, rowwise=True)
    scaled = orc.multiply(c.A, c.B, rowwise=True, scalei=si)
    for x in ("absent", "zero"):
        assert np.any(plain[0] == rows[x]) and not np.any(scaled[0] == rows[x])
    # the layouts: emitted tuples per row against products per row
    for ints in (False, True):
        A, B = c.operands(ints)
        wi = orc.multiply(A, B, rowwise=True)[0]
        emitted = np.bincount(wi, minlength=rec["nrow"])
        if layout == "distinct" and not ints:
            assert np.array_equal(emitted, rp)                         # every product a tuple of its own
        if layout == "one" and not ints:
            assert emitted[rows["full"]] == lb                         # la-term sums (64 terms on one column for 64 x 1)
        if layout == "mixed":
            assert np.any(emitted < rp)
            if la > 1:                                                 # x * b + (-x) * b: exactly 0 on every column
                assert rp[rows["cancel"]] == 2 * lb and emitted[rows["cancel"]] == 0
    if layout == "mixed":
        assert np.any(c.A.val == 0) and np.any(c.B.val == 0)           # explicit zeros stay in the trusted operands
    assert np.any(c.Ai.val == 0) and set(np.unique(c.Ai.val)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}


@pytest.mark.parametrize("la,lb", EXTRA_SHAPES)
@pytest.mark.parametrize("tA,tB", [("T", "."), (".", "T"), ("T", "T")])
def test_class_case_transposed_keeps_the_row_lengths(la, lb, tA, tB):
    c = lr.class_case(la, lb, "mixed", tA, tB, extra=True)
    _check_record(c)
    assert c.rec["rowprod"].max() == la * lb == c.rec["rowprod"][c.rec["rows"]["full"]]
    sj, sk = c.kw["scalej"], c.kw["scalek"]
    assert c.rec["full_k"][la // 2] not in sj.idx and sj.nnz < c.rec["K"]      # a term of the full row is dropped
    assert sk.nnz < c.rec["ncol"] or c.rec["ncol"] < 8
    assert c.kw["C_"] != 1.0
    # the integer twin stays exact under the scale vectors: its values are multiples of 1/16 far below 2^53
    v = orc.multiply(c.Ai, c.Bi, rowwise=True, **c.kw)[2]
    assert np.all(v * 16 == np.round(v * 16)) and np.abs(v).sum() < 1e9


def test_undershoot_case():
    c = lr.undershoot_case()
    _check_record(c)
    assert c.rec["maxp"] == 66 and c.rec["S"] is None and 60 <= c.rec["rowprod"].max() <= 64
    assert np.any(c.rec["rowprod"] == 0)


@pytest.mark.parametrize("S", KEY_S)
@pytest.mark.parametrize("ncol", lr.KEY_NCOLS)
@pytest.mark.parametrize("tall", [True, False])
def test_key_case(S, ncol, tall):
    c = lr.key_case(S, ncol, tall)
    _check_record(c)
    rec = c.rec
    rows, la, lb = rec["rows"], rec["la"], rec["lb"]
    assert rec["S"] == S == la * lb and rec["wide"] == lr.wide_variant(ncol, S) and c.B.shape[1] == ncol
    assert c.A.nnz < 1000 and c.B.nnz < 1000
    r, k, _ = lr.op_rows(c.A, ".")
    br, bc, _ = lr.op_rows(c.B, ".")
    for name, col in (("top", ncol - 1), ("bottom", 0)) + ((("both", 0), ("both", ncol - 1)) if lb > 1 else ()):
        ks = k[r == rows[name]]
        assert ks.size == la and rec["rowprod"][rows[name]] == S                  # the row fills its class
        for kk in (ks[0], ks[-1]):                                                # first and last A tuple: their B rows hold the column
            assert col in bc[br == kk]
        assert sum(int(np.sum(bc[br == kk] == col)) for kk in ks) == 2            # two products on it
    wi, wj, _, _ = orc.multiply(c.A, c.B, rowwise=True)
    for name, col in (("top", ncol - 1), ("bottom", 0)):
        assert np.sum((wi == rows[name]) & (wj == col)) == 1                      # the oracle emits the pair's sum
    assert not np.any(c.Ai.val == 0) and not np.any(c.Bi.val == 0)                # (twin: no zero term hides a lost product)


@pytest.mark.parametrize("cu", [256, 32])
@pytest.mark.parametrize("S", KEY_S)
def test_pipeline_rounds(S, cu):
    G, R = 64 // S, lr.rows_per_round(S, cu)
    small, big = lr.pipe_nrows(S, cu)
    assert R == {8: 1024, 16: 512, 32: 256, 64: 128}[S] * cu
    assert small == (1, 4 * G - 1, 4 * G, 4 * G + 1) and big == (R - 1, R + 1, 2 * R + 4 * G + 1)
    for n in small:
        assert lr.rounds(n, S, cu)[:2] == (1, 1)
    assert lr.rounds(R - 1, S, cu) == (1, 1, 4 * G - 1)                    # one round, the last group a row short
    assert lr.rounds(R, S, cu) == (1, 1, 4 * G)
    assert lr.rounds(R + 1, S, cu) == (1, 2, 1)                            # one workgroup takes a second round of one row
    assert lr.rounds(2 * R + 4 * G + 1, S, cu) == (2, 3, 1)                # three rounds beside two, a ragged last group


@pytest.mark.parametrize("S", KEY_S)
def test_pipe_case(S):
    """The cases themselves at 32 compute units (the builder does not depend on the count): nothing repeats at distance R."""
    cu = 32
    R = lr.rows_per_round(S, cu)
    nrow = lr.pipe_nrows(S, cu)[1][2]
    c = lr.pipe_case(S, nrow)
    _check_record(c)
    rec = c.rec
    assert rec["S"] == S and rec["nrow"] == nrow and rec["rowprod"].max() <= S
    r, k, v = lr.op_rows(c.A, ".")
    alen = np.bincount(r, minlength=nrow)
    assert alen[rec["star"]] == rec["la"] and set(np.unique(alen)) == set(range(rec["la"] + 1))
    # a row and the row R below it: different lengths or different first tuples nearly everywhere
    ptr = np.concatenate([[0], np.cumsum(alen)])
    both = (alen[:-R] > 0) & (alen[R:] > 0)
    first_k, first_v = k[np.minimum(ptr[:-1], k.size - 1)], v[np.minimum(ptr[:-1], k.size - 1)]
    same = both & (alen[:-R] == alen[R:]) & (first_k[:-R] == first_k[R:])
    assert same.sum() < 0.01 * both.sum() and not np.any(both & (first_v[:-R] == first_v[R:]))
    si = c.kw["scalei"]
    assert 0.03 * nrow < nrow - si.nnz < 0.07 * nrow
    for n in lr.pipe_nrows(S, cu)[0]:
        s = lr.pipe_case(S, n)
        _check_record(s)
        assert s.rec["nrow"] == n
