"""tests/masked_edges.py without a GPU: join_ref pinned to the oracle (tests/masked_ref.py) and its product count to the
oracle's joins, dense_ref pinned to join_ref, and every input of tests/test_gpu_masked_edges.py checked for what it claims:
list lengths, the positions of the matches, the class of every key under every masked_path, and that the reference emits
a key of every kind the case is about (and drops the cancelling ones)."""
import numpy as np
import pytest

from oracle import binding as orc
from tests import add_ref as ar
from tests import masked_edges as me
from tests import masked_ref as mr

CS = (1.0, -0.75, 3.1)


def _unique_operand(rng, shape, nnz):
    nnz = min(nnz, shape[0] * shape[1])
    k = rng.choice(shape[0] * shape[1], nnz, replace=False)
    return (k // shape[1]).astype(np.int32), (k % shape[1]).astype(np.int32), rng.standard_normal(nnz)


def _op(X, shape, t):
    return ((X[1], X[0], X[2]), shape[::-1]) if t == 'T' else (X, shape)


def _oracle_products(A, ashape, B, bshape, M, scalei, scalej, scalek):
    """The terms the reference adds, counted by the oracle's own joins: join2 of the two lists, join3 under scalej."""
    ap, ak, _ = me._lists(A[0], A[1], A[2], ashape[0])
    bp, bk, _ = me._lists(B[1], B[0], B[2], bshape[1])
    iok, _ = me._dense_scale(scalei, ashape[0])
    jok, _ = me._dense_scale(scalek, bshape[1])
    n = 0
    for i, j in zip(*(x.tolist() for x in me.mask_keys(M, bshape[1]))):
        if iok[i] and jok[j]:
            a, b = ak[ap[i]:ap[i + 1]], bk[bp[j]:bp[j + 1]]
            n += len(orc.join2(a, b) if scalej is None else orc.join3(a, scalej[0], b))
    return n


@pytest.mark.parametrize("block", range(3))
def test_join_ref_matches_masked_ref(block):
    """300 seeded NaN-free cases: dimensions 1..39, up to 600 tuples per operand, both transposes, the three scales
    present or absent with missing and zero entries, C in {1, -0.75, 3.1}: every index and every bit of every value, and
    the number of terms."""
    for seed in range(block * 100, block * 100 + 100):
        rng = np.random.default_rng(7000 + seed)
        nrow, inner, ncol = (int(x) for x in rng.integers(1, 40, 3))
        tA, tB = ('.', 'T')[seed % 2], ('.', 'T')[(seed // 2) % 2]
        ash = (inner, nrow) if tA == 'T' else (nrow, inner)
        bsh = (ncol, inner) if tB == 'T' else (inner, ncol)
        A, B = _unique_operand(rng, ash, int(rng.integers(0, 601))), _unique_operand(rng, bsh, int(rng.integers(0, 601)))
        sc = [mr.random_scale(rng, d, bool((seed // 4 >> n) & 1)) for n, d in enumerate((nrow, inner, ncol))]
        ov = [None if s is None else orc.Vec(s[0], s[1], d) for s, d in zip(sc, (nrow, inner, ncol))]
        M = mr.random_mask(rng, (nrow, ncol), int(rng.integers(1, 900)))
        C_ = CS[seed % 3]
        want = mr.masked_ref(orc.Mat(*A, ash), orc.Mat(*B, bsh), M, C_, ov[0], tA, ov[1], tB, ov[2])
        (Ao, asho), (Bo, bsho) = _op(A, ash, tA), _op(B, bsh, tB)
        got = me.join_ref(Ao, asho, Bo, bsho, M, C_, *sc)
        assert ar.same_tuples(got[:3], want), "seed %d" % seed
        assert got[3] == _oracle_products(Ao, asho, Bo, bsho, M, *sc), "seed %d" % seed


def test_dense_ref_matches_join_ref():
    for seed in range(60):
        rng = np.random.default_rng(8000 + seed)
        nrow, ncol, inner = int(rng.integers(1, 41)), int(rng.integers(1, 41)), int(rng.integers(1, 17))
        A = _unique_operand(rng, (nrow, inner), int(rng.integers(0, nrow * inner + 1)))
        B = _unique_operand(rng, (inner, ncol), int(rng.integers(0, inner * ncol + 1)))
        sc = [mr.random_scale(rng, d, bool((seed >> n) & 1)) for n, d in enumerate((nrow, inner, ncol))]
        mi, mj = np.divmod(np.arange(nrow * ncol), ncol)
        want = me.join_ref(A, (nrow, inner), B, (inner, ncol), (mi, mj), CS[seed % 3], *sc)
        got = me.dense_ref(A, (nrow, inner), B, (inner, ncol), CS[seed % 3], *sc)
        assert ar.same_tuples(got[:3], want[:3]) and got[3] == want[3], "seed %d" % seed


def test_classes():
    la = np.array([0, 5, 31, 32, 32, 4096, 4097, 4097, 40])
    lb = np.array([5, 0, 40, 31, 32, 1, 1, 5000, 40])
    ok = (la > 0) & (la <= me.MASK_ROW_CAP)
    N, E, R, W = me.NONE, me.ENTRY, me.ROW, me.WAVE
    assert me.classes(la, lb, 0, ok).tolist() == [N, N, E, E, W, E, E, W, W]
    assert me.classes(la, lb, 1, ok).tolist() == [N, N, E, E, E, E, E, E, E]
    assert me.classes(la, lb, 2, ok).tolist() == [N, N, R, R, R, R, E, E, R]
    assert me.classes(la, lb, 3, ok).tolist() == [N, N, W, W, W, W, W, W, W]
    assert me.classes(la, lb, 3, ok, np.arange(9) != 4).tolist() == [N, N, W, W, N, W, W, W, W]


# ------------------------------------------------------------------------------------------------ the inputs

def _lists_of(case):
    ap, ak, _ = me._lists(case.A[0], case.A[1], case.A[2], case.ashape[0])
    bp, bk, _ = me._lists(case.B[1], case.B[0], case.B[2], case.bshape[1])
    return (lambda i: ak[ap[i]:ap[i + 1]]), (lambda j: bk[bp[j]:bp[j + 1]])


def _table(case, scalej=True):
    """{(i, j): (la, lb, allowed, matched, products, sum)} of the case's keys."""
    t = me.join_keys(case.A, case.ashape, case.B, case.bshape, case.M, case.scalei, case.scalej if scalej else None, case.scalek)
    return {(int(r[0]), int(r[1])): r[2:] for r in zip(*t)}


def _emitted(name, scalej=True):
    i, j, v, _ = me.reference(name, scalej)
    assert not np.isnan(v).any() and np.all(v != 0)
    return set(zip(i.tolist(), j.tolist()))


def _check_pairs(case, name, scalej=True):
    """Every key that claims its lists' lengths and its matches has them; returns the keys by kind."""
    row, col = _lists_of(case)
    tab, kinds = _table(case, scalej), {}
    for c in case.info:
        a, b = row(c["i"]), col(c["j"])
        assert (a.size, b.size) == (c["la"], c["lb"]) == tuple(tab[c["i"], c["j"]][:2])
        if "match" in c:
            short, long_ = (a, b) if c["a_short"] else (b, a)
            assert short.size <= long_.size
            assert np.array_equal(np.intersect1d(a, b), short[list(c["match"])]), (name, c["kind"])
        kinds.setdefault(c["kind"], []).append((c["i"], c["j"]))
    return tab, kinds


def _check_cancel(tab, kinds, emitted):
    assert kinds["cancel"]
    for key in kinds["cancel"]:
        assert tab[key][4] == 2 and tab[key][5] == 0 and key not in emitted


def test_short_case():
    case = me.short_case()
    for sj in (True, False):
        tab, kinds = _check_pairs(case, "short", sj)
        emitted = _emitted("short", sj)
        _check_cancel(tab, kinds, emitted)
        seen = set()
        for c in case.info:
            key, t = (c["i"], c["j"]), tab[c["i"], c["j"]]
            if c["kind"] == "cancel":
                continue
            assert t[3] == len(c["match"]) and t[4] == t[3] - (c["skipped"] if sj else 0)
            if t[4]:
                assert key in emitted
                seen.add((c["la"], c["lb"], c["kind"]))
        for la in me.SHORT_LENS:
            for lb in me.SHORT_LENS:
                for kind in ("all", "first", "last", "alternate"):
                    assert (la, lb, kind) in seen, (la, lb, kind)
    assert all(c["skipped"] == 1 for c in case.info if c["kind"] == "all" and min(c["la"], c["lb"]) >= 7)
    t, cls = me.case_classes(case, 0)
    assert set(cls.tolist()) == {me.ENTRY}                              # every list is shorter than MASK_WAVE_MIN
    assert set(me.case_classes(case, 2)[1].tolist()) == {me.ROW} and set(me.case_classes(case, 3)[1].tolist()) == {me.WAVE}


def test_gallop_case():
    case = me.gallop_case()
    row, col = _lists_of(case)
    tab, kinds = _check_pairs(case, "gallop")
    emitted = _emitted("gallop")
    _check_cancel(tab, kinds, emitted)
    variants = set()
    for c in case.info:
        if c["kind"] == "cancel":
            continue
        a, b = row(c["i"]), col(c["j"])
        short, long_ = (a, b) if c["a_short"] else (b, a)
        assert 12 <= short.size <= 40 and long_.size == me.GALLOP_LONG
        pos = np.searchsorted(long_, np.intersect1d(a, b))
        assert tuple(pos) == c["pos_long"] and tuple(np.diff(pos)) == c["gaps"]
        if c["variant"] == "ends_on_last":
            assert pos[-1] == long_.size - 1
        if c["variant"] == "short_beyond":
            assert short[-1] > long_[-1] and short[-2] > long_[-1]
        if c["variant"] == "short_below":
            assert short[0] < long_[0] and short[1] < long_[0]
        t = tab[c["i"], c["j"]]
        assert 0 < t[4] < t[3] and (c["i"], c["j"]) in emitted          # scalej skipped a matched k, the key is emitted
        variants.add((c["a_short"], c["variant"], c["gaps"] == me.GAPS))
    assert {g for c in case.info if "gaps" in c for g in c["gaps"]} == set(me.GAPS)
    assert variants >= {(r, v, True) for r in (True, False) for v in ("plain", "ends_on_last", "short_beyond", "short_below")}
    _, cls = me.case_classes(case, 0)
    assert {me.ENTRY, me.WAVE} == set(cls.tolist())                    # short lists of 12..40: both sides of MASK_WAVE_MIN
    assert set(me.case_classes(case, 1)[1].tolist()) == {me.ENTRY}


def test_wave_case():
    case = me.wave_case()
    for sj in (True, False):
        tab, kinds = _check_pairs(case, "wave", sj)
        emitted = _emitted("wave", sj)
        _check_cancel(tab, kinds, emitted)
        seen, skipped2 = set(), set()
        for c in case.info:
            t = tab[c["i"], c["j"]]
            assert min(c["la"], c["lb"]) == c["s"] and max(c["la"], c["lb"]) == c["l"] and t[3] == len(c["match"])
            if c["kind"] != "cancel" and t[4]:
                assert (c["i"], c["j"]) in emitted
                seen.add((c["s"], c["l"] - c["s"] if c["l"] != me.WAVE_LONG else "long", c["kind"], c["a_short"]))
            if t[3] - t[4] >= 2 and t[4] > 0:
                skipped2.add((c["s"], c["a_short"]))
        for s in me.WAVE_S:
            for l in (0, 1, "long"):
                for name, match, _, _ in me.wave_patterns(s):
                    for a_short in (True, False):
                        # (under scalej a key may lose its only term to another key's missing k)
                        assert not match or sj or (s, l, name, a_short) in seen, (s, l, name, a_short)
        if sj:
            assert skipped2 >= {(s, r) for s in me.WAVE_S if s >= 31 for r in (True, False)}
            # every pattern still has an emitted key on every step edge, in both roles, under scalej
            for name in ("all", "first", "last", "e63", "e64", "e63_e64", "long_ends_63_64", "long_ends_127_128"):
                for a_short in (True, False):
                    assert any(k[2] == name and k[3] == a_short for k in seen), name
    row, col = _lists_of(case)
    for c in case.info:
        a, b = row(c["i"]), col(c["j"])
        short, long_ = (a, b) if c["a_short"] else (b, a)
        if c["kind"] == "below":
            assert long_[-1] < short[0]
        if c["kind"] == "above":
            assert long_[0] > short[-1]
        if c["kind"] == "long_ends_63_64":
            assert short[63] <= long_[-1] < short[64]
        if c["kind"] == "long_ends_127_128":
            assert short[127] <= long_[-1] < short[128]
        if c["kind"] == "none":
            assert c["s"] == 1 or (long_[0] < short[-1] and long_[-1] > short[0])       # interleaved
    t, cls = me.case_classes(case, 0)
    want = np.where(np.minimum(t[2], t[3]) >= 32, me.WAVE, me.ENTRY)
    assert np.array_equal(cls, want) and {1, 31} == set(np.minimum(t[2], t[3])[cls == me.ENTRY].tolist())
    assert set(me.case_classes(case, 3)[1].tolist()) == {me.WAVE}


def test_big_inner_case():
    case = me.big_inner_case()
    assert case.ashape[1] == 1 << 31 and case.scalej is None
    tab, kinds = _check_pairs(case, "big_inner", False)
    row, col = _lists_of(case)
    emitted = _emitted("big_inner", False)
    for c in case.info:
        a, b = row(c["i"]), col(c["j"])
        assert a[0] == b[0] == 0 and a[-1] == b[-1] == (1 << 31) - 1 and (c["i"], c["j"]) in emitted
    assert [tuple(sorted((c["la"], c["lb"]))) for c in case.info] == [(65, 5000), (65, 5000), (3, 4)]


def test_row_case():
    case = me.row_case()
    tab, kinds = _check_pairs(case, "row")
    emitted = _emitted("row")
    t, cls = me.case_classes(case, 2)
    mi, mj, la, lb, allowed, matched, products, sums = t
    dead = np.isin(mi, case.claims["missing"] + case.claims["zero"])
    assert len(case.claims["missing"]) == len(case.claims["zero"]) == 3 and np.array_equal(dead, ~allowed)
    assert np.all(cls[dead] == me.NONE) and np.all(cls[lb == 0] == me.NONE)
    live = ~dead & (lb > 0)
    assert np.all(cls[live & (la <= 4096)] == me.ROW) and np.all(cls[live & (la == 4097)] == me.ENTRY)
    assert set(la.tolist()) == set(me.ROW_LENS) and lb.max() == 40 and lb.min() == 0
    for n in me.ROW_LENS:
        widths = {int(np.sum(mi == i)) for i in set(mi[(la == n) & ~dead].tolist())}
        assert widths == set(me.ROW_WIDTHS), (n, widths)
        for w in (255, 256, 257, 600):
            # a row of that width has an emitted key in each pass of the 256 lanes and a NONE key between evaluated ones
            i = [i for i in set(mi[(la == n) & ~dead].tolist()) if np.sum(mi == i) == w][0]
            r = np.flatnonzero(mi == i)
            e = np.array([(i, int(j)) in emitted for j in mj[r]])
            assert e[:256].any() and e[256 * ((w - 1) // 256):].any() and e[-1 if w != 600 else -2]
            assert np.any(cls[r][1:-1] == me.NONE) and cls[r][0] != me.NONE
        # the last staged element (LDS position la - 1) alone decides a key: column 3 holds only k = inner - 1
        keys3 = [(int(i), 3) for i in mi[(la == n) & ~dead & (mj == 3)]]
        assert keys3 and all(k in emitted and tab[k][3] == 1 for k in keys3)
        keys1 = [(int(i), 1) for i in mi[(la == n) & ~dead & (mj == 1)]]
        assert keys1 and all(tab[k][4] == 2 and tab[k][5] == 0 and k not in emitted for k in keys1)      # cancels
    auto = me.case_classes(case, 0)[1]                                   # auto: columns of 32 to 40 tuples go to the wave kernel
    assert np.array_equal(auto[live], np.where(lb[live] >= 32, me.WAVE, me.ENTRY)) and np.any(auto == me.WAVE)


@pytest.mark.parametrize("num_cu", (4, 256, 304))
def test_stride_cases(num_cu):
    c = me.stride_dense_case(num_cu)
    n = me.stride_side(num_cu)
    assert c.claims["keys"] == n * n == len(c.M[0]) and n * n >= 1.1 * c.claims["entry_cap"] > c.claims["entry_cap"]
    assert n * n > c.claims["wave_cap"] and (num_cu < 64 or n * n > c.claims["digest_cap"])
    assert num_cu != 256 or n == 1519
    ca, cb = np.bincount(c.A[0], minlength=n), np.bincount(c.B[1], minlength=n)
    assert ca.min() >= 1 and ca.max() <= 3 and cb.min() >= 1 and cb.max() <= 3 and c.ashape[1] == 8
    i, j, v, products = me.reference("stride_dense", True, num_cu)
    assert np.all(v == np.round(v)) and np.abs(v).max() <= 3 * 49 and 0 < len(v) < n * n and products >= len(v)
    # emitted keys beyond every first pass
    flat = i.astype(np.int64) * n + j
    assert flat.max() >= c.claims["entry_cap"]
    r = me.stride_row_case(num_cu)
    cap = r.claims["row_cap"]
    assert cap == num_cu * 32 and r.claims["rows"] == cap + 300 == r.ashape[0]
    la = np.bincount(r.A[0], minlength=r.ashape[0])
    assert np.array_equal(la, 40 - np.arange(cap + 300) % 40) and np.array_equal(np.bincount(r.M[0]), np.full(cap + 300, 2))
    assert r.claims["shorter_second"] > 0 and r.A[1].max() < 48
    ri, rj, rv, _ = me.reference("stride_row", True, num_cu)
    second = ri >= cap
    assert second.any() and (~second).any()
    # a stale tail would be seen: some second row is shorter than its workgroup's first one, whose tail holds k's of the
    # second row's columns
    t, cls = me.case_classes(r, 2)
    assert set(cls.tolist()) == {me.ROW}


def test_coverage_table(capsys):
    """Prints, per input and masked_path, how many keys each kernel evaluates and how many of those the reference emits
    (value non-zero); asserts that no kernel that an input is meant for is left without an emitted key."""
    lines = ["%-10s %4s  %s" % ("input", "path", "  ".join("%-13s" % n for n in me.CLASS_NAMES))]
    meant = {"short": {0: "entry", 1: "entry", 2: "row", 3: "wave"}, "gallop": {0: "entry", 1: "entry", 2: "row", 3: "wave"},
             "wave": {0: "wave", 1: "entry", 2: "row", 3: "wave"}, "big_inner": {0: "wave", 1: "entry", 2: "row", 3: "wave"},
             "row": {0: "entry", 1: "entry", 2: "row", 3: "wave"}}
    for name, make in me.CASES.items():
        case = make()
        for path in me.PATHS:
            t, cls = me.case_classes(case, path)
            cells = []
            for c in range(4):
                cells.append("%6d/%-6d" % (np.sum(cls == c), np.sum((cls == c) & (t[7] != 0))))
            lines.append("%-10s %4d  %s" % (name, path, "  ".join(cells)))
            c = me.CLASS_NAMES.index(meant[name][path])
            assert np.sum((cls == c) & (t[7] != 0)) > 0, (name, path)
            assert np.sum((cls == me.NONE) & (t[7] != 0)) == 0
    with capsys.disabled():
        print("\nkeys / keys with a non-zero reference value, by class\n" + "\n".join(lines))
