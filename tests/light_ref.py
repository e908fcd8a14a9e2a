"""Seeded inputs for the light-row kernels (k_light.hip) and a record of what each must reach.  Needs numpy and the oracle only
(tests/test_light_host.py pins the records without a GPU; tests/test_gpu_light_edges.py runs the cases).

Every builder works in op-space -- rows of op(A) over the inner index k, rows of op(B) over the columns -- with the tuples
sorted and unique, and stores an operand for '.' or 'T' with the sort0 that both the oracle and the library trust
(Consolidate<>, algorithm.hpp:360).  So the row lengths are exactly the built ones under either flag and explicit zero
values stay in the operands.  A case holds two value sets on one structure: random normals (a wrong summation order
changes bits) and an integer twin (-2 .. 2, zeros included: every sum is exact in any order, for the digest checks)."""
import numpy as np

from oracle import binding as orc

LAYOUTS = ("distinct", "one", "mixed")
# maxlen(A) x maxlen(B): 8, 9, 16, 17, 32, 33 and 64 products, each side of every class limit of the direct kernel
CLASS_SHAPES = [(1, 1), (1, 8), (8, 1), (2, 4), (3, 3), (1, 9), (4, 4), (2, 8), (16, 1), (17, 1), (1, 17), (4, 8), (32, 1), (1, 32),
                (2, 16), (3, 11), (33, 1), (8, 8), (64, 1), (1, 64), (2, 32), (32, 2), (4, 16), (16, 4)]
STEP_OUT = [(5, 13), (65, 1), (1, 65)]                    # 65 products: out of the direct kernel
EXTRA_SHAPES = [(2, 4), (3, 3), (4, 8), (3, 11), (8, 8), (64, 1), (1, 64)]      # with C, scalej, scalek and 'T' as well
KEY_S = (8, 16, 32, 64)
SCALES = np.array([0.5, 1.0, 2.0, -1.0, -2.0])          # scale values: powers of two, so the integer twin stays exact


def s_class(maxp):
    """Slots per row of the direct kernel for a maxlen(A) * maxlen(B) of maxp; None: the product is not all-light."""
    for S in (8, 16, 32, 64):
        if maxp <= S:
            return S
    return None


def wide_variant(ncol, S):
    """Does an all-light product of ncol columns in class S take the wide variant (64-bit keys and addressing)?  The
    narrow key (column << log2 S | A position) needs bits(ncol - 1) + 6 <= 32, and its largest value must stay below
    the 32-bit NOKEY: at S = 64 and 2^26 columns it would not.  (The operand-size rules of the
    narrow variant, 2^29 tuples, are out of any test's reach.)"""
    bits = max(1, int(ncol - 1).bit_length())
    top = ((ncol - 1) << (S.bit_length() - 1)) | (S - 1)
    return bits + 6 > 32 or top >= 0xFFFFFFFF


def rounds(nrow, S, cu):
    """(fewest, most) rounds of the grid-stride loop over groups of 4 * (64 / S) rows among the workgroups of a launch on
    `cu` compute units (at most cu * 32 workgroups), and the rows of the last group."""
    per = 4 * (64 // S)
    nvb = (nrow + per - 1) // per
    grid = min(nvb, cu * 32)
    return nvb // grid, (nvb + grid - 1) // grid, nrow - (nvb - 1) * per


def rows_per_round(S, cu):
    return cu * 32 * 4 * (64 // S)


def pipe_nrows(S, cu):
    """(small, big) row counts of the pipeline cases."""
    G, R = 64 // S, rows_per_round(S, cu)
    return (1, 4 * G - 1, 4 * G, 4 * G + 1), (R - 1, R + 1, 2 * R + 4 * G + 1)


class Case:
    """Operands as stored (A, B: normals; Ai, Bi: the integer twin), the flags and scale vectors that go with them (kw),
    and rec: la, lb (longest rows of op(A), op(B)), maxp, S, rowprod (products per row of op(A), scale vectors aside),
    named rows, ncol."""

    def __init__(self, A, B, Ai, Bi, kw, rec):
        self.A, self.B, self.Ai, self.Bi, self.kw, self.rec = A, B, Ai, Bi, kw, rec

    def operands(self, ints):
        return (self.Ai, self.Bi) if ints else (self.A, self.B)


def _store(r, k, v, shape, t):
    """Op-space tuples, sorted by (r, k) and unique, as the stored operand whose op() they are."""
    if t == "T":
        return orc.Mat(k, r, v, (shape[1], shape[0]), sort0=1)
    return orc.Mat(r, k, v, shape, sort0=0)


def op_rows(M, t):
    """(row, minor, val) of op(M) for a stored operand."""
    return (M.idx1, M.idx0, M.val) if t == "T" else (M.idx0, M.idx1, M.val)


def rowprod(case, kw):
    """Products per row of op(A) as the kernels count them under kw: a row that scalei skips (no entry, or 0) has none, nor
    has an A tuple whose k scalej lacks."""
    rec = case.rec
    r, k, _ = op_rows(case.A, kw.get("tA", "."))
    w = rec["blen"][k].astype(np.int64)
    if kw.get("scalej") is not None:
        w = w * np.isin(k, kw["scalej"].idx)
    rp = np.bincount(r, weights=w, minlength=rec["nrow"]).astype(np.int64)
    si = kw.get("scalei")
    if si is not None:
        on = np.zeros(rec["nrow"], bool)
        on[si.idx[si.val != 0]] = True
        rp[~on] = 0
    return rp


def _ints(rng, n):
    return rng.integers(-2, 3, n).astype(np.float64)


def _scale(rng, n, absent=(), zero=(), p=1.0):
    """Scale vector over n indices: present with probability p, never at `absent`, value 0 at `zero`."""
    on = rng.uniform(size=n) < p
    on[list(zero)] = True
    on[list(absent)] = False
    idx = np.flatnonzero(on)
    val = SCALES[rng.integers(0, SCALES.size, idx.size)]
    val[np.isin(idx, list(zero))] = 0.0
    return orc.Vec(idx, val, n, sort0=0)


def _record(ar_, ak, br, nrow, K, ncol, la, lb, **more):
    blen = np.bincount(br, minlength=K)
    alen = np.bincount(ar_, minlength=nrow)
    rec = dict(la=la, lb=lb, maxp=la * lb, S=s_class(la * lb), nrow=nrow, K=K, ncol=ncol,
               maxlen_a=int(alen.max()), maxlen_b=int(blen.max()), blen=blen,
               rowprod=np.bincount(ar_, weights=blen[ak], minlength=nrow).astype(np.int64))
    rec.update(more)
    return rec


# ------------------------------------------------------------------------------------------------ class edges

def class_case(la, lb, layout, tA=".", tB=".", extra=False):
    """A few dozen rows around the class limit la * lb.  Inner index k: k % 3 == 0 an empty row of op(B), 1 a full one (lb
    tuples), 2 one tuple short (empty when lb == 1).  Named rows (rec["rows"]): full (la tuples on full rows: exactly
    la * lb products), short and short_first (one product less), alt (A tuples alternate between empty and full B rows,
    starting on an empty one), ends (first and last A tuple on empty B rows), absent and zero (full rows that scalei
    skips: no entry, entry 0), cancel (two A tuples x, -x on twin B rows: under the mixed layout every sum is exactly 0),
    zeroed (a full row whose first A value is an explicit 0: in the integer twin, and in the normals under the mixed layout),
    empty rows, random rows, and a second full row at the end.
    Layouts: distinct (every product of op(B) on a column of its own, columns interleaving the A positions), one (every
    B row on the same lb columns: la-term sums), mixed (columns from a small pool, twin rows, an explicit zero in B: the last tuple of the twins, or row 7 when lb == 1).
    kw: scalei always (run the case with and without it); extra adds C != 1, scalej and scalek with absent entries."""
    li = LAYOUTS.index(layout)
    rng = np.random.default_rng([la, lb, li, int(tA == "T") + 2 * int(tB == "T"), int(extra)])
    K = 3 * (max(la, 3) + 2)
    kind = np.arange(K) % 3
    blen = np.where(kind == 1, lb, np.where(kind == 2, lb - 1, 0))
    # ---- op(B)
    if layout == "distinct":
        ncol, perm = lb * K, rng.permutation(K)
        cols = [np.arange(blen[k]) * K + perm[k] for k in range(K)]
    elif layout == "one":
        ncol = 7 * lb + 5
        cols = [3 + 7 * np.arange(blen[k]) for k in range(K)]
    else:
        ncol = lb + 3
        cols = [np.sort(rng.choice(ncol, blen[k], replace=False)) for k in range(K)]
        cols[4] = cols[1].copy()                                    # twins: rows 1 and 4 (both full)
    br = np.repeat(np.arange(K), blen)
    bc = np.concatenate(cols).astype(np.int64)
    bv, bvi = rng.standard_normal(br.size), _ints(rng, br.size)
    if layout == "mixed":
        for v in (bv, bvi):
            v[br == 4] = v[br == 1]
            for k in ((1, 4) if lb > 1 else (7,)):                  # an explicit zero in B
                v[np.flatnonzero(br == k)[-1]] = 0.0
    # ---- op(A)
    full = 3 * np.arange(la) + 1
    if lb > 1:
        short, short_first = full.copy(), full.copy()
        short[la // 2] += 1
        short_first[0] += 1
    else:
        short, short_first = full[:-1], full[1:]
    alt = (3 * (np.arange(la) // 2) + np.arange(la) % 2)
    ends = np.concatenate([[0], full[1:la - 1], [3 * la - 3]]) if la > 1 else np.array([0])
    none = np.zeros(0, np.int64)
    named = [("full", full), ("short", short), ("short_first", short_first), ("empty", none), ("alt", alt), ("ends", ends),
             ("empty2", none), ("absent", full), ("zero", full), ("cancel", np.array([1, 4]) if la > 1 else none), ("zeroed", full)]
    rows = [x[1] for x in named]
    for _ in range(26):
        rows.append(np.sort(rng.choice(K, int(rng.integers(0, la + 1)), replace=False)))
    rows.append(full)
    names = {n: i for i, (n, _) in enumerate(named)}
    names["full_last"] = len(rows) - 1
    nrow = len(rows) + 2                                            # two more empty rows at the bottom
    ar_ = np.repeat(np.arange(len(rows)), [len(x) for x in rows])
    ak = np.concatenate(rows).astype(np.int64)
    av, avi = rng.standard_normal(ar_.size), _ints(rng, ar_.size)
    for v in (av, avi):
        c = np.flatnonzero(ar_ == names["cancel"])
        if c.size:
            v[c[0]] = 1.5 if v is av else 2.0
            v[c[1]] = -v[c[0]]
    avi[np.flatnonzero(ar_ == names["zeroed"])[0]] = 0.0            # an explicit zero in A: the first tuple of a full row
    if layout == "mixed":
        av[np.flatnonzero(ar_ == names["zeroed"])[0]] = 0.0
    kw = {"tA": tA, "tB": tB, "scalei": _scale(rng, nrow, absent=[names["absent"]], zero=[names["zero"]])}
    if extra:
        kw.update(C_=-1.5, scalej=_scale(rng, K, absent=[full[la // 2]], p=0.85), scalek=_scale(rng, ncol, p=0.85))
    rec = _record(ar_, ak, br, nrow, K, ncol, la, lb, rows=names, layout=layout, full_k=full)
    return Case(_store(ar_, ak, av, (nrow, K), tA), _store(br, bc, bv, (K, ncol), tB),
                _store(ar_, ak, avi, (nrow, K), tA), _store(br, bc, bvi, (K, ncol), tB), kw, rec)


def undershoot_case():
    """maxlen(A) * maxlen(B) = 6 * 11 = 66, yet no row has more than 64 products: rows of 6 A tuples meet B rows of at
    most 10 tuples, and the B row of 11 is met by rows of at most 5.  Not all-light by the maxlen rule, so the binned light
    kernels take it with no knob set."""
    rng = np.random.default_rng(66)
    la, lb, K, ncol = 6, 11, 40, 300
    blen = rng.integers(0, 11, K)
    blen[3], blen[10:16] = 11, 10
    br = np.repeat(np.arange(K), blen)
    bc = np.concatenate([np.sort(rng.choice(ncol, n, replace=False)) for n in blen]).astype(np.int64)
    rows = [np.arange(10, 16), np.array([3, 10, 11, 12, 13]), np.zeros(0, np.int64)]
    for _ in range(30):
        n = int(rng.integers(0, 7))
        ks = np.sort(rng.choice(K, n, replace=False))
        rows.append(ks[ks != 3] if n == 6 else ks)
    ar_ = np.repeat(np.arange(len(rows)), [len(x) for x in rows])
    ak = np.concatenate(rows).astype(np.int64)
    nrow = len(rows) + 1
    rec = _record(ar_, ak, br, nrow, K, ncol, la, lb)
    return Case(_store(ar_, ak, rng.standard_normal(ar_.size), (nrow, K), "."), _store(br, bc, rng.standard_normal(br.size), (K, ncol), "."),
                _store(ar_, ak, _ints(rng, ar_.size), (nrow, K), "."), _store(br, bc, _ints(rng, br.size), (K, ncol), "."), {}, rec)


# ------------------------------------------------------------------------------------------------ key width

KEY_NCOLS = ((1 << 26) - 1, 1 << 26, (1 << 26) + 1, 1 << 31)      # 2^31: the widest shape check_operand lets through (spsparse_amd.h)


def key_case(S, ncol, tall=True):
    """An all-light product of class S with ncol columns: la x lb = S x 1 (tall: the largest A position there is) or
    2 x S/2.  Every B row is full, so every row of la A tuples fills the class.  Row `top` has its first and its last A tuple
    on B rows that hold column ncol - 1 (two products on the top column), row `bottom` the same with column 0, row `both`
    (lb > 1) with both columns; the other B rows hold random columns, among them 2^26 - 1 and 2^26 where they exist.  The integer twin holds no zero
    here: a lost product must change its sums."""
    la, lb = (S, 1) if tall else (2, S // 2)
    rng = np.random.default_rng([S, ncol, int(tall)])
    K = 2 * la + 10
    cols = []
    for k in range(K):
        c = set(int(x) for x in rng.integers(1, ncol - 1, lb))
        if k % 5 == 3:
            c.add(min((1 << 26) - (k % 2), ncol - 2))
        while len(c) < lb:
            c.add(int(rng.integers(1, ncol - 1)))
        cols.append(sorted(c)[:lb])
    for k in (0, K - 1):
        cols[k][-1] = ncol - 1
    for k in (1, K - 2):
        cols[k][0] = 0
    if lb > 1:
        for k in (2, K - 3):
            cols[k][0], cols[k][-1] = 0, ncol - 1
    mid = np.arange(3, K - 3)
    def row(first, last):
        return np.concatenate([[first], np.sort(rng.choice(mid, la - 2, replace=False)), [last]]).astype(np.int64)
    named = [("top", row(0, K - 1)), ("bottom", row(1, K - 2)), ("empty", np.zeros(0, np.int64))]
    if lb > 1:
        named.append(("both", row(2, K - 3)))
    rows = [x[1] for x in named]
    for _ in range(9):
        rows.append(np.sort(rng.choice(K, int(rng.integers(0, la + 1)), replace=False)))
    names = {n: i for i, (n, _) in enumerate(named)}
    br = np.repeat(np.arange(K), lb)
    bc = np.array(cols, np.int64).reshape(-1)
    ar_ = np.repeat(np.arange(len(rows)), [len(x) for x in rows])
    ak = np.concatenate(rows).astype(np.int64)
    nrow = len(rows)
    def nz(v):
        return np.where(v == 0, 1.0, v)
    rec = _record(ar_, ak, br, nrow, K, ncol, la, lb, rows=names, wide=wide_variant(ncol, S))
    return Case(_store(ar_, ak, rng.standard_normal(ar_.size), (nrow, K), "."), _store(br, bc, rng.standard_normal(br.size), (K, ncol), "."),
                _store(ar_, ak, nz(_ints(rng, ar_.size)), (nrow, K), "."), _store(br, bc, nz(_ints(rng, br.size)), (K, ncol), "."), {}, rec)


# ------------------------------------------------------------------------------------------------ pipeline rounds

PIPE_SHAPE = {8: (4, 2), 16: (4, 4), 32: (8, 4), 64: (8, 8)}
PIPE_K, PIPE_NCOL = 512, 777


def _unique_pairs(rng, lens, width):
    """Sorted unique (row, x) pairs: lens[r] draws of x in 0 .. width - 1 for row r (repeats merge: a row may get shorter)."""
    r = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    key = np.unique(r * width + rng.integers(0, width, r.size))
    return key // width, key % width


def pipe_case(S, nrow):
    """nrow rows of class S with nothing regular about them: A row lengths random in 0 .. la (row nrow // 2 holds la tuples,
    so the class holds), random inner indices, columns and values; B row lengths random in 0 .. lb (row 5 holds lb); about
    5 % of the rows skipped through scalei (kw)."""
    la, lb = PIPE_SHAPE[S]
    rng = np.random.default_rng([S, nrow])
    br, bc = _unique_pairs(rng, rng.integers(0, lb + 1, PIPE_K), PIPE_NCOL)
    keep = br != 5
    br, bc = np.concatenate([br[keep], np.full(lb, 5)]), np.concatenate([bc[keep], 11 + 97 * np.arange(lb)])
    o = np.lexsort((bc, br))
    br, bc = br[o], bc[o]
    ar_, ak = _unique_pairs(rng, rng.integers(0, la + 1, nrow), PIPE_K)
    star = nrow // 2
    keep = ar_ != star
    ar_, ak = np.concatenate([ar_[keep], np.full(la, star)]), np.concatenate([ak[keep], 5 + 3 * np.arange(la)])
    o = np.lexsort((ak, ar_))
    ar_, ak = ar_[o], ak[o]
    kw = {"scalei": _scale(rng, nrow, p=0.95)}
    rec = _record(ar_, ak, br, nrow, PIPE_K, PIPE_NCOL, la, lb, star=star)
    return Case(_store(ar_, ak, rng.standard_normal(ar_.size), (nrow, PIPE_K), "."), _store(br, bc, rng.standard_normal(br.size), (PIPE_K, PIPE_NCOL), "."),
                _store(ar_, ak, _ints(rng, ar_.size), (nrow, PIPE_K), "."), _store(br, bc, _ints(rng, br.size), (PIPE_K, PIPE_NCOL), "."), kw, rec)
