"""spsamd_multiply_masked at the edges of its kernels (k_masked.hip): a direct reference of the operation and the seeded
inputs of tests/test_gpu_masked_edges.py.  Needs no GPU; tests/test_masked_edges_host.py pins the reference to the oracle
and asserts what every input claims.

    join_ref    for each key of M: A_i and B_j joined in ascending k, the terms summed serially in IEEE doubles
    dense_ref   the same for a complete mask and an inner dimension of at most 16, vectorised over all keys
    classes     k_masked_classify on the host: which kernel a key with lists of la and lb tuples goes to
    *_case      the inputs: operands with unique keys in the '.' orientation, a mask, scale vectors, and `claims`

Python floats and numpy float64 element operations are IEEE doubles without contraction, so for NaN-free inputs every bit
of a value is defined by the order of the terms, which is ascending k."""
import functools
import math
from types import SimpleNamespace

import numpy as np

NONE, ENTRY, ROW, WAVE = 0, 1, 2, 3
CLASS_NAMES = ("none", "entry", "row", "wave")
MASK_SHORT, MASK_WAVE_MIN, MASK_ROW_CAP = 8, 32, 4096          # k_masked.hip
PATHS = (0, 1, 2, 3)                                          # masked_path: auto, entry, row, wave
GRID_WG_PER_CU, DIGEST_WG = 32, 2048                          # the grid-stride launches' caps


# ------------------------------------------------------------------------------------------------ the reference

def _lists(lead, other, val, nlead):
    """(ptr, k, v): the tuples grouped by `lead`, ascending `other` inside a group."""
    lead, other = np.asarray(lead, np.int64), np.asarray(other, np.int64)
    o = np.lexsort((other, lead))
    key = lead[o] * (int(other.max()) + 1 if other.size else 1) + other[o]
    assert np.all(key[1:] > key[:-1]), "operands with unique keys only"
    return np.searchsorted(lead[o], np.arange(nlead + 1)), other[o], np.asarray(val, np.float64)[o]


def _dense_scale(scale, dim):
    """(allowed, value) per index: a missing or zero entry is not allowed; no vector is 1 everywhere."""
    if scale is None:
        return np.ones(dim, bool), np.ones(dim)
    val = np.zeros(dim)
    val[np.asarray(scale[0], np.int64)] = scale[1]
    return val != 0, val


def mask_keys(M, ncol):
    k = np.unique(np.asarray(M[0], np.int64) * ncol + np.asarray(M[1], np.int64))
    return k // ncol, k % ncol


def join_keys(A, ashape, B, bshape, M, scalei=None, scalej=None, scalek=None):
    """Per unique key of M, ascending: (i, j, la, lb, allowed, matched, products, sum).  matched: k in both lists;
    products: those of them in scalej (the terms added); sum: their serial sum from 0.0."""
    nrow, inner = ashape
    ncol = bshape[1]
    assert bshape[0] == inner
    ap, ak, av = _lists(A[0], A[1], A[2], nrow)
    bp, bk, bv = _lists(B[1], B[0], B[2], ncol)
    mi, mj = mask_keys(M, ncol)
    iok, _ = _dense_scale(scalei, nrow)
    jok, _ = _dense_scale(scalek, ncol)
    if scalej is not None:
        sjk, sjv = np.asarray(scalej[0], np.int64), np.asarray(scalej[1], np.float64)
    n = mi.size
    la, lb = ap[mi + 1] - ap[mi], bp[mj + 1] - bp[mj]
    allowed = iok[mi] & jok[mj]
    matched, products, sums = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n)
    for t in np.flatnonzero(allowed & (la > 0) & (lb > 0)).tolist():
        a0, a1, b0, b1 = ap[mi[t]], ap[mi[t] + 1], bp[mj[t]], bp[mj[t] + 1]
        k, ia, ib = np.intersect1d(ak[a0:a1], bk[b0:b1], assume_unique=True, return_indices=True)     # ascending k
        matched[t] = k.size
        if k.size == 0:
            continue
        a, b = av[a0 + ia], bv[b0 + ib]
        if scalej is not None:
            q = np.minimum(np.searchsorted(sjk, k), sjk.size - 1) if sjk.size else np.zeros(k.size, np.int64)
            hit = sjk[q] == k if sjk.size else np.zeros(k.size, bool)
            p = (a[hit] * sjv[q[hit]]) * b[hit]
        else:
            p = a * b
        s = 0.0
        for x in p.tolist():
            s = s + x
        products[t], sums[t] = p.size, s
    return mi, mj, la, lb, allowed, matched, products, sums


def _emit(mi, mj, sums, C_, scalei, scalej_unused, scalek, nrow, ncol):
    _, iv = _dense_scale(scalei, nrow)
    _, jv = _dense_scale(scalek, ncol)
    e = sums != 0                                                   # (a NaN sum is emitted)
    with np.errstate(all="ignore"):
        v = ((sums[e] * np.float64(C_)) * iv[mi[e]]) * jv[mj[e]]
    return mi[e].astype(np.int32), mj[e].astype(np.int32), v


def join_ref(A, ashape, B, bshape, M, C_=1.0, scalei=None, scalej=None, scalek=None):
    """(i, j, v, products) of op(A) * op(B) on M's keys, row-major."""
    mi, mj, _, _, _, _, products, sums = join_keys(A, ashape, B, bshape, M, scalei, scalej, scalek)
    return _emit(mi, mj, sums, C_, scalei, None, scalek, ashape[0], bshape[1]) + (int(products.sum()),)


def dense_ref(A, ashape, B, bshape, C_=1.0, scalei=None, scalej=None, scalek=None):
    """join_ref for the complete mask; inner dimension at most 16."""
    nrow, inner = ashape
    ncol = bshape[1]
    assert bshape[0] == inner and inner <= 16
    a, pa = np.zeros((nrow, inner)), np.zeros((nrow, inner), bool)
    b, pb = np.zeros((inner, ncol)), np.zeros((inner, ncol), bool)
    a[A[0], A[1]], pa[A[0], A[1]] = A[2], True
    b[B[0], B[1]], pb[B[0], B[1]] = B[2], True
    iok, _ = _dense_scale(scalei, nrow)
    jok, _ = _dense_scale(scalek, ncol)
    pa &= iok[:, None]
    pb &= jok[None, :]
    sj = None if scalej is None else dict(zip(np.asarray(scalej[0]).tolist(), np.asarray(scalej[1]).tolist()))
    s, products = np.zeros((nrow, ncol)), 0
    for k in range(inner):
        if sj is not None and k not in sj:
            continue
        ak = a[:, k, None] if sj is None else a[:, k, None] * np.float64(sj[k])
        both = pa[:, k, None] & pb[None, k, :]
        s = np.where(both, s + ak * b[None, k, :], s)
        products += int(pa[:, k].sum()) * int(pb[k, :].sum())
    mi, mj = np.divmod(np.arange(nrow * ncol, dtype=np.int64), ncol)
    return _emit(mi, mj, s.ravel(), C_, scalei, None, scalek, nrow, ncol) + (products,)


def classes(la, lb, path, row_ok, allowed=True):
    """k_masked_classify: the class of keys with |A_i| = la and |B_j| = lb under masked_path = path.  row_ok: the row
    kernel may take the key's mask row (0 < la <= MASK_ROW_CAP and scalei allows it); it does so only under path 2.
    allowed: neither the row's nor the column's scale is missing or zero."""
    la, lb = np.asarray(la), np.asarray(lb)
    if path == 3:
        c = np.full(la.shape, WAVE)
    elif path == 1:
        c = np.full(la.shape, ENTRY)
    elif path == 2:
        c = np.where(row_ok, ROW, ENTRY)
    else:
        c = np.where(np.minimum(la, lb) >= MASK_WAVE_MIN, WAVE, ENTRY)
    return np.where((la > 0) & (lb > 0) & allowed, c, NONE)


def case_classes(case, path, scalej=True):
    """(per-key table of join_keys, class per key) of a case under a path."""
    t = join_keys(case.A, case.ashape, case.B, case.bshape, case.M, case.scalei, case.scalej if scalej else None, case.scalek)
    mi, _, la, lb, allowed = t[:5]
    iok, _ = _dense_scale(case.scalei, case.ashape[0])
    return t, classes(la, lb, path, (la > 0) & (la <= MASK_ROW_CAP) & iok[mi], allowed)


# ------------------------------------------------------------------------------------------------ building inputs

def _vals(rng, n):
    """Values that are no powers of two: +-[1.1, 1.9)."""
    return rng.uniform(1.1, 1.9, n) * rng.choice([-1.0, 1.0], n)


class _Build:
    """Rows of A and columns of B as sorted k lists, the keys of M between them, and what each key claims."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rows, self.cols, self.keys, self.info = [], [], [], []
        self.sj_drop, self.sj_keep = set(), set()

    def _list(self, ks, vs):
        ks = np.asarray(ks, np.int64)
        assert np.all(ks[1:] > ks[:-1])
        return ks, (_vals(self.rng, ks.size) if vs is None else np.asarray(vs, np.float64))

    def row(self, ks, vs=None):
        self.rows.append(self._list(ks, vs))
        return len(self.rows) - 1

    def col(self, ks, vs=None):
        self.cols.append(self._list(ks, vs))
        return len(self.cols) - 1

    def key(self, i, j, **claim):
        self.keys.append((i, j))
        self.info.append(dict(claim, i=i, j=j, la=self.rows[i][0].size, lb=self.cols[j][0].size))

    def pair(self, short, long_, a_short, vshort=None, vlong=None, **claim):
        """A key with a row and a column of its own; a_short: the short list is A's."""
        if a_short:
            i, j = self.row(short, vshort), self.col(long_, vlong)
        else:
            i, j = self.row(long_, vlong), self.col(short, vshort)
        self.key(i, j, a_short=a_short, **claim)

    def finish(self, inner=None, sj_missing=0.0, scalei=None, scalek=None, C_=1.0, **claims):
        rng = self.rng
        top = max([int(k[-1]) for k, _ in self.rows + self.cols if k.size] + [0])
        inner = top + 1 if inner is None else inner
        assert top < inner

        def cat(lists, lead_first):
            lead = np.concatenate([np.full(k.size, x, np.int64) for x, (k, _) in enumerate(lists)] + [np.zeros(0, np.int64)])
            k = np.concatenate([k for k, _ in lists] + [np.zeros(0, np.int64)])
            v = np.concatenate([v for _, v in lists] + [np.zeros(0)])
            o = rng.permutation(k.size)                          # stored unsorted: the call consolidates
            i0, i1 = (lead, k) if lead_first else (k, lead)
            return i0[o].astype(np.int32), i1[o].astype(np.int32), v[o]
        A, B = cat(self.rows, True), cat(self.cols, False)
        M = (np.array([k[0] for k in self.keys], np.int32), np.array([k[1] for k in self.keys], np.int32))
        scalej = None
        if inner <= 1 << 24:
            present = rng.random(inner) >= sj_missing
            present[np.fromiter(self.sj_drop, np.int64, len(self.sj_drop))] = False
            present[np.fromiter(self.sj_keep, np.int64, len(self.sj_keep))] = True
            idx = np.flatnonzero(present).astype(np.int32)
            val = _vals(rng, idx.size)
            val[np.isin(idx, np.fromiter(self.sj_keep, np.int64, len(self.sj_keep)))] = 2.0
            scalej = (idx, val)
        return SimpleNamespace(A=A, ashape=(len(self.rows), inner), B=B, bshape=(inner, len(self.cols)), M=M, C=C_,
                               scalei=scalei, scalej=scalej, scalek=scalek, info=self.info, claims=claims)

    def cancel(self, ks, short_n, long_n, a_short, kind="cancel"):
        """A key whose two matched terms are x and -x exactly ((1.5 * 2) * 2.5 under scalej, whose entries at both k are
        2): products > 0, sum +0, so it must not be emitted.  ks: the two k; the lists are padded with odd k's."""
        k0, k1 = ks
        pad = lambda n, lo: 2 * np.arange(lo, lo + n) + 1
        short = np.sort(np.concatenate([[k0, k1], pad(short_n - 2, k1)]))
        long_ = np.sort(np.concatenate([[k0, k1], pad(long_n - 2, k1 + short_n)]))
        vs = np.full(short.size, 1.5)
        vl = np.where(long_ == k1, -2.5, 2.5)
        self.sj_keep.update((int(k0), int(k1)))
        self.pair(short, long_, a_short, vs, vl, kind=kind, match=(0, 1))


def two_lists(rng, s, l, match, where="inter", cut=None):
    """A short list of s even k's and a long one of l k's that holds short[e] for e in match and odd k's otherwise.
    where: the odd k's lie anywhere over the short list's span ('inter'), all below it or all above it; cut = e: all of
    the long list lies below short[e] and its largest k is short[e - 1] + 1 or short[e - 1] itself."""
    match = np.asarray(sorted(match), np.int64)
    nodd = l - match.size
    assert nodd >= 0 and (cut is None or (match.size == 0 or match[-1] < cut))
    span = 2 * max(s, nodd) + 8
    base = nodd + 1 if (where == "below" or cut is not None) else 0
    x = base + np.sort(rng.choice(span, s, replace=False))
    if cut is not None:
        oddx = rng.choice(int(x[cut]), nodd, replace=False)
        if nodd and x[cut - 1] not in oddx:
            oddx[0] = x[cut - 1]                                    # the long list's largest k: between short[cut - 1] and short[cut]
    elif where == "below":
        oddx = rng.choice(base, nodd, replace=False)
    elif where == "above":
        oddx = int(x[-1]) + 1 + rng.choice(nodd + 4, nodd, replace=False)
    else:
        oddx = rng.choice(base + span, nodd, replace=False)
    short = 2 * x
    return short, np.sort(np.concatenate([short[match], 2 * oddx.astype(np.int64) + 1]))


# ------------------------------------------------------------------------------------------------ b. MASK_SHORT

SHORT_LENS = (1, 7, 8, 9)


@functools.lru_cache(None)
def short_case():
    """la, lb over {1, 7, 8, 9}^2 (8 / 9: the register join against the gallop walk), five match patterns each, every key
    in a k range of its own (64 wide); scalej misses one matched k of every key with at least two; one cancelling key per
    side of the edge."""
    b = _Build(101)
    rng, t = b.rng, 0
    for la in SHORT_LENS:
        for lb in SHORT_LENS:
            s, l = min(la, lb), max(la, lb)
            pats = {"none": (), "all": tuple(range(s)), "first": (0,), "last": (s - 1,), "alternate": tuple(range(0, s, 2))}
            for name, match in pats.items():
                short, long_ = two_lists(rng, s, l, match)
                short, long_ = short + 64 * t, long_ + 64 * t
                assert long_[-1] < 64 * (t + 1) and short[-1] < 64 * (t + 1)
                if len(match) >= 2:
                    b.sj_drop.add(int(short[match[1]]))
                b.pair(short, long_, la <= lb, kind=name, match=match, skipped=int(len(match) >= 2))
                t += 1
    for sn, ln, a_short in ((2, 2, True), (8, 8, True), (8, 9, True), (8, 9, False), (2, 9, False)):
        b.cancel((64 * t + 2, 64 * t + 4), sn, ln, a_short)
        t += 1
    return b.finish()


# ------------------------------------------------------------------------------------------------ c. gallop

GAPS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
GALLOP_LONG = 3000


@functools.lru_cache(None)
def gallop_case():
    """A short list of 12 to 40 elements against a long one of 3000 (even k's); consecutive matches lie GAPS apart in
    the long list, in ascending, descending and shuffled order of the gaps; variants: the last match is the long list's
    final element, the final short element lies beyond the long list's end, the first below its start.  Both roles."""
    b = _Build(102)
    rng = b.rng
    total = sum(GAPS)
    orders = {"up": list(GAPS), "down": list(GAPS)[::-1], "mixed": [int(g) for g in rng.permutation(GAPS)], "half": list(GAPS[:11])}
    for a_short in (True, False):
        for oname, gaps in orders.items():
            for variant in ("plain", "ends_on_last", "short_beyond", "short_below"):
                base = 10
                long_ = 2 * (base + np.arange(GALLOP_LONG))
                first = GALLOP_LONG - 1 - sum(gaps) if variant == "ends_on_last" else int(rng.integers(0, GALLOP_LONG - 1 - total))
                pos = first + np.concatenate([[0], np.cumsum(gaps)])
                extra = {"short_beyond": [long_[-1] + 1, long_[-1] + 7], "short_below": [1, 5]}.get(variant, [])
                nfree = int(rng.integers(0, 40 - pos.size - len(extra) + 1))
                free = 2 * (base + rng.choice(GALLOP_LONG - 1, nfree, replace=False)) + 1        # odd: in no long list
                short = np.sort(np.concatenate([long_[pos], extra, free]).astype(np.int64))
                assert 12 <= short.size <= 40
                b.sj_drop.add(int(long_[pos[2]]))
                b.pair(short, long_, a_short, kind="%s/%s" % (oname, variant), pos_long=tuple(int(p) for p in pos),
                       gaps=tuple(gaps), variant=variant)
    b.cancel((2 * 4000, 2 * 4001), 12, 3000, True)
    b.cancel((2 * 4000, 2 * 4001), 40, 3000, False)
    return b.finish()


# ------------------------------------------------------------------------------------------------ d. wave steps

WAVE_S = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
WAVE_LONG = 5000


def wave_patterns(s):
    """(name, matched short elements, where, cut) for a short list of s elements."""
    p = [("none", (), "inter", None), ("all", tuple(range(s)), "inter", None), ("first", (0,), "inter", None),
         ("last", (s - 1,), "inter", None), ("below", (), "below", None), ("above", (), "above", None)]
    if s > 63:
        p.append(("e63", (63,), "inter", None))
    if s > 64:
        p += [("e64", (64,), "inter", None), ("e63_e64", (63, 64), "inter", None), ("long_ends_63_64", (5, 63), "inter", 64)]
    if s > 128:
        p.append(("long_ends_127_128", (5, 63, 64, 127), "inter", 128))
    return p


@functools.lru_cache(None)
def wave_case():
    """Short lengths over the wave kernel's 64-element steps and MASK_WAVE_MIN, long lengths s (the tie, A short), s + 1
    and 5000, the match patterns of wave_patterns, each with A short and with B short; all lists over one k range.
    scalej misses the second and the second-last k of every 'all' key's short list; cancelling keys whose two terms sit in
    lanes 63 and 0 of consecutive steps."""
    b = _Build(103)
    rng = b.rng
    for s in WAVE_S:
        for l in (s, s + 1, WAVE_LONG):
            for name, match, where, cut in wave_patterns(s):
                if len(match) > l:
                    continue
                for a_short in (True, False):
                    short, long_ = two_lists(rng, s, l, match, where, cut)
                    if name == "all" and s >= 4:
                        b.sj_drop.update((int(short[1]), int(short[s - 2])))
                    b.pair(short, long_, a_short, kind=name, match=match, s=s, l=l)
    # two terms that cancel across the step boundary: short elements 63 and 64
    for a_short in (True, False):
        x = 40000 + np.arange(65)
        short = 2 * x
        long_ = np.sort(np.concatenate([short[[63, 64]], 2 * (x[-1] + 1 + np.arange(64)) + 1]))
        b.sj_keep.update((int(short[63]), int(short[64])))
        b.pair(short, long_, a_short, np.full(65, 1.5), np.where(long_ == short[64], -2.5, 2.5), kind="cancel", match=(63, 64), s=65, l=66)
    return b.finish()


BIG_INNER = 1 << 31          # the largest dimension check_operand accepts; consolidation needs no memory in proportion to it


@functools.lru_cache(None)
def big_inner_case():
    """An inner dimension of 2^31: matches at k = 0 and at k = 2^31 - 1, short lists of 65 (two steps) against 5000, both
    roles, and one key of short lists for the entry kernel's register join.  No scalej (its dense position table would
    take memory in proportion to the inner dimension)."""
    b = _Build(104)
    rng = b.rng
    top = BIG_INNER - 1
    for a_short in (True, False):
        short = np.sort(np.concatenate([[0, top], rng.choice(np.arange(1, top, 2 ** 16), 63, replace=False)]))
        long_ = np.sort(np.concatenate([[0, top], short[[7, 63]], rng.choice(np.arange(2, top, 2 ** 12 + 2), WAVE_LONG - 4, replace=False)]))
        long_ = np.unique(long_)
        b.pair(short, long_, a_short, kind="ends", match=(0, 7, 63, 64))
    b.pair(np.array([0, 5, top]), np.array([0, 6, top - 1, top]), True, kind="short_ends", match=(0, 2))
    return b.finish(inner=BIG_INNER)


# ------------------------------------------------------------------------------------------------ e. row cap and widths

ROW_LENS = (4095, 4096, 4097)
ROW_WIDTHS = (1, 255, 256, 257, 600)
ROW_INNER = 20000


@functools.lru_cache(None)
def row_case():
    """A rows of 4095, 4096 and 4097 tuples (MASK_ROW_CAP) in an inner dimension of 20 000, one mask row of each length
    for each of 1, 255, 256, 257 and 600 keys (one to three passes of the row kernel's 256 lanes), plus one row of each
    length that scalei lacks and one whose scalei entry is 0.  600 B columns of 0 to 40 tuples; every A row holds k = 0
    and k = inner - 1 (its first and last staged element) with value 1.5, column 1 holds only those two k's with 2.5 and
    -2.5 (cancels), columns 2 and 3 one of them each; every fifth column is empty (class NONE inside a row)."""
    b = _Build(105)
    rng = b.rng
    top = ROW_INNER - 1
    for j in range(600):
        if j == 1:
            b.col([0, top], [2.5, -2.5])
        elif j == 2:
            b.col([0])
        elif j == 3:
            b.col([top])
        elif j % 5 == 4:
            b.col([])
        else:
            b.col(np.sort(rng.choice(ROW_INNER, int(rng.integers(1, 41)), replace=False)))
    missing, zero = [], []
    for la in ROW_LENS:
        for w in ROW_WIDTHS + ("missing", "zero"):
            ks = np.sort(np.concatenate([[0, top], 1 + rng.choice(ROW_INNER - 2, la - 2, replace=False)]))
            v = _vals(rng, la)
            v[0] = v[-1] = 1.5
            i = b.row(ks, v)
            if w == "missing":
                missing.append(i)
            elif w == "zero":
                zero.append(i)
            width = 257 if isinstance(w, str) else w
            cols = [0] if width == 1 else np.sort(rng.choice(600, width, replace=False)) if width < 600 else np.arange(600)
            if 1 < width < 600:
                cols = np.unique(np.concatenate([[1, 2, 3, 4], cols]))[:width]
            for j in cols:
                b.key(i, int(j), kind="row", width=w)
    b.sj_keep.update((0, top))
    nrow = len(b.rows)
    idx = np.array([i for i in range(nrow) if i not in missing], np.int32)
    val = _vals(rng, idx.size)
    val[np.isin(idx, zero)] = 0.0
    return b.finish(inner=ROW_INNER, sj_missing=0.02, scalei=(idx, val), C_=-0.75, missing=tuple(missing), zero=tuple(zero))


# ------------------------------------------------------------------------------------------------ f. grid strides

def stride_side(num_cu):
    """Side of the complete mask whose keys exceed the entry launch's num_cu * 32 workgroups of 256 keys by 10 %."""
    return int(math.ceil(math.sqrt(1.1 * num_cu * GRID_WG_PER_CU * 256)))


@functools.lru_cache(None)
def stride_dense_case(num_cu):
    """side x 8 times 8 x side on the complete mask: every A row and B column has 1 to 3 tuples of small integers (every
    sum exact in any order).  side^2 keys exceed the entry kernel's num_cu * 32 * 256, the wave kernel's num_cu * 32 * 4
    and the digest kernel's 2048 * 256."""
    rng = np.random.default_rng(106)
    n, inner = stride_side(num_cu), 8

    def operand():
        cnt = rng.integers(1, 4, n)
        lead = np.repeat(np.arange(n), cnt)
        k = np.concatenate([rng.choice(inner, c, replace=False) for c in cnt.tolist()])
        v = rng.integers(1, 8, lead.size) * rng.choice([-1.0, 1.0], lead.size)
        return lead.astype(np.int32), k.astype(np.int32), v
    A = operand()
    bl, bk, bv = operand()
    mi, mj = np.divmod(np.arange(n * n, dtype=np.int64), n)
    return SimpleNamespace(A=A, ashape=(n, inner), B=(bk, bl, bv), bshape=(inner, n), M=(mi.astype(np.int32), mj.astype(np.int32)),
                           C=1.0, scalei=None, scalej=None, scalek=None, info=None,
                           claims=dict(keys=n * n, entry_cap=num_cu * GRID_WG_PER_CU * 256, wave_cap=num_cu * GRID_WG_PER_CU * 4,
                                       digest_cap=DIGEST_WG * 256))


@functools.lru_cache(None)
def stride_row_case(num_cu):
    """num_cu * 32 + 300 mask rows of 2 keys over 64 columns, for masked_path = 2: the first 300 workgroups of the row
    kernel take a second row.  The A row lengths cycle through 40, 39, ..., 1 with every k below 48, so a second row that
    is shorter than the first would match against the first one's stale LDS tail."""
    rng = np.random.default_rng(107)
    cap = num_cu * GRID_WG_PER_CU
    nrow, ncol, inner = cap + 300, 64, 48
    la = 40 - np.arange(nrow) % 40
    ai = np.repeat(np.arange(nrow), la)
    ak = np.concatenate([np.sort(rng.choice(inner, n, replace=False)) for n in la.tolist()])
    lb = rng.integers(1, 7, ncol)
    bj = np.repeat(np.arange(ncol), lb)
    bk = np.concatenate([rng.choice(inner, n, replace=False) for n in lb.tolist()])
    mj = np.stack([rng.integers(0, 32, nrow), rng.integers(32, 64, nrow)], 1).ravel()
    second = np.arange(300) + cap
    return SimpleNamespace(A=(ai.astype(np.int32), ak.astype(np.int32), _vals(rng, ai.size)), ashape=(nrow, inner),
                           B=(bk.astype(np.int32), bj.astype(np.int32), _vals(rng, bj.size)), bshape=(inner, ncol),
                           M=(np.repeat(np.arange(nrow), 2).astype(np.int32), mj.astype(np.int32)),
                           C=1.0, scalei=None, scalej=None, scalek=None, info=None,
                           claims=dict(rows=nrow, row_cap=cap, la=la, shorter_second=int(np.sum(la[second] < la[second - cap]))))


CASES = {"short": short_case, "gallop": gallop_case, "wave": wave_case, "big_inner": big_inner_case, "row": row_case}


@functools.lru_cache(None)
def reference(name, scalej=True, num_cu=0):
    """join_ref / dense_ref of a case, computed once per process and shared (read-only) by the tests."""
    if name == "stride_dense":
        c = stride_dense_case(num_cu)
        return dense_ref(c.A, c.ashape, c.B, c.bshape)
    c = stride_row_case(num_cu) if name == "stride_row" else CASES[name]()
    return join_ref(c.A, c.ashape, c.B, c.bshape, c.M, c.C, c.scalei, c.scalej if scalej else None, c.scalek)
