"""The full-size value checks (tests/projection.py) checked on the CPU: on oracle products their projections stay inside
the linearity bound (bit for bit for integer stencils with integer weights), each typical rank/scatter bug is flagged,
and the chunked COO reducer does not depend on its chunk size."""
import numpy as np
import pytest

import projection as pj
from oracle import binding as orc
from spsparse_amd import workloads as wl


def _rand(rng, shape, nnz, signed=False):
    i = rng.integers(0, shape[0], nnz)
    j = rng.integers(0, shape[1], nnz)
    v = rng.uniform(0.5, 2.0, nnz)
    if signed:
        v *= rng.choice([-1.0, 1.0], nnz)
    return i.astype(np.int32), j.astype(np.int32), v, shape      # duplicates kept


def _scale(rng, n, signed=False):
    """Dense scale vector with some entries absent (0); the oracle gets only the present ones."""
    s = rng.uniform(0.5, 2.0, n) * (rng.choice([-1.0, 1.0], n) if signed else 1.0)
    s[rng.random(n) < 0.15] = 0.0
    return s


def _vec(s):
    if s is None:
        return None
    idx = np.nonzero(s)[0]
    return orc.Vec(idx, s[idx], s.size, sort0=0)


def _signed(x):
    i, j, v, shape = x
    return i, j, v * pj.sign_of(i, j), shape


def _case(name):
    """(a, b, kwargs of the product, weight kind)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "random":
        return _rand(rng, (300, 400), 3000), _rand(rng, (400, 250), 3000), {}, "real"
    if name == "rmat11_signed_AB":
        return _signed(wl.rmat(11, seed=3)), _signed(wl.rmat(11, seed=4)), {}, "real"
    if name.startswith("rmat"):
        a = wl.rmat(int(name[4:]), seed=2)
        return a, a, {}, "real"
    if name == "scaled_signed":
        a, b = _rand(rng, (200, 300), 2500, True), _rand(rng, (300, 220), 2500, True)
        return a, b, dict(C_=-0.75, si=_scale(rng, 200, True), sj=_scale(rng, 300, True), sk=_scale(rng, 220, True)), "real"
    if name == "transposed":
        a, b = _rand(rng, (300, 200), 2500, True), _rand(rng, (250, 300), 2500)
        return a, b, dict(C_=3.0, tA='T', tB='T', si=_scale(rng, 200)), "real"
    if name == "poisson":
        a = wl.poisson2d(48)
        return a, a, {}, "int"
    if name == "galerkin_RA":
        return wl.aggregation3d(8), wl.laplace3d(8), {}, "int"
    raise KeyError(name)


CASES = ["random", "rmat10", "rmat11", "rmat12", "rmat11_signed_AB", "scaled_signed", "transposed", "poisson", "galerkin_RA"]


def _oracle(a, b, kw):
    args = {k: v for k, v in kw.items() if k in ("C_", "tA", "tB")}
    for k in ("si", "sj", "sk"):
        if k in kw:
            args[{"si": "scalei", "sj": "scalej", "sk": "scalek"}[k]] = _vec(kw[k])
    i, j, v, shape = orc.multiply(orc.Mat(*a), orc.Mat(*b), rowwise=True, nthreads=4, **args)
    return i, j, v, shape


def _reduce(c, w, u, chunk=1 << 27):
    return pj.reduce_coo(pj.host_source(*c[:3]), len(c[2]), c[3], w=w, u=u, chunk=chunk)


@pytest.mark.parametrize("name", CASES)
def test_oracle_products_inside_the_bound(name):
    """The oracle's tuples, reduced on the CPU, against the linearity reference: every row projection (with 1 and w) and
    every column projection (with u) inside its bound; integer stencils with integer weights bit for bit."""
    a, b, kw, kind = _case(name)
    c = _oracle(a, b, kw)
    assert len(c[2]) > 0
    ref = pj.Reference(a, b, **kw)
    w, u = pj.weights(ref.m, 1, kind), pj.weights(ref.n, 2, kind)
    s = _reduce(c, w, u)
    cnt, _, h = orc.digest(*c[:3])
    assert pj.failures(s, ref, w, u, want=(cnt, np.bincount(c[0], minlength=ref.n), h), exact=kind == "int") == []
    ratios = [pj.within(got, *proj)[1] for got, proj in ((s.row_sum, ref.rows(np.ones(ref.m))), (s.row_w, ref.rows(w)),
                                                           (s.col_u, ref.cols(u)))]
    print("%s: largest error/bound %.3g" % (name, max(ratios)))
    if kind == "int":
        assert max(ratios) == 0.0


def test_weights_are_deterministic_and_in_range():
    w = pj.weights(100000, 7)
    assert np.array_equal(w, pj.weights(100000, 7)) and not np.array_equal(w, pj.weights(100000, 8))
    assert w.min() >= 1.0 and w.max() < 2.0 and len(np.unique(w)) > 99000
    k = pj.weights(100000, 7, "int")
    assert k.min() >= 1 and k.max() <= 1 << 16 and np.array_equal(k, np.round(k)) and len(np.unique(k)) > 50000


def test_row_sums_by_linearity_is_the_unweighted_projection():
    a = wl.rmat(10, seed=5)
    ref = pj.Reference(a, a)
    val, _ = ref.rows(np.ones(ref.m))
    assert np.array_equal(pj.row_sums_by_linearity(a, a, ref.n, ref.ni), val)


# ------------------------------------------------------------------------------------------------ mutations

def _base(name="rmat11"):
    a, b, kw, kind = _case(name)
    c = _oracle(a, b, kw)
    ref = pj.Reference(a, b, **kw)
    w, u = pj.weights(ref.m, 1, kind), pj.weights(ref.n, 2, kind)
    cnt, _, h = orc.digest(*c[:3])
    want = (cnt, np.bincount(c[0], minlength=ref.n), h)
    return [x.copy() for x in c[:3]] + [c[3]], ref, w, u, want


def _longest_row(c):
    rows, starts, counts = np.unique(c[0], return_index=True, return_counts=True)
    r = int(np.argmax(counts))
    return int(starts[r]), int(starts[r] + counts[r])


def _swap_values(c):
    lo, hi = _longest_row(c)
    seg = c[2][lo:hi]
    p, q = lo + int(np.argmax(seg)), lo + int(np.argmin(seg))
    c[2][[p, q]] = c[2][[q, p]]


def _move_column(c):
    """The largest value of the longest row whose next column is unused (and not the row's next tuple): order kept."""
    lo, hi = _longest_row(c)
    for p in sorted(range(lo, hi), key=lambda e: -abs(c[2][e])):
        nxt = c[1][p + 1] if p + 1 < hi else c[3][1]
        if c[1][p] + 1 < nxt:
            c[1][p] += 1
            return
    raise AssertionError("no gap in the longest row")


def _swap_adjacent(c):
    lo, _ = _longest_row(c)
    for x in c[:3]:
        x[[lo, lo + 1]] = x[[lo + 1, lo]]


def _drop(c):
    lo, _ = _longest_row(c)
    return [np.delete(x, lo + 1) for x in c[:3]] + [c[3]]


def _duplicate(c):
    lo, _ = _longest_row(c)
    return [np.insert(x, lo + 1, x[lo + 1]) for x in c[:3]] + [c[3]]


def _perturb(c):
    lo, hi = _longest_row(c)
    p = lo + int(np.argmax(np.abs(c[2][lo:hi])))
    c[2][p] *= 1 + 1e-9


def _next_row(c):
    """The largest tuple of the longest row whose column the next row lacks is stored in the next row instead, at its
    place there: order kept."""
    lo, hi = _longest_row(c)
    r = c[0][lo]
    nxt = set(c[1][c[0] == r + 1].tolist())
    p = next(e for e in sorted(range(lo, hi), key=lambda e: -abs(c[2][e])) if c[1][e] not in nxt)
    c[0][p] += 1
    order = np.lexsort((c[1], c[0]))
    return [x[order] for x in c[:3]] + [c[3]]


@pytest.mark.parametrize("mutate,caught_by,case", [
    (_swap_values, {"row_w", "col_u"}, "rmat11"),
    (_swap_values, {"row_w", "col_u"}, "scaled_signed"),
    (_move_column, {"row_w", "col_u", "hash"}, "rmat11"),
    (_swap_adjacent, {"order"}, "rmat11"),
    (_drop, {"count", "row_nnz", "hash", "row_sum", "row_w", "col_u"}, "rmat11"),
    (_duplicate, {"order", "count", "row_nnz", "hash", "row_sum", "row_w", "col_u"}, "rmat11"),
    (_perturb, {"row_sum", "row_w", "col_u"}, "random"),
    (_next_row, {"row_nnz", "hash", "row_sum", "row_w", "col_u"}, "rmat11"),
], ids=lambda x: getattr(x, "__name__", None) if callable(x) else None)
def test_each_mutation_is_flagged(mutate, caught_by, case):
    """A correct result passes; each typical rank/scatter bug applied to it is flagged by exactly the checks that can
    see it: the value-only ones (values swapped, moved to an unused column) only by the projections, the order-only one
    only by the order check.  Without the named checks the mutation would pass."""
    c, ref, w, u, want = _base(case)
    assert pj.failures(_reduce(c, w, u), ref, w, u, want) == []
    c = mutate(c) or c
    got = set(pj.failures(_reduce(c, w, u), ref, w, u, want))
    assert got == caught_by, got


def test_index_beyond_the_shape_stops_the_walk():
    c, ref, w, u, want = _base("random")
    c[1][5] = ref.m
    s = _reduce(c, w, u)
    assert not s.complete and pj.failures(s, ref, w, u, want) == ["bounds"]


def test_nan_is_flagged():
    c, ref, w, u, want = _base("random")
    c[2][7] = np.nan
    assert "nan" in pj.failures(_reduce(c, w, u), ref, w, u, want)


# ------------------------------------------------------------------------------------------------ the reducer

def test_reducer_hash_is_the_oracle_digest():
    a = wl.rmat(12, seed=6)
    c = _oracle(a, a, {})
    s = _reduce(c, None, None)
    cnt, tot, h = orc.digest(*c[:3])
    assert (s.nnz, s.hash) == (cnt, h)
    assert abs(s.row_sum.sum() - tot) <= 1e-12 * abs(tot)
    w = orc.multiply_digest(orc.Mat(*a), orc.Mat(*a), rowstats=True)
    assert np.array_equal(s.row_nnz, w.row_nnz) and s.hash == w.hash


@pytest.mark.parametrize("chunk", [1, 7, 1000, 1 << 27])
def test_reducer_does_not_depend_on_the_chunk_size(chunk):
    """Chunks of one tuple, of sizes that split rows, and one chunk: the same figures (the sums to their last bits,
    being split into other partial sums), order checked across chunk boundaries (a disorder exactly at a boundary is
    found)."""
    a, b, kw, _ = _case("random")
    c = _oracle(a, b, kw)
    ref = pj.Reference(a, b, **kw)
    w, u = pj.weights(ref.m, 1), pj.weights(ref.n, 2)
    whole = _reduce(c, w, u)
    part = _reduce(c, w, u, chunk=chunk)
    assert (part.nnz, part.hash, part.ordered, part.vmin, part.vmax) == (whole.nnz, whole.hash, True, whole.vmin, whole.vmax)
    assert np.array_equal(part.row_nnz, whole.row_nnz)
    for x in ("row_sum", "row_w", "col_u"):        # the same sums, split into other partial sums
        assert np.allclose(getattr(part, x), getattr(whole, x), rtol=1e-14, atol=0), x
    if chunk < len(c[0]):
        bad = [x.copy() for x in c[:3]] + [c[3]]
        e = chunk if chunk > 1 else 1
        for x in bad[:3]:
            x[[e - 1, e]] = x[[e, e - 1]]
        s = _reduce(bad, w, u, chunk=chunk)
        assert not s.ordered and s.first_disorder == e
