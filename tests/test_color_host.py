"""tests/color_ref.py against colourings worked out by hand, and its two restatements of spsamd_color's loop against each
other (CPU only)."""
import numpy as np
import pytest

from tests import color_ref as cr
from tests import solve_ref as sr

SEED = 7
# h(v, 7) for v = 0 .. 5: the visiting order is 1, 4, 2, 0, 3, 5
H7 = [2025593743, 4176287394, 2026417946, 568106410, 3428013136, 559472614]


def sym(edges):
    a, b = [e[0] for e in edges], [e[1] for e in edges]
    return cr.unique_keys(a + b, b + a)


HAND = [
    # name, K, n, order, colours, rounds
    ("path", sym([(i, i + 1) for i in range(5)]), 6, cr.HASH, [1, 0, 1, 2, 0, 1], [1, 0, 1, 2, 0, 1]),
    ("triangle", sym([(0, 1), (1, 2), (0, 2)]), 3, cr.HASH, [2, 0, 1], [2, 0, 1]),
    ("star, by hash: three leaves, the centre, two leaves", sym([(0, i) for i in range(1, 6)]), 6, cr.HASH,
     [1, 0, 0, 0, 0, 0], [1, 0, 0, 2, 0, 2]),
    ("star, by degree: the centre first", sym([(0, i) for i in range(1, 6)]), 6, cr.DEGREE, [0, 1, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1]),
    ("K5", cr.clique(5), 5, cr.HASH, [3, 0, 2, 4, 1], [3, 0, 2, 4, 1]),
    ("grid 4 x 4, by hash", cr.grid2d(4), 16, cr.HASH, [1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1],
     [1, 0, 1, 2, 0, 5, 6, 1, 1, 4, 5, 0, 0, 3, 2, 1]),
    ("grid 4 x 4, by degree", cr.grid2d(4), 16, cr.DEGREE, [1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 0, 1, 0, 1],
     [3, 2, 3, 4, 2, 1, 2, 3, 3, 0, 1, 2, 4, 3, 2, 3]),
]


def test_hash_is_the_six_lines():
    assert [cr.hash32_scalar(v, SEED) for v in range(6)] == H7
    rng = np.random.default_rng(1)
    v = np.r_[0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, rng.integers(0, 2 ** 32, 300)]
    for seed in (0, 1, SEED, 2 ** 32 - 1):
        assert [int(x) for x in cr.hash32(v, seed)] == [cr.hash32_scalar(int(x), seed) for x in v]


def test_hash_is_a_bijection_on_a_sample():
    for seed in (0, SEED, 0xDEADBEEF):
        for lo in (0, 2 ** 31 - 2 ** 15, 2 ** 32 - 2 ** 16):
            assert np.unique(cr.hash32(np.arange(lo, lo + 2 ** 16, dtype=np.uint64), seed)).size == 2 ** 16


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_by_hand(case):
    _name, K, n, order, colors, rounds = case
    for fn in (cr.greedy_ref, cr.rounds_fast):
        c, r = fn(K, n, order, SEED)
        assert list(c) == colors and list(r) == rounds, fn.__name__


def test_isolated_vertices_and_the_empty_graph():
    K = (np.array([1, 3]), np.array([1, 3]))                           # two diagonal-only rows of five
    ref = cr.reference(K, 5, fast=False)
    assert list(ref["color"]) == [0] * 5 and (ref["ncolors"], ref["rounds"], ref["adjacency"]) == (1, 1, 0)
    assert list(ref["perm"]) == [0, 1, 2, 3, 4] and list(ref["color_ptr"]) == [0, 5]
    ref = cr.reference((np.zeros(0, int), np.zeros(0, int)), 0)
    assert (ref["ncolors"], ref["rounds"]) == (0, 0) and list(ref["color_ptr"]) == [0]


def test_the_two_restatements_agree_on_random_patterns():
    rng = np.random.default_rng(22)
    for it in range(200):
        n = int(rng.integers(1, 41))
        symmetric = bool(it & 1)
        K = cr.random_pattern(rng, n, symmetric)
        order, seed = int(rng.integers(0, 2)), int(rng.integers(0, 2 ** 32))
        for flags in (0, cr.SYMMETRIC):
            c0, r0 = cr.greedy_ref(K, n, order, seed, flags)
            c1, r1 = cr.rounds_fast(K, n, order, seed, flags)
            assert np.array_equal(c0, c1) and np.array_equal(r0, r1), (it, flags)
            if flags and not symmetric:                                 # a false promise: the loop is still defined, vertex by vertex
                continue
            assert cr.proper(K, c0, n, flags) and cr.conflicts(K, c0) == 0
            ref = cr.reference(K, n, order, seed, flags)
            perm, cptr, nc = ref["perm"], ref["color_ptr"], ref["ncolors"]
            assert sorted(perm) == list(range(n)) and cptr[0] == 0 and cptr[nc] == n and cptr.size == nc + 1
            for c in range(nc):
                part = perm[cptr[c]:cptr[c + 1]]
                assert part.size and np.all(c0[part] == c) and np.all(np.diff(part) > 0)
            assert nc <= ref["max_degree"] + 1
        if symmetric:                                                   # the flag changes nothing on a symmetric pattern
            assert np.array_equal(c0, cr.greedy_ref(K, n, order, seed, 0)[0])


def test_a_false_promise_of_symmetry_shows_in_the_conflicts():
    K = (np.array([0]), np.array([1]))                                  # the one key (0, 1): row 1 does not see vertex 0
    c, _ = cr.greedy_ref(K, 2, cr.HASH, SEED, cr.SYMMETRIC)
    assert list(c) == [1, 0] and cr.conflicts(K, c) == 0                # (vertex 1 comes first: 0; vertex 0 sees it: 1)
    K = (np.array([1]), np.array([0]))                                  # the one key (1, 0): vertex 1 first, then 0 unaware of it
    c, _ = cr.greedy_ref(K, 2, cr.HASH, SEED, cr.SYMMETRIC)
    assert list(c) == [0, 0] and cr.conflicts(K, c) == 1
    assert cr.conflicts(K, cr.greedy_ref(K, 2, cr.HASH, SEED, 0)[0]) == 0


def reordered(K, perm):
    """P A P^T: new index r is old vertex perm[r]."""
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    r, c = cr.unique_keys(inv[K[0]], inv[K[1]])
    return r, c, np.ones(r.size)


@pytest.mark.parametrize("order", [cr.HASH, cr.DEGREE])
def test_the_reordered_pattern_has_at_most_ncolors_levels(order):
    rng = np.random.default_rng(5)
    for K, n in ((cr.grid2d(12), 144), (cr.random_pattern(rng, 60, True), 60), (cr.random_pattern(rng, 60, False), 60)):
        ref = cr.reference(K, n, order, 3)
        before = sr.schedule_stats((K[0], K[1], np.ones(K[0].size)), n)[0]
        after = sr.schedule_stats(reordered(K, ref["perm"]), n)[0]
        assert after <= ref["ncolors"], (before, after, ref["ncolors"])
    K = cr.grid2d(12)
    assert sr.schedule_stats((K[0], K[1], np.ones(K[0].size)), 144)[0] == 23          # 2 N - 1 levels in the natural order


def test_by_rounds_has_the_sizes_it_was_asked_for():
    rng = np.random.default_rng(9)
    sizes = [1, 5, 64, 65, 3, 1, 1, 200, 2]
    K, rnd = cr.by_rounds(rng, sizes, 11)
    n = sum(sizes)
    c, r = cr.rounds_fast(K, n, cr.HASH, 11)
    assert np.array_equal(r, rnd) and list(np.bincount(r)) == sizes
    assert cr.proper(K, c, n) and c.max() == 1


def test_plan():
    rnd = np.repeat(np.arange(5), [2000, 1500, 300, 10, 1])
    thread = np.ones(rnd.size, int)
    assert cr.plan(rnd, thread, 1024, 0) == (3, 3)                      # 3811 and 1811 vertices in launches of their own, then 311
    assert cr.plan(rnd, thread, 1024, 1) == (5, 0)
    assert cr.plan(rnd, thread, 1024, 2) == (1, 5)
    cls = thread.copy()
    cls[-11] = 2                                                        # a wave-class vertex of round 3
    assert cr.plan(rnd, cls, 1024, 0) == (2 + 2 + 1, 3)                  # two launches a round while the list is wide
    assert cr.plan(rnd, cls, 1024, 1) == (2 + 2 + 2 + 2 + 1, 0)
    assert cr.plan(rnd, cls, 1024, 2) == (1, 5)
    assert cr.plan(rnd, np.zeros(rnd.size, int), 1024, 0) == (0, 0)
    assert list(cr.classes([0, 1, 64, 65], 64)) == [0, 1, 1, 2] and list(cr.classes([0, 3], 64, 2)) == [0, 2]


def test_no_colouring_kernel_uses_scratch():
    """Every kernel of k_color.hip in the built library: no scratch, no spill (resource figures only, no GPU)."""
    from scripts import kernel_resources
    from spsparse_amd import build
    found = {name: f for name, f in kernel_resources.library_kernels(build.build()).items() if "k_col_" in name}
    want = ("sym_keys", "first", "unique", "init", "thread", "wave", "commit", "fused", "conflicts", "keys", "bounds")
    assert all(any("k_col_" + k in name for name in found) for k in want), sorted(found)
    for name, f in found.items():
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, (name, f)
