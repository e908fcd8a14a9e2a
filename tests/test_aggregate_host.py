"""tests/aggregate_ref.py against aggregations worked out by hand, and its two restatements of spsamd_aggregate's roots
against each other (CPU only)."""
import numpy as np
import pytest

from tests import aggregate_ref as ar
from tests import color_ref as cr


def sym(edges):
    a, b = [e[0] for e in edges], [e[1] for e in edges]
    return cr.unique_keys(a + b, b + a)


PATH7 = sym([(i, i + 1) for i in range(6)])
STAR = sym([(0, i) for i in range(1, 5)])
PATH5 = sym([(i, i + 1) for i in range(4)])

HAND = [
    # name, K, n, keys, roots, agg, ring, members, agg_ptr, rounds
    ("path of 7, keys descending from vertex 0: a root every third vertex, two rounds apart", PATH7, 7, [7, 6, 5, 4, 3, 2, 1],
     [0, 3, 6], [0, 0, 1, 1, 1, 2, 2], [0, 1, 1, 0, 1, 1, 0], [0, 1, 3, 2, 4, 6, 5], [0, 2, 5, 7], 5),
    ("path of 7, the largest key in the middle: 3 and 6 win round 0, 0 waits for 1 and 2 to go out", PATH7, 7, [1, 2, 3, 7, 4, 5, 6],
     [0, 3, 6], [0, 0, 1, 1, 1, 2, 2], [0, 1, 1, 0, 1, 1, 0], [0, 1, 3, 2, 4, 6, 5], [0, 2, 5, 7], 3),
    ("star, the hub is the root", STAR, 5, [9, 1, 2, 3, 4], [0], [0] * 5, [0, 1, 1, 1, 1], [0, 1, 2, 3, 4], [0, 5], 2),
    ("star, leaf 1 is the root: the hub is its ring 1, the other leaves its ring 2", STAR, 5, [1, 9, 2, 3, 4],
     [1], [0] * 5, [1, 0, 2, 2, 2], [1, 0, 2, 3, 4], [0, 5], 2),
    ("two triangles joined by the edge 2 - 3: 3 is within distance 2 of root 0, so 4 is the second root", sym([(0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (2, 3)]), 6,
     [6, 5, 4, 3, 2, 1], [0, 4], [0, 0, 0, 1, 1, 1], [0, 1, 1, 1, 0, 1], [0, 1, 2, 4, 3, 5], [0, 3, 6], 4),
    ("path of 5, roots at both ends: 2 has ring-1 neighbours of both aggregates and follows 3, whose key is larger", PATH5, 5,
     [9, 3, 1, 5, 8], [0, 4], [0, 0, 1, 1, 1], [0, 1, 2, 1, 0], [0, 1, 4, 3, 2], [0, 2, 5], 2),
    ("the same with the keys of 1 and 3 exchanged: 2 follows 1", PATH5, 5,
     [9, 5, 1, 3, 8], [0, 4], [0, 0, 0, 1, 1], [0, 1, 2, 1, 0], [0, 1, 2, 4, 3], [0, 3, 5], 2),
    ("five isolated vertices (two diagonal keys): five roots in one round", (np.array([1, 3]), np.array([1, 3])), 5, [3, 1, 4, 5, 2],
     [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0] * 5, [0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5], 1),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0].split(":")[0] for c in HAND])
def test_by_hand(case):
    _name, K, n, key, roots, agg, ring, members, aptr, rounds = case
    for flags in (0, ar.SYMMETRIC):
        for serial in (False, True):
            ref = ar.reference(K, n, flags=flags, serial=serial, key=key)
            assert list(np.flatnonzero(ref["root"])) == roots and list(ref["agg"]) == agg and list(ref["ring"]) == ring
            assert list(ref["members"]) == members and list(ref["agg_ptr"]) == aptr
            assert (ref["naggregates"], ref["rounds"]) == (len(roots), rounds)
            assert (ref["ring1"], ref["ring2"]) == (ring.count(1), ring.count(2))
            assert (ref["max_size"], ref["min_size"]) == (max(np.diff(aptr)), min(np.diff(aptr)))
            ar.invariants(K, ref["agg"], ref["members"], ref["agg_ptr"])


def test_the_lists_of_the_first_path():
    """Round by round: the undecided list, and the spread list, which a vertex leaves after the round that found a root or no
    undecided vertex in its closed neighbourhood."""
    _root, rounds, lists = ar.rounds_ref(PATH7, 7, key=[7, 6, 5, 4, 3, 2, 1])
    assert rounds == 5
    assert [list(U) for U, _S in lists] == [[0, 1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6], [3, 4, 5, 6], [4, 5, 6], [6]]
    assert [list(S) for _U, S in lists] == [[0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6], [2, 3, 4, 5, 6], [2, 3, 4, 5, 6], [5, 6]]
    assert [ar.path_undecided(7, t) for t in range(6)] == [7, 6, 4, 3, 1, 0]


def test_the_empty_graph():
    ref = ar.reference((np.zeros(0, int), np.zeros(0, int)), 0)
    assert (ref["naggregates"], ref["rounds"], ref["max_size"], ref["min_size"]) == (0, 0, 0, 0)
    assert ref["agg"].size == 0 and ref["members"].size == 0 and list(ref["agg_ptr"]) == [0]


def test_a_directed_key_under_the_flag():
    K = (np.array([0, 1, 2]), np.array([1, 0, 0]))                      # (2, 0) has no reverse
    assert ar.asymmetric(K) == 1 and ar.reference(K, 3, flags=ar.SYMMETRIC) == dict(asymmetric=1)
    assert ar.reference(K, 3)["asymmetric"] == 0 and ar.reference(K, 3)["naggregates"] == 1
    assert ar.asymmetric((np.array([0, 1, 1]), np.array([1, 0, 1]))) == 0


def test_the_two_restatements_agree_on_random_patterns():
    rng = np.random.default_rng(24)
    for it in range(300):
        n = int(rng.integers(1, 41))
        K = cr.random_pattern(rng, n, bool(it & 1))
        order, seed = int(rng.integers(0, 2)), int(rng.integers(0, 2 ** 32))
        for flags in ((0, ar.SYMMETRIC) if it & 1 else (0,)):
            root, rounds, lists = ar.rounds_ref(K, n, order, seed, flags)
            assert np.array_equal(root, ar.greedy_ref(K, n, order, seed, flags)), it
            assert rounds == len(lists) >= 1 and lists[0][0].size == n == lists[0][1].size
            for (U0, S0), (U1, S1) in zip(lists, lists[1:]):            # both lists only shrink
                assert set(U1) < set(U0) and set(S1) <= set(S0) and set(U1) <= set(S1)
            ref = ar.reference(K, n, order, seed, flags)
            ar.invariants(K, ref["agg"], ref["members"], ref["agg_ptr"])
            assert ref["naggregates"] + ref["ring1"] + ref["ring2"] == n
            if flags:
                ref0 = ar.reference(K, n, order, seed, 0)
                assert all(np.array_equal(ref[k], ref0[k]) for k in ("agg", "members", "agg_ptr")) and ref["rounds"] == ref0["rounds"]


def test_by_rounds_has_the_lists_it_says():
    K, usizes = ar.by_rounds([1] * 5 + [2, 3, 4, 7, 7, 30], 11)
    n = 5 + 2 + 3 + 4 + 14 + 30
    _root, rounds, lists = ar.rounds_ref(K, n, ar.HASH, 11)
    assert [U.size for U, _S in lists] == usizes and rounds == len(usizes) == 20 and usizes[0] == n
    assert usizes[:3] == [n, n - 5 - 6, n - 5 - 6 - 1 - 2 - 2 - 4 - 2]


def test_plan():
    def lists(*sizes):
        return [(np.arange(u), np.arange(s)) for u, s in sizes]
    L = lists((3000, 3000), (1500, 2000), (300, 1100), (10, 40), (1, 3))
    thread = np.ones(3000, int)
    assert ar.plan(L, thread, 1024, 0) == (2 + 2 + 2 + 1, 2)             # the spread list of round 2 is still too long
    assert ar.plan(L, thread, 2000, 0) == (2 + 1, 4)
    assert ar.plan(L, thread, 1024, 1) == (10, 0)
    assert ar.plan(L, thread, 1024, 2) == (1, 5)
    cls = thread.copy()
    cls[5] = 2                                                          # a wave-class vertex on both lists until round 3
    assert ar.plan(L, cls, 1024, 0) == (4 + 4 + 4 + 1, 2)
    cls = thread.copy()
    cls[20] = 2                                                         # ... that leaves the undecided list after round 2
    assert ar.plan(L, cls, 1024, 1) == (4 + 4 + 4 + 3 + 2, 0)
    assert ar.plan([], thread, 1024, 0) == (0, 0)
    assert list(ar.classes([0, 1, 16, 17], 16)) == [1, 1, 1, 2] and list(ar.classes([0, 3], 16, 2)) == [1, 2]


def test_no_aggregation_kernel_uses_scratch():
    """Every kernel of k_aggregate.hip in the built library: no scratch, no spill (resource figures only, no GPU)."""
    from scripts import kernel_resources
    from spsparse_amd import build
    found = {name: f for name, f in kernel_resources.library_kernels(build.build()).items() if "k_agg_" in name}
    want = ("words", "asym", "spread_thread", "spread_wave", "decide_thread", "decide_wave", "fused", "flags", "ring1", "ring2", "keys", "sizes")
    assert all(any("k_agg_" + k in name for name in found) for k in want), sorted(found)
    for name, f in found.items():
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, (name, f)
