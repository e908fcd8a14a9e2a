"""Host restatement of spsamd_aggregate (include/spsparse_amd.h): the yardstick of the device kernels.

K, the graph N(i) and key(v) are spsamd_color's (tests/color_ref.py).  u is within distance 2 of v when u != v and u is in
N[w] for some w in N[v].  The roots are a distance-2 maximal independent set in descending key:

    root[v] = 0 for all v
    for v in descending key:   root[v] = 1 unless some u within distance 2 of v has root[u] = 1

and the aggregates grow around them in two rings (assign).

asymmetric   the keys (i, j) of K, i != j, whose reverse is not in K
greedy_ref   the loop as written, vertex by vertex; takes an explicit key array, so that hand cases need no hash
rounds_ref   the synchronous form the device runs: (root, rounds, lists), lists[t] the undecided and the spread list of round t
assign       (agg, ring) from the roots
members_of   (members, agg_ptr): the vertices ascending in (aggregate, ring, index)
reference    everything the call returns, as a dict
classes, plan   the kernel class of every vertex, and the launches of the sweep: the host loop of aggregate_graph (k_aggregate.hip)
by_rounds    disjoint paths whose keys descend along the path: the undecided list's length in every round is known
invariants   what any MIS(2) aggregation satisfies, checked from K and the outputs alone
"""
import numpy as np

from tests import color_ref as cr

HASH, DEGREE = 0, 1
SYMMETRIC = 1
ROOT = np.uint64(0xFFFFFFFFFFFFFFFF)


def asymmetric(K):
    r, c = np.asarray(K[0], np.int64), np.asarray(K[1], np.int64)
    have = set(zip(r.tolist(), c.tolist()))
    return sum(1 for i, j in have if i != j and (j, i) not in have)


def _neighbours(ptr, adj, n):
    return [set(int(u) for u in adj[ptr[v]:ptr[v + 1]]) - {v} for v in range(n)]


def _within2(nb, v):
    out = set(nb[v])
    for w in nb[v]:
        out |= nb[w]
    out.discard(v)
    return out


def greedy_ref(K, n, order=HASH, seed=0, flags=0, key=None):
    """root (0 / 1 per vertex) by the loop as written.  key: an explicit key per vertex instead of key(v)."""
    ptr, adj, deg = cr.adjacency(K, n, flags)
    key = [int(x) for x in (cr.keys(deg, n, order, seed) if key is None else key)]
    nb = _neighbours(ptr, adj, n)
    root = np.zeros(n, np.int64)
    for v in sorted(range(n), key=lambda x: -key[x]):
        root[v] = 0 if any(root[u] for u in _within2(nb, v)) else 1
    return root


def rounds_ref(K, n, order=HASH, seed=0, flags=0, key=None):
    """(root, rounds, lists) by the synchronous rounds of the header.  lists[t] = (U, S): the undecided vertices at the start
    of round t, and the spread list of that round -- S of round 0 is every vertex, and w stays on it after a round at whose
    start N[w] held an undecided vertex and no root."""
    ptr, adj, deg = cr.adjacency(K, n, flags)
    key = (cr.keys(deg, n, order, seed) if key is None else np.asarray(key)).astype(np.uint64)
    src = np.r_[np.repeat(np.arange(n), deg), np.arange(n)].astype(np.int64)          # N[w]: the row and w itself
    dst = np.r_[adj, np.arange(n)].astype(np.int64)
    word = key + np.uint64(1)
    on_s = np.ones(n, bool)
    lists, t = [], 0
    while True:
        und = (word != 0) & (word != ROOT)
        if not und.any():
            break
        lists.append((np.flatnonzero(und), np.flatnonzero(on_s)))
        t1 = np.zeros(n, np.uint64)
        np.maximum.at(t1, src, word[dst])
        has_und = np.zeros(n, bool)
        has_und[src[und[dst]]] = True
        on_s &= has_und & (t1 != ROOT)
        t2 = np.zeros(n, np.uint64)
        np.maximum.at(t2, src, t1[dst])
        new = word.copy()
        new[und & (t2 == ROOT)] = 0
        new[und & (t2 == word)] = ROOT
        word = new
        t += 1
    return (word == ROOT).astype(np.int64), t, lists


def assign(K, n, root, order=HASH, seed=0, flags=0, key=None):
    """(agg, ring): ring 0 a root, ring 1 a neighbour of a root, ring 2 the rest, which take the aggregate of their ring-1
    neighbour with the largest key."""
    ptr, adj, deg = cr.adjacency(K, n, flags)
    key = [int(x) for x in (cr.keys(deg, n, order, seed) if key is None else key)]
    nb = _neighbours(ptr, adj, n)
    ids = np.cumsum(root) - root
    agg, ring = np.full(n, -1, np.int64), np.full(n, 2, np.int64)
    for v in range(n):
        if root[v]:
            agg[v], ring[v] = ids[v], 0
            continue
        r = [u for u in nb[v] if root[u]]
        assert len(r) <= 1, "two roots adjacent to vertex %d" % v
        if r:
            agg[v], ring[v] = ids[r[0]], 1
    for v in range(n):
        if ring[v] == 2:
            w = max((u for u in nb[v] if ring[u] == 1), key=lambda u: key[u])
            agg[v] = agg[w]
    return agg, ring


def members_of(agg, ring):
    agg, ring = np.asarray(agg, np.int64), np.asarray(ring, np.int64)
    members = np.argsort(agg * 4 + ring, kind="stable")
    na = int(agg.max()) + 1 if agg.size else 0
    return members.astype(np.int32), np.r_[0, np.cumsum(np.bincount(agg, minlength=na))].astype(np.int32)


def reference(K, n, order=HASH, seed=0, flags=0, serial=False, key=None):
    """Every output and stat of the call.  Under SYMMETRIC on a pattern that is not, only `asymmetric` (the call refuses)."""
    asym = asymmetric(K) if flags & SYMMETRIC else 0
    if asym:
        return dict(asymmetric=asym)
    root, rounds, lists = rounds_ref(K, n, order, seed, flags, key)
    if serial:
        root = greedy_ref(K, n, order, seed, flags, key)
    agg, ring = assign(K, n, root, order, seed, flags, key)
    members, aptr = members_of(agg, ring)
    _ptr, _adj, deg = cr.adjacency(K, n, flags)
    size = np.diff(aptr)
    return dict(agg=agg.astype(np.int32), members=members, agg_ptr=aptr, root=root, ring=ring, deg=deg, lists=lists,
                naggregates=int(root.sum()), rounds=rounds, ring1=int(np.count_nonzero(ring == 1)),
                ring2=int(np.count_nonzero(ring == 2)), max_size=int(size.max()) if n else 0, min_size=int(size.min()) if n else 0,
                adjacency=int(deg.sum()), max_degree=int(deg.max()) if n else 0, asymmetric=0)


def classes(deg, wave_deg, agg_row=0):
    """Per vertex: 1 thread, 2 wave.  A vertex of degree 0 is thread-class whatever agg_row says."""
    deg = np.asarray(deg)
    cl = np.where(deg <= wave_deg, 1, 2) if agg_row == 0 else np.full(deg.shape, agg_row)
    return np.where(deg == 0, 1, cl)


def plan(lists, cls, fuse_rows, agg_path=0):
    """(launches, fused_rounds) of the sweep.  A round is a spread and a decide launch per class present on the spread and the
    undecided list, until both lists hold at most fuse_rows vertices (agg_path 2: whatever their lengths; 1: never): the
    rest is one launch."""
    cls = np.asarray(cls)
    launches = 0
    for t, (U, S) in enumerate(lists):
        if agg_path != 1 and (agg_path == 2 or (U.size <= fuse_rows and S.size <= fuse_rows)):
            return launches + 1, len(lists) - t
        launches += sum(int(np.any(cls[L] == k)) for L in (S, U) for k in (1, 2))
    return launches, 0


def path_undecided(m, t):
    """The undecided vertices of a path of m vertices with keys descending along it at the start of round t: vertex 3k becomes
    a root in round 2k, vertices 3k + 1 and 3k + 2 go out in round 2k + 1."""
    return max(0, m - (3 * (t // 2) + t % 2))


def by_rounds(lengths, seed):
    """((rows, cols), usizes): disjoint paths of the given numbers of vertices (1: an isolated vertex), each along a stretch
    of the visiting order under HASH, so that its keys descend along it; usizes[t] = the undecided list's length in round t."""
    lengths = [int(m) for m in lengths]
    n = sum(lengths)
    visit = np.argsort(-cr.hash32(np.arange(n), seed).astype(np.int64), kind="stable")
    a, b, off = [], [], 0
    for m in lengths:
        p = visit[off:off + m]
        a.append(p[:-1])
        b.append(p[1:])
        off += m
    a, b = np.concatenate(a), np.concatenate(b)
    usizes, t = [], 0
    while True:
        u = sum(path_undecided(m, t) for m in lengths)
        if not u:
            break
        usizes.append(u)
        t += 1
    return cr.unique_keys(np.r_[a, b], np.r_[b, a]), usizes


def invariants(K, agg, members, agg_ptr):
    """The roots are pairwise farther apart than distance 2; every vertex lies within distance 2 of its root, through a
    member of its own aggregate; members and agg_ptr say what agg says.  Raises AssertionError."""
    agg, members, agg_ptr = np.asarray(agg, np.int64), np.asarray(members, np.int64), np.asarray(agg_ptr, np.int64)
    n, na = agg.size, agg_ptr.size - 1
    assert agg_ptr[0] == 0 and agg_ptr[na] == n and np.all(np.diff(agg_ptr) >= 1 if n else True)
    assert sorted(members.tolist()) == list(range(n)) and np.all(agg >= 0) and np.all(agg < max(na, 1))
    ptr, adj, _deg = cr.adjacency(K, n, 0)
    nb = _neighbours(ptr, adj, n)
    roots = members[agg_ptr[:-1]]
    assert np.all(np.diff(roots) > 0)                                   # numbered in ascending vertex index
    isroot = np.zeros(n, bool)
    isroot[roots] = True
    for a in range(na):
        part, r = members[agg_ptr[a]:agg_ptr[a + 1]], int(roots[a])
        assert np.all(agg[part] == a)
        assert not any(isroot[u] for u in _within2(nb, r)), "roots %d within distance 2" % r
        ring = [0 if v == r else 1 if v in nb[r] else 2 for v in part.tolist()]
        assert ring == sorted(ring), "aggregate %d is not in ring order" % a
        for v, g in zip(part.tolist(), ring):
            assert g < 2 or any(agg[w] == a and w in nb[r] for w in nb[v]), "vertex %d does not reach its root" % v
        for g in (0, 1, 2):
            assert np.all(np.diff(part[np.asarray(ring) == g]) > 0)
