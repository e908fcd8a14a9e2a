"""Host restatement of spsamd_color (include/spsparse_amd.h): the yardstick of the device kernels.

K = (rows, cols) is the sorted unique key set of op(A) (unique_keys).  The graph: N(i) = { j != i : (i, j) in K or (j, i) in K },
or row i alone under SYMMETRIC.  The vertices are visited in descending key(v) = (deg(v) if DEGREE else 0) << 32 | h(v):

    color[v] = -1 for all v
    for v in descending key:   color[v] = the smallest c >= 0 that no u in N(v) with color[u] >= 0 holds
    round(v) = 0 if no u in N(v) precedes v, else 1 + max round(u) over those u

hash32, hash32_scalar   h, on a uint32 array and as the six lines of the header on one Python int
unique_keys, adjacency  K, and the graph as (ptr, adj, deg)
greedy_ref   the loop as written, vertex by vertex (small cases): (color, round)
rounds_fast  the same by rounds, a round's winners vectorised (larger cases)
perm_of      (perm, color_ptr): the vertices ascending in (colour, index), the colours' bounds in that list
conflicts    the keys (i, j) of K with i != j and color[i] == color[j]
reference    everything the call returns, as a dict
classes, plan   the kernel class of every vertex, and the launches of the sweep: the host loop of color_graph (k_color.hip)
by_rounds    a pattern whose round sizes are known by construction
"""
import numpy as np

HASH, DEGREE = 0, 1
SYMMETRIC = 1


def hash32(v, seed):
    with np.errstate(over="ignore"):
        h = np.asarray(v).astype(np.uint32) + np.uint32((int(seed) * 0x9E3779B9) & 0xFFFFFFFF)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def hash32_scalar(v, seed):
    m = 0xFFFFFFFF
    h = (v + seed * 0x9E3779B9) & m
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    h ^= h >> 16
    return h


def unique_keys(rows, cols):
    """The sorted unique (row, col) keys of tuples in any order, duplicates included."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    keep = np.r_[True, (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])] if rows.size else np.zeros(0, bool)
    return rows[keep], cols[keep]


def adjacency(K, n, flags=0):
    """(ptr, adj, deg): N(i) = adj[ptr[i]:ptr[i + 1]], ascending."""
    r, c = np.asarray(K[0], np.int64), np.asarray(K[1], np.int64)
    off = r != c
    r, c = r[off], c[off]
    if not flags & SYMMETRIC:
        r, c = unique_keys(np.r_[r, c], np.r_[c, r])
    ptr = np.searchsorted(r, np.arange(n + 1), side="left")
    return ptr, c, np.diff(ptr)


def keys(deg, n, order, seed):
    k = hash32(np.arange(n), seed).astype(np.uint64)
    if order == DEGREE:
        k |= np.asarray(deg).astype(np.uint64) << np.uint64(32)
    return k


def greedy_ref(K, n, order=HASH, seed=0, flags=0):
    """(color, round) by the loop as written."""
    ptr, adj, deg = adjacency(K, n, flags)
    key = [int(x) for x in keys(deg, n, order, seed)]
    color, rnd = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for v in sorted(range(n), key=lambda x: -key[x]):
        nb = [int(u) for u in adj[ptr[v]:ptr[v + 1]]]
        held = {int(color[u]) for u in nb if color[u] >= 0}
        c = 0
        while c in held:
            c += 1
        color[v] = c
        before = [int(rnd[u]) for u in nb if key[u] > key[v]]
        rnd[v] = 1 + max(before) if before else 0
    return color, rnd


def rounds_fast(K, n, order=HASH, seed=0, flags=0):
    """(color, round) by rounds: a vertex wins when no uncoloured neighbour precedes it; the winners of a round take the
    smallest colour their coloured neighbours do not hold."""
    ptr, adj, deg = adjacency(K, n, flags)
    key = keys(deg, n, order, seed)
    src = np.repeat(np.arange(n), deg)
    color, rnd = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    act = np.arange(src.size)                                           # the edges whose source is uncoloured
    r = 0
    while act.size:
        s, d = src[act], adj[act]
        lose = np.zeros(n, bool)
        lose[s[(color[d] < 0) & (key[d] > key[s])]] = True
        e = ~lose[s]                                                    # the winners' edges: their other ends are coloured, or later
        ws, wc = s[e], color[d[e]]
        held = (wc >= 0) & (key[d[e]] > key[ws])                        # (rows taken under SYMMETRIC may name a later vertex coloured already)
        pairs = np.unique(ws[held] * np.int64(n + 1) + wc[held])        # (winner, held colour), ascending
        pv, pc = pairs // (n + 1), pairs % (n + 1)
        cnt = np.bincount(pv, minlength=n)
        start = np.cumsum(cnt) - cnt
        rank = np.arange(pv.size) - start[pv]
        mex = cnt.copy()                                                # every rank held: the count itself
        gap = pc != rank
        np.minimum.at(mex, pv[gap], rank[gap])
        win = np.unique(ws)
        color[win] = mex[win]
        rnd[win] = r
        act = act[~e]
        if r == 0:
            color[deg == 0] = 0                                         # round 0 too: whoever names one and comes later waits a round
        r += 1
    color[deg == 0] = 0
    return color, rnd


def perm_of(color):
    color = np.asarray(color, np.int64)
    perm = np.argsort(color, kind="stable")
    nc = int(color.max()) + 1 if color.size else 0
    return perm.astype(np.int32), np.r_[0, np.cumsum(np.bincount(color, minlength=nc))].astype(np.int32)


def conflicts(K, color):
    r, c = np.asarray(K[0], np.int64), np.asarray(K[1], np.int64)
    color = np.asarray(color)
    return int(np.count_nonzero((r != c) & (color[r] == color[c])))


def reference(K, n, order=HASH, seed=0, flags=0, fast=True):
    color, rnd = (rounds_fast if fast else greedy_ref)(K, n, order, seed, flags)
    _ptr, _adj, deg = adjacency(K, n, flags)
    perm, cptr = perm_of(color)
    return dict(color=color.astype(np.int32), perm=perm, color_ptr=cptr, round=rnd, deg=deg,
                ncolors=int(color.max()) + 1 if n else 0, rounds=int(rnd.max()) + 1 if n else 0,
                adjacency=int(deg.sum()), max_degree=int(deg.max()) if n else 0, conflicts=conflicts(K, color))


def proper(K, color, n, flags=0):
    """No edge of the graph joins two vertices of one colour."""
    ptr, adj, deg = adjacency(K, n, flags)
    src = np.repeat(np.arange(n), deg)
    color = np.asarray(color)
    return bool(np.all(color >= 0)) and not np.any(color[src] == color[adj])


def classes(deg, wave_deg, color_row=0):
    """Per vertex: 0 isolated, 1 thread, 2 wave."""
    deg = np.asarray(deg)
    cl = np.where(deg <= wave_deg, 1, 2) if color_row == 0 else np.full(deg.shape, color_row)
    return np.where(deg == 0, 0, cl)


def plan(rnd, cls, fuse_rows, color_path=0, flags=0):
    """(launches, fused_rounds) of the sweep.  The worklist of round r holds the vertices of degree >= 1 and round >= r; each
    round is a launch per class present, until the worklist has at most fuse_rows vertices of either class (color_path 2:
    whatever their number; 1: never): the rest is one launch.  Under SYMMETRIC the vertices of degree
    0 are on the thread-class worklist of round 0 (a row may name them), without it they are coloured beforehand."""
    rnd, cls = np.asarray(rnd), np.asarray(cls)
    if flags & SYMMETRIC:
        cls = np.where(cls == 0, 1, cls)
    if not np.any(cls > 0):
        return 0, 0
    R = int(rnd[cls > 0].max()) + 1
    launches = 0
    for r in range(R):
        act = (cls > 0) & (rnd >= r)
        nt, nw = int(np.count_nonzero(act & (cls == 1))), int(np.count_nonzero(act & (cls == 2)))
        if color_path != 1 and (color_path == 2 or nt + nw <= fuse_rows):
            return launches + 1, R - r
        launches += (nt > 0) + (nw > 0)
    return launches, 0


def by_rounds(rng, sizes, seed, order=HASH):
    """((rows, cols), round): a symmetric pattern on n = sum(sizes) vertices with sizes[r] vertices of round r.  The first
    sizes[0] vertices of the visiting order are round 0, the next sizes[1] round 1, and so on; every round-r vertex gets one
    edge, to a vertex of round r - 1, which precedes it.  Under HASH the visiting order does not depend on the edges; under
    DEGREE it does, and the construction does not apply."""
    if order != HASH:
        raise ValueError("by_rounds: the visiting order must not depend on the edges (HASH)")
    sizes = [int(s) for s in sizes]
    n = sum(sizes)
    visit = np.argsort(-hash32(np.arange(n), seed).astype(np.int64), kind="stable")
    off = np.r_[0, np.cumsum(sizes)]
    rnd = np.zeros(n, np.int64)
    a, b = [], []
    for r in range(1, len(sizes)):
        cur, prev = visit[off[r]:off[r + 1]], visit[off[r - 1]:off[r]]
        rnd[cur] = r
        a.append(cur)
        b.append(prev[rng.integers(0, prev.size, cur.size)])
    a, b = (np.concatenate(a), np.concatenate(b)) if a else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    return unique_keys(np.r_[a, b], np.r_[b, a]), rnd


# ---------------------------------------------------------------- inputs

def grid2d(N):
    """The 5-point pattern on an N x N grid, diagonal included (Poisson)."""
    i = np.arange(N * N)
    x, y = i % N, i // N
    r = [i, i[x > 0], i[x < N - 1], i[y > 0], i[y < N - 1]]
    c = [i, i[x > 0] - 1, i[x < N - 1] + 1, i[y > 0] - N, i[y < N - 1] + N]
    return unique_keys(np.concatenate(r), np.concatenate(c))


def clique(n):
    i, j = np.indices((n, n))
    return unique_keys(i.ravel(), j.ravel())


def hubs(nhub, leaves):
    """A clique of nhub hubs, each with `leaves` leaves of its own: symmetric, no diagonal.  Hub h is vertex h."""
    hi, hj = np.indices((nhub, nhub))
    off = hi != hj
    leaf = nhub + np.arange(nhub * leaves)
    own = np.repeat(np.arange(nhub), leaves)
    return unique_keys(np.r_[hi[off], own, leaf], np.r_[hj[off], leaf, own]), nhub * (leaves + 1)


def random_pattern(rng, n, symmetric):
    """Random keys on n vertices: some rows empty, some diagonal-only; mirrored if `symmetric`."""
    nnz = int(rng.integers(0, 4 * n + 1))
    r, c = rng.integers(0, n, nnz), rng.integers(0, n, nnz)
    quiet = rng.random(n) < 0.2                                         # rows and columns that keep at most their diagonal
    keep = ~quiet[r] & ~quiet[c]
    r, c = r[keep], c[keep]
    d = np.flatnonzero(rng.random(n) < 0.5)
    r, c = np.r_[r, d], np.r_[c, d]
    if symmetric:
        r, c = np.r_[r, c], np.r_[c, r]
    return unique_keys(r, c)
