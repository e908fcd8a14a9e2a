"""The sharded step (spsamd_dist_multiply, csrc/dist.hip) restated in numpy, and the catalogue of cases that
tests/test_dist_host.py checks on the CPU and tests/test_gpu_dist_edges.py runs on the GPU.  Importing it needs no GPU.

The model: from the oracle's consolidations of the WHOLE op(A) and op(B) by rows and the two sets of bounds, the exact bytes
every rank hands to the transport for every peer in the five calls of a step without zero_nan --

    round 1   call 0   an 8-byte header, all zero (status 0)
              call 1   need_q[b_bounds[p] : b_bounds[p + 1]] as 0 / 1 bytes: which of p's rows rank q's A block selects
              call 2   the lengths of the rank's own op(B) rows, uint32, the same to every peer
    round 2   call 3   int32 columns of the own rows peer p needs, row after row
              call 4   their float64 values

-- and the four DistStats counters.  Under zero_nan a sixth call (the key round) comes first; its encoding is internal, so
those steps are checked end to end only.

All values are small integers (and NaN in the zero_nan cases): every sum is exact in any order, so products compare bit for
bit with the oracle's."""
import functools

import numpy as np

from oracle import binding as orc
from tests import tile_plan as tp

ADD, LEAVE_ALONE, REPLACE = orc.ADD, orc.LEAVE_ALONE, orc.REPLACE
POLICIES = (ADD, LEAVE_ALONE, REPLACE)
MID_MAX = tp.MID_MAX                    # a row above MID_MAX products is heavy
ROWS_LONG = 2048                        # csrc/dist.hip: a panel row above this many tuples is filled by a workgroup
SCAN_BATCH_MAX, MAX_WORLD = 12, 64      # csrc/internal.h, csrc/dist.hip


def op(M, t):
    """(rows, cols) of op(M)."""
    return (M.idx1, M.idx0) if t == 'T' else (M.idx0, M.idx1)


def op_shape(M, t):
    return (M.shape[1], M.shape[0]) if t == 'T' else M.shape


class Case:
    """One sharded product: whole operands (B None: B is A, given as B_block = NULL), flags, policy, the row bounds of
    op(A) and of op(B), the knobs every rank's context runs under, and what the case claims about itself."""

    def __init__(self, name, world, A, B, tA, tB, policy, a_bounds, b_bounds, knobs=None, zero_nan=False, **claims):
        self.name, self.world, self.A, self.B, self.tA, self.tB, self.policy = name, world, A, B, tA, tB, policy
        self.a_bounds, self.b_bounds = [int(x) for x in a_bounds], [int(x) for x in b_bounds]
        self.knobs, self.zero_nan, self.claims = dict(knobs or {}), zero_nan, claims
        self.nrow, self.inner = op_shape(A, tA)
        self.ncol = op_shape(self.Bm, tB)[1]
        assert op_shape(self.Bm, tB)[0] == self.inner
        assert len(self.a_bounds) == len(self.b_bounds) == world + 1
        assert self.a_bounds[0] == 0 and self.a_bounds[-1] == self.nrow and self.b_bounds[0] == 0 and self.b_bounds[-1] == self.inner
        assert all(x <= y for x, y in zip(self.a_bounds, self.a_bounds[1:])) and all(x <= y for x, y in zip(self.b_bounds, self.b_bounds[1:]))
        if B is None:
            assert tA == tB and self.a_bounds == self.b_bounds

    @property
    def Bm(self):
        return self.A if self.B is None else self.B

    def _block(self, M, t, lo, hi):
        r = op(M, t)[0]
        keep = (r >= lo) & (r < hi)                     # storage order kept: LEAVE_ALONE and REPLACE depend on it
        return M.idx0[keep], M.idx1[keep], M.val[keep], M.shape

    def block_a(self, rank):
        """The rank's block of the stored A: (idx0, idx1, val, shape)."""
        return self._block(self.A, self.tA, self.a_bounds[rank], self.a_bounds[rank + 1])

    def block_b(self, rank):
        return None if self.B is None else self._block(self.B, self.tB, self.b_bounds[rank], self.b_bounds[rank + 1])

    def my_n(self, rank):
        return self.b_bounds[rank + 1] - self.b_bounds[rank]


_WANT = {}


def oracle_product(case, zero_nan=False):
    """The oracle's (i, j, v) of the whole product, row-major: computed once per case, never changed."""
    key = (case.name, bool(zero_nan))
    if key not in _WANT:
        _WANT[key] = orc.multiply(case.A, case.Bm, 1.0, None, case.tA, None, case.tB, None, case.policy, zero_nan,
                                  rowwise=True, nthreads=4)[:3]
    return _WANT[key]


def rows_of(t, lo, hi):
    keep = (t[0] >= lo) & (t[0] < hi)
    return t[0][keep], t[1][keep], t[2][keep]


class Model:
    """What every rank of a step without zero_nan sends, receives and counts."""

    def __init__(self, case):
        self.case = c = case
        ar, ac = op(c.A, c.tA)
        self.a = orc.consolidate(ar, ac, c.A.val, 0, c.policy)
        br, bc = op(c.Bm, c.tB)
        self.b = orc.consolidate(br, bc, c.Bm.val, 0, c.policy)
        self.blen = np.bincount(self.b[0], minlength=c.inner).astype(np.uint32)
        self.bptr = np.concatenate([[0], np.cumsum(self.blen, dtype=np.int64)])
        self.need = []
        for q in range(c.world):
            m = np.zeros(c.inner, np.uint8)
            m[self.block_a(q)[1]] = 1
            self.need.append(m)
        self._seg = {}

    def block_a(self, rank):
        """The rank's consolidated A block (rows global)."""
        return rows_of(self.a, self.case.a_bounds[rank], self.case.a_bounds[rank + 1])

    def nmine(self, rank):
        lo, hi = self.case.b_bounds[rank], self.case.b_bounds[rank + 1]
        return int(self.bptr[hi] - self.bptr[lo])

    def selected(self, owner, peer):
        """Mask over the consolidated B's tuples: those of `owner`'s rows that `peer` needs."""
        lo, hi = self.case.b_bounds[owner], self.case.b_bounds[owner + 1]
        r = self.b[0]
        return (r >= lo) & (r < hi) & (self.need[peer][r] == 1)

    def sent_count(self, owner, peer):
        """t of the pack kernel's three cases."""
        return int(self.selected(owner, peer).sum())

    def calls(self, rank):
        """The rank's five calls: calls(rank)[call][peer] -> bytes."""
        if rank not in self._seg:
            c, W = self.case, self.case.world
            lo, hi = c.b_bounds[rank], c.b_bounds[rank + 1]
            own_len = self.blen[lo:hi].tobytes()
            sel = [self.selected(rank, p) for p in range(W)]
            self._seg[rank] = [
                [bytes(8)] * W,
                [self.need[rank][c.b_bounds[p]:c.b_bounds[p + 1]].tobytes() for p in range(W)],
                [own_len] * W,
                [np.ascontiguousarray(self.b[1][s], np.int32).tobytes() for s in sel],
                [np.ascontiguousarray(self.b[2][s], np.float64).tobytes() for s in sel]]
        return self._seg[rank]

    def panel(self, rank):
        """The op(B) rows the rank's block needs, row-major: what round 2 assembles."""
        s = self.need[rank][self.b[0]] == 1
        return self.b[0][s], self.b[1][s], self.b[2][s]

    def stats(self, rank):
        c = self.case
        lo, hi = c.b_bounds[rank], c.b_bounds[rank + 1]
        mine = self.need[rank] == 1
        outside = mine.copy()
        outside[lo:hi] = False
        return dict(block_nnz_a=int(self.block_a(rank)[0].size), panel_tuples=int(self.blen[mine].sum()),
                    remote_tuples=int(self.blen[outside].sum()),
                    sent_tuples=sum(self.sent_count(rank, p) for p in range(c.world) if p != rank))


SEGMENT = ("header", "need mask", "row lengths", "columns", "values")
ELEMENT = (np.uint8, np.uint8, np.uint32, np.int32, np.float64)
BITS = (np.uint8, np.uint8, np.uint32, np.int32, np.int64)      # ... compared as bits


def compare_sends(model, rank, calls, what):
    """The rank's recorded calls of one step (calls[call][peer] -> bytes) against the model's; the message names rank, round,
    segment, peer and the first differing element."""
    want = model.calls(rank)
    assert len(calls) == len(want), "%s: rank %d: %d transport calls in the step, want %d" % (what, rank, len(calls), len(want))
    for k, (g, w) in enumerate(zip(calls, want)):
        for p in range(model.case.world):
            if g[p] == w[p]:
                continue
            where = "%s: rank %d, round %d, segment %d (%s), to peer %d" % (what, rank, 1 if k < 3 else 2, k if k < 3 else k - 3, SEGMENT[k], p)
            if len(g[p]) != len(w[p]):
                raise AssertionError("%s: %d bytes sent, want %d" % (where, len(g[p]), len(w[p])))
            ga, wa = np.frombuffer(g[p], ELEMENT[k]), np.frombuffer(w[p], ELEMENT[k])
            bad = np.flatnonzero(np.frombuffer(g[p], BITS[k]) != np.frombuffer(w[p], BITS[k]))[0]
            raise AssertionError("%s: first difference at element %d: %r sent, want %r" % (where, bad, ga[bad], wa[bad]))


# ---- operands ------------------------------------------------------------------------------------------------------

def rand_mat(rng, shape, nnz, signed=True):
    """nnz random tuples (duplicates where the shape is small): values 1 .. 3, negative in the stored columns = 3 (mod 4),
    so duplicates never cancel."""
    i0 = rng.integers(0, shape[0], nnz)
    i1 = rng.integers(0, shape[1], nnz)
    v = rng.integers(1, 4, nnz).astype(np.float64)
    if signed:
        v *= np.where(i1 % 4 == 3, -1.0, 1.0)
    return orc.Mat(i0, i1, v, shape)


def rows_mat(rng, lens, ncol):
    """A matrix whose row k holds exactly lens[k] tuples on distinct columns (no duplicates), rows in order."""
    rows = np.repeat(np.arange(len(lens)), lens)
    cols = np.concatenate([np.sort(rng.choice(ncol, int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)])
    v = (1.0 + (cols + rows) % 3) * np.where(cols % 4 == 3, -1.0, 1.0)
    return orc.Mat(rows, cols, v, (len(lens), ncol))


def cuts(rng, n, world, repeat=True):
    """world + 1 ascending bounds over n with random cuts, one of them repeated (an empty block) where world > 2."""
    b = sorted(int(x) for x in rng.integers(0, n + 1, world - 1))
    if repeat and world > 2:
        b[world // 2] = b[world // 2 - 1]
    return [0] + sorted(b) + [n]


def even(n, world):
    return [n * q // world for q in range(world + 1)]


# ---- grid_edges: own-block sizes and inner dimensions at the 256-thread block and the 1024-element scan tile

GRID_MY_N = (0, 1, 255, 256, 257, 1023, 1024, 1025)
GRID_INNER_W2 = (255, 256, 257, 1023, 1024)


@functools.lru_cache(maxsize=None)
def grid_edges(n_inner):
    rng = np.random.default_rng(7000 + n_inner)
    if n_inner == sum(GRID_MY_N):
        world, m, nnz_a = 8, 64, 3000
        b_bounds = np.concatenate([[0], np.cumsum(GRID_MY_N)])
        a_bounds = [0, 0, 5, 9, 23, 24, 40, 50, 64]          # an empty block, a one-row block, blocks of more than 256 tuples
    else:
        world, m, nnz_a = 2, 20, 700
        b_bounds, a_bounds = [0, 2 * n_inner // 3, n_inner], [0, 7, 20]
    B = rows_mat(rng, rng.integers(0, 5, n_inner), 50)       # about two tuples a row, a fifth of the rows empty
    A = rand_mat(rng, (m, n_inner), nnz_a)
    return Case("grid_edges_%d" % n_inner, world, A, B, '.', '.', ADD, a_bounds, b_bounds, my_n=list(np.diff(b_bounds)))


# ---- worlds: the [peer][own row] tables, the scan batches (12 per batch), all MAX_WORLD slots

WORLDS = (3, 4, 12, 13, 25, 64)
WORLD_DIMS = {3: (37, 29, 41), 4: (40, 33, 29), 12: (70, 61, 35), 13: (66, 75, 50), 25: (90, 83, 47), 64: (50, 40, 60)}   # m, k, n


@functools.lru_cache(maxsize=None)
def worlds(W):
    i = WORLDS.index(W)
    rng = np.random.default_rng(7100 + W)
    m, k, n = WORLD_DIMS[W]
    tA, tB, policy = ".T"[i % 2], ".T"[(i // 2) % 2], POLICIES[i % 3]
    A = rand_mat(rng, (k, m) if tA == 'T' else (m, k), 400)
    B = rand_mat(rng, (n, k) if tB == 'T' else (k, n), 400)
    return Case("worlds_%d" % W, W, A, B, tA, tB, policy, cuts(rng, m, W), cuts(rng, k, W))


@functools.lru_cache(maxsize=None)
def worlds_same():
    """B_block = NULL with tA = tB = 'T': the stored array's idx1 is the row of op(A) and of op(B)."""
    rng = np.random.default_rng(7199)
    A = rand_mat(rng, (33, 33), 350)
    b = cuts(rng, 33, 4)
    return Case("worlds_same", 4, A, None, 'T', 'T', ADD, b, b)


# ---- pack_edges: the pack kernel's three cases per peer

PACK_NMINE = (255, 256, 257)
PACK_NEEDS = ("every", "none", "but_last", "first", "last", "nonempty")
PACK_ROWS = 100                         # rows of each of the three owners


def pack_need(o, q):
    """What peer q needs of owner o's rows: every kind once per owner."""
    return PACK_NEEDS[(o + q) % 6]


@functools.lru_cache(maxsize=None)
def pack_edges():
    rng = np.random.default_rng(7200)
    W, tail = 6, (7, 0, 12)
    lens = []
    for T in PACK_NMINE:
        ln = np.where(np.arange(PACK_ROWS) % 7 == 3, 0, 2)      # rows 3, 10, .. empty; the first and the last are not
        live = np.flatnonzero(ln)
        ln[live[:T - int(ln.sum())]] += 1
        assert ln.sum() == T and ln[0] and ln[-1]
        lens.append(ln)
    lens.append(rng.integers(0, 4, sum(tail)))
    lens = np.concatenate(lens)
    b_bounds = np.concatenate([[0], np.cumsum((PACK_ROWS,) * 3 + tail)])
    n_inner = int(b_bounds[-1])
    B = rows_mat(rng, lens, 300)
    ai, ak = [], []
    for q in range(W):
        ks = []
        for o in range(3):
            lo = int(b_bounds[o])
            rows = np.arange(lo, lo + PACK_ROWS)
            live = rows[lens[rows] > 0]
            kind = pack_need(o, q)
            ks.append({"every": rows, "none": rows[:0], "but_last": rows[rows != live[-1]], "first": rows[:1], "last": rows[-1:],
                       "nonempty": live}[kind])
        ks.append(rng.integers(3 * PACK_ROWS, n_inner, 5))
        ks = np.concatenate(ks)
        ai.append(4 * q + ks % 4)
        ak.append(ks)
    ai, ak = np.concatenate(ai), np.concatenate(ak)
    A = orc.Mat(ai, ak, 1.0 + (ai + ak) % 3, (4 * W, n_inner))
    return Case("pack_edges", W, A, B, '.', '.', ADD, even(4 * W, W), b_bounds)


# ---- panel_rows: the panel's row array, read by the heavy rows' window counts

PANEL_INNER = (63, 64, 65, 257)
PANEL_NCOL = 8192
PANEL_SPECIAL = {63: {0: 2048, 1: 1, 2: 0, 62: 2049},
                 64: {0: 2049, 1: 0, 62: 2048, 63: 5000},
                 65: {0: 0, 62: 1, 63: 2048, 64: 2049},
                 257: {0: 2049, 62: 5000, 63: 2048, 64: 1, 256: 5000}}
PANEL_EMPTY_GROUP = (128, 192)          # rows of the wholly empty 64-row group at n_inner = 257
PANEL_HUB, PANEL_HUB_RANK = 5, 1


@functools.lru_cache(maxsize=None)
def panel_rows(n_inner):
    rng = np.random.default_rng(7300 + n_inner)
    lens = np.where(np.arange(n_inner) % 5 == 2, 0, 2)          # empty rows inside every group
    if n_inner > PANEL_EMPTY_GROUP[0]:
        lens[PANEL_EMPTY_GROUP[0]:PANEL_EMPTY_GROUP[1]] = 0
    for k, n in PANEL_SPECIAL[n_inner].items():
        lens[k] = n
    B = rows_mat(rng, lens, PANEL_NCOL)
    m = 12
    oi = np.repeat(np.delete(np.arange(m), PANEL_HUB), 3)
    ok = rng.integers(0, n_inner, oi.size)
    hub = np.arange(n_inner)                                    # one tuple at every inner index: every panel row is read
    ai, ak = np.concatenate([oi, np.full(n_inner, PANEL_HUB)]), np.concatenate([ok, hub])
    A = orc.Mat(ai, ak, 1.0 + (ai + ak) % 3, (m, n_inner))
    return Case("panel_rows_%d" % n_inner, 3, A, B, '.', '.', ADD, [0, 4, 8, 12], even(n_inner, 3), special=PANEL_SPECIAL[n_inner])


# ---- planned_tiles: the block product's own configuration (Prepared view over the panel's pointer, static tile walk)

PLANNED = {"class": (tp.l_class, (64,), tp.HASH2), "range": (tp.bm_range, (8192,), tp.BITMAP)}
PLANNED_A_BOUNDS = {("class", 2): [0, 1, 2], ("class", 3): [0, 1, 1, 2], ("range", 2): [0, 0, 1], ("range", 3): [0, 1, 1, 1]}


@functools.lru_cache(maxsize=None)
def planned_tiles(kind, W):
    make, args, scheme = PLANNED[kind]
    p = make(*args)
    knobs = dict(p.knobs, tiles_v1=tp.TILES_V1[scheme])
    return Case("planned_tiles_%s_W%d" % (kind, W), W, p.A, p.B, '.', '.', ADD, PLANNED_A_BOUNDS[kind, W], even(p.A.shape[1], W),
                knobs=knobs, plan=p, scheme=scheme)


def planned_cut(case, rank):
    """The plan's cut of the rank's rows of A: what the block product must report."""
    p = case.claims["plan"]
    i0, i1, v, shape = case.block_a(rank)
    return tp.Cut(orc.Mat(i0, i1, v, shape), p.B, case.claims["scheme"], p.W, coo=True, **p.cut_kw)


# ---- zero_nan: the leading run is the whole matrix', not a block's

def _nan_mat(rng, shape, nnz, bounds, junk_block, lead_rows=True):
    """Random tuples with NaNs and zeros sprinkled in.  Column 0 holds a NaN or a zero in the first row of every block but
    the last (and nothing else there), and a kept value in the last block: the first kept tuple of the column-major
    sequence lies in the last block.  The rows of block `junk_block` hold NaNs and zeros only."""
    i0 = rng.integers(0, shape[0], nnz)
    i1 = rng.integers(1, shape[1], nnz)
    v = rng.integers(1, 4, nnz).astype(np.float64)
    v[rng.random(nnz) < 0.12] = np.nan
    v[rng.random(nnz) < 0.06] = 0.0
    blocks = [q for q in range(len(bounds) - 1) if bounds[q + 1] - bounds[q] >= 2]
    last = blocks[-1]
    c0 = [bounds[q] for q in blocks[:-1]] + [bounds[last], bounds[last + 1] - 1]       # (the last block's own first row: a NaN too)
    v0 = [np.nan if t % 2 == 0 else 0.0 for t in range(len(blocks) - 1)] + [np.nan, 2.0]
    i0 = np.concatenate([np.asarray(c0, np.int64), i0])
    i1 = np.concatenate([np.zeros(len(c0), np.int64), i1])
    v = np.concatenate([np.asarray(v0, np.float64), v])
    junk = (i0 >= bounds[junk_block]) & (i0 < bounds[junk_block + 1])
    v[junk] = np.where(np.arange(int(junk.sum())) % 3 == 0, 0.0, np.nan)
    if lead_rows:                                               # row-major too: the matrix' first tuple is a NaN
        i0, i1, v = np.concatenate([[0], i0]), np.concatenate([[1], i1]), np.concatenate([[np.nan], v])
    return orc.Mat(i0, i1, v, shape)


ZERO_NAN = ((3, False), (3, True), (13, False), (13, True))
ZERO_NAN_JUNK = {3: 1, 13: 5}


@functools.lru_cache(maxsize=None)
def zero_nan(W, same):
    rng = np.random.default_rng(7400 + 2 * W + same)
    k = 31 if W == 3 else 57
    b_bounds = even(k, W)
    if same:
        A = _nan_mat(rng, (k, k), 300, b_bounds, ZERO_NAN_JUNK[W])
        return Case("zero_nan_W%d_same" % W, W, A, None, '.', '.', ADD, b_bounds, b_bounds, zero_nan=True)
    m = 26 if W == 3 else 44
    a_bounds = even(m, W)
    A = _nan_mat(rng, (m, k), 300, a_bounds, ZERO_NAN_JUNK[W])
    B = _nan_mat(rng, (k, 35), 300, b_bounds, ZERO_NAN_JUNK[W])
    return Case("zero_nan_W%d" % W, W, A, B, '.', '.', ADD, a_bounds, b_bounds, zero_nan=True)


def first_kept(M, t, ref_lead_cols):
    """Index (into M's storage) of the first tuple of op(M)'s reference sequence that is neither 0 nor NaN: the sequence is
    row-major for A, column-major for B (multiply_sparse.hpp:168)."""
    r, c = op(M, t)
    order = np.lexsort((r, c)) if ref_lead_cols else np.lexsort((c, r))
    kept = ~(np.isnan(M.val[order]) | (M.val[order] == 0))
    return int(order[np.flatnonzero(kept)[0]])


# ---- the catalogue: name -> (maker, arguments)

CATALOGUE = {"grid_edges_W8": (grid_edges, (sum(GRID_MY_N),))}
CATALOGUE.update({"grid_edges_W2_%d" % n: (grid_edges, (n,)) for n in GRID_INNER_W2})
CATALOGUE.update({"worlds_%d" % W: (worlds, (W,)) for W in WORLDS})
CATALOGUE["worlds_same"] = (worlds_same, ())
CATALOGUE["pack_edges"] = (pack_edges, ())
CATALOGUE.update({"panel_rows_%d" % n: (panel_rows, (n,)) for n in PANEL_INNER})
CATALOGUE.update({"planned_tiles_%s_W%d" % kw: (planned_tiles, kw) for kw in PLANNED_A_BOUNDS})
CATALOGUE.update({"zero_nan_W%d%s" % (W, "_same" if s else ""): (zero_nan, (W, s)) for W, s in ZERO_NAN})


def case(name):
    make, args = CATALOGUE[name]
    return make(*args)


@functools.lru_cache(maxsize=None)
def model(name):
    return Model(case(name))
