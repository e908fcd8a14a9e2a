"""The sharded step's numpy model, its catalogue of cases and the in-process rank harness, on the CPU.

tests/dist_ref.py restates what every rank of spsamd_dist_multiply sends; tests/test_gpu_dist_edges.py holds the C code to
it on the GPU.  Here: the model is sound (the modelled panels multiplied block by block through the oracle give the whole
product; its counters agree with a direct count), every catalogue case is what it claims to be, and tests/dist_ranks.py
routes, checks sizes and fails together, on host memory."""
import ctypes
import threading
import time

import numpy as np
import pytest

from oracle import binding as orc
from tests import dist_ranks as dk
from tests import dist_ref as dr
from tests.add_ref import same_tuples


# ---- the model is sound

@pytest.mark.parametrize("name", list(dr.CATALOGUE))
def test_model_panels_give_the_whole_product(name):
    """Each rank's modelled panel times its consolidated A block, concatenated in rank order, is the oracle's product of the
    whole matrices (without zero_nan: the model's domain) -- C's rows are independent, no reduction."""
    c, m = dr.case(name), dr.model(name)
    want = dr.oracle_product(c, False)
    parts = []
    for q in range(c.world):
        a, p = m.block_a(q), m.panel(q)
        A = orc.Mat(a[0], a[1], a[2], (c.nrow, c.inner), sort0=0)
        P = orc.Mat(p[0], p[1], p[2], (c.inner, c.ncol), sort0=0)
        parts.append(orc.multiply(A, P, duplicate_policy=c.policy, rowwise=True)[:3])
        assert same_tuples(parts[-1], dr.rows_of(want, c.a_bounds[q], c.a_bounds[q + 1])), "rank %d" % q
    assert same_tuples(tuple(np.concatenate([p[t] for p in parts]) for t in range(3)), want)


@pytest.mark.parametrize("name", list(dr.CATALOGUE))
def test_model_stats_agree_with_a_direct_count(name):
    """The four counters, counted tuple by tuple from the raw operands with Python sets; and the bytes of the five calls
    have the sizes b_bounds fixes."""
    c, m = dr.case(name), dr.model(name)
    ar, ac = dr.op(c.A, c.tA)
    br, bc = dr.op(c.Bm, c.tB)
    live_a = c.A.val != 0                               # exact zeros never survive a consolidation
    live_b = c.Bm.val != 0
    b_keys = {}
    for r, k in set(zip(br[live_b].tolist(), bc[live_b].tolist())):
        b_keys[r] = b_keys.get(r, 0) + 1
    owner = lambda k: next(q for q in range(c.world) if c.b_bounds[q] <= k < c.b_bounds[q + 1])      # noqa: E731
    needs = []
    for q in range(c.world):
        mine = live_a & (ar >= c.a_bounds[q]) & (ar < c.a_bounds[q + 1])
        needs.append(set(ac[mine].tolist()))
    for q in range(c.world):
        mine = live_a & (ar >= c.a_bounds[q]) & (ar < c.a_bounds[q + 1])
        want = dict(block_nnz_a=len(set(zip(ar[mine].tolist(), ac[mine].tolist()))),
                    panel_tuples=sum(b_keys.get(k, 0) for k in needs[q]),
                    remote_tuples=sum(b_keys.get(k, 0) for k in needs[q] if owner(k) != q),
                    sent_tuples=sum(b_keys.get(k, 0) for p in range(c.world) if p != q for k in needs[p] if owner(k) == q))
        assert m.stats(q) == want, "rank %d" % q
        calls = m.calls(q)
        assert [len(x) for x in calls[1]] == [c.my_n(p) for p in range(c.world)]
        assert all(len(x) == 4 * c.my_n(q) for x in calls[2])
        assert all(2 * len(x) == len(y) for x, y in zip(calls[3], calls[4]))
        assert sum(len(m.calls(p)[3][q]) for p in range(c.world)) == 4 * want["panel_tuples"]


# ---- every case is what it claims to be

def test_grid_edges_block_sizes():
    c = dr.case("grid_edges_W8")
    assert (c.world, c.inner) == (8, 3841) and [c.my_n(q) for q in range(8)] == [0, 1, 255, 256, 257, 1023, 1024, 1025]
    m = dr.model("grid_edges_W8")
    assert min(m.stats(q)["block_nnz_a"] for q in range(8)) == 0 and max(m.stats(q)["block_nnz_a"] for q in range(8)) > 256
    assert max(m.nmine(q) for q in range(8)) > 1024 and (m.blen == 0).sum() > 100
    assert sorted(dr.case("grid_edges_W2_%d" % n).inner for n in dr.GRID_INNER_W2) == [255, 256, 257, 1023, 1024]


def test_worlds_cover_the_scan_batches_and_empty_blocks():
    assert [dr.case("worlds_%d" % W).world for W in dr.WORLDS] == [3, 4, 12, 13, 25, 64]
    assert dr.SCAN_BATCH_MAX == 12 and dr.MAX_WORLD == 64      # 13 starts a second batch, 25 a third, 64 fills PackDst
    flags, policies = set(), set()
    for W in dr.WORLDS:
        c = dr.case("worlds_%d" % W)
        flags.add((c.tA, c.tB)); policies.add(c.policy)
        assert c.B is not None and c.nrow != c.inner != c.ncol
        assert 0 in np.diff(c.a_bounds) and 0 in np.diff(c.b_bounds), "W = %d: no empty block" % W
        a = dr.model("worlds_%d" % W).a
        assert a[0].size < c.A.nnz, "no duplicate for the policy to settle"
    assert {t for f in flags for t in f} == {'.', 'T'} and ('T', 'T') in flags and policies == set(dr.POLICIES)
    c = dr.case("worlds_64")
    assert c.inner == 40
    s = dr.case("worlds_same")
    assert s.B is None and (s.tA, s.tB) == ('T', 'T')


def test_pack_edges_pairs():
    c, m = dr.case("pack_edges"), dr.model("pack_edges")
    assert c.world == 6 and [m.nmine(o) for o in range(3)] == [255, 256, 257]
    seen = set()
    for o in range(3):
        lo = c.b_bounds[o]
        own = m.blen[lo:lo + dr.PACK_ROWS]
        live = np.flatnonzero(own)
        assert own[0] and own[-1] and (own == 0).sum() >= 10
        for q in range(6):
            mask, t, kind = m.need[q][lo:lo + dr.PACK_ROWS], m.sent_count(o, q), dr.pack_need(o, q)
            seen.add((o, kind))
            if kind == "every":
                assert mask.all() and t == m.nmine(o)
            elif kind == "none":
                assert not mask.any() and t == 0
            elif kind == "but_last":
                assert mask.sum() == dr.PACK_ROWS - 1 and not mask[live[-1]] and 0 < t == m.nmine(o) - own[live[-1]]
            elif kind == "first":
                assert mask.sum() == 1 and mask[0] and t == own[0]
            elif kind == "last":
                assert mask.sum() == 1 and mask[-1] and t == own[-1]
            else:                                       # t == nmine with a mask that is not all ones
                assert t == m.nmine(o) and not mask.all() and np.array_equal(np.flatnonzero(mask), live)
    assert len(seen) == 18


@pytest.mark.parametrize("n_inner", dr.PANEL_INNER)
def test_panel_rows_lengths_and_hub(n_inner):
    c, m = dr.case("panel_rows_%d" % n_inner), dr.model("panel_rows_%d" % n_inner)
    assert (c.world, c.inner, c.ncol) == (3, n_inner, 8192)
    for k, n in dr.PANEL_SPECIAL[n_inner].items():
        assert k in (0, 1, 2, 62, 63, 64, n_inner - 1) and m.blen[k] == n
    hub = m.a[1][m.a[0] == dr.PANEL_HUB]
    assert np.array_equal(hub, np.arange(n_inner)) and c.a_bounds[dr.PANEL_HUB_RANK] <= dr.PANEL_HUB < c.a_bounds[dr.PANEL_HUB_RANK + 1]
    assert int(m.blen.sum()) > dr.MID_MAX                # the hub's products: heavy
    p = m.panel(dr.PANEL_HUB_RANK)
    assert p[0].size == m.b[0].size                      # its panel is the whole of B: every entry of the row array is read
    assert m.stats(dr.PANEL_HUB_RANK)["panel_tuples"] == int(m.blen.sum())
    plen = np.bincount(p[0], minlength=n_inner)
    assert np.array_equal(plen, m.blen)
    for g in range(0, n_inner, 64):                     # empty rows inside every group that holds anything
        grp = plen[g:g + 64]
        assert grp.sum() == 0 or (grp == 0).any() or grp.size == 1


def test_panel_rows_cover_the_row_array_edges():
    lens = {n: dr.model("panel_rows_%d" % n).blen for n in dr.PANEL_INNER}
    assert sorted(n % 64 for n in dr.PANEL_INNER) == [0, 1, 1, 63]
    assert any((v == dr.ROWS_LONG).any() for v in lens.values()) and any((v == dr.ROWS_LONG + 1).any() for v in lens.values())
    assert lens[63][62] == 2049 and lens[64][63] == 5000 and lens[65][64] == 2049 and lens[257][256] == 5000    # a long last row
    assert lens[64][62] == 2048 and lens[65][63] == 2048 and lens[257][63] == 2048                                # 2048: not long
    assert lens[257][128:192].sum() == 0 and lens[257][64:128].sum() > 0 and lens[257][192:256].sum() > 0       # a wholly empty group
    assert {0, 1} <= set(lens[63][:3].tolist()) and lens[65][0] == 0


@pytest.mark.parametrize("kind,W", list(dr.PLANNED_A_BOUNDS))
def test_planned_tiles_blocks_keep_the_plan(kind, W):
    c = dr.case("planned_tiles_%s_W%d" % (kind, W))
    p = c.claims["plan"]
    whole = p.cut(c.claims["scheme"])
    cut = [dr.planned_cut(c, q) for q in range(W)]
    assert sum(x.rows_heavy for x in cut) == whole.rows_heavy == p.A.shape[0]
    assert sum(x.products_tiles for x in cut) == whole.products_tiles > 0
    assert sum(x.tiles for x in cut) == whole.tiles
    assert c.knobs["window"] == p.W and c.knobs["tiles_v1"] == dr.tp.TILES_V1[c.claims["scheme"]]
    assert any(x.rows_heavy == 0 for x in cut) == (0 in np.diff(c.a_bounds))
    assert c.b_bounds[-1] == p.B.shape[0] and min(np.diff(c.b_bounds)) > 0       # B cut over the inner index, every rank an owner


@pytest.mark.parametrize("W,same", dr.ZERO_NAN)
def test_zero_nan_first_kept_tuple_is_in_the_last_block(W, same):
    c = dr.zero_nan(W, same)
    assert c.zero_nan and c.world == W and (c.B is None) == same
    k = dr.first_kept(c.Bm, c.tB, True)                 # op(B)'s reference sequence is column-major
    row = int(dr.op(c.Bm, c.tB)[0][k])
    assert c.b_bounds[W - 1] <= row < c.b_bounds[W]
    first = np.lexsort((dr.op(c.A, c.tA)[1], dr.op(c.A, c.tA)[0]))[0]
    assert np.isnan(c.A.val[first])                     # op(A)'s own sequence starts with a NaN
    for M, t, bounds in ((c.A, c.tA, c.a_bounds), (c.Bm, c.tB, c.b_bounds)):
        lo, hi = bounds[dr.ZERO_NAN_JUNK[W]], bounds[dr.ZERO_NAN_JUNK[W] + 1]
        r = dr.op(M, t)[0]
        v = M.val[(r >= lo) & (r < hi)]
        assert v.size > 3 and np.all(np.isnan(v) | (v == 0)) and np.isnan(v).any() and (v == 0).any()
    # NaNs that only a per-block leading run would drop: the two settings differ, and so do they with the NaNs kept
    w1, w0 = dr.oracle_product(c, True), dr.oracle_product(c, False)
    assert not same_tuples(w1, w0) and np.isnan(w1[2]).any()


# ---- the harness on host memory

def play(model, fail=None, lie=None, timeout=dk.TIMEOUT):
    """Fake ranks play the model's five calls through run_ranks on host buffers; each returns what it received as
    got[call][peer] -> bytes.  lie = (rank, call, peer): that rank announces one byte more than its peer sends."""
    W = model.case.world
    ex = dk.Exchange(W, fail=fail, timeout=timeout)

    def fake(rank, _ctx, xfer):
        got = []
        for k in range(5):
            send = [ctypes.create_string_buffer(model.calls(rank)[k][p], max(1, len(model.calls(rank)[k][p]))) for p in range(W)]
            sendb = [len(model.calls(rank)[k][p]) for p in range(W)]
            recvb = [len(model.calls(p)[k][rank]) for p in range(W)]
            if lie and lie[:2] == (rank, k):
                recvb[lie[2]] += 1
            recv = [ctypes.create_string_buffer(max(1, n + 1)) for n in recvb]
            xfer([ctypes.addressof(b) for b in send], sendb, [ctypes.addressof(b) for b in recv], recvb, None)
            got.append([recv[p].raw[:recvb[p]] for p in range(W)])
        return got
    return ex, dk.run_ranks(W, fake, timeout=timeout, copy=ctypes.memmove, exchange=ex)


@pytest.mark.parametrize("name", ["worlds_3", "worlds_64"])
def test_harness_routes_send_p_q_to_recv_q_p(name):
    m = dr.model(name)
    W = m.case.world
    ex, out = play(m)
    out.raise_first()
    for q in range(W):
        for k in range(5):
            for p in range(W):
                assert out.values[q][k][p] == m.calls(p)[k][q], (q, k, p)
            assert ex.log[q][k] == m.calls(q)[k]
        assert len(ex.log[q]) == 5
        dr.compare_sends(m, q, ex.log[q], name)


def test_compare_sends_names_the_place():
    m = dr.model("worlds_3")
    r, p = next((r, p) for r in range(3) for p in range(3) if len(m.calls(r)[3][p]) >= 8)
    calls = [list(x) for x in m.calls(r)]
    bad = np.frombuffer(calls[3][p], np.int32).copy()
    bad[1] += 1
    calls[3][p] = bad.tobytes()
    with pytest.raises(AssertionError, match=r"rank %d, round 2, segment 0 \(columns\), to peer %d: first difference at element 1" % (r, p)):
        dr.compare_sends(m, r, calls, "planted")
    with pytest.raises(AssertionError, match="4 transport calls"):
        dr.compare_sends(m, r, calls[:4], "planted")


def test_harness_reports_a_size_mismatch():
    """Rank 2 expects one byte more of rank 0's row lengths than rank 0 sends: RCCL would hang, the harness says which."""
    t0 = time.monotonic()
    ex, out = play(dr.model("worlds_3"), lie=(2, 2, 0))
    assert all(e is not None for e in out.errors)
    assert isinstance(out.errors[2], dk.SizeMismatch) and "rank 0 sends" in str(out.errors[2]) and "rank 2" in str(out.errors[2])
    assert all(isinstance(e, (dk.SizeMismatch, threading.BrokenBarrierError)) for e in out.errors)
    assert time.monotonic() - t0 < dk.TIMEOUT / 4


@pytest.mark.parametrize("name,bad", [("worlds_3", 1), ("worlds_64", 37)])
def test_a_rank_that_raises_fails_every_rank(name, bad):
    """A failure planted in one rank's second call: every rank returns an error well inside the timeout, and no thread is
    left behind."""
    before = threading.active_count()
    t0 = time.monotonic()
    ex, out = play(dr.model(name), fail=lambda rank, call: (rank, call) == (bad, 1))
    assert isinstance(out.errors[bad], dk.PlantedFailure)
    assert all(isinstance(e, threading.BrokenBarrierError) for r, e in enumerate(out.errors) if r != bad)
    assert all(v is None for v in out.values)
    assert time.monotonic() - t0 < dk.TIMEOUT / 4 and threading.active_count() == before and not dk._hung
    with pytest.raises(AssertionError, match="rank %d of" % bad):
        out.raise_first()


def test_a_rank_that_raises_outside_the_transport():
    """fn itself raises on one rank between two calls: the others, already waiting in the next call, are released."""
    m = dr.model("worlds_3")

    def fn(rank, _ctx, xfer):
        if rank == 0:
            raise ValueError("planted")
        buf = ctypes.create_string_buffer(8)
        xfer([ctypes.addressof(buf)] * 3, [8] * 3, [ctypes.addressof(buf)] * 3, [8] * 3, None)
    out = dk.run_ranks(m.case.world, fn, copy=ctypes.memmove)
    assert isinstance(out.errors[0], ValueError) and all(isinstance(e, threading.BrokenBarrierError) for e in out.errors[1:])
