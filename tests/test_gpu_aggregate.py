"""spsamd_aggregate on the device against tests/aggregate_ref.py (pinned on the host by tests/test_aggregate_host.py): agg,
members, agg_ptr, naggregates, rounds, the rings, the sizes, adjacency and max_degree exactly equal -- all are functions of
the key set, the order, the seed and the flag alone.  The agg_path, agg_row and threshold knobs run so that every vertex meets
both row kernels and every round both ways of running it; launches, fused_rounds and the rows by class are checked against
host restatements."""
import ctypes as C

import numpy as np
import pytest

from spsparse_amd import workloads as wl
from tests import aggregate_ref as ar
from tests import color_ref as cr
from tests import factor_ref as fr
from tests.gpu_util import Knobs, check_tuples as _check, coo as _coo, ctx  # noqa: F401
from tests.test_gpu_color import _operand

pytestmark = pytest.mark.gpu

SENT = -77
STATS = ("naggregates", "rounds", "ring1", "ring2", "max_size", "min_size", "adjacency", "max_degree", "asymmetric")


def _stats(st):
    return {k: getattr(st, k) for k in STATS}


def _same(got, ref, what):
    agg, members, aptr, st = got
    assert _stats(st) == {k: ref[k] for k in STATS}, "%s: stats %r, want %r" % (what, _stats(st), {k: ref[k] for k in STATS})
    for name, g in (("agg", agg), ("members", members), ("agg_ptr", aptr)):
        assert g.dtype == np.int32 and np.array_equal(g, ref[name]), "%s: %s differs" % (what, name)


def _launches(st, ref, what, fuse=None, path=0, row=0, wave_deg=None):
    from spsparse_amd import capi
    cl = ar.classes(ref["deg"], wave_deg or capi.agg_wave_deg, row)
    assert (st.rows_thread, st.rows_wave) == (int(np.count_nonzero(cl == 1)), int(np.count_nonzero(cl == 2))), what
    want = ar.plan(ref["lists"], cl, fuse or capi.agg_fuse_rows, path)
    assert (st.launches, st.fused_rounds) == want, "%s: launches %d fused %d, want %r" % (what, st.launches, st.fused_rounds, want)
    return want


def _agg_device(ctx, a, n, order, seed, flags, t='.', with_members=True, with_ptr=True):
    """The call into sentinel-filled device tensors, four entries longer than needed: (agg, members, agg_ptr, stats) as host
    arrays, the tails checked untouched."""
    import torch
    d = torch.device("cuda:0")
    ta, tm, tq = (torch.full((m + 4,), SENT, dtype=torch.int32, device=d) for m in (n, n, n + 1))
    na, st = ctx.aggregate(a, order, seed, flags, t, out=(ta, tm if with_members else None, tq if with_ptr else None), stats=True)
    ha, hm, hq = ta.cpu().numpy(), tm.cpu().numpy(), tq.cpu().numpy()
    assert na == st.naggregates
    assert np.all(ha[n:] == SENT) and np.all(hm[n if with_members else 0:] == SENT) and np.all(hq[na + 1 if with_ptr else 0:] == SENT)
    return ha[:n], hm[:n], hq[:na + 1], st


def _device_coo(K, n, keep):
    return _coo((K[0], K[1], np.ones(K[0].size)), (n, n), 0, device=True, keep=keep)


def test_semantic_fuzz(ctx):
    """200 patterns of n <= 40, symmetric and not, with empty and diagonal-only rows; the operand kind is the trial's base-4
    digit and (agg_path, agg_row) its base-9 digit above that, so every kind meets every setting; transposes, host and device
    operands and buffers, the order and the seed are drawn.  Every trial runs without the flag (the other transpose must give
    the same) and with it: on a symmetric pattern the same aggregation, on any other SPSAMD_EINVAL and untouched buffers."""
    import torch
    from spsparse_amd import capi
    rng = np.random.default_rng(2401)
    seen = set()
    for trial in range(200):
        n = int(rng.integers(1, 41))
        mode, combo = trial % 4, (trial // 4) % 9
        path, row = combo % 3, combo // 3
        symmetric, t = bool(rng.integers(2)), '.' if rng.integers(2) == 0 else 'T'
        order, seed = int(rng.integers(2)), int(rng.integers(0, 2 ** 32))
        dev_a, dev_out = bool(rng.integers(2)), bool(rng.integers(2))
        per = int(rng.choice((0, 1, 20)))                               # the thread kernels: an entry a thread | four | four on lists of 20 and more
        K = cr.random_pattern(rng, n, symmetric)
        keep = []
        a, h = _operand(ctx, rng, K, n, mode, t, dev_a, keep)
        what = "trial %d n %d mode %d %s sym %d order %d path %d row %d per %d dev %d/%d" % (trial, n, mode, t, symmetric, order, path, row, per, dev_a, dev_out)
        try:
            with Knobs(ctx, {"agg_path": path, "agg_row": row, "agg_per_rows": per}):
                for flags in (0, capi.AGG_SYMMETRIC):
                    ref = ar.reference(K, n, order, seed, flags, serial=bool(trial & 8))
                    seen.add(("asym", flags, symmetric, ref["asymmetric"] > 0))
                    if ref["asymmetric"]:                               # the promise is false: refused, nothing written
                        if dev_out:
                            b = [torch.full((n + 1,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(3)]
                            p = [x.data_ptr() for x in b]
                        else:
                            b = [np.full(n + 1, SENT, np.int32) for _ in range(3)]
                            p = [x.ctypes.data for x in b]
                        cnt, st = C.c_size_t(0), capi.AggregateStats()
                        rc = ctx.L.spsamd_aggregate(ctx.h, C.byref(a), t.encode(), order, seed, flags, p[0], p[1], p[2], n + 1,
                                                    capi.MEM_DEVICE if dev_out else capi.MEM_HOST, C.byref(cnt), C.byref(st), None)
                        assert rc == -2 and "not symmetric" in ctx.L.spsamd_last_error(ctx.h).decode(), what
                        assert st.asymmetric == ref["asymmetric"] and all(bool((x == SENT).all()) for x in b), what
                        continue
                    if dev_out:
                        got = _agg_device(ctx, a, n, order, seed, flags, t)
                    else:
                        res = capi.Result()
                        got = ctx.aggregate(a, order, seed, flags, t, stats=True, result=res)
                        assert (res.shape0, res.shape1, res.nnz_a) == (n, n, K[0].size), what
                    _same(got, ref, "%s flags %d" % (what, flags))
                    _launches(got[3], ref, what, path=path, row=row)
                    ar.invariants(K, *got[:3])
                    if flags == 0 and mode < 2:                         # the same stored arrays read the other way round: the graph is the same
                        _same(ctx.aggregate(a, order, seed, 0, 'T' if t == '.' else '.', stats=True), ref, what + " transposed")
                    if flags:
                        assert np.array_equal(got[0], ar.reference(K, n, order, seed, 0)["agg"]), what
        finally:
            if h is not None:
                h.close()
        seen.add(("combo", mode, path, row)); seen.add(("op", t, dev_a, dev_out)); seen.add(("order", order)); seen.add(("per", per, path))
    assert len([s for s in seen if s[0] == "combo"]) == 36 and len([s for s in seen if s[0] == "op"]) == 8
    assert len([s for s in seen if s[0] == "order"]) == 2 and len([s for s in seen if s[0] == "per"]) == 9
    assert ("asym", 1, False, True) in seen and ("asym", 1, True, False) in seen and ("asym", 1, True, True) not in seen


def _by_rank(n, seed, roles):
    """Vertex labels by key rank under HASH: roles is a list of counts; returns one index array per role, the first role
    taking the vertices that come first in the visiting order."""
    visit = np.argsort(-cr.hash32(np.arange(n), seed).astype(np.int64), kind="stable")
    off = np.r_[0, np.cumsum(roles)]
    return [visit[off[k]:off[k + 1]] for k in range(len(roles))]


@pytest.mark.parametrize("d", [15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129])
def test_hub_degrees(ctx, d):
    """A hub of degree d against agg_wave_deg 16 and the default (32), the wave kernels' stride of 64 and the ring kernels' long rows: a star (the
    hub a root by DEGREE, ring 1 by HASH with a leaf first in the order), a double star (one hub the root, the other its
    ring 1 with ring-2 leaves) and a spider whose legs are a middle vertex and a pendant (by HASH with the pendants first and
    the hub last, the pendants are the roots and the hub is ring 2 with d ring-1 neighbours of d aggregates).  With and
    without the flag (the diagonal stored, so that a row names its own vertex), every agg_row."""
    from spsparse_amd import capi
    seed = 5
    cases = []
    leaf, hub = _by_rank(d + 1, seed, [d, 1])
    cases.append(("star", (np.full(d, hub[0]), leaf), d + 1, {cr.DEGREE: 0, cr.HASH: 1}, hub[0]))
    h1, h2, l1, l2 = _by_rank(2 * d, seed, [1, 1, d - 1, d - 1])
    cases.append(("double star", (np.r_[h1, np.full(d - 1, h1[0]), np.full(d - 1, h2[0])], np.r_[h2, l1, l2]), 2 * d, {cr.HASH: 1}, h2[0]))
    pend, mid, hub = _by_rank(2 * d + 1, seed, [d, d, 1])
    cases.append(("spider", (np.r_[np.full(d, hub[0]), mid], np.r_[mid, pend]), 2 * d + 1, {cr.DEGREE: 0, cr.HASH: 2}, hub[0]))
    keep = []
    for name, (ea, eb), n, rings, hubv in cases:
        K = cr.unique_keys(np.r_[ea, eb, np.arange(n)], np.r_[eb, ea, np.arange(n)])
        a = _device_coo(K, n, keep)
        for order, ring in rings.items():
            ref = ar.reference(K, n, order, seed)
            assert ref["deg"][hubv] == d == ref["max_degree"] and ref["ring"][hubv] == ring, (name, order)
            if name == "spider" and order == cr.HASH:
                assert ref["naggregates"] == d and ref["agg"][hubv] == ref["agg"][mid[0]]      # the middle vertex with the largest key
            for row, wave_deg in ((0, 16), (0, 0), (1, 0), (2, 0)):
                for flags in (0, capi.AGG_SYMMETRIC):
                    what = "%s d %d order %d row %d wave_deg %d flags %d" % (name, d, order, row, wave_deg, flags)
                    with Knobs(ctx, {"agg_row": row, "agg_wave_deg": wave_deg}):
                        got = _agg_device(ctx, a, n, order, seed, flags)
                    _same(got, ref, what)
                    _launches(got[3], ref, what, row=row, wave_deg=wave_deg)
                    if row == 0:
                        assert got[3].rows_wave == np.count_nonzero(ref["deg"] > (wave_deg or capi.agg_wave_deg)) == (d > (wave_deg or 32)) * (2 if name == "double star" else 1)
            for per in (0, 1):
                with Knobs(ctx, {"agg_path": 1, "agg_wave_deg": 16, "agg_per_rows": per}):
                    got = ctx.aggregate(a, order, seed, stats=True)
                _same(got, ref, name + " launched round by round")
                _launches(got[3], ref, name, path=1, wave_deg=16)


ROUND_CASES = {
    # The spread list of round 2 is 1023, 1024 and 1025 long: a path of 4 keeps two vertices on it, a path of 5 three.  (The
    # undecided list is part of the spread list -- an undecided vertex has itself in its closed neighbourhood -- so it is the
    # spread list that crosses agg_fuse_rows last.)
    "fuse 1023": [4] * 510 + [5],
    "fuse 1024": [4] * 512,
    "fuse 1025": [4] * 511 + [5],
    # grid edges of the wide kernels: 255, 256, 257 and 65 * 64 + 1 vertices in round 0
    "n 255": [1] * 100 + [5] * 31,
    "n 256": [1] * 101 + [5] * 31,
    "n 257": [1] * 102 + [5] * 31,
    "n 4161": [1] * 4000 + [7] * 23,
    # one deep path: 400 rounds, all but the first few fused
    "deep": [600, 1500, 1, 1],
}


@pytest.mark.parametrize("name", list(ROUND_CASES))
def test_round_widths(ctx, name):
    """Paths with descending keys (by_rounds): the undecided list's length is known in every round."""
    from spsparse_amd import capi
    lengths = ROUND_CASES[name]
    K, usizes = ar.by_rounds(lengths, 9)
    n = sum(lengths)
    ref = ar.reference(K, n, ar.HASH, 9)
    assert [U.size for U, _S in ref["lists"]] == usizes and ref["rounds"] == len(usizes)
    assert all(set(U) <= set(S) for U, S in ref["lists"])
    if name.startswith("fuse"):
        assert ref["lists"][2][1].size == int(name.split()[1]) and ref["lists"][1][1].size > 1025
        # two launches a round until the spread list holds 1024: never, for the last one
        assert ar.plan(ref["lists"], np.ones(n, int), capi.agg_fuse_rows) == {"fuse 1023": (5, 2), "fuse 1024": (5, 1), "fuse 1025": (8, 0)}[name]
    if name == "deep":
        assert ref["rounds"] == 1000
    keep = []
    a = _device_coo(K, n, keep)
    plans = set()
    # (agg_per_rows: every list by four entries a thread, whose workgroups take 1024 entries; and only the lists of 1024 and more)
    for knobs in ({}, {"agg_path": 1}, {"agg_path": 2}, {"agg_fuse_rows": 256}, {"agg_row": 2}, {"agg_row": 2, "agg_path": 2},
                  {"agg_path": 1, "agg_per_rows": 1}, {"agg_per_rows": 1}, {"agg_path": 1, "agg_per_rows": 1024}):
        with Knobs(ctx, knobs):
            got = ctx.aggregate(a, ar.HASH, 9, capi.AGG_SYMMETRIC, stats=True)
        what = "%s %r" % (name, knobs)
        _same(got, ref, what)
        plans.add(_launches(got[3], ref, what, fuse=knobs.get("agg_fuse_rows"), path=knobs.get("agg_path", 0), row=knobs.get("agg_row", 0)))
    assert len(plans) >= 2


def _tridiagonal(n):
    i = np.arange(n)
    return cr.unique_keys(np.r_[i, i[1:], i[:-1]], np.r_[i, i[:-1], i[1:]])


@pytest.mark.parametrize("name", ["poisson64", "laplace16", "rmat10", "tridiagonal4097"])
def test_larger_shapes(ctx, name):
    from spsparse_amd import capi
    if name == "poisson64":
        S, n = fr.sorted_unique(*wl.poisson2d(64)[:3]), 64 * 64
    elif name == "laplace16":
        S, n = fr.sorted_unique(*wl.laplace3d(16)[:3]), 16 ** 3
    elif name == "rmat10":
        S, n = fr.rmat_sym(10, 8, 3, 50.0)
    else:
        n = 4097
        S = _tridiagonal(n)
    K = (np.asarray(S[0], np.int64), np.asarray(S[1], np.int64))
    keep = []
    a = _device_coo(K, n, keep)
    for order in (ar.HASH, ar.DEGREE):
        ref = ar.reference(K, n, order, 4)
        got = _agg_device(ctx, a, n, order, 4, capi.AGG_SYMMETRIC)
        _same(got, ref, "%s order %d" % (name, order))
        _launches(got[3], ref, name)
        ar.invariants(K, *got[:3])
        _same(ctx.aggregate(a, order, 4, 0, stats=True), ref, "%s order %d without the flag" % (name, order))
    if name == "tridiagonal4097":
        assert ref["max_size"] <= 5 and ref["min_size"] >= 1 and 4097 / 5 <= ref["naggregates"] <= 4097 / 3 + 1


def test_refusals(ctx):
    """SPSAMD_ECAPACITY reports the aggregates and leaves sentinel-filled buffers alone; every SPSAMD_EINVAL and SPSAMD_EDIM
    of the header, with nothing written."""
    import torch
    from spsparse_amd import capi
    L = ctx.L
    keep = []
    n = 9
    K = _tridiagonal(n)                                                 # three aggregates at least
    A = (K[0].astype(np.int32), K[1].astype(np.int32), np.ones(K[0].size))
    a = _coo(A, (n, n), 0, keep=keep)
    ref = ar.reference(K, n, ar.HASH, 1)
    na = ref["naggregates"]
    cnt = C.c_size_t(99)

    def bufs(device):
        if device:
            return [torch.full((16,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        return [np.full(16, SENT, np.int32) for _ in range(3)]

    def ptr(x):
        return None if x is None else (x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)

    def call(a, b, t=b'.', order=0, flags=0, cap=16, mem=None, pa=None, pcnt=None):
        mem = (capi.MEM_DEVICE if isinstance(b[0], torch.Tensor) else capi.MEM_HOST) if mem is None else mem
        rc = L.spsamd_aggregate(ctx.h, C.byref(a) if pa is None else pa, t, order, 1, flags, ptr(b[0]), ptr(b[1]), ptr(b[2]), cap, mem,
                                C.byref(cnt) if pcnt is None else pcnt, None, None)
        return rc, L.spsamd_last_error(ctx.h).decode()

    def untouched(b):
        return all(bool((x == SENT).all()) for x in b if x is not None)

    for device in (False, True):
        b = bufs(device)
        for cap in (0, na):
            cnt.value = 99
            rc, msg = call(a, b, cap=cap)
            assert rc == -5 and cnt.value == na and "agg_ptr" in msg and untouched(b), (device, cap)
        assert call(a, b, cap=na + 1)[0] == 0 and cnt.value == na
        got = [x.cpu().numpy() if device else x for x in b]
        assert np.array_equal(got[0][:n], ref["agg"]) and np.array_equal(got[1][:n], ref["members"])
        assert np.array_equal(got[2][:na + 1], ref["agg_ptr"]) and np.all(got[2][na + 1:] == SENT)
        b = bufs(device)
        assert call(a, [b[0], None, None], cap=0)[0] == 0               # without agg_ptr the capacity means nothing
        assert np.array_equal((b[0].cpu().numpy() if device else b[0])[:n], ref["agg"]) and untouched(b[1:])
        b = bufs(device)
        assert call(a, [b[0], None, b[2]])[0] == 0 and call(a, [b[0], b[1], None], cap=0)[0] == 0
        got = [x.cpu().numpy() if device else x for x in b]
        assert np.array_equal(got[1][:n], ref["members"]) and np.array_equal(got[2][:na + 1], ref["agg_ptr"])
        b = bufs(device)
        assert call(a, b, pa=C.POINTER(capi.Coo)())[0] == -2 and call(a, [None, b[1], b[2]])[0] == -2
        assert call(a, b, pcnt=C.POINTER(C.c_size_t)())[0] == -2
        assert call(a, b, order=2)[0] == -2 and call(a, b, order=-1)[0] == -2 and call(a, b, flags=2)[0] == -2
        assert call(a, b, mem=2)[0] == -2 and call(a, b, mem=3)[0] == -2
        rc, msg = call(_coo(A, (n, n + 1), 0, keep=keep), b)
        assert rc == -1 and "square" in msg
        assert call(_coo((A[0], np.where(A[1] == n - 1, n, A[1]).astype(np.int32), A[2]), (n, n), -1, keep=keep), b)[0] == -2   # out of bounds
        assert call(_coo((A[0][::-1].copy(), A[1], A[2]), (n, n), 0, keep=keep), b)[0] == -2                                    # a false sort0
        assert (A[0][1], A[1][1]) == (0, 1)
        rc, msg = call(_coo(tuple(np.delete(x, 1) for x in A), (n, n), 0, keep=keep), b, flags=capi.AGG_SYMMETRIC)             # (0, 1) is gone
        assert rc == -2 and "not symmetric" in msg
        assert untouched(b), device
        one = torch.full((32,), SENT, dtype=torch.int32, device="cuda:0") if device else np.full(32, SENT, np.int32)
        views = (one[0:16], one[4:20], one[20:32])
        rc, msg = call(a, [views[0], views[1], views[2]])
        assert rc == -2 and "overlap" in msg
        assert call(a, [views[0], views[2], views[1]], cap=na + 1)[0] == -2 and bool((one == SENT).all())
    # ... with A's arrays (device operand, device buffers), and a device buffer inside an output set
    t = [torch.from_numpy(x).cuda() for x in A[:2]]
    ad = capi.device_coo(t[0].data_ptr(), t[1].data_ptr(), None, len(A[0]), (n, n), 0)
    b = bufs(True)
    rc, msg = call(ad, [t[1][:n], b[1], b[2]])
    assert rc == -2 and "A's arrays" in msg and np.array_equal(t[1].cpu().numpy(), A[1])
    r0 = ctx.consolidate(a, 0)
    rc = L.spsamd_aggregate(ctx.h, C.byref(a), b'.', 0, 1, 0, b[0].data_ptr(), r0.idx1, None, 0, capi.MEM_DEVICE, C.byref(cnt), None, None)
    assert rc == -2 and "output set" in L.spsamd_last_error(ctx.h).decode()
    _check(ctx.fetch(r0), A, "a result made before the refusals")
    # a chained result is read in place and stays valid
    agg, members, aptr = ctx.aggregate(capi.result_operand(r0), seed=1)
    assert np.array_equal(agg, ref["agg"])
    _check(ctx.fetch(r0), A, "the operand after the aggregation")
    # n = 0, and a matrix without tuples
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    agg, members, aptr, st = ctx.aggregate(_coo(e, (0, 0), -1, keep=keep), stats=True)
    assert agg.size == 0 and members.size == 0 and list(aptr) == [0] and (st.naggregates, st.rounds, st.max_size, st.min_size) == (0, 0, 0, 0)
    agg, members, aptr, st = ctx.aggregate(_coo(e, (5, 5), -1, keep=keep), stats=True)
    assert list(agg) == list(range(5)) == list(members) and list(aptr) == list(range(6))
    assert (st.naggregates, st.rounds, st.adjacency, st.launches, st.fused_rounds, st.max_size, st.min_size) == (5, 1, 0, 1, 1, 1, 1)


def test_prolongator_end_to_end(ctx):
    """Poisson 32^2 with integer values, chained: P = prolongator(agg), A P, then P^T (A P) through spsamd_multiply, against
    the relabel-and-sum (agg[i], agg[j], sum of v) of numpy -- integer sums, so exactly equal.  A stays fetchable."""
    import torch
    from spsparse_amd import capi
    N = 32
    n = N * N
    S = fr.sorted_unique(*wl.poisson2d(N)[:3])
    assert np.array_equal(S[2], np.round(S[2]))
    keep = []
    ref = ar.reference((S[0], S[1]), n, ar.HASH, 3)
    na = ref["naggregates"]
    want = fr.sorted_unique(*_relabel(S, ref["agg"]))
    for device in (True, False):
        ra = ctx.consolidate(_coo(S, (n, n), 0, keep=keep), 0)
        a = capi.result_operand(ra)
        ta = torch.full((n,), SENT, dtype=torch.int32, device="cuda:0")
        assert ctx.aggregate(a, capi.AGG_ORDER_HASH, 3, capi.AGG_SYMMETRIC, out=(ta, None, None)) == na
        agg = ta.cpu().numpy()
        assert np.array_equal(agg, ref["agg"])
        _check(ctx.fetch(ra), S, "A after the aggregation")
        P, pkeep = capi.prolongator(ta if device else agg, na, device=device)
        assert (P.shape0, P.shape1, P.nnz, P.sort0) == (n, na, n, 0)
        ap = ctx.multiply(a, P, sink=capi.SINK_COO)
        _check(ctx.fetch(ra), S, "A after A P")
        ac = ctx.multiply(P, capi.result_operand(ap), tA='T', sink=capi.SINK_COO)
        _check(ctx.fetch(ac), want, "P^T A P, device %d" % device)
        del pkeep


def _relabel(S, agg):
    key = agg[S[0]].astype(np.int64) * (int(agg.max()) + 1) + agg[S[1]]
    u, inv = np.unique(key, return_inverse=True)
    return u // (int(agg.max()) + 1), u % (int(agg.max()) + 1), np.bincount(inv, weights=S[2])
