"""spsamd_color on the device against tests/color_ref.py (pinned on the host by tests/test_color_host.py): color, perm,
color_ptr, ncolors, rounds, adjacency, max_degree and conflicts exactly equal -- all are functions of the key set, the
order, the seed and the flag alone.  The color_path, color_row and threshold knobs run so that every vertex meets both
round kernels and every round both ways of running it; launches, fused_rounds and the rows by class are checked against
host restatements."""
import ctypes as C

import numpy as np
import pytest

from spsparse_amd import workloads as wl
from tests import color_ref as cr
from tests import factor_ref as fr
from tests.gpu_util import Knobs, check_tuples as _check, coo as _coo, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SENT = -77


def _stats(st):
    return dict(ncolors=st.ncolors, rounds=st.rounds, adjacency=st.adjacency, max_degree=st.max_degree, conflicts=st.conflicts)


def _same(got, ref, what):
    color, perm, cptr, st = got
    assert _stats(st) == {k: ref[k] for k in _stats(st)}, "%s: stats %r, want %r" % (what, _stats(st), {k: ref[k] for k in _stats(st)})
    for name, g in (("color", color), ("perm", perm), ("color_ptr", cptr)):
        assert g.dtype == np.int32 and np.array_equal(g, ref[name]), "%s: %s differs" % (what, name)


def _color_device(ctx, a, n, order, seed, flags, t='.', with_perm=True, with_ptr=True):
    """The call into sentinel-filled device tensors, four entries longer than needed: (color, perm, color_ptr, stats) as
    host arrays, the tails checked untouched."""
    import torch
    d = torch.device("cuda:0")
    tc, tp, tq = (torch.full((m + 4,), SENT, dtype=torch.int32, device=d) for m in (n, n, n + 1))
    nc, st = ctx.color(a, order, seed, flags, t, out=(tc, tp if with_perm else None, tq if with_ptr else None), stats=True)
    hc, hp, hq = tc.cpu().numpy(), tp.cpu().numpy(), tq.cpu().numpy()
    assert nc == st.ncolors
    assert np.all(hc[n:] == SENT) and np.all(hp[n if with_perm else 0:] == SENT) and np.all(hq[nc + 1 if with_ptr else 0:] == SENT)
    return hc[:n], hp[:n], hq[:nc + 1], st


def _operand(ctx, rng, K, n, mode, t, device, keep):
    """op(A) with the key set K, stored for transpose t.  mode 0: raw, shuffled, a third of the keys repeated, explicit
    zeros among the values (or val NULL); 1: trusted, sorted, sort0 naming op()'s rows; 2: a chained select result that keeps
    K out of a larger operand; 3: a prepared handle.  Returns (Coo, handle or None)."""
    from spsparse_amd import capi
    r, c = K
    if mode == 0:
        dup = rng.integers(0, r.size, r.size // 3) if r.size else np.zeros(0, np.int64)
        r, c = np.r_[r, r[dup]], np.r_[c, c[dup]]
        o = rng.permutation(r.size)
        r, c = r[o], c[o]
        v = rng.choice((0.0, 1.0, -2.0), r.size)
        i0, i1 = (c, r) if t == 'T' else (r, c)
        return _coo((i0, i1, v), (n, n), -1, device=device, keep=keep, no_val=bool(rng.integers(2))), None
    if mode == 1:
        i0, i1 = (c, r) if t == 'T' else (r, c)
        return _coo((i0, i1, np.zeros(r.size)), (n, n), 1 if t == 'T' else 0, device=device, keep=keep), None
    if mode == 2:                                                       # stored keys: K's (transposed for 'T') at 1.0, extras at 0.25
        i0, i1 = (c, r) if t == 'T' else (r, c)
        extra = rng.integers(0, n, (2, n))
        s0, s1 = cr.unique_keys(np.r_[i0, extra[0]], np.r_[i1, extra[1]])
        big = np.isin(s0 * n + s1, i0 * n + i1)
        sres = ctx.select(_coo((s0, s1, np.where(big, 1.0, 0.25)), (n, n), 0, device=device, keep=keep), capi.SELECT_ABS_GE, dparam=0.5)
        return capi.result_operand(sres), None
    i0, i1 = (c, r) if t == 'T' else (r, c)
    h = capi.Operand(ctx, _coo((i0, i1, np.ones(r.size)), (n, n), -1, device=device, keep=keep), t, capi.AS_A)
    return h.coo, h


def test_semantic_fuzz(ctx):
    """200 patterns of n <= 40, symmetric and not, with empty and diagonal-only rows; the operand kind is the trial's base-4
    digit and (color_path, color_row) its base-9 digit above that, so every kind meets every setting; transposes, host and
    device operands and buffers, the order and the seed are drawn.  Every trial runs without the flag (against the
    symmetrised reference; the other transpose must give the same) and with it (against the row-only reference, which on a
    symmetric pattern is the same colouring, and whose conflicts count a false promise)."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2201)
    seen = set()
    for trial in range(200):
        n = int(rng.integers(1, 41))
        mode, combo = trial % 4, (trial // 4) % 9
        path, row = combo % 3, combo // 3
        symmetric, t = bool(rng.integers(2)), '.' if rng.integers(2) == 0 else 'T'
        order, seed = int(rng.integers(2)), int(rng.integers(0, 2 ** 32))
        dev_a, dev_out = bool(rng.integers(2)), bool(rng.integers(2))
        K = cr.random_pattern(rng, n, symmetric)
        keep = []
        a, h = _operand(ctx, rng, K, n, mode, t, dev_a, keep)
        what = "trial %d n %d mode %d %s sym %d order %d path %d row %d dev %d/%d" % (trial, n, mode, t, symmetric, order, path, row, dev_a, dev_out)
        try:
            with Knobs(ctx, {"color_path": path, "color_row": row}):
                for flags in (0, capi.COLOR_SYMMETRIC):
                    ref = cr.reference(K, n, order, seed, flags, fast=bool(trial & 8))
                    if dev_out:
                        got = _color_device(ctx, a, n, order, seed, flags, t)
                    else:
                        res = capi.Result()
                        got = ctx.color(a, order, seed, flags, t, stats=True, result=res)
                        assert (res.shape0, res.shape1, res.nnz_a) == (n, n, K[0].size), what
                    _same(got, ref, "%s flags %d" % (what, flags))
                    st = got[3]
                    cl = cr.classes(ref["deg"], capi.color_wave_deg, row)
                    assert (st.rows_thread, st.rows_wave) == (int(np.count_nonzero(cl == 1)), int(np.count_nonzero(cl == 2))), what
                    assert (st.launches, st.fused_rounds) == cr.plan(ref["round"], cl, capi.color_fuse_rows, path, flags), what
                    if flags == 0:
                        assert st.conflicts == 0, what
                        if mode < 2:                                    # the same stored arrays read the other way round: the graph is the same
                            _same(ctx.color(a, order, seed, 0, 'T' if t == '.' else '.', stats=True), ref, what + " transposed")
                    elif symmetric:
                        assert np.array_equal(got[0], cr.reference(K, n, order, seed, 0)["color"]), what
                    seen.add(("conf", flags, symmetric, ref["conflicts"] > 0))
        finally:
            if h is not None:
                h.close()
        seen.add(("combo", mode, path, row)); seen.add(("op", t, dev_a, dev_out)); seen.add(("order", order))
    assert len([s for s in seen if s[0] == "combo"]) == 36 and len([s for s in seen if s[0] == "op"]) == 8
    assert len([s for s in seen if s[0] == "order"]) == 2
    assert ("conf", 1, False, True) in seen and ("conf", 1, True, True) not in seen and ("conf", 0, False, True) not in seen


@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_cliques_cross_the_colour_windows(ctx, n):
    """K_n: the colours are 0 .. n - 1 in visiting order, so the last vertices find one or two windows of 64 full."""
    from spsparse_amd import capi
    K = cr.clique(n)
    ref = cr.reference(K, n, cr.HASH, 5)
    assert ref["ncolors"] == n == ref["rounds"]
    keep = []
    a = _coo((K[0], K[1], np.ones(K[0].size)), (n, n), 0, device=True, keep=keep)
    for row in (0, 1, 2):
        for path in (1, 2):
            with Knobs(ctx, {"color_row": row, "color_path": path}):
                got = ctx.color(a, cr.HASH, 5, stats=True)
            _same(got, ref, "K%d row %d path %d" % (n, row, path))
            wave = row == 2 or (row == 0 and n - 1 > capi.color_wave_deg)
            assert (got[3].rows_thread, got[3].rows_wave) == ((0, n) if wave else (n, 0))
            assert (got[3].launches, got[3].fused_rounds) == ((n, 0) if path == 1 else (1, n))


def test_hubs_beyond_the_first_window(ctx):
    """A clique of 70 hubs, each with 5000 leaves: wave-class rows whose colours lie beyond the first window of 64."""
    from spsparse_amd import capi
    K, n = cr.hubs(70, 5000)
    keep = []
    a = _coo((K[0], K[1], np.ones(K[0].size)), (n, n), 0, device=True, keep=keep)
    for order in (cr.HASH, cr.DEGREE):
        ref = cr.reference(K, n, order, 1)
        assert ref["color"][:70].max() >= 64 and ref["max_degree"] == 5069
        got = _color_device(ctx, a, n, order, 1, 0)
        _same(got, ref, "hubs order %d" % order)
        assert (got[3].rows_thread, got[3].rows_wave) == (n - 70, 70)
        cl = cr.classes(ref["deg"], capi.color_wave_deg)
        assert (got[3].launches, got[3].fused_rounds) == cr.plan(ref["round"], cl, capi.color_fuse_rows)
    got = ctx.color(a, cr.DEGREE, 1, 1, stats=True)                     # the pattern is symmetric: the flag changes nothing
    _same(got, ref, "hubs with the flag")


@pytest.mark.parametrize("sizes", [[1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000, 1, 1, 1, 5000, 2],
                                   [2000, 1, 767, 1, 255, 1]], ids=["wide", "edges"])
def test_round_widths(ctx, sizes):
    """Rounds of known sizes (by_rounds).  The worklist of round r holds the rounds from r on: in the second list it is
    3025, 1025, 1024, 257, 256 and 1 vertices long, one more and exactly color_fuse_rows 1024 and 256.  In the first the
    one vertex of round 13 has 5000 neighbours: wave-class unless color_row says thread, a launch more per round while
    the rounds are launched one by one, and a row for a wave of the fused run."""
    from spsparse_amd import capi
    rng = np.random.default_rng(2203)
    K, rnd = cr.by_rounds(rng, sizes, 9)
    n = sum(sizes)
    ref = cr.reference(K, n, cr.HASH, 9)
    assert np.array_equal(ref["round"], rnd) and list(np.bincount(rnd)) == sizes
    keep = []
    a = _coo((K[0], K[1], np.ones(K[0].size)), (n, n), 0, device=True, keep=keep)
    plans = set()
    for row in (0, 1):
        for knob, value in (("color_fuse_rows", 0), ("color_fuse_rows", 256), ("color_fuse_rows", 1024), ("color_path", 1), ("color_path", 2)):
            with Knobs(ctx, {knob: value, "color_row": row}):
                got = ctx.color(a, cr.HASH, 9, capi.COLOR_SYMMETRIC, stats=True)
            what = "%s %d row %d" % (knob, value, row)
            _same(got, ref, what)
            fuse = value if knob == "color_fuse_rows" and value else capi.color_fuse_rows
            want = cr.plan(rnd, cr.classes(ref["deg"], capi.color_wave_deg, row), fuse, value if knob == "color_path" else 0, capi.COLOR_SYMMETRIC)
            assert (got[3].launches, got[3].fused_rounds) == want, "%s: launches %d fused %d, want %r" % (what, got[3].launches, got[3].fused_rounds, want)
            plans.add(want)
    assert len(plans) >= 4


def test_degrees_at_the_class_threshold(ctx):
    """Stars whose centres have color_wave_deg - 1, + 0 and + 1 leaves, under the default threshold and under 10."""
    from spsparse_amd import capi
    for wave_deg, knob in ((capi.color_wave_deg, 0), (10, 10)):
        a_, b_, base = [], [], 3
        for leaves in (wave_deg - 1, wave_deg, wave_deg + 1):
            a_.append(np.full(leaves, leaves - wave_deg + 1))
            b_.append(base + np.arange(leaves))
            base += leaves
        n = base
        a_, b_ = np.concatenate(a_), np.concatenate(b_)                 # centres 0, 1, 2
        K = cr.unique_keys(np.r_[a_, b_], np.r_[b_, a_])
        ref = cr.reference(K, n, cr.DEGREE, 2)
        assert list(ref["deg"][:3]) == [wave_deg - 1, wave_deg, wave_deg + 1]
        keep = []
        with Knobs(ctx, {"color_wave_deg": knob}):
            got = ctx.color(_coo((K[0], K[1], np.ones(K[0].size)), (n, n), -1, keep=keep), cr.DEGREE, 2, stats=True)
        _same(got, ref, "stars, wave_deg %d" % wave_deg)
        assert (got[3].rows_thread, got[3].rows_wave) == (n - 1, 1)


def _reordered(S, perm, n):
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return fr.sorted_unique(inv[S[0]], inv[S[1]], S[2])


@pytest.mark.parametrize("name", ["poisson64", "rmat10"])
def test_chain_into_the_factorisation(ctx, name):
    """colour -> extract(perm, perm) -> factor_ilu0: the reordered matrix has at most ncolors levels and F has the bits of
    factor_ref on the reordered S."""
    from spsparse_amd import capi
    if name == "poisson64":
        S = fr.sorted_unique(*wl.poisson2d(64)[:3])
        n = 64 * 64
    else:
        S, n = fr.rmat_sym(10, 8, 3, 50.0)
    keep = []
    a = _coo(S, (n, n), 0, device=True, keep=keep)
    for order in (cr.HASH, cr.DEGREE):
        color, perm, cptr, st = ctx.color(a, order, 4, capi.COLOR_SYMMETRIC, stats=True)
        ref = cr.reference((S[0], S[1]), n, order, 4)
        _same((color, perm, cptr, st), ref, name)
        P = ctx.extract(a, perm, perm)
        want = _reordered(S, perm, n)
        _check(ctx.fetch(P), want, "P A P^T")
        res, fst = ctx.factor_ilu0(capi.result_operand(P), stats=True)
        assert fst.levels <= st.ncolors, (fst.levels, st.ncolors)
        f, _rs = fr.ilu0_fast(want, n)
        _check(ctx.fetch(res), (want[0], want[1], f), "F of the reordered matrix")
    if name == "poisson64":
        assert st.ncolors <= 5 and ctx.factor_ilu0(a, stats=True)[1].levels == 127


def test_refusals(ctx):
    """SPSAMD_ECAPACITY reports the colours and leaves sentinel-filled buffers alone; every SPSAMD_EINVAL and SPSAMD_EDIM of
    the header, with nothing written."""
    import torch
    from spsparse_amd import capi
    L = ctx.L
    keep = []
    K = cr.clique(6)
    n = 6
    A = (K[0].astype(np.int32), K[1].astype(np.int32), np.ones(K[0].size))
    a = _coo(A, (n, n), 0, keep=keep)
    cnt = C.c_size_t(99)

    def bufs(device):
        if device:
            return [torch.full((16,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        return [np.full(16, SENT, np.int32) for _ in range(3)]

    def ptr(x):
        return None if x is None else (x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)

    def call(a, b, t=b'.', order=0, flags=0, cap=16, mem=None, pa=None, pcnt=None):
        mem = (capi.MEM_DEVICE if isinstance(b[0], torch.Tensor) else capi.MEM_HOST) if mem is None else mem
        rc = L.spsamd_color(ctx.h, C.byref(a) if pa is None else pa, t, order, 1, flags, ptr(b[0]), ptr(b[1]), ptr(b[2]), cap, mem,
                            C.byref(cnt) if pcnt is None else pcnt, None, None)
        return rc, L.spsamd_last_error(ctx.h).decode()

    def untouched(b):
        return all(bool((x == SENT).all()) for x in b if x is not None)

    for device in (False, True):
        b = bufs(device)
        for cap in (0, 6):
            cnt.value = 99
            rc, msg = call(a, b, cap=cap)
            assert rc == -5 and cnt.value == 6 and "color_ptr" in msg and untouched(b), (device, cap)
        assert call(a, b, cap=7)[0] == 0 and cnt.value == 6
        got = [x.cpu().numpy() if device else x for x in b]
        assert sorted(got[0][:6]) == list(range(6)) and list(got[2][:7]) == list(range(7)) and np.all(got[2][7:] == SENT)
        assert call(a, [b[0], None, None], cap=0)[0] == 0               # without color_ptr the capacity means nothing
        b = bufs(device)
        assert call(a, b, pa=C.POINTER(capi.Coo)())[0] == -2 and call(a, [None, b[1], b[2]])[0] == -2
        assert call(a, b, pcnt=C.POINTER(C.c_size_t)())[0] == -2
        assert call(a, b, order=2)[0] == -2 and call(a, b, order=-1)[0] == -2 and call(a, b, flags=2)[0] == -2
        assert call(a, b, mem=2)[0] == -2 and call(a, b, mem=3)[0] == -2
        rc, msg = call(_coo(A, (6, 7), 0, keep=keep), b)
        assert rc == -1 and "square" in msg
        assert call(_coo((A[0], np.where(A[1] == 5, 6, A[1]).astype(np.int32), A[2]), (n, n), -1, keep=keep), b)[0] == -2      # out of bounds
        assert call(_coo((A[0][::-1].copy(), A[1], A[2]), (n, n), 0, keep=keep), b)[0] == -2                                    # a false sort0
        big = _coo(A, (n, n), -1, keep=keep)
        big.nnz = 1 << 31
        assert call(big, b)[0] == -2
        assert untouched(b), device
        # overlaps: the buffers with each other
        if device:
            one = torch.full((32,), SENT, dtype=torch.int32, device="cuda:0")
            views = (one[0:16], one[4:20], one[20:32])
        else:
            one = np.full(32, SENT, np.int32)
            views = (one[0:16], one[4:20], one[20:32])
        rc, msg = call(a, [views[0], views[1], views[2]])
        assert rc == -2 and "overlap" in msg
        assert call(a, [views[0], views[2], views[1]], cap=7)[0] == -2 and bool((one == SENT).all())
    # ... with A's arrays (device operand, device buffers), and a device buffer inside an output set
    t = [torch.from_numpy(x).cuda() for x in A[:2]]
    ad = capi.device_coo(t[0].data_ptr(), t[1].data_ptr(), None, len(A[0]), (n, n), 0)
    b = bufs(True)
    rc, msg = call(ad, [t[1][:6], b[1], b[2]])
    assert rc == -2 and "A's arrays" in msg and np.array_equal(t[1].cpu().numpy(), A[1])
    r0 = ctx.consolidate(a, 0)

    rc = L.spsamd_color(ctx.h, C.byref(a), b'.', 0, 1, 0, b[0].data_ptr(), r0.idx1, None, 0, capi.MEM_DEVICE, C.byref(cnt), None, None)
    assert rc == -2 and "output set" in L.spsamd_last_error(ctx.h).decode()
    _check(ctx.fetch(r0), A, "a result made before the refusals")
    # a chained result is read in place and stays valid
    color, perm, cptr = ctx.color(capi.result_operand(r0), seed=1)
    assert sorted(color) == list(range(6))
    _check(ctx.fetch(r0), A, "the operand after the colouring")
    # n = 0, and a matrix without tuples
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    color, perm, cptr, st = ctx.color(_coo(e, (0, 0), -1, keep=keep), stats=True)
    assert color.size == 0 and perm.size == 0 and list(cptr) == [0] and (st.ncolors, st.rounds) == (0, 0)
    color, perm, cptr, st = ctx.color(_coo(e, (5, 5), -1, keep=keep), stats=True)
    assert list(color) == [0] * 5 and list(perm) == list(range(5)) and list(cptr) == [0, 5]
    assert (st.ncolors, st.rounds, st.adjacency, st.launches) == (1, 1, 0, 0)
