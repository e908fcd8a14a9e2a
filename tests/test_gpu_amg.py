"""spsamd_amg_apply and spsamd_solve_pcg_amg on the device against tests/amg_ref.py (pinned on the host by
tests/test_amg_host.py): x, the history, the iteration count, the stop reason, bb, rr0 and rr, every float as an int64 bit
pattern with zero tolerance -- each is defined by the loops of the header.  The amg_path, amg_fuse_rows, pcg_fuse and
pcg_check_every knobs run so that the level kernels, the wave kernel's rows and the fused tail meet one definition."""
import ctypes as C

import numpy as np
import pytest

from tests import add_ref as ar
from tests import amg_ref as am
from tests import krylov_ref as kr
from tests.gpu_util import Knobs, bits_same, coo as _coo, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SENT = -7.5
RAW, TRUSTED, PREPARED = 0, 1, 2
_cache = {}


def _poisson64():
    """(levels, b) of Poisson 64^2 with b = A 1, made once for the module and never written."""
    if "p64" not in _cache:
        S, n = kr.poisson2d(64)
        levels = am.hierarchy(S, n)
        assert [lv["n"] for lv in levels] == [4096, 585, 65, 8]
        _cache["p64"] = (levels, kr.apply(S, n, np.ones(n)))
    return _cache["p64"]


def _want(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _op(ctx, X, shape, t, form, keep, handles):
    """op()'s row-major tuples X as an operand that is passed with flag t: raw on the host, trusted on the device, prepared."""
    from spsparse_amd import capi
    lead = 1 if t == 'T' else 0
    st = X if t == '.' else (X[1], X[0], X[2])
    shp = shape if t == '.' else (shape[1], shape[0])
    if form == TRUSTED:
        return _coo(st, shp, lead, device=True, keep=keep)
    if form == PREPARED and min(shp) > 0:                              # (spsamd_operand_prepare does not take a dimension of 0)
        h = capi.Operand(ctx, _coo(st, shp, -1, keep=keep), t, capi.AS_A, ar.ADD, False)
        handles.append(h)
        return h.coo
    return _coo(st, shp, -1, keep=keep)


def _operands(ctx, levels, form, keep, handles, r_is_pt=True):
    """The level list Context.amg_apply takes.  r_is_pt: R is the struct of P passed with 'T' (under PREPARED: P prepared
    a second time, for 'T'); else R is an operand of its own with '.'."""
    out = []
    for l, lv in enumerate(levels):
        n = lv["n"]
        A = _op(ctx, lv["S"], (n, n), '.', form, keep, handles)
        if lv["P"] is None:
            out.append((A, '.', None, '.', None, '.'))
            continue
        nc = levels[l + 1]["n"]
        P = _op(ctx, lv["P"], (n, nc), '.', form, keep, handles)
        if not r_is_pt:
            out.append((A, '.', P, '.', _op(ctx, lv["R"], (nc, n), '.', form, keep, handles), '.'))
        elif form == PREPARED:
            out.append((A, '.', P, '.', _op(ctx, lv["R"], (nc, n), 'T', form, keep, handles), 'T'))
        else:
            out.append((A, '.', P, '.', P, 'T'))
    return out


def _close(handles):
    for h in handles:
        h.close()


def _apply(ctx, ops, params, b, device=False):
    b = np.ascontiguousarray(b, np.float64)
    if device:
        import torch
        tb, tx = torch.from_numpy(b.copy()).cuda(), torch.full((b.size,), SENT, dtype=torch.float64).cuda()
        torch.cuda.synchronize()
        _, st = ctx.amg_apply(ops, params, tb, tx)
        gx, gb = tx.cpu().numpy(), tb.cpu().numpy()
    else:
        gb, gx = b.copy(), np.full(b.size, SENT)
        _, st = ctx.amg_apply(ops, params, gb, gx)
    assert np.array_equal(gb.view(np.int64), b.view(np.int64)), "b was written"
    return gx, st


def _solve(ctx, ops, params, b, x0, tol=1e-8, max_iter=100, device=False, cap=None, result=None):
    b = np.ascontiguousarray(b, np.float64)
    if device:
        import torch
        tb, tx = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(np.array(x0, np.float64)).cuda()
        torch.cuda.synchronize()
        _, hist, st, ast = ctx.solve_pcg_amg(ops, params, tb, tx, tol, max_iter, cap, result=result)
        gx, gb = tx.cpu().numpy(), tb.cpu().numpy()
    else:
        gb, gx = b.copy(), np.array(x0, np.float64)
        _, hist, st, ast = ctx.solve_pcg_amg(ops, params, gb, gx, tol, max_iter, cap, result=result)
    assert np.array_equal(gb.view(np.int64), b.view(np.int64)), "b was written"
    got = {"x": gx, "hist": hist, "iterations": int(st.iterations), "reason": int(st.reason),
           "bb": np.float64(st.bb), "rr0": np.float64(st.rr0), "rr": np.float64(st.rr)}
    return got, st, ast


def _same(got, want, what):
    assert (got["iterations"], got["reason"]) == (want["iterations"], want["reason"]), "%s: stop (%d, %d), want (%d, %d)" % (
        what, got["iterations"], got["reason"], want["iterations"], want["reason"])
    for key in ("bb", "rr0", "rr", "x", "hist"):
        bits_same(np.atleast_1d(got[key]), np.atleast_1d(want[key]), "%s: %s" % (what, key))


PARAMS = [(pre, post, coarse, 2.0 / 3.0) for pre, post in ((1, 1), (2, 1), (0, 2), (2, 0)) for coarse in (0, 1, 4)]


# ---------------------------------------------------------------- Poisson 64^2

def test_poisson_cycle_every_parameter_set_and_operand_form(ctx):
    """amg_apply on 4096 / 585 / 65 / 8: V(1,1), V(2,1), V(0,2), V(2,0) with 0, 1 and 4 coarse sweeps; the operand forms,
    R as P with 'T' and as an operand of its own, host and device vectors take turns so that each is met by several sets."""
    levels, b = _poisson64()
    for k, prm in enumerate(PARAMS):
        keep, handles = [], []
        form, device, r_is_pt = k % 3, bool((k // 3) % 2), k % 4 != 3
        try:
            ops = _operands(ctx, levels, form, keep, handles, r_is_pt)
            want = _want(("cycle", prm), lambda: am.cycle(levels, prm, b))
            gx, st = _apply(ctx, ops, prm, b, device)
            bits_same(gx, want, "cycle %r form %d device %d" % (prm, form, device))
            assert st.levels == 4 and list(st.rows[:4]) == [4096, 585, 65, 8]
            assert list(st.nnz[:4]) == [len(lv["S"][2]) for lv in levels]
            assert st.operator_complexity == sum(len(lv["S"][2]) for lv in levels) / len(levels[0]["S"][2])
            assert st.fused_levels == 3 and st.long_rows == 0
        finally:
            _close(handles)


def test_poisson_pcg_converges_with_the_reference_bits(ctx):
    levels, b = _poisson64()
    prm = (1, 1, 4, 2.0 / 3.0)
    want = _want(("pcg", prm, 200), lambda: am.pcg(levels, prm, b, np.zeros(4096), 1e-8, 200))
    assert want["reason"] == am.CONVERGED and want["iterations"] < 166        # (166: the unpreconditioned count)
    for form, device in ((RAW, False), (TRUSTED, True), (PREPARED, True)):
        keep, handles = [], []
        try:
            got, st, ast = _solve(ctx, _operands(ctx, levels, form, keep, handles), prm, b, np.zeros(4096), 1e-8, 200, device)
            _same(got, want, "pcg V(1,1) form %d" % form)
            assert ast.levels == 4 and ast.fused_levels == 3
        finally:
            _close(handles)


def test_poisson_pcg_other_parameter_sets(ctx):
    """Six iterations from a start that is not zero: the sets that are no symmetric preconditioner are still the loop."""
    levels, b = _poisson64()
    x0 = 0.001 * (np.arange(4096) % 11) - 0.004
    keep, handles = [], []
    try:
        ops = _operands(ctx, levels, PREPARED, keep, handles)
        for prm in PARAMS:
            want = _want(("pcg6", prm), lambda: am.pcg(levels, prm, b, x0, 0.0, 6))
            got, _st, _ast = _solve(ctx, ops, prm, b, x0, 0.0, 6, device=True, cap=4)
            want = dict(want, hist=want["hist"][:4])
            _same(got, want, "pcg %r" % (prm,))
    finally:
        _close(handles)


def _enqueued(readbacks, every, max_iter):
    done = 0
    for _ in range(readbacks - 1):
        done += min(every, max_iter - done)
    return done


def test_the_knobs_never_show(ctx):
    """amg_path x amg_fuse_rows x pcg_check_every x pcg_fuse: one set of bits; launches, fused_levels and
    launches_per_cycle as the thresholds say."""
    levels, b = _poisson64()
    prm = (1, 1, 4, 2.0 / 3.0)
    want = _want(("pcg", prm, 12), lambda: am.pcg(levels, prm, b, np.zeros(4096), 1e-8, 12))
    fused_at = {8: 1, 64: 1, 585: 3, 10 ** 6: 4}
    per_cycle = set()
    keep, handles = [], []
    try:
        ops = _operands(ctx, levels, PREPARED, keep, handles)
        for path in (0, 1, 2):
            for rows in (8, 64, 585, 10 ** 6):
                for every in (1, 3, 64):
                    for fuse in (0, 1):
                        what = "amg_path %d amg_fuse_rows %d pcg_check_every %d pcg_fuse %d" % (path, rows, every, fuse)
                        with Knobs(ctx, {"amg_path": path, "amg_fuse_rows": rows, "pcg_check_every": every, "pcg_fuse": fuse}):
                            got, st, ast = _solve(ctx, ops, prm, b, np.zeros(4096), 1e-8, 12, device=True)
                        _same(got, want, what)
                        assert ast.fused_levels == (0 if path == 1 else 4 if path == 2 else fused_at[rows]), what
                        outside = 10 if fuse else 7
                        assert st.launches == (outside + ast.launches_per_cycle) * _enqueued(st.readbacks, every, 12), what
                        if path == 2:
                            assert ast.launches_per_cycle == 1, what
                        per_cycle.add((int(ast.fused_levels), int(ast.launches_per_cycle)))
        # V(1,1), 4 coarse sweeps: 3 launches down and 2 up per level outside the tail; the tail is 1, an unfused last level 4
        assert per_cycle == {(0, 19), (1, 16), (3, 6), (4, 1)}, per_cycle
        for path in (1, 2):
            with Knobs(ctx, {"amg_path": path}):
                gx, _st = _apply(ctx, ops, prm, b, device=True)
            bits_same(gx, _want(("cycle", prm), lambda: am.cycle(levels, prm, b)), "cycle amg_path %d" % path)
    finally:
        _close(handles)


def test_workspace_does_not_depend_on_the_iteration_count(ctx):
    from spsparse_amd import capi
    levels, b = _poisson64()
    keep, handles = [], []
    try:
        ops = _operands(ctx, levels, PREPARED, keep, handles)
        used = []
        for max_iter in (2, 40):
            res = capi.Result()
            _got, st, _ = _solve(ctx, ops, (1, 1, 4, 2.0 / 3.0), b, np.zeros(4096), 0.0, max_iter, device=True, cap=3, result=res)
            assert st.iterations == max_iter
            used.append(int(res.workspace_bytes))
        assert used[0] == used[1] and used[0] > 0, used
    finally:
        _close(handles)


# ---------------------------------------------------------------- the edges of the kernels

def _random_levels(rng, orders, touch_all=False, arrow=(), long_r=()):
    """Level operators with a dominant diagonal and up to four random off-diagonal tuples a row, P with 0 to 3 tuples a row
    whose last coarse column no row touches (orders above 1), R random and of its own: nothing here is a Galerkin product.
    arrow: levels whose operator gets a full first row and column.  long_r: levels whose R gets a full first row."""
    levels = []
    for l, n in enumerate(orders):
        A = np.zeros((n, n)) if n <= 2100 else None
        i = np.repeat(np.arange(n), 4)
        j = rng.integers(0, max(n, 1), i.size)
        A[i, j] = 0.25 * rng.standard_normal(i.size)
        A[np.arange(n), np.arange(n)] = 2.0 + rng.random(n)
        if l in arrow:
            A[0, :] = 0.01 * rng.standard_normal(n)
            A[:, 0] = 0.01 * rng.standard_normal(n)
            A[0, 0] = 3.0
        ai, aj = np.nonzero(A)
        lv = {"n": n, "S": (ai.astype(np.int32), aj.astype(np.int32), A[ai, aj]), "P": None, "R": None}
        if l + 1 < len(orders):
            nc = orders[l + 1]
            hi = nc - 1 if nc > 1 and not touch_all else nc
            P, R = np.zeros((n, nc)), np.zeros((nc, n))
            if hi and n:
                for k in range(3):
                    on = rng.random(n) < 0.5
                    P[np.flatnonzero(on), rng.integers(0, hi, int(on.sum()))] = rng.standard_normal(int(on.sum()))
                ri = np.repeat(np.arange(nc), 3)
                R[ri, rng.integers(0, n, ri.size)] = rng.standard_normal(ri.size)
                if l in long_r:
                    R[0, :] = 0.01 * rng.standard_normal(n)
            pi, pj = np.nonzero(P)
            ri, rj = np.nonzero(R)
            lv["P"] = (pi.astype(np.int32), pj.astype(np.int32), P[pi, pj])
            lv["R"] = (ri.astype(np.int32), rj.astype(np.int32), R[ri, rj])
        levels.append(lv)
    return levels


def _long_rows(levels, knobs):
    """stats.long_rows as the header defines it: the rows above spmm_long_min of S, P and R on the levels outside the tail."""
    orders = [lv["n"] for lv in levels]
    path, rows = knobs.get("amg_path", 0), knobs.get("amg_fuse_rows", 1024)
    tail = 0 if path == 2 else len(orders)
    while path == 0 and tail > 0 and orders[tail - 1] <= rows:
        tail -= 1
    long_min, total = knobs.get("spmm_long_min", 64), 0
    for lv in levels[:tail]:
        for X in (lv["S"], lv["P"], lv["R"]):
            if X is not None and len(X[0]):
                total += int(np.count_nonzero(np.bincount(X[0]) > long_min))
    return total


def _check_all_paths(ctx, levels, what, settings, params=((2, 1, 2, 0.7), (0, 2, 1, 0.7)), min_long=0):
    rng = np.random.default_rng(len(what))
    n = levels[0]["n"]
    b = rng.standard_normal(n)
    for prm in params:
        want = am.cycle(levels, prm, b)
        wantp = am.pcg(levels, prm, b, np.zeros(n), 0.0, 3)
        for k, knobs in enumerate(settings):
            keep, handles = [], []
            try:
                ops = _operands(ctx, levels, (RAW, TRUSTED, PREPARED)[k % 3], keep, handles, r_is_pt=False)
                with Knobs(ctx, knobs):
                    gx, st = _apply(ctx, ops, prm, b, device=bool(k % 2))
                    got, _st, _ast = _solve(ctx, ops, prm, b, np.zeros(n), 0.0, 3, device=not k % 2)
                bits_same(gx, want, "%s %r %r" % (what, prm, knobs))
                _same(got, wantp, "%s pcg %r %r" % (what, prm, knobs))
                assert st.long_rows == _long_rows(levels, knobs), (what, knobs, st.long_rows, _long_rows(levels, knobs))
                if knobs.get("amg_path", 0) == 1:
                    assert st.long_rows >= min_long, (what, knobs, st.long_rows)
            finally:
                _close(handles)
    return st


PATHS = ({}, {"amg_path": 1}, {"amg_path": 2}, {"amg_fuse_rows": 64})


def test_level_orders_at_the_block_and_tail_edges(ctx):
    """Orders 2049, 1025, 1024, 1023, 65, 64, 63 and 1 in one hierarchy of random operators: the grid edges of the level
    kernels, the default tail threshold from both sides, a coarse column no row of P touches."""
    levels = _random_levels(np.random.default_rng(77), (2049, 1025, 1024, 1023, 65, 64, 63, 1))
    st = _check_all_paths(ctx, levels, "orders", PATHS)
    assert st.levels == 8 and st.fused_levels == 3                                   # (amg_fuse_rows 64: 64, 63, 1)


def test_an_inner_level_of_order_zero_and_a_single_level(ctx):
    levels = _random_levels(np.random.default_rng(5), (5, 0, 3))
    _check_all_paths(ctx, levels, "order 0 inside", PATHS, params=((1, 1, 2, 0.5), (0, 0, 1, 0.5)))
    b = np.array([1.0, -0.0, 3.0, -2.0, 0.5])
    want = am.cycle(levels, (1, 0, 2, -0.5), b)                                      # the correction is +0.0: added all the same
    keep = []
    gx, _ = _apply(ctx, _operands(ctx, levels, RAW, keep, []), (1, 0, 2, -0.5), b)
    bits_same(gx, want, "order 0 inside, a -0.0 from the sweep")
    for n in (1, 300):
        one = _random_levels(np.random.default_rng(n), (n,))
        _check_all_paths(ctx, one, "one level of order %d" % n, PATHS, params=((1, 1, 0, 0.5), (1, 1, 1, 0.5), (0, 0, 3, 0.5)))
    # a chained SINK_COO result as the level operator: read in place, and still there for the next call (no output set is written)
    from spsparse_amd import capi
    S, prm = one[0]["S"], (0, 0, 3, 0.5)
    A = capi.result_operand(ctx.consolidate(_coo(S, (300, 300), -1, keep=keep), 0, ar.ADD, False))
    b = np.random.default_rng(12).standard_normal(300)
    want, wantp = am.cycle(one, prm, b), am.pcg(one, prm, b, np.zeros(300), 0.0, 4)
    for k in range(2):
        gx, _ = _apply(ctx, [(A, '.', None, '.', None, '.')], prm, b, device=bool(k))
        bits_same(gx, want, "a chained level operator, call %d" % k)
        got, _st, _ast = _solve(ctx, [(A, '.', None, '.', None, '.')], prm, b, np.zeros(300), 0.0, 4, device=not k)
        _same(got, wantp, "a chained level operator, pcg, call %d" % k)


def test_long_rows_on_a_level_in_the_tail_and_in_r(ctx):
    """Rows above spmm_long_min (64): an arrow operator on level 0 outside the tail and on level 1 inside it, a full row of
    R; then spmm_long_min = 2, which sends most rows of A, P and R to the wave kernel."""
    rng = np.random.default_rng(91)
    levels = _random_levels(rng, (300, 100, 5), touch_all=True, arrow=(0, 1), long_r=(0,))
    _check_all_paths(ctx, levels, "arrow", ({"amg_fuse_rows": 128}, {"amg_path": 1}, {"amg_path": 2}, {"amg_fuse_rows": 4}),
                     min_long=3)
    _check_all_paths(ctx, levels, "spmm_long_min 2", ({"amg_path": 1, "spmm_long_min": 2}, {"amg_fuse_rows": 8, "spmm_long_min": 2}),
                     params=((2, 2, 2, 0.7), (0, 1, 1, 0.7)), min_long=100)


def test_special_values_break_down_with_the_reference_bits(ctx):
    """Six vertices, two levels: a NaN with a payload, an Inf, a stored zero diagonal (trusted, so it stays) and a missing
    diagonal.  Nothing is checked on the way: the loop stops with BREAKDOWN, every returned bit the reference's."""
    A = np.array([[4, -1, 0, 0, 0, -1], [-1, 4, -1, 0, 0, 0], [0, -1, 4, -1, 0, 0], [0, 0, -1, 4, -1, 0], [0, 0, 0, -1, 4, -1],
                  [-1, 0, 0, 0, -1, 4]], np.float64)
    i, j = np.nonzero(A)
    P = (np.arange(6, dtype=np.int32), np.array([0, 0, 0, 1, 1, 1], np.int32), np.ones(6))
    b = np.array([1.0, -2.0, 0.5, 3.0, -0.75, 0.125])
    nan = np.zeros(1)
    nan.view(np.uint64)[0] = 0x7FF80000DEADBEEF
    d2 = int(np.flatnonzero((i == 2) & (j == 2))[0])
    for what, at, val in (("NaN", 3, nan[0]), ("Inf", 3, np.inf), ("zero diagonal", d2, 0.0), ("missing diagonal", d2, None)):
        v = A[i, j].copy()
        keepm = np.ones(v.size, bool)
        if val is None:
            keepm[at] = False
        else:
            v[at] = val
        S = (i[keepm].astype(np.int32), j[keepm].astype(np.int32), v[keepm])
        Sc = (np.array([0, 0, 1, 1], np.int32), np.array([0, 1, 0, 1], np.int32), np.array([8.0, -2.0, -2.0, 8.0]))
        levels = [{"n": 6, "S": S, "P": P, "R": am.transposed(P)}, {"n": 2, "S": Sc, "P": None, "R": None}]
        prm = (1, 1, 2, 2.0 / 3.0)
        want = am.pcg(levels, prm, b, np.zeros(6), 1e-10, 20)
        assert want["reason"] == am.BREAKDOWN, what
        wantc = am.cycle(levels, prm, b)
        for knobs in PATHS[:3]:
            keep = []
            ops = _operands(ctx, levels, TRUSTED, keep, [])
            with Knobs(ctx, knobs):
                got, _st, _ast = _solve(ctx, ops, prm, b, np.zeros(6), 1e-10, 20)
                gx, _ = _apply(ctx, ops, prm, b)
            _same(got, want, "%s %r" % (what, knobs))
            bits_same(gx, wantc, "%s cycle %r" % (what, knobs))


# ---------------------------------------------------------------- the refusals

def test_refusals_leave_x_untouched(ctx):
    from spsparse_amd import capi
    levels = _random_levels(np.random.default_rng(3), (6, 2))
    keep = []
    A0, _, P0, _, R0, _ = _operands(ctx, levels, RAW, keep, [], r_is_pt=False)[0]
    A1 = _operands(ctx, levels, RAW, keep, [], r_is_pt=False)[1][0]
    b, x = np.arange(6, dtype=np.float64), np.full(6, SENT)
    L = ctx.L

    def table(rows):
        arr = (capi.AmgLevel * len(rows))()
        for k, (a, p, r) in enumerate(rows):
            arr[k] = capi.AmgLevel(None if a is None else C.pointer(a), b'.', None if p is None else C.pointer(p), b'.',
                                   None if r is None else C.pointer(r), b'.')
        return arr

    def shaped(X, s0, s1):
        Y = capi.Coo.from_buffer_copy(X)
        Y.shape0, Y.shape1 = s0, s1
        return Y

    good = table([(A0, P0, R0), (A1, None, None)])
    prm = capi.AmgParams(1, 1, 1, 0.5)

    def both(want, levels_=good, nlevels=2, params=prm, pb=b.ctypes.data, px=x.ctypes.data, mem=capi.MEM_HOST, pol=ar.ADD, what=""):
        pp = None if params is None else C.byref(params)
        rc = L.spsamd_amg_apply(ctx.h, levels_, nlevels, pp, pb, px, mem, pol, 0, None, None)
        assert rc == want, "amg_apply, %s: rc %d" % (what, rc)
        rc = L.spsamd_solve_pcg_amg(ctx.h, levels_, nlevels, pp, pb, px, mem, 1e-8, 5, None, 0, pol, 0, None, None, None)
        assert rc == want, "solve_pcg_amg, %s: rc %d" % (what, rc)
        assert L.spsamd_last_error(ctx.h), what
        assert np.all(x == SENT), "%s: x was written" % what

    EINVAL, EDIM = -2, -1
    both(EINVAL, levels_=None, what="levels NULL")
    both(EINVAL, params=None, what="params NULL")
    both(EINVAL, levels_=table([(None, P0, R0), (A1, None, None)]), what="A NULL")
    both(EINVAL, pb=None, what="b NULL")
    both(EINVAL, px=None, what="x NULL")
    both(EINVAL, nlevels=0, what="nlevels 0")
    both(EINVAL, levels_=table([(A0, P0, R0)] * 32 + [(A1, None, None)]), nlevels=33, what="nlevels 33")
    both(EINVAL, levels_=table([(A0, None, R0), (A1, None, None)]), what="P missing")
    both(EINVAL, levels_=table([(A0, P0, None), (A1, None, None)]), what="R missing")
    both(EINVAL, levels_=table([(A0, P0, R0), (A1, P0, None)]), what="P on the last level")
    both(EINVAL, levels_=table([(A0, P0, R0), (A1, None, R0)]), what="R on the last level")
    for om in (np.nan, np.inf, -np.inf):
        both(EINVAL, params=capi.AmgParams(1, 1, 1, om), what="omega %r" % om)
    both(EINVAL, mem=5, what="mem")
    both(EINVAL, pol=7, what="policy")
    both(EINVAL, px=b.ctypes.data, what="x is b")
    both(EINVAL, px=int(P0.val), what="x overlaps P's values")
    huge = capi.Coo.from_buffer_copy(A1)
    huge.nnz = 1 << 31
    both(EINVAL, levels_=table([(A0, P0, R0), (huge, None, None)]), what="2^31 tuples")
    oob = levels[0]["S"]
    bad = _coo((oob[0], np.where(np.arange(oob[1].size) == 2, 6, oob[1]), oob[2]), (6, 6), -1, keep=keep)
    both(EINVAL, levels_=table([(bad, P0, R0), (A1, None, None)]), what="an index out of bounds")
    both(EDIM, levels_=table([(shaped(A0, 6, 7), P0, R0), (A1, None, None)]), what="A not square")
    both(EDIM, levels_=table([(A0, shaped(P0, 6, 3), R0), (A1, None, None)]), what="P does not chain")
    both(EDIM, levels_=table([(A0, P0, shaped(R0, 2, 5)), (A1, None, None)]), what="R does not chain")
    both(EDIM, levels_=table([(A0, P0, R0), (shaped(A1, 3, 3), None, None)]), what="the next level has another order")
    rc = L.spsamd_solve_pcg_amg(ctx.h, good, 2, C.byref(prm), b.ctypes.data, x.ctypes.data, capi.MEM_HOST, -1.0, 5, None, 0, ar.ADD, 0,
                                None, None, None)
    assert rc == EINVAL and np.all(x == SENT), "negative tol"
    # n_0 == 0 returns as solve_pcg does
    empty = _coo((np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)), (0, 0), -1, keep=keep)
    st, hist = capi.PcgStats(), np.full(2, SENT)
    rc = L.spsamd_solve_pcg_amg(ctx.h, table([(empty, None, None)]), 1, C.byref(prm), None, None, capi.MEM_HOST, 1e-8, 5, hist.ctypes.data, 2,
                                ar.ADD, 0, C.byref(st), None, None)
    assert rc == 0 and (st.iterations, st.reason) == (0, capi.PCG_CONVERGED) and hist[0] == 0.0 and hist[1] == SENT
    assert L.spsamd_amg_apply(ctx.h, table([(empty, None, None)]), 1, C.byref(prm), None, None, capi.MEM_HOST, ar.ADD, 0, None, None) == 0


def test_hierarchy_helper_builds_what_the_reference_builds(ctx):
    """capi.Hierarchy on Poisson 64^2 (device aggregation, two multiplies a level, prepared operands): the orders of
    amg_ref.hierarchy, whose aggregates are the same loop, and the same bits from the solve."""
    import torch
    from spsparse_amd import capi
    levels, b = _poisson64()
    S = levels[0]["S"]
    keep = []
    A = _coo(S, (4096, 4096), 0, device=True, keep=keep)
    h = capi.Hierarchy(ctx, A, flags=capi.AGG_SYMMETRIC, min_coarse=10)
    try:
        assert h.rows == [4096, 585, 65, 8] and h.nnz == [len(lv["S"][2]) for lv in levels]
        prm = (1, 1, 4, 2.0 / 3.0)
        tb = torch.from_numpy(b.copy()).cuda()
        x, hist, st, ast = ctx.solve_pcg_amg(h, prm, tb, None, 1e-8, 200)
        want = _want(("pcg", prm, 200), lambda: am.pcg(levels, prm, b, np.zeros(4096), 1e-8, 200))
        got = {"x": x.cpu().numpy(), "hist": hist, "iterations": int(st.iterations), "reason": int(st.reason),
               "bb": np.float64(st.bb), "rr0": np.float64(st.rr0), "rr": np.float64(st.rr)}
        _same(got, want, "Hierarchy")
    finally:
        h.close()
