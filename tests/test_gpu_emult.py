"""spsamd_emult on the device against tests/emult_ref.py (pinned on the host by tests/test_emult_host.py): indices equal and
values as int64 bit patterns, zero tolerance.  Every case runs under emult_path 0 (auto), 1 (merge), 2 (probe A in B) and 3
(probe B in A); the forced probes must report the tuples they searched in `products`, the merge must report 0.
The one exception to bit equality is the DIGEST sink's value sums (`sum`, ROWSTATS `row_sum`): the shared sink tail adds them
with floating-point atomics in no fixed order, so they are compared with the rounding bound of such a sum, n * 2^-53 * sum|v|
(test_sinks); the digest's nnz, hash and row_nnz, and every tuple, are compared exactly."""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as orc
from spsparse_amd import workloads as wl
from tests import add_ref as ar
from tests import emult_ref as er
from tests import select_ref as sr
from tests.gpu_util import check_tuples as _check, coo as _coo, ctx, device_operand, forced  # noqa: F401

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2, 3)
FORMS = ((er.TIMES, False), (er.FIRST, False), (er.FIRST, True))


def _emult(ctx, op, a, b, path=0, **kw):
    with forced(ctx, "emult_path", path):
        return ctx.emult(op, a, b, **kw)


def _all_paths(ctx, op, comp, a, b, want, what, alpha=1.0, **kw):
    """The call under every path against `want`; returns the last result."""
    res = None
    for path in PATHS:
        res = _emult(ctx, op, a, b, path, alpha=alpha, complement=comp, **kw)
        _check(ctx.fetch(res), want, "%s path %d" % (what, path))
        assert res.nnz == len(want[2]), what
        if res.nnz_a and res.nnz_b:
            assert (res.products == 0) if path == 1 else (res.products > 0) if path else True, "%s path %d products %d" % (what, path, res.products)
    return res


def _stored(r, c, t):
    """op()-oriented keys as the stored index arrays of an operand used with transpose t."""
    return (c, r) if t == 'T' else (r, c)


def _partner(rng, SA, opshape, tB, n_from_a, n_other, kind):
    """A stored operand B whose op(B) shares n_from_a keys with S_A and has n_other random ones; kind 0: unique keys,
    special values anywhere; 1: duplicate keys (NaN / Inf on keys that occur once only)."""
    ra, ca = np.asarray(SA[0], np.int64), np.asarray(SA[1], np.int64)
    pick = rng.choice(len(ra), min(n_from_a, len(ra)), replace=False) if len(ra) else np.zeros(0, np.int64)
    r = np.concatenate([ra[pick], rng.integers(0, opshape[0], n_other)])
    c = np.concatenate([ca[pick], rng.integers(0, opshape[1], n_other)])
    if kind == 0:
        _, first = np.unique((r << 32) | c, return_index=True)
        first = rng.permutation(first)
        r, c = r[first], c[first]
        v = sr.special_values(rng, len(r), 0.3)
    else:
        o = rng.permutation(len(r))
        r, c = r[o], c[o]
        v = sr.special_values(rng, len(r), 0.3)
        _, inv, cnt = np.unique((r << 32) | c, return_inverse=True, return_counts=True)
        bad = (cnt[inv] > 1) & ~np.isfinite(v)
        v[bad] = rng.standard_normal(int(bad.sum()))
    i0, i1 = _stored(r.astype(np.int32), c.astype(np.int32), tB)
    return i0, i1, v


def test_semantic_sweep(ctx):
    """Raw (unique keys with NaN / Inf / +-0; duplicate keys) and trusted (sorted by the full key: duplicates and special
    values anywhere) operands on either side, host and device, both transposes on either side, the three policies, zero_nan,
    alpha 1 / 0 / -0.75 / Inf, B->val NULL under FIRST, every path."""
    rng = np.random.default_rng(171)
    for trial in range(72):
        big = trial % 6 == 0
        opshape = (int(rng.integers(1, 300 if big else 40)), int(rng.integers(1, 300 if big else 40)))
        tA, tB = ('.', 'T')[trial % 2], ('.', 'T')[(trial // 2) % 2]
        la, lb = int(tA == 'T'), int(tB == 'T')
        shA, shB = (opshape[::-1] if la else opshape), (opshape[::-1] if lb else opshape)
        pol, zn = trial % 3, trial % 5 == 0
        nnz = int(rng.integers(0, 4000 if big else 300))
        kindA, kindB = trial % 3, (trial // 3) % 3
        A = sr.unique_key_operand(rng, shA, nnz) if kindA == 0 else sr.duplicate_key_operand(rng, shA, nnz)
        sortA = sortB = -1
        if kindA == 2:
            A, sortA = ar.sort_storage(A, la), la
        SA = sr.operand_S(A, tA, pol, zn, sortA)
        B = _partner(rng, SA, opshape, tB, int(rng.integers(0, nnz + 1)), int(rng.integers(0, 200)), min(kindB, 1))
        if kindB == 2:
            B, sortB = ar.sort_storage(B, lb), lb
        keep = []
        a = _coo(A, shA, sortA, device=trial % 2 == 1, keep=keep)
        alpha = (1.0, 0.0, -0.75, np.inf)[trial % 4]
        for op, comp in FORMS:
            b = _coo(B, shB, sortB, device=trial % 4 < 2, keep=keep, no_val=op == er.FIRST and trial % 2 == 0)
            S = er.operands(A, B, op, tA, tB, pol, zn, sortA, sortB)
            want = er.emult_ref(S[0], S[1], op, alpha, comp)
            what = "trial %d op %d comp %d %s%s pol %d zn %d kinds %d %d" % (trial, op, comp, tA, tB, pol, zn, kindA, kindB)
            res = _all_paths(ctx, op, comp, a, b, want, what, alpha=alpha, tA=tA, tB=tB, duplicate_policy=pol, zero_nan=zn)
            assert (res.shape0, res.shape1) == opshape, what
            assert res.nnz_a == len(S[0][2]), what
            assert res.nnz_b == (len(S[1][0]) if op == er.TIMES else len(np.unique(er.keys(S[1][0], S[1][1])))), what


def test_prepared_operands_both_transposes(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(172)
    shape = (35, 25)
    X = ar.random_operand(rng, shape, 700, special=0.0)
    Y = ar.random_operand(rng, shape, 700, special=0.0)
    keep = []
    for tprep in ('.', 'T'):
        lead = int(tprep == 'T')
        hx = capi.Operand(ctx, _coo(X, shape, -1, False, keep), tprep, capi.AS_A, capi.ADD, False)
        hy = capi.Operand(ctx, _coo(Y, shape, -1, True, keep), tprep, capi.AS_A, capi.ADD, False)
        try:
            PX = orc.consolidate(X[0], X[1], X[2], lead, ar.ADD, False)
            PY = orc.consolidate(Y[0], Y[1], Y[2], lead, ar.ADD, False)
            for t in ('.', 'T'):
                for op, comp in FORMS:
                    S = er.operands(PX, PY, op, t, t, sortA=lead, sortB=lead) if t == tprep else er.operands(PX, PY, op, t, t)
                    want = er.emult_ref(S[0], S[1], op, 2.5, comp)
                    _all_paths(ctx, op, comp, hx.coo, hy.coo, want, "handles %s used %s op %d comp %d" % (tprep, t, op, comp), alpha=2.5, tA=t, tB=t)
                    # a handle on one side only, the other a raw host operand
                    S = er.operands(X, PY, op, t, t, sortB=lead) if t == tprep else er.operands(X, PY, op, t, t)
                    _all_paths(ctx, op, comp, _coo(X, shape, -1, False, keep), hy.coo, er.emult_ref(S[0], S[1], op, 1.0, comp),
                               "raw with handle %s used %s op %d comp %d" % (tprep, t, op, comp), tA=t, tB=t)
        finally:
            hx.close(); hy.close()


def test_chained_results_plain_and_permuted(ctx):
    """A SINK_COO result as either operand, read in place: sort0 = 0, and sort0 = 1 after SINK_PERMUTE."""
    from spsparse_amd import capi
    rng = np.random.default_rng(173)
    shape = (40, 30)
    X = sr.unique_key_operand(rng, shape, 600)
    Y = sr.unique_key_operand(rng, shape, 500)
    keep = []
    y = _coo(Y, shape, -1, True, keep)
    SX = sr.operand_S(X)
    for op, comp in FORMS:
        for side in (0, 1):
            r = ctx.select(_coo(X, shape, -1, False, keep), sr.TRIU, iparam=-10 ** 6)          # keeps everything
            x = capi.result_operand(r)
            a, b, A, B, sA, sB = (x, y, SX, Y, 0, -1) if side == 0 else (y, x, Y, SX, -1, 0)
            S = er.operands(A, B, op, sortA=sA, sortB=sB)
            _all_paths(ctx, op, comp, a, b, er.emult_ref(S[0], S[1], op, -2.0, comp), "chained side %d op %d comp %d" % (side, op, comp), alpha=-2.0)
            # permuted: the same tuples of X^T's select, handed back as the column-major operand they are
            r = ctx.select(_coo(X, shape, -1, False, keep), sr.TRIU, iparam=-10 ** 6, transpose='T', flags=capi.SINK_PERMUTE)
            assert (r.shape0, r.shape1) == shape
            p = capi.Coo(r.idx0, r.idx1, r.val, int(r.nnz), shape[0], shape[1], 1, capi.MEM_DEVICE)
            a, b = (p, y) if side == 0 else (y, p)
            tA, tB = ('T', 'T')
            XT = sr.operand_S(X, 'T')                                        # what p holds, in op()'s orientation
            PX = (XT[1], XT[0], XT[2])                                       # ... and as p stores it: sorted by idx1
            S = er.operands(PX, Y, op, 'T', 'T', sortA=1) if side == 0 else er.operands(Y, PX, op, 'T', 'T', sortB=1)
            _all_paths(ctx, op, comp, a, b, er.emult_ref(S[0], S[1], op, 1.0, comp), "permuted side %d op %d comp %d" % (side, op, comp), tA=tA, tB=tB)


def test_sinks(ctx):
    import torch
    from spsparse_amd import capi
    from tests import projection as pj
    rng = np.random.default_rng(174)
    shape = (300, 200)
    A = ar.random_operand(rng, shape, 20_000, special=0.0)
    B = ar.random_operand(rng, shape, 20_000, special=0.0)
    keep = []
    a, b = _coo(A, shape, -1, True, keep), _coo(B, shape, -1, True, keep)
    for op, comp in FORMS:
        S = er.operands(A, B, op)
        wi, wj, wv = er.emult_ref(S[0], S[1], op, 1.5, comp)
        for path in PATHS:
            d = _emult(ctx, op, a, b, path, alpha=1.5, complement=comp, sink=capi.SINK_DIGEST, flags=capi.SINK_ROWSTATS)
            assert d.nnz == len(wv) and d.nnz_a == len(S[0][2])
            assert np.array_equal(ctx.to_host(d.row_nnz, shape[0], np.int64), np.bincount(wi, minlength=shape[0]))
            rs, ra = np.zeros(shape[0]), np.zeros(shape[0])
            np.add.at(rs, wi, wv); np.add.at(ra, wi, np.abs(wv))
            # sums in any order: |error| <= (n - 1) u sum|v| for each of the two sums compared, u = 2^-53
            u = 2.0 ** -53
            cnt = np.bincount(wi, minlength=shape[0])
            assert np.all(np.abs(ctx.to_host(d.row_sum, shape[0], np.float64) - rs) <= 2 * cnt * u * ra)
            assert abs(d.sum - wv.sum()) <= 2 * len(wv) * u * np.abs(wv).sum()
            mix = pj.mix64_t(torch.from_numpy(wi.astype(np.int64)), torch.from_numpy(wj.astype(np.int64)))
            assert d.hash == int(mix.sum().item()) & (2 ** 64 - 1)
            d2 = _emult(ctx, op, a, b, path, alpha=1.5, complement=comp, sink=capi.SINK_DIGEST)
            assert (d2.nnz, d2.hash) == (d.nnz, d.hash) and not d2.row_nnz
        for flags in (capi.SINK_ORDERED, capi.SINK_EXACT_PATTERN):          # accepted, change nothing
            _check(ctx.fetch(ctx.emult(op, a, b, alpha=1.5, complement=comp, flags=flags)), (wi, wj, wv), "flags %d" % flags)
    # scatter_dense of a restriction
    res = ctx.emult(er.FIRST, a, b)
    dense = torch.zeros(shape, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.scatter_dense(res, dense.data_ptr(), shape[1])
    S = er.operands(A, B, er.FIRST)
    wi, wj, wv = er.emult_ref(S[0], S[1], er.FIRST)
    want = np.zeros(shape); want[wi, wj] = wv
    assert np.array_equal(dense.cpu().numpy(), want)


def _sorted_keys(flat, ncol):
    flat = np.sort(np.asarray(flat, np.int64))
    return (flat // ncol).astype(np.int32), (flat % ncol).astype(np.int32)


def _forms_on(ctx, A, B, shape, what, sortA=0, sortB=0, device=True, alpha=-1.25):
    keep = []
    a, b = _coo(A, shape, sortA, device, keep), _coo(B, shape, sortB, device, keep)
    for op, comp in FORMS:
        S = er.operands(A, B, op, sortA=sortA, sortB=sortB)
        _all_paths(ctx, op, comp, a, b, er.emult_ref(S[0], S[1], op, alpha, comp), "%s op %d comp %d" % (what, op, comp), alpha=alpha)


def test_merge_tile_edges(ctx):
    """nnz(A) + nnz(B) around the lane's 8 items and the tile's 2048; all keys equal, disjoint, A wholly before and after B."""
    from spsparse_amd import capi
    T = capi.emult_tile
    rng = np.random.default_rng(175)
    ncol = 1 << 12
    shape = (64, ncol)
    for total in (1, 7, 8, 9, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 1):
        for na in sorted({0, 1, total // 2, total - 1, total} & set(range(total + 1))):
            nb = total - na
            pool = rng.choice(shape[0] * ncol, total, replace=False)
            shared = min(na, nb) // 2                                        # keys of both; the rest of B's are its own
            ka, kb = pool[:na], np.concatenate([pool[:shared], pool[na + shared:]])
            assert len(kb) == nb
            A = (*_sorted_keys(ka, ncol), rng.standard_normal(na))
            B = (*_sorted_keys(kb, ncol), rng.standard_normal(len(kb)))
            _forms_on(ctx, A, B, shape, "total %d na %d" % (total, na))
    n = T + T // 2 + 3
    k = rng.choice(shape[0] * ncol, 2 * n, replace=False)
    same = (*_sorted_keys(k[:n], ncol), rng.standard_normal(n))
    _forms_on(ctx, same, (same[0], same[1], rng.standard_normal(n)), shape, "all keys equal")
    _forms_on(ctx, same, (*_sorted_keys(k[n:], ncol), rng.standard_normal(n)), shape, "disjoint keys")
    ks = np.sort(k)
    lowk, highk = (*_sorted_keys(ks[:n], ncol), rng.standard_normal(n)), (*_sorted_keys(ks[n:], ncol), rng.standard_normal(n))
    _forms_on(ctx, lowk, highk, shape, "A before B")
    _forms_on(ctx, highk, lowk, shape, "A after B")


def test_run_of_equal_keys_across_tiles(ctx):
    """A trusted A with a run of 5000 equal keys (it crosses two tile boundaries of the merge); B holds that key three times
    among smaller and larger keys, so the partner lies in the run's last tile or behind it, and every tuple of the run must
    name B's FIRST tuple of the key.  `before` moves the run, and B's partner, across the tiles."""
    rng = np.random.default_rng(176)
    shape = (50, 1000)
    for before_a, before_b in ((0, 0), (300, 1500), (1900, 100), (10, 4000)):
        ra = np.concatenate([np.full(before_a, 3), np.full(5000, 7), np.full(40, 9)]).astype(np.int32)
        ca = np.concatenate([np.sort(rng.integers(0, 1000, before_a)), np.full(5000, 11), np.sort(rng.integers(0, 1000, 40))]).astype(np.int32)
        rb = np.concatenate([np.full(before_b, 2), np.full(3, 7), np.full(25, 9)]).astype(np.int32)
        cb = np.concatenate([np.sort(rng.integers(0, 1000, before_b)), np.full(3, 11), np.sort(rng.integers(0, 1000, 25))]).astype(np.int32)
        A = (ra, ca, rng.standard_normal(len(ra)))
        B = (rb, cb, rng.standard_normal(len(rb)))
        _forms_on(ctx, A, B, shape, "run before %d %d" % (before_a, before_b))
        # and the run in B's place: A holds the key twice, B 5000 times (first-of-key across B's tiles)
        _forms_on(ctx, B, A, shape, "run in B before %d %d" % (before_a, before_b))


def test_key_width(ctx):
    """Shape (2^31 - 1)^2: the corners, and indices that differ in bit 30 only -- a compare on fewer than 64 bits, or on
    row * ncol + col in 32 bits, would call them equal."""
    N = 2 ** 31 - 1
    h = 1 << 30
    ka = [(0, 0), (0, N - 1), (5, 7), (5, 7 + h), (5 + h, 7 + h), (N - 1, 0), (N - 1, N - 1)]
    kb = [(0, 0), (0, N - 2), (5, 7 + h), (5 + h, 7), (5 + h, 7 + h), (N - 1, 1), (N - 1, N - 1)]
    rng = np.random.default_rng(177)
    A = (np.array([k[0] for k in ka], np.int32), np.array([k[1] for k in ka], np.int32), rng.standard_normal(len(ka)))
    B = (np.array([k[0] for k in kb], np.int32), np.array([k[1] for k in kb], np.int32), rng.standard_normal(len(kb)))
    for device in (False, True):
        _forms_on(ctx, A, B, (N, N), "key width device %d" % device, device=device)
    o = rng.permutation(len(ka))                                             # raw: through the consolidation and mask_keys' sort
    _forms_on(ctx, tuple(x[o] for x in A), tuple(x[o] for x in B), (N, N), "key width raw", sortA=-1, sortB=-1)


_PROBE = {}


def _probe_case():
    """A table with rows of exactly 0, 1, 2, 63, 64, 65, 4096, 4097, 0 and 3 tuples, and probe keys before the first column
    of a row, at the first, at the last, after the last, between neighbours, at hits in the middle, in the empty rows and in
    the last row."""
    if not _PROBE:
        rng = np.random.default_rng(178)
        lengths = [0, 1, 2, 63, 64, 65, 4096, 4097, 0, 3]
        ncol = 20_000
        table = sr.rows_of_lengths(rng, lengths, ncol, special=0.0)
        pr, pc = [], []
        for r, n in enumerate(lengths):
            c = table[1][table[0] == r].astype(np.int64)
            if n == 0:
                cand = [0, 5, ncol - 1]
            else:
                mid = c[rng.integers(0, n, min(n, 40))]
                cand = [c[0] - 1, c[0], c[-1], c[-1] + 1, 0, ncol - 1, *mid, *(mid + 1), *(mid - 1)]
            cand = np.unique([x for x in cand if 0 <= x < ncol])
            pr.append(np.full(len(cand), r, np.int32)); pc.append(cand.astype(np.int32))
        pr, pc = np.concatenate(pr), np.concatenate(pc)
        _PROBE["table"], _PROBE["probes"] = table, (pr, pc, rng.standard_normal(len(pr)))
        _PROBE["shape"] = (len(lengths), ncol)
    return _PROBE["table"], _PROBE["probes"], _PROBE["shape"]


def test_probe_edges(ctx):
    from spsparse_amd import capi
    table, probes, shape = _probe_case()
    keep = []
    p = _coo(probes, shape, 0, True, keep)
    h = capi.Operand(ctx, _coo(table, shape, 0, True, keep), '.', capi.AS_A, capi.ADD, False)
    try:
        for op, comp in FORMS:
            # the table on B's side: a handle (search inside the row), then a chained result (search over the whole stream)
            S = er.operands(probes, table, op, sortA=0, sortB=0)
            want = er.emult_ref(S[0], S[1], op, 3.0, comp)
            _all_paths(ctx, op, comp, p, h.coo, want, "table handle as B op %d comp %d" % (op, comp), alpha=3.0)
            r = ctx.select(_coo(table, shape, 0, True, keep), sr.TRIU, iparam=-10 ** 6)
            assert r.nnz == len(table[2])
            _all_paths(ctx, op, comp, p, capi.result_operand(r), want, "table chained as B op %d comp %d" % (op, comp), alpha=3.0)
            # the table on A's side (path 3 searches it)
            S = er.operands(table, probes, op, sortA=0, sortB=0)
            want = er.emult_ref(S[0], S[1], op, 3.0, comp)
            _all_paths(ctx, op, comp, h.coo, p, want, "table handle as A op %d comp %d" % (op, comp), alpha=3.0)
            r = ctx.select(_coo(table, shape, 0, True, keep), sr.TRIU, iparam=-10 ** 6)
            _all_paths(ctx, op, comp, capi.result_operand(r), p, want, "table chained as A op %d comp %d" % (op, comp), alpha=3.0)
    finally:
        h.close()
    # a trusted A with runs of 1, 2 and 70 equal keys, probed by B's keys at, before and after the runs
    rng = np.random.default_rng(179)
    ra = np.concatenate([np.full(1, 2), np.full(2, 2), np.full(70, 4), np.full(1, 4), np.full(70, 9)]).astype(np.int32)
    ca = np.concatenate([[5], [8, 8], np.full(70, 100), [101], np.full(70, 19_999)]).astype(np.int32)
    A = (ra, ca, rng.standard_normal(len(ra)))
    B = (np.array([2, 2, 2, 4, 4, 4, 4, 9, 9], np.int32), np.array([5, 7, 8, 99, 100, 100, 102, 0, 19_999], np.int32), rng.standard_normal(9))
    _forms_on(ctx, A, B, shape, "runs of 1, 2, 70")


def test_lopsided_sizes(ctx):
    """nnz(B) = 64 against nnz(A) = 200 000 and the reverse, every path; path 3 without COMPLEMENT makes no array of nnz(A)
    entries: its workspace stays below 4 * nnz(A) bytes (A: a device operand in row order, no sort is charged)."""
    rng = np.random.default_rng(180)
    n, ncol = 200_000, 2000
    shape = (2000, ncol)
    ka = rng.choice(shape[0] * ncol, n, replace=False)
    kb = np.unique(np.concatenate([rng.choice(ka, 40, replace=False), rng.choice(shape[0] * ncol, 24, replace=False)]))[:64]
    big = (*_sorted_keys(ka, ncol), rng.standard_normal(n))
    small = (*_sorted_keys(kb, ncol), rng.standard_normal(len(kb)))
    keep = []
    a, b = _coo(big, shape, 0, True, keep), _coo(small, shape, 0, True, keep)
    for op, comp in FORMS:
        S = er.operands(big, small, op, sortA=0, sortB=0)
        want = er.emult_ref(S[0], S[1], op, 0.5, comp)
        _all_paths(ctx, op, comp, a, b, want, "small B op %d comp %d" % (op, comp), alpha=0.5)
        if not comp:
            res = _emult(ctx, op, a, b, 3, alpha=0.5)
            assert res.nnz == len(want[2]) >= 40 and res.workspace_bytes < 4 * n, res.workspace_bytes
        S = er.operands(small, big, op, sortA=0, sortB=0)
        _all_paths(ctx, op, comp, b, a, er.emult_ref(S[0], S[1], op, 0.5, comp), "small A op %d comp %d" % (op, comp), alpha=0.5)


def test_cross_checks_against_other_operations(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(181)
    n = 120
    A = ar.consolidate(*sr.unique_key_operand(rng, (n, n), 3000, special=0.0))       # consolidated, zero-free
    B = sr.unique_key_operand(rng, (n, n), 2500)
    eye = (np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    keep = []
    a, b, e = _coo(A, (n, n), 0, True, keep), _coo(B, (n, n), -1, True, keep), _coo(eye, (n, n), 0, True, keep)
    masked = ctx.fetch(ctx.multiply_masked(a, e, b))
    assert len(masked[2]) > 0
    for path in PATHS:
        _check(ctx.fetch(_emult(ctx, er.FIRST, a, b, path)), masked, "FIRST(A, B) vs multiply_masked(A, I, B) path %d" % path)
    # restriction to a selection's pattern is the selection; off it, the selection's complement
    Xr = sr.duplicate_key_operand(rng, (n, n), 4000)
    x = _coo(Xr, (n, n), -1, True, keep)
    tril = ctx.fetch(ctx.select(x, sr.TRIL, iparam=0))
    rest = ctx.fetch(ctx.select(x, sr.TRIL, iparam=0, complement=True))
    for path in PATHS:
        lo = ctx.select(x, sr.TRIL, iparam=0)
        _check(ctx.fetch(_emult(ctx, er.FIRST, x, capi.result_operand(lo), path)), tril, "FIRST(A, tril(A)) path %d" % path)
        lo = ctx.select(x, sr.TRIL, iparam=0)
        _check(ctx.fetch(_emult(ctx, er.FIRST, x, capi.result_operand(lo), path, complement=True)), rest, "A off tril(A) path %d" % path)


def test_chain(ctx):
    """T = A*A, then FIRST(T, A) reads T in place from the output set; the result feeds spsamd_reduce and spsamd_select; with
    both output sets holding operands the call is refused."""
    from spsparse_amd import capi
    i0, i1, v, shape = wl.rmat(10, seed=5)
    keep = []
    a = _coo((i0, i1, v), shape, -1, True, keep)
    for path in PATHS:
        t = ctx.multiply(a, a, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)
        T = ctx.fetch(t)
        S = er.operands(T, (i0, i1, v), er.FIRST, sortA=0)
        for comp in (False, True):
            want = er.emult_ref(S[0], S[1], er.FIRST, complement=comp)
            r = _emult(ctx, er.FIRST, capi.result_operand(t), a, path, complement=comp)
            assert r.nnz_a == t.nnz and r.idx0 != t.idx0
            _check(ctx.fetch(r), want, "FIRST(A*A, A) comp %d path %d" % (comp, path))
            assert len(want[2]) > 0
            idx, val = ctx.reduce(capi.result_operand(r), capi.REDUCE_COUNT)
            assert np.array_equal(idx, np.unique(want[0])) and np.array_equal(val, np.bincount(want[0])[np.unique(want[0])])
            s = ctx.select(capi.result_operand(r), sr.DIAG, iparam=0)
            _check(ctx.fetch(s), sr.select_ref(want, shape[0], sr.DIAG, 0), "select of the restriction")
            t = ctx.multiply(a, a, sink=capi.SINK_COO, flags=capi.SINK_ORDERED)       # (the select took T's set)
    r1 = ctx.multiply(a, a, sink=capi.SINK_COO)
    r2 = ctx.select(capi.result_operand(r1), sr.TRIL, iparam=0)
    with pytest.raises(capi.SpsamdError) as e:
        ctx.emult(er.TIMES, capi.result_operand(r1), capi.result_operand(r2))
    assert e.value.code == -2 and "result buffers" in e.value.msg
    d = ctx.emult(er.TIMES, capi.result_operand(r1), capi.result_operand(r2), sink=capi.SINK_DIGEST)     # no output set is written
    assert d.nnz == r2.nnz


def test_a_times_a_and_strength_of_connection(ctx):
    """A o A with the same struct on both sides, and A o A^T of R-MAT scale 12 written by the device generator."""
    scale = 12
    ne, n = 16 << scale, 1 << scale
    a, t = device_operand(ctx, lambda p0, p1, pv: ctx.gen_rmat(scale, 9, 0, ne, p0, p1, pv), ne, (n, n))
    i0, i1, v = (x.cpu().numpy() for x in t)
    SA = orc.consolidate(i0, i1, v, 0, ar.ADD, False)
    ST = orc.consolidate(i1, i0, v, 0, ar.ADD, False)
    for path in PATHS:
        res = _emult(ctx, er.TIMES, a, a, path, alpha=2.0)
        _check(ctx.fetch(res), er.emult_ref(SA, SA, er.TIMES, 2.0), "A o A path %d" % path)
        res = _emult(ctx, er.TIMES, a, a, path, tB='T')
        want = er.emult_ref(SA, ST, er.TIMES)
        _check(ctx.fetch(res), want, "A o A^T path %d" % path)
        assert 0 < len(want[2]) < len(SA[2])
        for comp in (False, True):
            res = _emult(ctx, er.FIRST, a, a, path, tB='T', complement=comp)
            _check(ctx.fetch(res), er.emult_ref(SA, (ST[0], ST[1], None), er.FIRST, complement=comp), "A on A^T comp %d path %d" % (comp, path))


def _raw(ctx, A, B, res, op=1, fl=0, tA=b'.', tB=b'.', pol=1, zn=0, sink=1, flags=0):
    return ctx.L.spsamd_emult(ctx.h, op, fl, 1.0, None if A is None else C.byref(A), tA, None if B is None else C.byref(B), tB,
                              pol, zn, sink, flags, None if res is None else C.byref(res))


def test_errors_leave_the_context_usable(ctx):
    from spsparse_amd import capi
    rng = np.random.default_rng(182)
    A = sr.unique_key_operand(rng, (6, 8), 30)
    B = sr.unique_key_operand(rng, (6, 8), 30)
    keep = []
    a, b = _coo(A, (6, 8), -1, False, keep), _coo(B, (6, 8), -1, False, keep)
    res = capi.Result()
    held = {}

    def hold():
        held["res"] = ctx.emult(er.TIMES, a, b)
        held["tuples"] = ctx.fetch(held["res"])

    def refused(rc, code=-2):
        assert rc == code and len(ctx.L.spsamd_last_error(ctx.h)) > 0
        _check(ctx.fetch(held["res"]), held["tuples"], "an earlier result after a refused call")

    hold()

    refused(_raw(ctx, None, b, res)); refused(_raw(ctx, a, None, res)); refused(_raw(ctx, a, b, None))
    refused(_raw(ctx, a, b, res, op=0)); refused(_raw(ctx, a, b, res, op=3))
    refused(_raw(ctx, a, b, res, op=2, fl=2)); refused(_raw(ctx, a, b, res, op=1, fl=1))
    refused(_raw(ctx, a, b, res, pol=3)); refused(_raw(ctx, a, b, res, pol=-1))
    refused(_raw(ctx, a, b, res, sink=3)); refused(_raw(ctx, a, b, res, sink=0))
    refused(_raw(ctx, a, b, res, tB=b'T'), -1)                                    # 6 x 8 against 8 x 6
    refused(_raw(ctx, a, _coo(B, (6, 9), -1, False, keep), res), -1)
    for device in (False, True):
        for op in (1, 2):
            bad = (B[0].copy(), B[1].copy(), B[2])
            bad[1][5] = 8
            refused(_raw(ctx, a, _coo(bad, (6, 8), -1, device, keep), res, op=op))
            refused(_raw(ctx, _coo(bad, (6, 8), -1, device, keep), b, res, op=op))
            bad[1][5] = -1
            refused(_raw(ctx, a, _coo(bad, (6, 8), 0 if device else -1, device, keep), res, op=op))
        # a trusted operand whose full key descends (its rows ascend): either side
        lie = ar.sort_storage(A, 0)
        lie = (lie[0], lie[1][::-1].copy(), lie[2])
        assert np.all(np.diff(lie[0]) >= 0) and np.any(np.diff(er.keys(lie[0], lie[1])) < 0)
        for op in (1, 2):
            refused(_raw(ctx, _coo(lie, (6, 8), 0, device, keep), b, res, op=op))
            refused(_raw(ctx, a, _coo(lie, (6, 8), 0, device, keep), res, op=op))
    huge = capi.Coo(a.idx0, a.idx1, a.val, 2 ** 31, 6, 8, -1, capi.MEM_HOST)
    refused(_raw(ctx, huge, b, res)); refused(_raw(ctx, a, huge, res)); refused(_raw(ctx, a, huge, res, op=2))
    refused(_raw(ctx, a, _coo(B, (6, 8), -1, False, keep, no_val=True), res, op=1))          # TIMES reads B's values
    refused(_raw(ctx, _coo(A, (6, 8), -1, False, keep, no_val=True), b, res, op=2))
    assert _raw(ctx, a, _coo(B, (6, 8), -1, False, keep, no_val=True), res, op=2) == 0       # FIRST does not
    hold()
    # the knob: an unknown value is refused by the call, and 0 brings the call back
    with forced(ctx, "emult_path", 4):
        refused(_raw(ctx, a, b, res))
    with pytest.raises(capi.SpsamdError):
        ctx.set_tuning("emult_pth", 1)
    # empty operands
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    e = _coo(E, (6, 8), -1, False, keep)
    SA = sr.operand_S(A)
    for path in PATHS:
        for op, comp in FORMS:
            r = _emult(ctx, op, e, b, path, complement=comp)
            assert r.nnz == 0 and (r.shape0, r.shape1) == (6, 8)
            r = _emult(ctx, op, a, e, path, complement=comp)
            assert r.nnz == (len(SA[2]) if comp else 0) and r.nnz_a == len(SA[2])
            if comp:
                _check(ctx.fetch(r), SA, "A off an empty B")
    # an empty A does not excuse a bad B
    hold()
    bad = (B[0].copy(), B[1].copy(), B[2])
    bad[1][5] = 8
    for op in (1, 2):
        refused(_raw(ctx, e, _coo(bad, (6, 8), -1, False, keep), res, op=op))
        refused(_raw(ctx, e, _coo(lie, (6, 8), 0, True, keep), res, op=op))
    refused(_raw(ctx, e, _coo(B, (6, 8), -1, False, keep, no_val=True), res, op=1))
    r = ctx.emult(er.TIMES, e, _coo(E, (8, 6), -1, False, keep), tB='T', flags=capi.SINK_PERMUTE)
    assert r.nnz == 0 and (r.shape0, r.shape1) == (8, 6)
    # and the context still works
    S = er.operands(A, B, er.TIMES)
    _check(ctx.fetch(ctx.emult(er.TIMES, a, b)), er.emult_ref(S[0], S[1], er.TIMES), "after the errors")
