"""The shared wave-tile pass (devutil.h: wave_tile_count, wave_range_compact, wave_claim) at its own edges, through the public
API against the host references (select_ref, reduce_ref, emult_ref), bit for bit.

A count / compact pass takes its elements in ballots of 64, tiles of 512 (one wave) and workgroups of four tiles.  N lists
the element counts around each of those sizes; _patterns() the sets of kept elements that put the first, the last and the
neighbouring lanes of two ballots on either side of a boundary.  Every operand is trusted as stored (sort0 = 0), so the
element an operation sees at position i is the one built here.

SINK_COO results are compared tuple by tuple.  SINK_DIGEST results are compared exactly as well, the value sum included: every
value here is a small integer (or a product of three), so the sum is exact in any order of the sink's atomic adds."""
import numpy as np
import pytest

from tests import emult_ref as er
from tests import reduce_ref as rr
from tests import select_ref as sr
from tests.gpu_util import check_tuples as _check, coo as _coo, ctx, forced  # noqa: F401

pytestmark = pytest.mark.gpu

N = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2561)


def _patterns(n):
    i = np.arange(n)
    return {"none": np.zeros(n, bool), "all": np.ones(n, bool), "first": i == 0, "last": i == n - 1, "every other": i % 2 == 0,
            "ballot edges": (i % 64 == 63) | (i % 64 == 0)}


def _ints(n, lo=1, hi=4):
    """Values lo .. hi - 1 with alternating signs, by position."""
    i = np.arange(n)
    return (lo + i % (hi - lo)) * np.where(i % 2 == 0, 1.0, -1.0)


def _both_sinks(ctx, call, want, what):  # noqa: F811
    """call(sink) under SINK_COO and SINK_DIGEST against the tuples `want`."""
    import torch
    from spsparse_amd import capi
    from tests import projection as pj
    wi, wj, wv = want
    _check(ctx.fetch(call(capi.SINK_COO)), want, what)
    d = call(capi.SINK_DIGEST)
    mix = pj.mix64_t(torch.from_numpy(wi.astype(np.int64)), torch.from_numpy(wj.astype(np.int64)))
    assert d.nnz == len(wv), "%s digest: nnz %d, want %d" % (what, d.nnz, len(wv))
    assert d.hash == int(mix.sum().item()) & (2 ** 64 - 1), "%s digest: hash" % what
    assert d.sum == wv.sum(), "%s digest: sum %r, want %r" % (what, d.sum, wv.sum())


# ---------------------------------------------------------------- select

@pytest.mark.parametrize("n", N)
def test_select_flag_kernel_counts_while_it_flags(ctx, n):  # noqa: F811
    """ABS_GE: k_sel_flag's own count, then k_sel_compact.  The pattern's tuples have magnitude 2 or 3, the others 0.5; theta = 1,
    and under COMPLEMENT the others are the kept ones."""
    rows, cols = (np.arange(n) // 7).astype(np.int32), (np.arange(n) % 7).astype(np.int32)
    shape = (int(rows[-1]) + 1, 7)
    for name, mask in _patterns(n).items():
        A = (rows, cols, np.where(mask, _ints(n, 2, 4), 0.5 * _ints(n, 1, 2)))
        keep = []
        a = _coo(A, shape, 0, True, keep)
        for comp in (False, True):
            assert np.array_equal(sr.select_mask(A, shape[0], sr.ABS_GE, dparam=1.0, complement=comp), mask != comp)
            want = sr.select_ref(A, shape[0], sr.ABS_GE, dparam=1.0, complement=comp)
            _both_sinks(ctx, lambda sink: ctx.select(a, sr.ABS_GE, dparam=1.0, complement=comp, sink=sink), want,
                        "ABS_GE n %d %s comp %d" % (n, name, comp))


def _topk_rows(mask):
    """(rows, complement) for ROW_TOPK with k = 1 to keep exactly `mask` of n consecutive tuples: every row holds one kept
    tuple (magnitude 4) and the dropped ones (magnitude 1) next to it -- `every other` gives rows of two tuples; a kept tuple
    alone is a row of one, which stays whole; nothing kept is the complement of everything kept."""
    n = len(mask)
    if not mask.any():
        return np.arange(n), True
    kept = np.flatnonzero(mask)
    rows = np.searchsorted(kept, np.arange(n), side="right") - 1           # the kept tuple at or before this one ...
    return np.maximum(rows, 0), False                                      # ... and the first one's row for those before it


@pytest.mark.parametrize("n", N)
def test_select_separate_count_kernel(ctx, n):  # noqa: F811
    """ROW_TOPK: the row kernels write keep[], k_sel_count counts it, k_sel_compact stores."""
    for name, mask in _patterns(n).items():
        rows, comp = _topk_rows(mask)
        first = np.searchsorted(rows, rows, side="left")
        A = (rows.astype(np.int32), (np.arange(n) - first).astype(np.int32), np.where(mask != comp, 4.0, 1.0) * _ints(n, 1, 2))
        shape = (int(rows[-1]) + 1, n)
        assert np.array_equal(sr.select_mask(A, shape[0], sr.ROW_TOPK, iparam=1, complement=comp), mask)
        want = sr.select_ref(A, shape[0], sr.ROW_TOPK, iparam=1, complement=comp)
        keep = []
        a = _coo(A, shape, 0, True, keep)
        _both_sinks(ctx, lambda sink: ctx.select(a, sr.ROW_TOPK, iparam=1, complement=comp, sink=sink), want, "ROW_TOPK n %d %s" % (n, name))


# ---------------------------------------------------------------- reduce, sparse form: the rows are the elements

def _reduce_both_outputs(ctx, a, nrow, op, want, what):  # noqa: F811
    import torch
    wi, wv = want
    for device in (False, True):
        if device:
            idx = torch.full((nrow,), -3, dtype=torch.int32, device="cuda")
            val = torch.full((nrow,), -7.5, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            cnt = ctx.reduce(a, op, out=(idx, val))
            gi, gv = idx.cpu().numpy(), val.cpu().numpy()
            assert np.all(gi[cnt:] == -3) and np.all(gv[cnt:] == -7.5), what
            gi, gv = gi[:cnt], gv[:cnt]
        else:
            gi, gv = ctx.reduce(a, op)
        assert np.array_equal(gi, wi), "%s device %d: rows %r, want %r" % (what, device, gi[:10], wi[:10])
        assert np.array_equal(gv.view(np.int64), wv.view(np.int64)), "%s device %d: values" % (what, device)


@pytest.mark.parametrize("n", N)
def test_reduce_sparse_form(ctx, n):  # noqa: F811
    """SUM: the pattern's rows have one tuple, every third of them two, the other rows none: presence comes from the row
    pointer.  DIAG: every row has an off-diagonal tuple in column n, the pattern's rows a diagonal one before it: presence
    comes from has[]."""
    shape = (n, n + 1)
    for name, mask in _patterns(n).items():
        r = np.flatnonzero(mask)
        rows = np.repeat(r, np.where(r % 3 == 0, 2, 1))
        S = (rows.astype(np.int32), (np.arange(len(rows)) - np.searchsorted(rows, rows)).astype(np.int32), _ints(len(rows)))
        rows = np.repeat(np.arange(n), 1 + mask.astype(np.int64))
        first = np.arange(len(rows)) == np.searchsorted(rows, rows)
        D = (rows.astype(np.int32), np.where(mask[rows] & first, rows, n).astype(np.int32), _ints(len(rows)))
        keep = []
        for op, X in ((rr.SUM, S), (rr.DIAG, D)):
            wi, wv, _ = rr.reduce_ref(X, n, op)
            assert np.array_equal(wi, r), (name, op)
            _reduce_both_outputs(ctx, _coo(X, shape, 0, True, keep), n, op, (wi, wv), "reduce op %d n %d %s" % (op, n, name))


# ---------------------------------------------------------------- emult

FORMS = ((er.FIRST, False), (er.FIRST, True), (er.TIMES, False))
NCOL = 100


def _flat(keys, vals):
    keys = np.asarray(keys, np.int64)
    return (keys // NCOL).astype(np.int32), (keys % NCOL).astype(np.int32), vals


def _emult_forms(ctx, ka, others, mask, paths, what):  # noqa: F811
    """A holds the ascending flat keys `ka`; B the keys of A that `mask` names (under COMPLEMENT: the others of A) and the keys
    `others`, none of them A's.  Every form keeps exactly `mask` of A."""
    n = len(ka)
    A = _flat(ka, _ints(n))
    shape = (int(max(ka.max(), others.max() if len(others) else 0)) // NCOL + 1, NCOL)
    keep = []
    a = _coo(A, shape, 0, True, keep)
    for op, comp in FORMS:
        kb = np.sort(np.concatenate([ka[mask != comp], others]))
        B = _flat(kb, _ints(len(kb), 1, 3))
        b = _coo(B, shape, 0, True, keep)
        S = er.operands(A, B, op, sortA=0, sortB=0)
        want = er.emult_ref(S[0], S[1], op, 2.0, comp)
        assert np.array_equal(want[0].astype(np.int64) * NCOL + want[1], ka[mask]), what
        for path in paths:
            with forced(ctx, "emult_path", path):
                _both_sinks(ctx, lambda sink: ctx.emult(op, a, b, alpha=2.0, complement=comp, sink=sink), want,
                            "%s op %d comp %d path %d" % (what, op, comp, path))


@pytest.mark.parametrize("n", N)
def test_emult_flag_tail(ctx, n):  # noqa: F811
    """nnz(A) = n on even columns; B also holds three keys on odd columns.  Path 1 compacts the merge's ranges, 2 counts in
    k_em_probe_a, 3 in k_em_count (COMPLEMENT) or scans B's run lengths."""
    ka = 2 * np.arange(n, dtype=np.int64)
    others = np.array([1, 2 * (n // 2) + 1, 2 * n + 1], np.int64)
    for name, mask in _patterns(n).items():
        _emult_forms(ctx, ka, np.unique(others), mask, (1, 2, 3), "emult n %d %s" % (n, name))


def test_emult_merge_waves_without_a_tuples(ctx):  # noqa: F811
    """B outnumbers A by 20 to 1 and A lies in three clusters of 100 consecutive keys: most waves of a merge tile own B tuples
    only, and hand k_em_compact an empty range (a0 == a1) between ranges that are not."""
    starts = np.array([0, 2500, 5300], np.int64)
    ka = np.concatenate([s + np.arange(100) for s in starts])
    others = np.setdiff1d(np.arange(6300, dtype=np.int64), ka)
    assert len(others) == 20 * len(ka)
    for name, mask in _patterns(len(ka)).items():
        _emult_forms(ctx, ka, others, mask, (1,), "emult 20:1 %s" % name)


# ---------------------------------------------------------------- lists claimed from a counter

_LISTS = {}


def _list_case():
    """300 rows; every 41st has 4097 tuples, every third of the others 65, the rest 3: the rows of a listed class are spread
    over all five waves of the classify kernels, a few per ballot."""
    if not _LISTS:
        rng = np.random.default_rng(191)
        r = np.arange(300)
        lens = np.where(r % 41 == 0, 4097, np.where(r % 3 == 0, 65, 3))
        _LISTS["lens"] = lens
        _LISTS["X"] = sr.rows_of_lengths(rng, lens, 6000, special=0.0)
    return _LISTS["X"], _LISTS["lens"]


def test_select_lists(ctx):  # noqa: F811
    X, lens = _list_case()
    shape = (len(lens), 6000)
    keep = []
    a = _coo(X, shape, 0, True, keep)
    res = ctx.select(a, sr.ROW_TOPK, iparam=2)
    _check(ctx.fetch(res), sr.select_ref(X, shape[0], sr.ROW_TOPK, iparam=2), "ROW_TOPK lists")
    assert (res.rows_light, res.rows_mid, res.rows_heavy) == (np.sum(lens == 3), np.sum(lens == 65), np.sum(lens == 4097))
    assert (res.rows_mid, res.rows_heavy) == (97, 8)
    assert (res.tuples_mid, res.tuples_heavy) == (97 * 65, 8 * 4097)


def test_reduce_lists(ctx):  # noqa: F811
    from spsparse_amd import capi
    X, lens = _list_case()
    shape = (len(lens), 6000)
    keep = []
    a = _coo(X, shape, 0, True, keep)
    res = capi.Result()
    gi, gv = ctx.reduce(a, rr.SUM, result=res)
    wi, wv, _ = rr.reduce_ref(X, shape[0], rr.SUM)
    assert np.array_equal(gi, wi) and np.array_equal(gv.view(np.int64), wv.view(np.int64))
    assert (res.rows_light, res.rows_heavy) == (np.sum(lens == 3), np.sum(lens > 3))
    assert res.rows_heavy == 97 + 8 and res.tuples_heavy == 97 * 65 + 8 * 4097
