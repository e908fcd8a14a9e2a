"""The frame of a graph call (GraphCall), which spsamd_color and spsamd_aggregate share: which of two
refusals is reported, what a refusal leaves in res, stats, the count and the buffers, the n = 0 exits and the too-small
pointer buffer with the call after it.  Every case runs for both calls, on a graph of at most 64 vertices; the results
themselves are pinned by tests/test_gpu_color.py and tests/test_gpu_aggregate.py."""
import ctypes as C

import numpy as np
import pytest

from tests import color_ref as cr
from tests.gpu_util import coo as _coo, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SENT = -77
FILL = 0xA5                              # what res, stats and the count are filled with before a call
COUNT_FILL = int.from_bytes(bytes([FILL]) * C.sizeof(C.c_size_t), "little")
N = 40
#        the C function, the stats struct, the binding's method, the pointer buffer, the noun of the order's refusal
CALLS = {"color": ("spsamd_color", "ColorStats", "color", "color_ptr", "colouring"),
         "aggregate": ("spsamd_aggregate", "AggregateStats", "aggregate", "agg_ptr", "aggregation")}
both = pytest.mark.parametrize("which", sorted(CALLS))


def _graph():
    """A symmetric pattern on N vertices with empty and diagonal-only rows, as a host operand's arrays."""
    K = cr.random_pattern(np.random.default_rng(2601), N, True)
    assert K[0].size > N
    return K[0].astype(np.int32), K[1].astype(np.int32), np.ones(K[0].size)


def _filled(cls):
    x = cls()
    C.memset(C.byref(x), FILL, C.sizeof(x))
    return x


def _bytes(x):
    return C.string_at(C.addressof(x), C.sizeof(x))


def _bufs(device, size=N + 8):
    if device:
        import torch
        return [torch.full((size,), SENT, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    return [np.full(size, SENT, np.int32) for _ in range(3)]


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _untouched(b):
    return all(bool((_host(x) == SENT).all()) for x in b)


class Raw:
    """One call through the C ABI into res, stats and the count, all three filled with FILL beforehand."""

    def __init__(self, ctx, which):
        from spsparse_amd import capi
        self.ctx, self.capi = ctx, capi
        self.fn = getattr(ctx.L, CALLS[which][0])
        self.stats_cls = getattr(capi, CALLS[which][1])

    def __call__(self, a, b, order=0, flags=0, cap=N + 8, mem=None):
        capi = self.capi
        ptr = [None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()) for x in b]
        if mem is None:
            mem = capi.MEM_HOST if isinstance(b[0], np.ndarray) else capi.MEM_DEVICE
        self.res, self.stats, self.cnt = _filled(capi.Result), _filled(self.stats_cls), _filled(C.c_size_t)
        rc = self.fn(self.ctx.h, C.byref(a), b'.', order, 1, flags, ptr[0], ptr[1], ptr[2], cap, mem, C.byref(self.cnt),
                     C.byref(self.stats), C.byref(self.res))
        return rc, self.ctx.L.spsamd_last_error(self.ctx.h).decode()

    def all_filled(self):
        return all(_bytes(x) == bytes([FILL]) * C.sizeof(x) for x in (self.res, self.stats, self.cnt))


@both
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusal_order(ctx, which, device):
    """Calls wrong in two ways at once: the refusal reported is the one that comes first in order, flags, mem, square,
    overlap.  Each leaves res, stats, the count and the three buffers as they were."""
    A = _graph()
    keep = []
    a = _coo(A, (N, N), 0, keep=keep)
    wide = _coo(A, (N, N + 1), 0, keep=keep)
    call = Raw(ctx, which)
    b = _bufs(device)
    one = _bufs(device, 3 * N)[0]
    lapped = [one[0:N], one[N // 2:N // 2 + N], one[2 * N:3 * N]]
    noun = CALLS[which][4]
    for what, (rc, msg), code, word in (
            ("order, then square", call(wide, b, order=2), -2, "unknown %s order" % noun),
            ("flags, then mem", call(a, b, flags=2, mem=7), -2, "_flags"),
            ("mem, then square", call(wide, b, mem=7), -2, "mem of the output"),
            ("square, then overlap", call(wide, lapped, cap=N), -1, "square"),
            ("overlap alone", call(a, lapped, cap=N), -2, "overlap")):
        assert rc == code and word in msg, "%s: %d %r" % (what, rc, msg)
        assert call.all_filled() and _untouched(b) and _untouched([one]), what


@both
def test_refusal_from_the_keys(ctx, which):
    """An index out of range in a host operand is found when the keys are taken: after res and stats were zeroed (res holds
    the shape by then) and before the count is."""
    A = _graph()
    keep = []
    bad = _coo((A[0], np.where(A[1] == A[1].max(), N, A[1]).astype(np.int32), A[2]), (N, N), -1, keep=keep)
    call = Raw(ctx, which)
    b = _bufs(False)
    rc, msg = call(bad, b)
    assert rc == -2 and msg, (rc, msg)
    want = call.capi.Result()
    want.shape0 = want.shape1 = N
    assert _bytes(call.res) == _bytes(want), "res: zeroed but for the shape"
    assert _bytes(call.stats) == bytes(C.sizeof(call.stats)), "stats: zeroed"
    assert call.cnt.value == COUNT_FILL, "the count: not written"
    assert _untouched(b)


@both
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_no_vertices(ctx, which, device):
    """n = 0: the pointer buffer needs its one entry; with it the call succeeds, counts 0 and writes that entry alone."""
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
    keep = []
    a = _coo(e, (0, 0), -1, keep=keep)
    call = Raw(ctx, which)
    b = _bufs(device)
    rc, msg = call(a, b, cap=0)
    assert rc == -5 and CALLS[which][3] in msg and call.cnt.value == 0 and _untouched(b), (rc, msg)
    rc, msg = call(a, b, cap=1)
    assert rc == 0 and call.cnt.value == 0
    ptr = _host(b[2])
    assert ptr[0] == 0 and np.all(ptr[1:] == SENT) and _untouched(b[:2])
    assert (call.res.shape0, call.res.shape1, call.res.nnz_a) == (0, 0, 0) and _bytes(call.stats) == bytes(C.sizeof(call.stats))
    b = _bufs(device)
    assert call(a, [b[0], b[1], None], cap=0)[0] == 0 and call.cnt.value == 0 and _untouched(b)   # without it the capacity means nothing


@both
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_pointer_buffer_too_small(ctx, which, device):
    """n > 0: the count comes back, nothing is written and the message names the buffer; the context then serves the next
    call like a fresh one."""
    from spsparse_amd import capi
    A = _graph()
    keep = []
    a = _coo(A, (N, N), 0, keep=keep)
    fresh = capi.Context(0)
    try:
        want = getattr(fresh, CALLS[which][2])(a, seed=1, stats=True)
    finally:
        fresh.close()
    count = want[2].size - 1
    assert 1 <= count <= N
    call = Raw(ctx, which)
    b = _bufs(device)
    for cap in (0, count):
        rc, msg = call(a, b, cap=cap)
        assert rc == -5 and CALLS[which][3] in msg and "too small" in msg and call.cnt.value == count and _untouched(b), (cap, rc, msg)
    rc, msg = call(a, b, cap=count + 1)
    assert rc == 0 and call.cnt.value == count, (rc, msg)
    got = [_host(x) for x in b]
    for k, size in enumerate((N, N, count + 1)):
        assert np.array_equal(got[k][:size], want[k]) and np.all(got[k][size:] == SENT), k
    exact = [f for f, t in call.stats._fields_ if t is C.c_uint64]
    assert [getattr(call.stats, f) for f in exact] == [getattr(want[3], f) for f in exact]
    again = getattr(ctx, CALLS[which][2])(a, seed=1, stats=True)       # ... and through the binding's host path
    assert all(np.array_equal(again[k], want[k]) for k in range(3))
