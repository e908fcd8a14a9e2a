"""One dump of what spsamd_color and spsamd_aggregate return, to compare two checkouts:

    cd CHECKOUT && python PATH/TO/scripts/graph_frame_dump.py OUT

loads the package and tests/ of the current directory (the checkout needs tests/test_gpu_graph_frame.py for its raw call).
For both calls: the round-width graphs of tests/test_gpu_color.py and tests/test_gpu_aggregate.py under path 0 / 1 / 2 and
fuse_rows 256; poisson64 and rmat10 with every order and flag, every (path, row) and every (host | device buffers, with |
without the optional two), one dimension at a time from the defaults; the refusals, the n = 0 exits and the too-small
pointer buffer of tests/test_gpu_graph_frame.py, and a false SYMMETRIC promise.  Per call a header line naming the stats
fields, then per case one line: the return code and, where it is not 0, the message; the count; the sha256 (16 hex digits)
of each buffer's bytes, sentinel tail included; every stats field but the times; res's shape, nnz_a and workspace_bytes.
profiles/graph_frame/ has two of them and their diff."""
import hashlib
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402

from spsparse_amd import capi, workloads as wl  # noqa: E402
from tests import aggregate_ref as ar  # noqa: E402
from tests import color_ref as cr  # noqa: E402
from tests import factor_ref as fr  # noqa: E402
from tests.gpu_util import Knobs, coo as _coo  # noqa: E402
from tests.test_gpu_aggregate import ROUND_CASES  # noqa: E402
from tests.test_gpu_graph_frame import CALLS, N, Raw, _bufs, _graph, _host  # noqa: E402

PREFIX = {"color": "color", "aggregate": "agg"}                         # of the knobs
COLOR_ROUNDS = {"wide": [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000, 1, 1, 1, 5000, 2], "edges": [2000, 1, 767, 1, 255, 1]}


def sha(x):
    return "-" if x is None else hashlib.sha256(np.ascontiguousarray(_host(x)).tobytes()).hexdigest()[:16]


def main():
    out = open(sys.argv[1], "w")
    ctx = capi.Context(0)
    print("library", capi.__file__, file=sys.stderr)
    calls = {w: Raw(ctx, w) for w in sorted(CALLS)}

    def fields(which):
        return [f for f, _t in calls[which].stats_cls._fields_ if not f.startswith("ms_")]

    def case(name, which, a, n, device=False, optional=True, knobs=None, b=None, **kw):
        call = calls[which]
        b = _bufs(device, n + 8) if b is None else b
        if not optional:
            b = [b[0], None, None]
        kw.setdefault("cap", n + 8)
        with Knobs(ctx, {"%s_%s" % (PREFIX[which], k): v for k, v in (knobs or {}).items()}):
            rc, msg = call(a, b, **kw)
        r = call.res
        out.write("%s %s | %d%s %d | %s | %s | %d %d %d %d\n" % (
            which, name, rc, " " + repr(msg) if rc else "", call.cnt.value, " ".join(sha(x) for x in b),
            " ".join("%d" % getattr(call.stats, f) for f in fields(which)), r.shape0, r.shape1, r.nnz_a, r.workspace_bytes))
        out.flush()

    for which in sorted(CALLS):
        out.write("# %s NAME | rc ['message'] count | sha256 of the three buffers | %s | shape0 shape1 nnz_a workspace_bytes\n" % (which, " ".join(fields(which))))
        # ---- the round-width graphs
        graphs = [("color " + k, cr.by_rounds(np.random.default_rng(2203), s, 9)[0], sum(s)) for k, s in COLOR_ROUNDS.items()]
        graphs += [("agg " + k, ar.by_rounds(s, 9)[0], sum(s)) for k, s in ROUND_CASES.items()]
        for gname, K, n in graphs:
            keep = []
            a = _coo((K[0], K[1], np.ones(K[0].size)), (n, n), 0, device=True, keep=keep)
            for knobs in ({}, {"path": 1}, {"path": 2}, {"fuse_rows": 256}):
                case("rounds %s %s" % (gname, " ".join("%s %d" % kv for kv in sorted(knobs.items()))), which, a, n, device=True, knobs=knobs, flags=1)
        # ---- the larger shapes: one dimension at a time
        for gname in ("poisson64", "rmat10"):
            S, n = (fr.sorted_unique(*wl.poisson2d(64)[:3]), 64 * 64) if gname == "poisson64" else fr.rmat_sym(10, 8, 3, 50.0)
            keep = []
            a = _coo(S, (n, n), 0, device=True, keep=keep)
            for order in (0, 1):
                for flags in (0, 1):
                    case("%s order %d flags %d" % (gname, order, flags), which, a, n, order=order, flags=flags)
            for path in (0, 1, 2):
                for row in (0, 1, 2):
                    case("%s path %d row %d" % (gname, path, row), which, a, n, True, knobs={"path": path, "row": row})
            for device in (False, True):
                for optional in (True, False):
                    case("%s order 1 device %d optional %d" % (gname, device, optional), which, a, n, device, optional, order=1)
        # ---- the refusals and exits of tests/test_gpu_graph_frame.py
        A = _graph()
        keep = []
        a = _coo(A, (N, N), 0, keep=keep)
        wide = _coo(A, (N, N + 1), 0, keep=keep)
        bad = _coo((A[0], np.where(A[1] == A[1].max(), N, A[1]).astype(np.int32), A[2]), (N, N), -1, keep=keep)
        U = cr.random_pattern(np.random.default_rng(2602), N, False)     # not symmetric: aggregation refuses it under the flag
        oneway = _coo((U[0], U[1], np.ones(U[0].size)), (N, N), 0, keep=keep)
        empty = _coo((np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)), (0, 0), -1, keep=keep)
        for device in (False, True):
            one = _bufs(device, 3 * N)[0]
            lapped = [one[0:N], one[N // 2:N // 2 + N], one[2 * N:3 * N]]
            d = "device %d" % device
            case("refusal order+square " + d, which, wide, N, device, order=2)
            case("refusal flags+mem " + d, which, a, N, device, flags=2, mem=7)
            case("refusal mem+square " + d, which, wide, N, device, mem=7)
            case("refusal square+overlap " + d, which, wide, N, device, b=lapped, cap=N)
            case("refusal overlap " + d, which, a, N, device, b=lapped, cap=N)
            case("refusal keys " + d, which, bad, N, device)
            case("false promise " + d, which, oneway, N, device, flags=1)
            for cap in (0, 1):
                case("n0 cap %d %s" % (cap, d), which, empty, 0, device, cap=cap)
            case("n0 without the optional two " + d, which, empty, 0, device, optional=False, cap=0)
            for cap in (0, 1, N + 1):
                case("capacity %d %s" % (cap, d), which, a, N, device, cap=cap)
    ctx.close()
    out.close()


if __name__ == "__main__":
    main()
