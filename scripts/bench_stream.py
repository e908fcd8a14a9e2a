"""Measure spsamd_multiply_stream (the product delivered in row blocks while it is computed) against what a host caller
does without it: spsamd_multiply into the COO sink, then spsamd_result_fetch.  Both sides hand their chunks to the same
consumer (it counts tuples); the runs alternate in one process.

    python scripts/bench_stream.py [--only s17,cfg2,over] [--reps 3] [--budget 0]

Workloads (R-MAT A*A, device generator, operands resident in HBM):
  s17    scale 17
  cfg2   scale 20 (nnz(C) = 9.7e9: 155 GB of tuples in the plain path's output set)
  over   scale 21, streamed only: its COO output is larger than the device
Times: host wall clock around each call, median of --reps.  Rate: 16 B per tuple delivered / wall time.
One JSON line per measurement.
"""
import json
import time

import numpy as np
import torch

import opbench as ob
from opbench import capi

SCALES = {"s17": 17, "cfg2": 20, "over": 21}


class Counter:
    def __init__(self):
        self.n = 0

    def __call__(self, i, j, v):
        self.n += i.size


def plain(ctx, A):
    cnt = Counter()
    t0 = time.perf_counter()
    res = ctx.multiply(A, A)
    n = int(res.nnz)

    def cb(_u, pi, pj, pv, k):
        cnt(np.ctypeslib.as_array(pi, shape=(k,)), None, None)
        return 0
    ctx._check(ctx.L.spsamd_result_fetch(ctx.h, capi.C.byref(res), capi.CHUNK_FN(cb), None))
    ms = (time.perf_counter() - t0) * 1e3
    assert cnt.n == n
    return ms, n, res.ms_total


def streamed(ctx, A, budget):
    cnt = Counter()
    t0 = time.perf_counter()
    res, st = ctx.multiply_stream(A, A, block_tuples=budget, on_chunk=cnt)
    ms = (time.perf_counter() - t0) * 1e3
    assert cnt.n == res.nnz
    return ms, int(res.nnz), st


def main():
    ap = ob.parser("s17,cfg2", reps=3, warmup=None)
    ap.add_argument("--budget", type=int, default=0, help="block_tuples (0: the library's default)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = capi.Context(0)
    for name in args.only.split(","):
        A, keep = ob.rmat(ctx, dev, SCALES[name])
        rows = []
        for rep in range(args.reps):
            if name != "over":
                ms, n, ms_dev = plain(ctx, A)
                ob.record(rows, dict(workload=name, path="multiply+fetch", rep=rep, ms_wall=ms, nnz_c=n, ms_device=ms_dev,
                                     host_GBps=16 * n / ms / 1e6))
            ms, n, st = streamed(ctx, A, args.budget)
            ob.record(rows, dict(workload=name, path="stream", rep=rep, ms_wall=ms, nnz_c=n, ms_device=st.ms_device,
                                 ms_callback=st.ms_callback, blocks=st.blocks, block_tuples=st.block_tuples,
                                 device_output_bytes=st.device_output_bytes, host_GBps=16 * n / ms / 1e6))
        for path in ("multiply+fetch", "stream"):
            r = [x for x in rows if x["path"] == path]
            if r:
                print(json.dumps(dict(workload=name, path=path, median_ms_wall=float(np.median([x["ms_wall"] for x in r])),
                                      median_ms_device=float(np.median([x["ms_device"] for x in r])))), flush=True)
        del A, keep
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
