"""Measure spsamd_add (C = alpha op(A) + beta op(B), a merge of two sorted streams) against what a user does without it:
torch.cat of the two operands' (scaled) tuples on the device, then spsamd_consolidate.

    python scripts/bench_add.py [--only poisson,rmat,sa] [--reps 7] [--warmup 2]

Workloads (device generators):
  poisson_shift   Poisson 4096^2 A + 0.5 I, both sorted (sort0 = 0)
  poisson_AAt     Poisson 4096^2 A + A^T, B prepared for 'T'
  rmat_AAt        R-MAT scale 20 A + A^T, raw (unsorted, duplicates): both operands need sorting
  sa_add          smoothed aggregation on 256^3: T = -w D^-1 A R^T (one multiply), then P = R^T + T
  sa_chain        the whole chain: T, P, then P^T A P (P copied out of the output set before the last product)
Times: HIP events on the context's stream around the call, median of --reps after --warmup.
Byte model: 16 B per input tuple (two int32 indices and a double) + 16 B per output tuple, against 8 TB/s; it counts
what a merge must read and write once, not the sorts.  One JSON line per measurement, then a table.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spsparse_amd import capi  # noqa: E402

PEAK = 8.0e12


def dev_arrays(m, dev):
    return (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
            torch.empty(m, dtype=torch.float64, device=dev))


def ptrs(t):
    return [x.data_ptr() for x in t]


def time_call(stream, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), ms


def cat_consolidate(ctx, stream, parts, shape):
    """What a user does today: append op(A)'s and op(B)'s scaled tuples on the device, consolidate row-major.
    parts: [(rows, cols, vals, scale)] torch tensors."""
    with torch.cuda.stream(stream):
        r = torch.cat([p[0] for p in parts])
        c = torch.cat([p[1] for p in parts])
        v = torch.cat([p[2] if p[3] == 1.0 else p[2] * p[3] for p in parts])
    M = capi.device_coo(r.data_ptr(), c.data_ptr(), v.data_ptr(), r.numel(), shape, -1)
    res = ctx.consolidate(M, 0)
    return res, (r, c, v)


def record(rows, name, impl, med, ms, nin, nout):
    by = 16.0 * nin + 16.0 * nout
    r = {"workload": name, "impl": impl, "ms": round(med, 4), "ms_all": [round(x, 4) for x in ms], "tuples_in": nin,
         "tuples_out": nout, "algo_bytes": by, "tbps": round(by / med / 1e9, 3), "roofline": round(by / med / 1e9 / (PEAK / 1e12), 4)}
    print(json.dumps(r), flush=True)
    rows.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="poisson,rmat,sa")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx = capi.Context(0, stream.cuda_stream)
    rows = []
    only = a.only.split(",")

    def both(name, A, B, shape, parts, nin, **kw):
        med, ms = time_call(stream, lambda: ctx.add(A, B, **kw), a.reps, a.warmup)
        nout = int(ctx.add(A, B, **kw).nnz)
        record(rows, name, "spsamd_add", med, ms, nin, nout)
        med, ms = time_call(stream, lambda: cat_consolidate(ctx, stream, parts, shape), a.reps, a.warmup)
        record(rows, name, "cat+consolidate", med, ms, nin, nout)

    if "poisson" in only:
        N = 4096
        n = N * N
        t = dev_arrays(5 * N * N - 4 * N, dev)
        ctx.gen_poisson2d(N, *ptrs(t))
        eye = (torch.arange(n, dtype=torch.int32, device=dev),) * 2 + (torch.ones(n, dtype=torch.float64, device=dev),)
        torch.cuda.synchronize()
        A = capi.device_coo(*ptrs(t), t[2].numel(), (n, n), 0)
        I = capi.device_coo(*ptrs(eye), n, (n, n), 0)
        nA = t[2].numel()
        both("poisson_shift", A, I, (n, n), [(t[0], t[1], t[2], 1.0), (eye[0], eye[1], eye[2], 0.5)], nA + n, beta=0.5)
        op = capi.Operand(ctx, A, 'T', capi.AS_A)
        both("poisson_AAt", A, op.coo, (n, n), [(t[0], t[1], t[2], 1.0), (t[1], t[0], t[2], 1.0)], 2 * nA, tB='T')
        op.close()
        del t, eye
        torch.cuda.empty_cache()
    if "rmat" in only:
        scale = 20
        ne = 16 << scale
        t = dev_arrays(ne, dev)
        ctx.gen_rmat(scale, 1, 0, ne, *ptrs(t))
        torch.cuda.synchronize()
        n = 1 << scale
        A = capi.device_coo(*ptrs(t), ne, (n, n), -1)
        both("rmat_AAt", A, A, (n, n), [(t[0], t[1], t[2], 1.0), (t[1], t[0], t[2], 1.0)], 2 * ne, tB='T')
        del t
        torch.cuda.empty_cache()
    if "sa" in only:
        g, w = 256, 2.0 / 3.0
        nf, nc = g ** 3, (g // 2) ** 3
        ta, tr = dev_arrays(7 * g ** 3 - 6 * g * g, dev), dev_arrays(nf, dev)
        ctx.gen_laplace3d(g, *ptrs(ta))
        ctx.gen_aggregation3d(g, *ptrs(tr))
        dinv_i = torch.arange(nf, dtype=torch.int32, device=dev)
        dinv_v = torch.full((nf,), 1.0 / 6.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        A = capi.device_coo(*ptrs(ta), ta[2].numel(), (nf, nf), 0)
        R = capi.device_coo(*ptrs(tr), nf, (nc, nf), 0)
        D = capi.Vec(dinv_i.data_ptr(), dinv_v.data_ptr(), nf, nf, 0, capi.MEM_DEVICE)
        T = ctx.multiply(A, R, -w, scalei=D, tB='T')
        nT = int(T.nnz)
        Tc = dev_arrays(nT, dev)                                   # T kept in buffers of its own across the timed adds
        for x, src, sz in zip(Tc, (T.idx0, T.idx1, T.val), (4, 4, 8)):
            ctx.memcpy(x.data_ptr(), src, nT * sz)
        Top = capi.device_coo(*ptrs(Tc), nT, (nf, nc), 0)
        both("sa_add", R, Top, (nf, nc), [(tr[1], tr[0], tr[2], 1.0), (Tc[0], Tc[1], Tc[2], 1.0)], nf + nT, tA='T')
        keep = {}

        def chain():
            T = ctx.multiply(A, R, -w, scalei=D, tB='T')
            P = ctx.add(R, capi.result_operand(T), tA='T')
            m = int(P.nnz)
            if keep.get("n") != m:
                keep["P"], keep["n"] = dev_arrays(m, dev), m
            for x, src, sz in zip(keep["P"], (P.idx0, P.idx1, P.val), (4, 4, 8)):
                ctx.memcpy(x.data_ptr(), src, m * sz)
            Pc = capi.device_coo(*ptrs(keep["P"]), m, (nf, nc), 0)
            X = ctx.multiply(Pc, A, tA='T')
            return ctx.multiply(capi.result_operand(X), Pc)
        med, ms = time_call(stream, chain, a.reps, a.warmup)
        G = chain()
        r = {"workload": "sa_chain", "impl": "spsamd_add", "ms": round(med, 4), "ms_all": [round(x, 4) for x in ms],
             "nnz_P": keep["n"], "nnz_PtAP": int(G.nnz)}
        print(json.dumps(r), flush=True)
        rows.append(r)
    print("%-14s %-16s %10s %9s %9s" % ("workload", "impl", "ms", "TB/s", "of 8TB/s"))
    for r in rows:
        if "tbps" in r:
            print("%-14s %-16s %10.3f %9.2f %8.1f%%" % (r["workload"], r["impl"], r["ms"], r["tbps"], 100 * r["roofline"]))
        else:
            print("%-14s %-16s %10.3f" % (r["workload"], r["impl"], r["ms"]))
    ctx.close()


if __name__ == "__main__":
    main()
