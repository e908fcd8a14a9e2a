"""Measure spsamd_multiply_dense (Y += op(M) X, bit-exact ordered adds) on the device generators' workloads.

    python scripts/bench_dense.py [--only poisson,cfg5,rmat] [--nrhs 1,8,64] [--reps 7] [--warmup 2]

Workloads: Poisson 4096^2 (83.9 M tuples), the cfg5 operator R A R^T on 256^3 (a SINK_COO result used in place) and
R-MAT scale 20 (power-law rows, unsorted with duplicates).  Each is applied prepared (spsamd_operand_prepare once, its
packed tuples and row pointer kept) and raw (the tuples as stored: inspection, and the stable sort by output row where
the storage order is not row order).  Times: HIP events on the context's stream around the call, median of --reps after
--warmup.  Bytes: 12 per tuple + 8 nrhs per X row + 16 nrhs per Y row (read and write), against 8 TB/s.
One JSON line per measurement, then a table.
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


def workload(ctx, name, dev, keep):
    """(Coo as stored, shape) on the device."""
    if name == "poisson":
        N = 4096
        t = dev_arrays(5 * N * N - 4 * N, dev)
        ctx.gen_poisson2d(N, *ptrs(t))
        keep.append(t)
        return capi.device_coo(*ptrs(t), t[2].numel(), (N * N, N * N), -1)
    if name == "rmat":
        scale = 20
        ne = 16 << scale
        t = dev_arrays(ne, dev)
        ctx.gen_rmat(scale, 1, 0, ne, *ptrs(t))
        keep.append(t)
        return capi.device_coo(*ptrs(t), ne, (1 << scale, 1 << scale), -1)
    if name == "cfg5":
        g = 256
        ta, tr = dev_arrays(7 * g ** 3 - 6 * g * g, dev), dev_arrays(g ** 3, dev)
        ctx.gen_laplace3d(g, *ptrs(ta))
        ctx.gen_aggregation3d(g, *ptrs(tr))
        keep.extend([ta, tr])
        A = capi.device_coo(*ptrs(ta), ta[2].numel(), (g ** 3, g ** 3), 0)
        R = capi.device_coo(*ptrs(tr), g ** 3, ((g // 2) ** 3, g ** 3), 0)
        T = ctx.multiply(R, A)
        C = ctx.multiply(capi.result_operand(T), R, tB='T')
        return capi.result_operand(C)
    raise ValueError(name)


def time_call(ctx, stream, fn, reps, warmup):
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


def torch_csr_time(M, X, stream, reps, warmup):
    """torch.sparse_csr_tensor @ dense on the same operator (unordered sums: a reference point, not a bar)."""
    try:
        i0 = M["i0"]
        n = M["shape"][0]
        order = torch.argsort(i0.to(torch.int64), stable=True)
        crow = torch.zeros(n + 1, dtype=torch.int64, device=i0.device)
        crow[1:] = torch.cumsum(torch.bincount(i0.to(torch.int64), minlength=n), 0)
        A = torch.sparse_csr_tensor(crow, M["i1"].to(torch.int64)[order], M["v"][order], size=M["shape"])
        with torch.cuda.stream(stream):
            med, _ = time_call(None, stream, lambda: A @ X, reps, warmup)
        return med, None
    except Exception as e:                                         # noqa: BLE001
        return None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="poisson,cfg5,rmat")
    ap.add_argument("--nrhs", default="1,8,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="prepared,raw")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx = capi.Context(0, stream.cuda_stream)
    rows = []
    for name in a.only.split(","):
        keep = []
        M = workload(ctx, name, dev, keep)
        torch.cuda.synchronize()
        n = int(M.shape0)
        nnz = int(M.nnz)
        op = capi.Operand(ctx, M, '.', capi.AS_A) if "prepared" in a.modes else None
        nnz_prep = int(op.coo.nnz) if op else nnz
        for nrhs in [int(x) for x in a.nrhs.split(",")]:
            X = torch.rand((int(M.shape1), nrhs), dtype=torch.float64, device=dev)
            Y = torch.zeros((n, nrhs), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            for mode in a.modes.split(","):
                Mm = op.coo if mode == "prepared" else M
                tuples = nnz_prep if mode == "prepared" else nnz
                med, ms = time_call(ctx, stream, lambda: ctx.multiply_dense(Mm, X, Y), a.reps, a.warmup)
                by = 12.0 * tuples + 8.0 * nrhs * int(M.shape1) + 16.0 * nrhs * n
                r = {"workload": name, "mode": mode, "nrhs": nrhs, "tuples": tuples, "rows": n, "ms": round(med, 4),
                     "ms_all": [round(x, 4) for x in ms], "algo_bytes": by, "tbps": round(by / med / 1e9, 3),
                     "roofline": round(by / med / 1e9 / (PEAK / 1e12), 4)}
                print(json.dumps(r), flush=True)
                rows.append(r)
            if not a.no_torch and name == "poisson" and nrhs in (1, 8):
                Mt = {"i0": keep[0][0], "i1": keep[0][1], "v": keep[0][2], "shape": (n, n)}
                med, err = torch_csr_time(Mt, X, stream, a.reps, a.warmup)
                r = {"workload": name, "mode": "torch_csr", "nrhs": nrhs, "ms": None if med is None else round(med, 4), "error": err}
                print(json.dumps(r), flush=True)
                rows.append(r)
            del X, Y
            torch.cuda.empty_cache()
        if op:
            op.close()
        del keep
        torch.cuda.empty_cache()
    print("%-8s %-9s %5s %10s %9s %9s" % ("workload", "mode", "nrhs", "ms", "TB/s", "of 8TB/s"))
    for r in rows:
        if r["ms"] is None:
            print("%-8s %-9s %5d %10s  (%s)" % (r["workload"], r["mode"], r["nrhs"], "-", r.get("error")))
        elif "tbps" in r:
            print("%-8s %-9s %5d %10.3f %9.2f %8.1f%%" % (r["workload"], r["mode"], r["nrhs"], r["ms"], r["tbps"], 100 * r["roofline"]))
        else:
            print("%-8s %-9s %5d %10.3f" % (r["workload"], r["mode"], r["nrhs"], r["ms"]))
    ctx.close()


if __name__ == "__main__":
    main()
