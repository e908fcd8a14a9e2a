"""Measure spsamd_multiply_sampled (out[t] = P_i . Q_j over M's tuples, serial ascending-r sums) on the device generators'
workloads.

    python scripts/bench_sampled.py [--only poisson,cfg5,rmat] [--k 1,8,64,256] [--reps 7] [--warmup 2] [--paths 0]

Workloads: Poisson 4096^2 (83.9 M tuples, row-sorted), the cfg5 operator R A R^T on 256^3 (a SINK_COO result used in place)
and R-MAT scale 20 (16.8 M tuples, unsorted with duplicates).  Each is sampled raw (the tuples as stored, inspected) and
prepared (spsamd_operand_prepare once: its consolidated tuples, indices trusted).  --paths 0,1,2 sweeps the sampled_path
knob (auto | lane | slab).  Times: HIP events on the context's stream around the call, median of --reps after --warmup.
Byte models, against 8 TB/s:
  compulsory  8 per tuple (indices) + 8 per tuple (out) + 8 per tuple (v, when beta != 0) + 8 k per row of P and of Q
  gathered    8 per tuple (indices) + 8 per tuple (out) + 16 k per tuple (the P and Q rows of every tuple)
Reference points: the torch gather expression (P[rows] * Q[cols]).sum(1) and torch.sparse.sampled_addmm on CSR (if this
build runs it).  Neither sums in a fixed order.  One JSON line per measurement, then a table.
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
    """(Coo as stored on the device, its (i0, i1) tensors)."""
    if name == "poisson":
        N = 4096
        t = dev_arrays(5 * N * N - 4 * N, dev)
        ctx.gen_poisson2d(N, *ptrs(t))
        keep.append(t)
        return capi.device_coo(*ptrs(t), t[2].numel(), (N * N, N * N), -1), t
    if name == "rmat":
        scale = 20
        ne = 16 << scale
        t = dev_arrays(ne, dev)
        ctx.gen_rmat(scale, 1, 0, ne, *ptrs(t))
        keep.append(t)
        return capi.device_coo(*ptrs(t), ne, (1 << scale, 1 << scale), -1), t
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
        n = int(C.nnz)
        # a copy of the result's indices for the torch reference points (the result itself is sampled in place)
        t = dev_arrays(n, dev)
        ctx.memcpy(t[0].data_ptr(), C.idx0, 4 * n)
        ctx.memcpy(t[1].data_ptr(), C.idx1, 4 * n)
        ctx.memcpy(t[2].data_ptr(), C.val, 8 * n)
        keep.append(t)
        return capi.result_operand(C), t
    raise ValueError(name)


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


def torch_gather_time(t, P, Q, stream, reps, warmup):
    rows, cols = t[0].to(torch.int64), t[1].to(torch.int64)
    try:
        with torch.cuda.stream(stream):
            med, _ = time_call(stream, lambda: (P[rows] * Q[cols]).sum(1), reps, warmup)
        return med, None
    except Exception as e:                                         # noqa: BLE001
        return None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])


def torch_sampled_addmm_time(t, shape, P, Q, stream, reps, warmup):
    try:
        i0 = t[0].to(torch.int64)
        n = shape[0]
        order = torch.argsort(i0, stable=True)
        crow = torch.zeros(n + 1, dtype=torch.int64, device=i0.device)
        crow[1:] = torch.cumsum(torch.bincount(i0, minlength=n), 0)
        S = torch.sparse_csr_tensor(crow, t[1].to(torch.int64)[order], t[2][order], size=shape)
        Qt = Q.t()
        with torch.cuda.stream(stream):
            med, _ = time_call(stream, lambda: torch.sparse.sampled_addmm(S, P, Qt, beta=0.0), reps, warmup)
        return med, None
    except Exception as e:                                         # noqa: BLE001
        return None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="poisson,cfg5,rmat")
    ap.add_argument("--k", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="prepared,raw")
    ap.add_argument("--paths", default="0")
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx = capi.Context(0, stream.cuda_stream)
    rows = []
    for name in a.only.split(","):
        keep = []
        M, tens = workload(ctx, name, dev, keep)
        torch.cuda.synchronize()
        nrow, ncol, nnz = int(M.shape0), int(M.shape1), int(M.nnz)
        op = capi.Operand(ctx, M, '.', capi.AS_A) if "prepared" in a.modes else None
        for k in [int(x) for x in a.k.split(",")]:
            need = 8.0 * k * (nrow + ncol) + 2 * 16.0 * nnz
            if need > 200e9:
                print(json.dumps({"workload": name, "k": k, "skipped": "%.0f GB of device memory" % (need / 1e9)}), flush=True)
                continue
            P = torch.rand((nrow, k), dtype=torch.float64, device=dev)
            Q = torch.rand((ncol, k), dtype=torch.float64, device=dev)
            out = torch.empty(nnz, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            for mode in a.modes.split(","):
                Mm = op.coo if mode == "prepared" else M
                tuples = int(Mm.nnz)
                o = out[:tuples]
                for path in [int(x) for x in a.paths.split(",")]:
                    ctx.set_tuning("sampled_path", path)
                    med, ms = time_call(stream, lambda: ctx.multiply_sampled(Mm, P, Q, out=o, beta=a.beta), a.reps, a.warmup)
                    ctx.set_tuning("sampled_path", 0)
                    vb = 8.0 * tuples if a.beta != 0 else 0.0
                    comp = 16.0 * tuples + vb + 8.0 * k * (nrow + ncol)
                    gath = 16.0 * tuples + vb + 16.0 * k * tuples
                    r = {"workload": name, "mode": mode, "path": path, "k": k, "tuples": tuples, "ms": round(med, 4),
                         "ms_all": [round(x, 4) for x in ms], "compulsory_bytes": comp, "gathered_bytes": gath,
                         "compulsory_frac": round(comp / med / 1e9 / (PEAK / 1e12), 4),
                         "gathered_frac": round(gath / med / 1e9 / (PEAK / 1e12), 4)}
                    print(json.dumps(r), flush=True)
                    rows.append(r)
            if not a.no_torch:
                med, err = torch_gather_time(tens, P, Q, stream, a.reps, a.warmup)
                r = {"workload": name, "mode": "torch_gather", "k": k, "ms": None if med is None else round(med, 4), "error": err}
                print(json.dumps(r), flush=True)
                rows.append(r)
                med, err = torch_sampled_addmm_time(tens, (nrow, ncol), P, Q, stream, a.reps, a.warmup)
                r = {"workload": name, "mode": "torch_sampled_addmm", "k": k, "ms": None if med is None else round(med, 4), "error": err}
                print(json.dumps(r), flush=True)
                rows.append(r)
            del P, Q, out
            torch.cuda.empty_cache()
        if op:
            op.close()
        del keep, tens
        torch.cuda.empty_cache()
    print("%-8s %-20s %4s %5s %10s %11s %10s" % ("workload", "mode", "path", "k", "ms", "compulsory", "gathered"))
    for r in rows:
        if "skipped" in r:
            continue
        if r["ms"] is None:
            print("%-8s %-20s %4s %5d %10s  (%s)" % (r["workload"], r["mode"], "", r["k"], "-", r.get("error")))
        elif "compulsory_frac" in r:
            print("%-8s %-20s %4d %5d %10.3f %10.1f%% %9.1f%%" % (r["workload"], r["mode"], r["path"], r["k"], r["ms"],
                                                             100 * r["compulsory_frac"], 100 * r["gathered_frac"]))
        else:
            print("%-8s %-20s %4s %5d %10.3f" % (r["workload"], r["mode"], "", r["k"], r["ms"]))
    ctx.close()


if __name__ == "__main__":
    main()
