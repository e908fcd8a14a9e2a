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
import json

import torch

import opbench as ob
from opbench import capi


def workload(ctx, name, dev):
    """(Coo as stored on the device, its tuples as tensors, whatever else backs it)."""
    if name == "poisson":
        return ob.poisson2d(ctx, dev, sort0=-1) + (None,)
    if name == "rmat":
        return ob.rmat(ctx, dev, 20) + (None,)
    if name == "cfg5":
        (A, ta), (R, tr) = ob.laplace3d(ctx, dev), ob.aggregation3d(ctx, dev)
        C = ob.galerkin(ctx, A, R)
        # a copy of the result's tuples for the torch reference points (the result itself is sampled in place)
        return capi.result_operand(C), ob.copy_out(ctx, C, dev), (ta, tr)
    raise ValueError(name)


def torch_gather_time(t, P, Q, stream, reps, warmup):
    rows, cols = t[0].to(torch.int64), t[1].to(torch.int64)
    try:
        with torch.cuda.stream(stream):
            med, _ = ob.time_call(stream, lambda: (P[rows] * Q[cols]).sum(1), reps, warmup)
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
            med, _ = ob.time_call(stream, lambda: torch.sparse.sampled_addmm(S, P, Qt, beta=0.0), reps, warmup)
        return med, None
    except Exception as e:                                         # noqa: BLE001
        return None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])


def main():
    ap = ob.parser("poisson,cfg5,rmat")
    ap.add_argument("--k", default="1,8,64,256")
    ap.add_argument("--modes", default="prepared,raw")
    ap.add_argument("--paths", default="0")
    ap.add_argument("--beta", type=float, default=0.0)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    for name in a.only.split(","):
        M, tens, keep = workload(ctx, name, dev)
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
                    med, ms = ob.time_call(stream, lambda: ctx.multiply_sampled(Mm, P, Q, out=o, beta=a.beta), a.reps, a.warmup)
                    ctx.set_tuning("sampled_path", 0)
                    vb = 8.0 * tuples if a.beta != 0 else 0.0
                    comp = 16.0 * tuples + vb + 8.0 * k * (nrow + ncol)
                    gath = 16.0 * tuples + vb + 16.0 * k * tuples
                    ob.record(rows, {"workload": name, "mode": mode, "path": path, "k": k, "tuples": tuples, **ob.times(med, ms),
                                     "compulsory_bytes": comp, "gathered_bytes": gath,
                                     "compulsory_frac": round(comp / med / 1e9 / (ob.PEAK / 1e12), 4),
                                     "gathered_frac": round(gath / med / 1e9 / (ob.PEAK / 1e12), 4)})
            if not a.no_torch:
                med, err = torch_gather_time(tens, P, Q, stream, a.reps, a.warmup)
                ob.record(rows, {"workload": name, "mode": "torch_gather", "k": k, "ms": None if med is None else round(med, 4),
                                 "error": err})
                med, err = torch_sampled_addmm_time(tens, (nrow, ncol), P, Q, stream, a.reps, a.warmup)
                ob.record(rows, {"workload": name, "mode": "torch_sampled_addmm", "k": k, "ms": None if med is None else round(med, 4),
                                 "error": err})
            del P, Q, out
            torch.cuda.empty_cache()
        if op:
            op.close()
        del keep, tens
        torch.cuda.empty_cache()
    ob.table(rows, [("workload", -8, "%s", "workload"), ("mode", -20, "%s", "mode"), ("path", 4, "%d", "path"), ("k", 5, "%d", "k"),
                    ("ms", 10, "%.3f", "ms"), ("compulsory", 11, "%.1f%%", ob.pct("compulsory_frac")),
                    ("gathered", 10, "%.1f%%", ob.pct("gathered_frac"))],
             lambda r: "%-8s %-20s %4s %5d %10s  (%s)" % (r["workload"], r["mode"], "", r["k"], "-", r["error"]) if r["ms"] is None else None)
    ctx.close()


if __name__ == "__main__":
    main()
