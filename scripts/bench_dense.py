"""Measure spsamd_multiply_dense (Y += op(M) X, bit-exact ordered adds) on the device generators' workloads.

    python scripts/bench_dense.py [--only poisson,cfg5,rmat] [--nrhs 1,8,64] [--reps 7] [--warmup 2]

Workloads: Poisson 4096^2 (83.9 M tuples), the cfg5 operator R A R^T on 256^3 (a SINK_COO result used in place) and
R-MAT scale 20 (power-law rows, unsorted with duplicates).  Each is applied prepared (spsamd_operand_prepare once, its
packed tuples and row pointer kept) and raw (the tuples as stored: inspection, and the stable sort by output row where
the storage order is not row order).  Times: HIP events on the context's stream around the call, median of --reps after
--warmup.  Bytes: 12 per tuple + 8 nrhs per X row + 16 nrhs per Y row (read and write), against 8 TB/s.
One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi


def workload(ctx, name, dev):
    """(Coo as stored, the tensors behind it) on the device."""
    if name == "poisson":
        return ob.poisson2d(ctx, dev, sort0=-1)
    if name == "rmat":
        return ob.rmat(ctx, dev, 20)
    if name == "cfg5":
        (A, ta), (R, tr) = ob.laplace3d(ctx, dev), ob.aggregation3d(ctx, dev)
        return capi.result_operand(ob.galerkin(ctx, A, R)), (ta, tr)
    raise ValueError(name)


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
            med, _ = ob.time_call(stream, lambda: A @ X, reps, warmup)
        return med, None
    except Exception as e:                                         # noqa: BLE001
        return None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:200])


def main():
    ap = ob.parser("poisson,cfg5,rmat")
    ap.add_argument("--nrhs", default="1,8,64")
    ap.add_argument("--modes", default="prepared,raw")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    for name in a.only.split(","):
        M, keep = workload(ctx, name, dev)
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
                med, ms = ob.time_call(stream, lambda: ctx.multiply_dense(Mm, X, Y), a.reps, a.warmup)
                by = 12.0 * tuples + 8.0 * nrhs * int(M.shape1) + 16.0 * nrhs * n
                ob.record(rows, {"workload": name, "mode": mode, "nrhs": nrhs, "tuples": tuples, "rows": n, **ob.times(med, ms),
                                 "algo_bytes": by, "tbps": round(by / med / 1e9, 3),
                                 "roofline": round(by / med / 1e9 / (ob.PEAK / 1e12), 4)})
            if not a.no_torch and name == "poisson" and nrhs in (1, 8):
                Mt = {"i0": keep[0], "i1": keep[1], "v": keep[2], "shape": (n, n)}
                med, err = torch_csr_time(Mt, X, stream, a.reps, a.warmup)
                ob.record(rows, {"workload": name, "mode": "torch_csr", "nrhs": nrhs, "ms": None if med is None else round(med, 4),
                                 "error": err})
            del X, Y
            torch.cuda.empty_cache()
        if op:
            op.close()
        del keep
        torch.cuda.empty_cache()
    ob.table(rows, [("workload", -8, "%s", "workload"), ("mode", -9, "%s", "mode"), ("nrhs", 5, "%d", "nrhs"), ("ms", 10, "%.3f", "ms"),
                    ("TB/s", 9, "%.2f", "tbps"), ("of 8TB/s", 9, "%.1f%%", ob.pct("roofline"))],
             lambda r: "%-8s %-9s %5d %10s  (%s)" % (r["workload"], r["mode"], r["nrhs"], "-", r["error"]) if r["ms"] is None else None)
    ctx.close()


if __name__ == "__main__":
    main()
