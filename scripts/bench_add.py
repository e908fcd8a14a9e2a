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
import torch

import opbench as ob
from opbench import capi


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
    ob.record(rows, {"workload": name, "impl": impl, **ob.times(med, ms), "tuples_in": nin, "tuples_out": nout, "algo_bytes": by,
                     "tbps": round(by / med / 1e9, 3), "roofline": round(by / med / 1e9 / (ob.PEAK / 1e12), 4)})


def main():
    a = ob.parser("poisson,rmat,sa").parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []

    def both(name, A, B, shape, parts, nin, **kw):
        med, ms = ob.time_call(stream, lambda: ctx.add(A, B, **kw), a.reps, a.warmup)
        nout = int(ctx.add(A, B, **kw).nnz)
        record(rows, name, "spsamd_add", med, ms, nin, nout)
        med, ms = ob.time_call(stream, lambda: cat_consolidate(ctx, stream, parts, shape), a.reps, a.warmup)
        record(rows, name, "cat+consolidate", med, ms, nin, nout)

    def poisson():
        A, t = ob.poisson2d(ctx, dev)
        n, nA = int(A.shape0), t[2].numel()
        eye = (torch.arange(n, dtype=torch.int32, device=dev),) * 2 + (torch.ones(n, dtype=torch.float64, device=dev),)
        torch.cuda.synchronize()
        I = capi.device_coo(*ob.ptrs(eye), n, (n, n), 0)
        both("poisson_shift", A, I, (n, n), [(t[0], t[1], t[2], 1.0), (eye[0], eye[1], eye[2], 0.5)], nA + n, beta=0.5)
        op = capi.Operand(ctx, A, 'T', capi.AS_A)
        both("poisson_AAt", A, op.coo, (n, n), [(t[0], t[1], t[2], 1.0), (t[1], t[0], t[2], 1.0)], 2 * nA, tB='T')
        op.close()

    def rmat():
        A, t = ob.rmat(ctx, dev, 20)
        n, ne = int(A.shape0), t[2].numel()
        both("rmat_AAt", A, A, (n, n), [(t[0], t[1], t[2], 1.0), (t[1], t[0], t[2], 1.0)], 2 * ne, tB='T')

    def sa():
        g, w = 256, 2.0 / 3.0
        nf, nc = g ** 3, (g // 2) ** 3
        (A, ta), (R, tr) = ob.laplace3d(ctx, dev, g), ob.aggregation3d(ctx, dev, g)
        dinv_i = torch.arange(nf, dtype=torch.int32, device=dev)
        dinv_v = torch.full((nf,), 1.0 / 6.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        D = capi.Vec(dinv_i.data_ptr(), dinv_v.data_ptr(), nf, nf, 0, capi.MEM_DEVICE)
        T = ctx.multiply(A, R, -w, scalei=D, tB='T')
        nT = int(T.nnz)
        Tc = ob.copy_out(ctx, T, dev)                              # T kept in buffers of its own across the timed adds
        Top = capi.device_coo(*ob.ptrs(Tc), nT, (nf, nc), 0)
        both("sa_add", R, Top, (nf, nc), [(tr[1], tr[0], tr[2], 1.0), (Tc[0], Tc[1], Tc[2], 1.0)], nf + nT, tA='T')
        keep = {}

        def chain():
            T = ctx.multiply(A, R, -w, scalei=D, tB='T')
            P = ctx.add(R, capi.result_operand(T), tA='T')
            m = int(P.nnz)
            if keep.get("n") != m:
                keep["P"], keep["n"] = ob.dev_arrays(m, dev), m
            for x, src, sz in zip(keep["P"], (P.idx0, P.idx1, P.val), (4, 4, 8)):
                ctx.memcpy(x.data_ptr(), src, m * sz)
            Pc = capi.device_coo(*ob.ptrs(keep["P"]), m, (nf, nc), 0)
            X = ctx.multiply(Pc, A, tA='T')
            return ctx.multiply(capi.result_operand(X), Pc)
        med, ms = ob.time_call(stream, chain, a.reps, a.warmup)
        G = chain()
        ob.record(rows, {"workload": "sa_chain", "impl": "spsamd_add", **ob.times(med, ms), "nnz_P": keep["n"], "nnz_PtAP": int(G.nnz)})

    ob.run(a.only.split(","), [("poisson", poisson), ("rmat", rmat), ("sa", sa)])
    ob.table(rows, [("workload", -14, "%s", "workload"), ("impl", -16, "%s", "impl"), ("ms", 10, "%.3f", "ms"),
                    ("TB/s", 9, "%.2f", "tbps"), ("of 8TB/s", 9, "%.1f%%", ob.pct("roofline"))])
    ctx.close()


if __name__ == "__main__":
    main()
