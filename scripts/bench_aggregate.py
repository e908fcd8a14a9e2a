"""Measure spsamd_aggregate against spsamd_color on the same operand.

    python scripts/bench_aggregate.py [--only poisson,laplace,rmat,tridiag] [--reps 5] [--warmup 1] [--rmat-scale 16]
                                      [--tridiag-log2 20] [--sweep fuse|wave]

Workloads (device generators; those of scripts/bench_color.py):
  poisson  the 5-point Poisson matrix on 4096^2 points
  laplace  the 7-point Laplacian on 256^3 points
  rmat     R-MAT at --rmat-scale, 16 edges per vertex, A + A^T (spsamd_add) plus a diagonal of 2^scale
  tridiag  a tridiagonal matrix of 2^tridiag-log2 rows
For each, in one process, in hash order, with and without the SYMMETRIC flag, into device buffers:
  aggregate   ms and its adjacency, sweep and assign parts; aggregates and n / aggregates; the largest aggregate; rounds,
              launches, fused rounds
  color       spsamd_color, the reference point: it shares the adjacency and the round structure.  sweep_ratio on the
              aggregate lines is the aggregation's sweep over the colouring's.
Nothing outside the project runs here as a baseline.
--sweep fuse: agg_fuse_rows over the powers of two from 64 to 16384 on rmat; wave: agg_wave_deg over 8 .. 4096 on rmat.
Unflagged, hash order.
Times: HIP events on the context's stream, median of --reps after --warmup.
Byte model at 8 TB/s, a lower bound: a round is two passes, each at least one walk of every row on its list, an index and a
64-bit word per entry (12 B) and a word read, a word written and a list entry per vertex (20 B); the first round has every
vertex on both lists, and the model counts that round alone.  `of model` is that over what the sweep took.
One JSON line per measurement, then a table.
"""
import torch

import opbench as ob
from opbench import capi


def main():
    ap = ob.parser("poisson,laplace,rmat,tridiag", reps=5, warmup=1)
    ap.add_argument("--rmat-scale", type=int, default=16)
    ap.add_argument("--tridiag-log2", type=int, default=20)
    ap.add_argument("--sweep", default="")
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")

    def buffers(n):
        return tuple(torch.empty(m, dtype=torch.int32, device=dev) for m in (n, n, n + 1))

    def aggregate(A, out, flags):
        return ctx.aggregate(A, capi.AGG_ORDER_HASH, 1, flags, out=out, stats=True)[1]

    def color(A, out, flags):
        return ctx.color(A, capi.COLOR_ORDER_HASH, 1, flags, out=out, stats=True)[1]

    def stats_of(st, n):
        return {"aggregates": int(st.naggregates), "coarsening": round(n / max(int(st.naggregates), 1), 3), "max_size": int(st.max_size),
                "min_size": int(st.min_size), "ring1": int(st.ring1), "ring2": int(st.ring2), "rounds": int(st.rounds),
                "launches": int(st.launches), "fused_rounds": int(st.fused_rounds), "adjacency": int(st.adjacency),
                "max_degree": int(st.max_degree), "rows_thread": int(st.rows_thread), "rows_wave": int(st.rows_wave),
                "ms_adjacency": round(st.ms_adjacency, 4), "ms_sweep": round(st.ms_sweep, 4), "ms_assign": round(st.ms_assign, 4)}

    def measure(name, A, extra=None):
        n = int(A.shape0)
        base = dict({"workload": name, "rows": n, "tuples": int(A.nnz)}, **(extra or {}))
        out = buffers(n)
        for flags in (0, capi.AGG_SYMMETRIC):
            tag = " symmetric" if flags else ""
            s, ms = ob.time_call(stream, lambda: color(A, out, flags), a.reps, a.warmup)
            ct = color(A, out, flags)
            ob.record(rows, dict(base, what="color hash" + tag, **ob.times(s, ms), colors=int(ct.ncolors), rounds=int(ct.rounds),
                                 launches=int(ct.launches), fused_rounds=int(ct.fused_rounds), ms_adjacency=round(ct.ms_adjacency, 4),
                                 ms_sweep=round(ct.ms_color, 4)))
            s, ms = ob.time_call(stream, lambda: aggregate(A, out, flags), a.reps, a.warmup)
            st = aggregate(A, out, flags)
            by = 2 * (12.0 * st.adjacency + 20.0 * n)
            ob.record(rows, dict(base, what="aggregate hash" + tag, **ob.times(s, ms), **stats_of(st, n),
                                 sweep_ratio=round(st.ms_sweep / max(ct.ms_color, 1e-6), 3),
                                 model_ms_at_8TBps=round(by / ob.PEAK * 1e3, 4), of_model=round(by / ob.PEAK * 1e3 / max(st.ms_sweep, 1e-6), 5)))

    def sweep(name, A, knob, values):
        n = int(A.shape0)
        out = buffers(n)
        for v in values:
            ctx.set_tuning(knob, v)
            try:
                s, ms = ob.time_call(stream, lambda: aggregate(A, out, 0), a.reps, a.warmup)
                st = aggregate(A, out, 0)
            finally:
                ctx.set_tuning(knob, 0)
            ob.record(rows, dict({"workload": name + "_sweep", knob: v, "what": "%s %d" % (knob, v)}, **ob.times(s, ms), **stats_of(st, n)))

    def run_or_sweep(name, A, extra=None):
        pows = lambda lo, hi: [lo << k for k in range((hi // lo).bit_length())]      # noqa: E731
        if a.sweep == "fuse" and name.startswith("rmat"):
            sweep(name, A, "agg_fuse_rows", pows(64, 16384))
        elif a.sweep == "wave" and name.startswith("rmat"):
            sweep(name, A, "agg_wave_deg", pows(8, 4096))
        elif not a.sweep:
            measure(name, A, extra)

    def poisson():
        A, t = ob.poisson2d(ctx, dev)
        run_or_sweep("poisson", A)

    def laplace():
        A, t = ob.laplace3d(ctx, dev)
        run_or_sweep("laplace", A)

    def rmat():
        scale = a.rmat_scale
        n = 1 << scale
        R, raw = ob.rmat(ctx, dev, scale)
        sym = ctx.add(R, R, tB='T')
        i = torch.arange(n, dtype=torch.int32, device=dev)
        d = torch.full((n,), float(n), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        D = capi.device_coo(i.data_ptr(), i.data_ptr(), d.data_ptr(), n, (n, n), 0)
        t = ob.copy_out(ctx, ctx.add(capi.result_operand(sym), D), dev)
        A = capi.device_coo(*ob.ptrs(t), t[2].numel(), (n, n), 0)
        run_or_sweep("rmat%d_sym" % scale, A, {"rmat_scale": scale})

    def tridiag():
        n = 1 << a.tridiag_log2
        i = torch.arange(n, dtype=torch.int32, device=dev)
        r, c = torch.cat([i, i[1:], i[:-1]]), torch.cat([i, i[1:] - 1, i[:-1] + 1])
        v = torch.cat([torch.full((n,), 2.0, dtype=torch.float64, device=dev), torch.full((2 * n - 2,), -0.5, dtype=torch.float64, device=dev)])
        o = torch.argsort(r.long() * n + c.long())
        t = (r[o].contiguous(), c[o].contiguous(), v[o].contiguous())
        torch.cuda.synchronize()
        A = capi.device_coo(*ob.ptrs(t), 3 * n - 2, (n, n), 0)
        run_or_sweep("tridiag_2^%d" % a.tridiag_log2, A)

    ob.run(only, [("poisson", poisson), ("laplace", laplace), ("rmat", rmat), ("tridiag", tridiag)])
    ob.table(rows, [("workload", -16, "%s", "workload"), ("what", -26, "%s", "what"), ("ms", 10, "%.3f", "ms"),
                    ("adjacency", 10, "%.3f", "ms_adjacency"), ("sweep", 9, "%.3f", "ms_sweep"), ("assign", 9, "%.3f", "ms_assign"),
                    ("aggregates", 11, "%d", "aggregates"), ("n / agg", 8, "%.2f", "coarsening"), ("largest", 8, "%d", "max_size"),
                    ("rounds", 7, "%d", "rounds"), ("launches", 9, "%d", "launches"), ("fused", 6, "%d", "fused_rounds"),
                    ("x color", 8, "%.2f", "sweep_ratio"), ("model ms", 9, "%.3f", "model_ms_at_8TBps"),
                    ("of model", 9, "%.2f%%", ob.pct("of_model"))])
    ctx.close()


if __name__ == "__main__":
    main()
