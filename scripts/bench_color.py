"""Measure spsamd_color and what the colouring buys the level-scheduled kernels.

    python scripts/bench_color.py [--only poisson,laplace,rmat,tridiag] [--reps 5] [--warmup 1] [--rmat-scale 16]
                                  [--tridiag-log2 20] [--sweep fuse|wave]

Workloads (device generators; those of scripts/bench_factor.py):
  poisson  the 5-point Poisson matrix on 4096^2 points
  laplace  the 7-point Laplacian on 256^3 points
  rmat     R-MAT at --rmat-scale, 16 edges per vertex, A + A^T (spsamd_add) plus a diagonal of 2^scale
  tridiag  a tridiagonal matrix of 2^tridiag-log2 rows
For each, in one process:
  color    the colouring into device buffers, with and without SPSAMD_COLOR_SYMMETRIC, in both orders: ms, its adjacency and
           sweep parts, rounds, colours, launches, fused rounds
  extract  P A P^T = spsamd_extract(A, perm, perm) for the hash-order colouring (the degree-order one on rmat)
  natural / coloured   spsamd_factor_ilu0 on a prepared handle and spsamd_solve_tri(LOWER, NONUNIT, one right-hand side) on
           the natural and on the coloured ordering: ms and levels.  The natural ordering is the reference point
           (scripts/bench_factor.py measures the same calls).
  break_even   (colour + extract ms) / (natural - coloured factor-plus-solve ms): the applications that repay the reordering
Nothing outside the project runs here as a baseline.
--sweep fuse: color_fuse_rows over the powers of two from 64 to 16384 on poisson and rmat; wave: color_wave_deg over 8 .. 4096
on rmat.  Unflagged, hash order.
Times: HIP events on the context's stream, median of --reps after --warmup.
Byte model at 8 TB/s, a lower bound: every vertex walks its neighbours at least once, an index and a colour each (8 B per
adjacency entry), and writes a pending and a committed colour and a worklist entry (12 B per vertex).  A vertex that waits
walks again every round; the model does not count that, so `of model` is what one walk would take over what the sweep took.
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

    def color(A, out, order, flags):
        return ctx.color(A, order, 1, flags, out=out, stats=True)[1]

    def stats_of(st):
        return {"colors": int(st.ncolors), "rounds": int(st.rounds), "launches": int(st.launches), "fused_rounds": int(st.fused_rounds),
                "adjacency": int(st.adjacency), "max_degree": int(st.max_degree), "rows_thread": int(st.rows_thread),
                "rows_wave": int(st.rows_wave), "ms_adjacency": round(st.ms_adjacency, 4), "ms_color": round(st.ms_color, 4)}

    def factor_solve(name, what, A, base):
        """factor_ilu0 (prepared, the schedule kept) and solve_tri on A: (factor ms, solve ms)."""
        n = int(A.shape0)
        P = capi.Operand(ctx, A, '.', capi.AS_A)
        _, first = ctx.factor_ilu0(P.coo, stats=True)
        f, ms_f = ob.time_call(stream, lambda: ctx.factor_ilu0(P.coo), a.reps, a.warmup)
        B = torch.rand((n, 1), dtype=torch.float64, device=dev) + 0.5
        X = torch.empty_like(B)
        torch.cuda.synchronize()
        ctx.solve_tri(P.coo, B, X=X)
        s, ms_s = ob.time_call(stream, lambda: ctx.solve_tri(P.coo, B, X=X), a.reps, a.warmup)
        P.close()
        ob.record(rows, dict(base, what=what + " factor_ilu0", levels=int(first.levels), launches=int(first.launches), **ob.times(f, ms_f)))
        ob.record(rows, dict(base, what=what + " solve_tri", levels=int(first.levels), **ob.times(s, ms_s)))
        return f, s

    def measure(name, A, extra=None):
        n = int(A.shape0)
        base = dict({"workload": name, "rows": n, "tuples": int(A.nnz)}, **(extra or {}))
        out = buffers(n)
        ms_color = {}
        for order, oname in ((capi.COLOR_ORDER_HASH, "hash"), (capi.COLOR_ORDER_DEGREE, "degree")):
            for flags in (0, capi.COLOR_SYMMETRIC):
                s, ms = ob.time_call(stream, lambda: color(A, out, order, flags), a.reps, a.warmup)
                st = color(A, out, order, flags)
                by = 8.0 * st.adjacency + 12.0 * n
                ms_color[(order, flags)] = s
                ob.record(rows, dict(base, what="color %s%s" % (oname, " symmetric" if flags else ""), **ob.times(s, ms), **stats_of(st),
                                     model_ms_at_8TBps=round(by / ob.PEAK * 1e3, 4), of_model=round(by / ob.PEAK * 1e3 / max(st.ms_color, 1e-6), 5)))
        order = capi.COLOR_ORDER_DEGREE if name.startswith("rmat") else capi.COLOR_ORDER_HASH
        st = color(A, out, order, capi.COLOR_SYMMETRIC)
        perm = out[1]
        e, ms_e = ob.time_call(stream, lambda: ctx.extract(A, perm, perm), a.reps, a.warmup)
        ob.record(rows, dict(base, what="extract(perm, perm)", **ob.times(e, ms_e)))
        t = ob.copy_out(ctx, ctx.extract(A, perm, perm), dev)
        PA = capi.device_coo(*ob.ptrs(t), t[2].numel(), (n, n), 0)
        f0, s0 = factor_solve(name, "natural", A, base)
        f1, s1 = factor_solve(name, "coloured", PA, dict(base, colors=int(st.ncolors)))
        gain = (f0 + s0) - (f1 + s1)
        once = ms_color[(order, capi.COLOR_SYMMETRIC)] + e
        ob.record(rows, dict(base, what="break_even", ms=round(once, 4), gain_ms=round(gain, 4),
                             applications=round(once / gain, 3) if gain > 0 else None))

    def sweep(name, A, knob, values):
        n = int(A.shape0)
        out = buffers(n)
        for v in values:
            ctx.set_tuning(knob, v)
            try:
                s, ms = ob.time_call(stream, lambda: color(A, out, 0, 0), a.reps, a.warmup)
                st = color(A, out, 0, 0)
            finally:
                ctx.set_tuning(knob, 0)
            ob.record(rows, dict({"workload": name + "_sweep", knob: v, "what": "%s %d" % (knob, v)}, **ob.times(s, ms), **stats_of(st)))

    def run_or_sweep(name, A, extra=None):
        pows = lambda lo, hi: [lo << k for k in range((hi // lo).bit_length())]      # noqa: E731
        if a.sweep == "fuse" and (name == "poisson" or name.startswith("rmat")):
            sweep(name, A, "color_fuse_rows", pows(64, 16384))
        elif a.sweep == "wave" and name.startswith("rmat"):
            sweep(name, A, "color_wave_deg", pows(8, 4096))
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
    ob.table(rows, [("workload", -16, "%s", "workload"), ("what", -28, "%s", "what"), ("ms", 11, "%.3f", "ms"),
                    ("adjacency", 10, "%.3f", "ms_adjacency"), ("sweep", 10, "%.3f", "ms_color"), ("colours", 8, "%d", "colors"),
                    ("rounds", 7, "%d", "rounds"), ("levels", 8, "%d", "levels"), ("launches", 9, "%d", "launches"),
                    ("fused", 7, "%d", "fused_rounds"), ("model ms", 9, "%.3f", "model_ms_at_8TBps"),
                    ("of model", 9, "%.2f%%", ob.pct("of_model")), ("repaid after", 13, "%.2f", "applications")])
    ctx.close()


if __name__ == "__main__":
    main()
