"""Measure spsamd_emult (op(A) o op(B), and op(A) on or off op(B)'s pattern) against what a user does without it.

    python scripts/bench_emult.py [--only poisson,rmat,chain] [--reps 7] [--warmup 2] [--paths]

Workloads (device generators):
  poisson_AoAT     Poisson 4096^2, A o A^T, B a handle prepared for 'T'; and A restricted to A^T's pattern (FIRST)
  rmat20_AoAT      R-MAT scale 20 raw (unsorted, duplicates) on both sides: the consolidations are part of both sides
  chain_first      FIRST(T, A): T = A A of R-MAT scale 16 read in place from the context's output set, the pattern A's
                   consolidated tuples -- nnz(A) << nnz(T), the lopsided case
  chain_off        FIRST | COMPLEMENT of the same
Baselines: FIRST -- spsamd_multiply_masked(A, I, M = B), the only device route without this call (it cannot express TIMES or
the complement, so chain_off has no baseline and is reported alone); TIMES -- composed torch calls over the same device
arrays: 64-bit keys, torch.searchsorted into B's sorted keys, gather, multiply (B's keys sorted outside the timing where the
call reads a prepared handle; inside it, with the consolidations, for the raw operands).  The tuples are compared bit for
bit (values as int64) once per workload, before the timing.
Times: HIP events on the context's stream, median of --reps after --warmup, the call and its baseline alternating.
--paths also times the call with every emult_path value forced (1 merge, 2 probe A in B, 3 probe B in A): the comparison
that fixes the constant of the auto choice.
Byte model: 8 B per key read of both operands + 16 B per output tuple and 8 B per input value it reads (two under TIMES,
one under FIRST), against 8 TB/s: reported, not gated.
One JSON line per measurement, then a table; the gate: FIRST faster than the masked-identity route on every workload, same
tuples everywhere.
"""
import torch

import opbench as ob
from opbench import capi


def keys64(r, c):
    return (r.long() << 32) | c.long()


def torch_times(ta, kb_sorted, vb_sorted):
    """A o B over (rows, cols, vals) of A sorted row-major and B's sorted unique 64-bit keys with their values."""
    ka = keys64(ta[0], ta[1])
    p = torch.searchsorted(kb_sorted, ka).clamp_(max=max(kb_sorted.numel() - 1, 0))
    hit = kb_sorted[p] == ka
    return ta[0][hit], ta[1][hit], ta[2][hit] * vb_sorted[p[hit]]


def identity(dev, n):
    i = torch.arange(n, dtype=torch.int32, device=dev)
    t = (i, i.clone(), torch.ones(n, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    return capi.device_coo(*ob.ptrs(t), n, (n, n), 0), t


def main():
    ap = ob.parser("poisson,rmat,chain")
    ap.add_argument("--paths", action="store_true")
    a = ap.parse_args()
    dev, stream, ctx = ob.open_context()
    rows = []
    only = a.only.split(",")

    def measure(name, op, call, base, values, before=None):
        """call(): the emult call; base(): its baseline returning (rows, cols, vals) tensors or a Result, or None."""
        res = call()
        got = ob.copy_out(ctx, res, dev)
        same = None
        if base:
            out = base()
            want = out if isinstance(out, tuple) else ob.copy_out(ctx, out, dev)
            same = ob.same(got, want)
            (s, ms_s), (b, ms_b), res, _ = ob.time_pair(stream, call, base, a.reps, a.warmup, before)
        else:
            s, ms_s = ob.time_call(stream, call, a.reps, a.warmup)
        nin, nout = int(res.nnz_a) + int(res.nnz_b), int(res.nnz)
        by = 8.0 * nin + (16.0 + 8.0 * values) * nout
        r = {"workload": name, "impl": "spsamd_emult", "op": op, **ob.times(s, ms_s), "nnz_a": int(res.nnz_a), "nnz_b": int(res.nnz_b),
             "tuples_out": nout, "products": int(res.products), "model_bytes": by, "model_ms_at_8TBps": round(by / ob.PEAK * 1e3, 4),
             "of_model": round(by / ob.PEAK * 1e3 / s, 4)}
        if base:
            r.update({"same_tuples": bool(same), "ratio_to_baseline": round(s / b, 4)})
        ob.record(rows, r)
        if base:
            ob.record(rows, {"workload": name, "impl": "masked_identity" if op != "TIMES" else "torch", "op": op, **ob.times(b, ms_b)})
        if a.paths:
            for p in (1, 2, 3):
                ctx.set_tuning("emult_path", p)
                if before:
                    before()
                m, ms = ob.time_call(stream, call, a.reps, a.warmup)
                ob.record(rows, {"workload": name, "impl": "emult_path=%d" % p, "op": op, **ob.times(m, ms)})
            ctx.set_tuning("emult_path", 0)

    def pair(name, A, tA, B_for_call, Bt, I, torch_base):
        """TIMES and FIRST of op(A) with op(B) = A^T; Bt: what the masked route takes as its mask (A^T's pattern)."""
        measure(name, "TIMES", lambda: ctx.emult(capi.EMULT_TIMES, A, B_for_call, tB='T'), torch_base, 2)
        measure(name, "FIRST", lambda: ctx.emult(capi.EMULT_FIRST, A, B_for_call, tB='T'),
                lambda: ctx.multiply_masked(A, I, Bt), 1)

    def poisson():
        A, t = ob.poisson2d(ctx, dev)
        n = int(A.shape0)
        I, ti = identity(dev, n)
        h = capi.Operand(ctx, A, 'T', capi.AS_A, capi.ADD, False)
        kb, order = torch.sort(keys64(t[1], t[0]))               # A^T's keys; sorted outside the timing, like the handle
        vb = t[2][order]
        tt = (t[1][order].contiguous(), t[0][order].contiguous(), vb)      # A^T row-major, likewise: the masked route's mask
        torch.cuda.synchronize()
        At = capi.device_coo(*ob.ptrs(tt), vb.numel(), (n, n), 0)

        def base():
            with torch.cuda.stream(stream):
                return torch_times(t, kb, vb)
        pair("poisson_AoAT", A, '.', h.coo, At, I, base)
        h.close()

    def rmat20():
        R, raw = ob.rmat(ctx, dev, 20)
        n = int(R.shape0)
        I, ti = identity(dev, n)
        Rt = capi.device_coo(raw[1].data_ptr(), raw[0].data_ptr(), raw[2].data_ptr(), raw[2].numel(), (n, n), -1)

        def base():
            ta = ob.copy_out(ctx, ctx.consolidate(R, 0), dev)
            tb = ob.copy_out(ctx, ctx.consolidate(Rt, 0), dev)
            with torch.cuda.stream(stream):
                return torch_times(ta, keys64(tb[0], tb[1]), tb[2])
        pair("rmat20_AoAT", R, '.', R, Rt, I, base)

    def chain():
        R, raw = ob.rmat(ctx, dev, 16)
        A, ta = ob.consolidated(ctx, dev, R)
        n = int(A.shape0)
        I, ti = identity(dev, n)
        T = ob.square(ctx, R)
        top = capi.result_operand(T)
        measure("chain_first", "FIRST", lambda: ctx.emult(capi.EMULT_FIRST, top, A), lambda: ctx.multiply_masked(top, I, A), 1)
        measure("chain_off", "FIRST|COMPLEMENT", lambda: ctx.emult(capi.EMULT_FIRST, top, A, complement=True), None, 1)

    ob.run(only, [("poisson", poisson), ("rmat", rmat20), ("chain", chain)])
    ob.table(rows, [("workload", -14, "%s", "workload"), ("op", -17, "%s", "op"), ("impl", -16, "%s", "impl"), ("ms", 10, "%.3f", "ms"),
                    ("model ms", 10, "%.3f", "model_ms_at_8TBps"), ("of model", 9, "%.1f%%", ob.pct("of_model")),
                    ("ratio", 8, "%.3f", "ratio_to_baseline"), ("same", 6, "%s", "same_tuples")])
    ob.gate("FIRST faster than multiply_masked(A, I, B); same tuples everywhere",
            [r["workload"] + " " + r["op"] for r in rows if r["impl"] == "spsamd_emult" and "ratio_to_baseline" in r and
             (not r["same_tuples"] or (r["op"] == "FIRST" and r["ratio_to_baseline"] >= 1))])
    ctx.close()


if __name__ == "__main__":
    main()
