"""Measure spsamd_select (keep op(A)'s tuples by position, size or row top-k) against what a user does without it: composed
torch calls over the same device arrays.

    python scripts/bench_select.py [--only poisson,rmat,raw,galerkin,square] [--reps 7] [--warmup 2]

Workloads (device generators; operands consolidated and handed in as sort0 = 0 device operands unless noted):
  poisson_tril     Poisson 4096^2, TRIL(-1)
  rmat20_*         R-MAT scale 20, consolidated: TRIL(-1), ABS_GE at the median magnitude, ROW_REL 0.25, ROW_TOPK 8 and 32
  rmat20_raw_tril  the same matrix raw (unsorted, duplicates): the consolidation is part of both sides
  galerkin_rowrel  R A R^T on 256^3, the product read in place from the context's output set, ROW_REL 0.25
  square_topk32    A A of R-MAT scale 16, read in place, ROW_TOPK 32
Baseline: tuple-wise and row-relative predicates -- a boolean mask (scatter_reduce amax over the rows for the row maximum)
and boolean indexing of the three arrays; top-k -- two stable sorts (by -|v|, then by row), a rank from the row pointer, the
mask, and a sort back to (row, col) order.  Its tuples are compared with spsamd_select's once per workload.
Times: HIP events on the context's stream, median of --reps after --warmup, select and baseline alternating.
Byte model: 16 B per tuple of S for every pass that reads it (tuple-wise: flag + compact = 2; ROW_REL: row maximum, flag,
compact = 3; ROW_TOPK: row pointer, selection, compact = 3) + 16 B per kept tuple, against 8 TB/s: reported, not gated.
One JSON line per measurement, then a table with the ratio select / baseline (the gate: < 1 everywhere).
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
PASSES = {capi.SELECT_TRIL: 2, capi.SELECT_ABS_GE: 2, capi.SELECT_ROW_REL: 3, capi.SELECT_ROW_TOPK: 3}


def dev_arrays(m, dev):
    return (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
            torch.empty(m, dtype=torch.float64, device=dev))


def ptrs(t):
    return [x.data_ptr() for x in t]


def copy_out(ctx, res, dev):
    """A SINK_COO result in torch tensors of its own."""
    n = int(res.nnz)
    t = dev_arrays(n, dev)
    for x, src, sz in zip(t, (res.idx0, res.idx1, res.val), (4, 4, 8)):
        if n:
            ctx.memcpy(x.data_ptr(), src, n * sz)
    return t


def torch_select(t, nrow, pred, ip, dp):
    """The composed-torch form of one predicate over (rows, cols, vals) sorted row-major."""
    r, c, v = t
    if pred == capi.SELECT_ROW_TOPK:
        n = r.numel()
        o1 = torch.sort(-v.abs(), stable=True).indices
        r1 = r[o1]
        o2 = torch.sort(r1, stable=True).indices
        perm, rs = o1[o2], r1[o2].long()
        counts = torch.bincount(r, minlength=nrow)
        start = torch.cumsum(counts, 0) - counts
        rank = torch.arange(n, device=r.device) - start[rs]
        kept = torch.sort(perm[rank < ip]).values
        return r[kept], c[kept], v[kept]
    if pred == capi.SELECT_TRIL:
        keep = (c - r) <= ip
    elif pred == capi.SELECT_ABS_GE:
        keep = v.abs() >= dp
    else:
        a, rl = v.abs(), r.long()
        m = torch.zeros(nrow, dtype=torch.float64, device=r.device).scatter_reduce(0, rl, a, "amax", include_self=True)
        keep = a >= dp * m[rl]
    return r[keep], c[keep], v[keep]


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="poisson,rmat,raw,galerkin,square")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ctx = capi.Context(0, stream.cuda_stream)
    rows = []
    only = a.only.split(",")

    def measure(name, A, t, nrow, pred, ip=0, dp=0.0, baseline=None):
        """A: the operand of spsamd_select; t: the same tuples as torch tensors for the baseline."""
        sel = lambda: ctx.select(A, pred, iparam=ip, dparam=dp)            # noqa: E731

        def base():
            with torch.cuda.stream(stream):
                return baseline() if baseline else torch_select(t, nrow, pred, ip, dp)
        ms_s, ms_b = [], []
        for rep in range(a.warmup + a.reps):
            m1, res = timed(stream, sel)
            m2, out = timed(stream, base)
            if rep >= a.warmup:
                ms_s.append(m1); ms_b.append(m2)
        got = copy_out(ctx, sel(), dev)              # (a baseline that consolidates writes the output set: select once more)
        same = all(x.numel() == y.numel() for x, y in zip(got, out)) and torch.equal(got[0], out[0]) and \
            torch.equal(got[1], out[1]) and torch.equal(got[2].view(torch.int64), out[2].view(torch.int64))
        nin, nout = int(res.nnz_a), int(res.nnz)
        by = 16.0 * nin * PASSES[pred] + 16.0 * nout
        s, b = float(np.median(ms_s)), float(np.median(ms_b))
        for impl, med, ms in (("spsamd_select", s, ms_s), ("torch", b, ms_b)):
            r = {"workload": name, "impl": impl, "ms": round(med, 4), "ms_all": [round(x, 4) for x in ms], "tuples_in": nin,
                 "tuples_out": nout, "same_tuples": bool(same)}
            if impl == "spsamd_select":
                r.update({"passes": PASSES[pred], "model_bytes": by, "model_ms_at_8TBps": round(by / PEAK * 1e3, 4),
                          "of_model": round(by / PEAK * 1e3 / med, 4), "ratio_to_torch": round(s / b, 4),
                          "rows_light": int(res.rows_light), "rows_mid": int(res.rows_mid), "rows_heavy": int(res.rows_heavy)})
            print(json.dumps(r), flush=True)
            rows.append(r)

    if "poisson" in only:
        N = 4096
        n = N * N
        t = dev_arrays(5 * N * N - 4 * N, dev)
        ctx.gen_poisson2d(N, *ptrs(t))
        torch.cuda.synchronize()
        A = capi.device_coo(*ptrs(t), t[2].numel(), (n, n), 0)
        measure("poisson_tril", A, t, n, capi.SELECT_TRIL, ip=-1)
        del t
        torch.cuda.empty_cache()
    if "rmat" in only or "raw" in only:
        scale = 20
        ne, n = 16 << scale, 1 << scale
        raw = dev_arrays(ne, dev)
        ctx.gen_rmat(scale, 1, 0, ne, *ptrs(raw))
        torch.cuda.synchronize()
        R = capi.device_coo(*ptrs(raw), ne, (n, n), -1)
        t = copy_out(ctx, ctx.consolidate(R, 0), dev)
        A = capi.device_coo(*ptrs(t), t[2].numel(), (n, n), 0)
        if "rmat" in only:
            med = float(t[2].abs().median().item())
            measure("rmat20_tril", A, t, n, capi.SELECT_TRIL, ip=-1)
            measure("rmat20_absge", A, t, n, capi.SELECT_ABS_GE, dp=med)
            measure("rmat20_rowrel", A, t, n, capi.SELECT_ROW_REL, dp=0.25)
            measure("rmat20_topk8", A, t, n, capi.SELECT_ROW_TOPK, ip=8)
            measure("rmat20_topk32", A, t, n, capi.SELECT_ROW_TOPK, ip=32)
        if "raw" in only:
            def raw_base():
                c = copy_out(ctx, ctx.consolidate(R, 0), dev)
                return torch_select(c, n, capi.SELECT_TRIL, -1, 0.0)
            measure("rmat20_raw_tril", R, None, n, capi.SELECT_TRIL, ip=-1, baseline=raw_base)
        del raw, t
        torch.cuda.empty_cache()
    if "galerkin" in only:
        g = 256
        nf, nc = g ** 3, (g // 2) ** 3
        ta, tr = dev_arrays(7 * g ** 3 - 6 * g * g, dev), dev_arrays(nf, dev)
        ctx.gen_laplace3d(g, *ptrs(ta))
        ctx.gen_aggregation3d(g, *ptrs(tr))
        torch.cuda.synchronize()
        A = capi.device_coo(*ptrs(ta), ta[2].numel(), (nf, nf), 0)
        R = capi.device_coo(*ptrs(tr), nf, (nc, nf), 0)
        T = ctx.multiply(R, A)
        G = ctx.multiply(capi.result_operand(T), R, tB='T')
        t = copy_out(ctx, G, dev)
        measure("galerkin_rowrel", capi.result_operand(G), t, nc, capi.SELECT_ROW_REL, dp=0.25)
        del ta, tr, t
        torch.cuda.empty_cache()
    if "square" in only:
        scale = 16
        ne, n = 16 << scale, 1 << scale
        raw = dev_arrays(ne, dev)
        ctx.gen_rmat(scale, 1, 0, ne, *ptrs(raw))
        torch.cuda.synchronize()
        R = capi.device_coo(*ptrs(raw), ne, (n, n), -1)
        P = ctx.multiply(R, R)
        t = copy_out(ctx, P, dev)
        measure("square_topk32", capi.result_operand(P), t, n, capi.SELECT_ROW_TOPK, ip=32)
        del raw, t
        torch.cuda.empty_cache()

    print("%-16s %-14s %10s %10s %9s %8s %6s" % ("workload", "impl", "ms", "model ms", "of model", "ratio", "same"))
    for r in rows:
        if r["impl"] == "spsamd_select":
            print("%-16s %-14s %10.3f %10.3f %8.1f%% %8.3f %6s" % (r["workload"], r["impl"], r["ms"], r["model_ms_at_8TBps"],
                                                                   100 * r["of_model"], r["ratio_to_torch"], r["same_tuples"]))
        else:
            print("%-16s %-14s %10.3f" % (r["workload"], r["impl"], r["ms"]))
    bad = [r["workload"] for r in rows if r["impl"] == "spsamd_select" and (r["ratio_to_torch"] >= 1 or not r["same_tuples"])]
    print("gate (select faster than torch, same tuples):", "holds" if not bad else "MISSED by " + ", ".join(bad))
    ctx.close()


if __name__ == "__main__":
    main()
