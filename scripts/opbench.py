"""What the operation benchmarks (scripts/bench_*.py) share: device arrays and copies, event timing on the context's stream,
the command line, JSON lines, the closing table and gate line, and the device workloads.  A benchmark keeps its docstring, its
baseline, its byte model and its list of workloads, and does `import opbench as ob` (its own directory is sys.path[0]).
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


# ---- device arrays and copies
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


def same(got, want):
    """Two (rows, cols, vals) tensor triples bit for bit: values compare as int64."""
    return all(x.numel() == y.numel() for x, y in zip(got, want)) and torch.equal(got[0], want[0]) and \
        torch.equal(got[1], want[1]) and torch.equal(got[2].view(torch.int64), want[2].view(torch.int64))


# ---- timing: HIP events on the context's stream
def timed(stream, fn):
    """(ms, fn()) of one call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def time_call(stream, fn, reps, warmup):
    """(median ms, [ms]) of `reps` calls after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    ms = [timed(stream, fn)[0] for _ in range(reps)]
    return float(np.median(ms)), ms


def time_pair(stream, call, base, reps, warmup, before=None):
    """`call` and its baseline alternating, call first; before(): run untimed ahead of every repetition (a baseline that
    overwrites the output set the call's operand lives in).  ((median ms, [ms]) of the call, the same of the baseline, and
    what the last call and the last baseline returned)."""
    ms_c, ms_b = [], []
    for rep in range(warmup + reps):
        if before:
            before()
        m1, res = timed(stream, call)
        m2, out = timed(stream, base)
        if rep >= warmup:
            ms_c.append(m1); ms_b.append(m2)
    return (float(np.median(ms_c)), ms_c), (float(np.median(ms_b)), ms_b), res, out


# ---- command line and output
def parser(only, reps=7, warmup=2):
    """--only, --reps and --warmup (warmup None: a script that has none); the script adds its own options."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=only)
    ap.add_argument("--reps", type=int, default=reps)
    if warmup is not None:
        ap.add_argument("--warmup", type=int, default=warmup)
    return ap


def open_context():
    """(device, a stream of its own, a context on that stream)."""
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    return dev, stream, capi.Context(0, stream.cuda_stream)


def record(rows, r):
    """One measurement: a JSON line now, a table line at the end."""
    print(json.dumps(r), flush=True)
    rows.append(r)


def times(med, ms):
    return {"ms": round(med, 4), "ms_all": [round(x, 4) for x in ms]}


def table(rows, cols, other=None):
    """cols: (title, width, format, value) -- a negative width left-justifies; value is a key of the row or a function of it,
    and a cell whose value is None stays blank.  other(r): a whole line for a row that is no measurement ('' drops the row)."""
    def cell(text, w):
        return text.ljust(-w) if w < 0 else text.rjust(w)
    print(" ".join(cell(title, w) for title, w, _, _ in cols))
    for r in rows:
        line = other(r) if other else None
        if line is None:
            vals = [v(r) if callable(v) else r.get(v) for _, _, _, v in cols]
            line = " ".join(cell("" if x is None else f % x, w) for (_, w, f, _), x in zip(cols, vals)).rstrip()
        if line:
            print(line)


def pct(key):
    """A table value: the fraction r[key] as a percentage, None where the row has none."""
    return lambda r: 100 * r[key] if key in r else None


def gate(what, bad):
    print("gate (%s):" % what, "holds" if not bad else "MISSED by " + ", ".join(bad))


def run(only, workloads):
    """workloads: (keys, function) in order; a function runs if one of its space-separated keys is in `only`.  Its tensors are
    its locals, so they are gone when it returns, and the cache is emptied before the next workload allocates."""
    for keys, fn in workloads:
        if any(k in only for k in keys.split()):
            fn()
            torch.cuda.empty_cache()


# ---- device workloads: every builder returns the operand and the tensors that back it (keep them as long as the operand)
def poisson2d(ctx, dev, N=4096, sort0=0):
    """The 5-point Poisson matrix on N^2 points, row-major as generated: (Coo, tensors)."""
    n = N * N
    t = dev_arrays(5 * N * N - 4 * N, dev)
    ctx.gen_poisson2d(N, *ptrs(t))
    torch.cuda.synchronize()
    return capi.device_coo(*ptrs(t), t[2].numel(), (n, n), sort0), t


def rmat(ctx, dev, scale):
    """R-MAT at `scale`, 16 edges per vertex, raw (unsorted, duplicates): (Coo, tensors)."""
    ne, n = 16 << scale, 1 << scale
    raw = dev_arrays(ne, dev)
    ctx.gen_rmat(scale, 1, 0, ne, *ptrs(raw))
    torch.cuda.synchronize()
    return capi.device_coo(*ptrs(raw), ne, (n, n), -1), raw


def consolidated(ctx, dev, R):
    """R consolidated row-major into tensors of its own, as a sort0 = 0 device operand: (Coo, tensors)."""
    t = copy_out(ctx, ctx.consolidate(R, 0), dev)
    return capi.device_coo(*ptrs(t), t[2].numel(), (int(R.shape0), int(R.shape1)), 0), t


def laplace3d(ctx, dev, g=256):
    """The 7-point Laplacian on g^3 points, sort0 = 0: (Coo, tensors)."""
    n = g ** 3
    t = dev_arrays(7 * g ** 3 - 6 * g * g, dev)
    ctx.gen_laplace3d(g, *ptrs(t))
    torch.cuda.synchronize()
    return capi.device_coo(*ptrs(t), t[2].numel(), (n, n), 0), t


def aggregation3d(ctx, dev, g=256):
    """R of the 2x2x2 aggregation of g^3 points, (g/2)^3 x g^3 with one 1.0 per column, sort0 = 0: (Coo, tensors)."""
    nf, nc = g ** 3, (g // 2) ** 3
    t = dev_arrays(nf, dev)
    ctx.gen_aggregation3d(g, *ptrs(t))
    torch.cuda.synchronize()
    return capi.device_coo(*ptrs(t), nf, (nc, nf), 0), t


def galerkin(ctx, A, R):
    """R A R^T chained in place: the result lives in the context's output set until the call after the next."""
    T = ctx.multiply(R, A)
    return ctx.multiply(capi.result_operand(T), R, tB='T')


def square(ctx, R):
    """R R in the context's output set."""
    return ctx.multiply(R, R)
