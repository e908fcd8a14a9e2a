#!/usr/bin/env python3
"""What the stand-alone operations compute, in a form two builds can be compared by: for select, extract, emult (every
path) and add on R-MAT scale 16 the DIGEST sink's nnz / hash / sum and a SHA-256 of the SINK_COO tuples; for reduce and
multiply_dense a SHA-256 of the output.  One JSON line per call (developer tool).

    python scripts/op_digests.py [root of another checkout of this repository, built]

Two builds agree if every field but `sum` is equal: the DIGEST sum is added with floating-point atomics in no fixed order
and differs in its last bits from run to run of one build."""
import hashlib
import json
import os
import sys

ROOT = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import opbench as ob  # noqa: E402
from opbench import capi  # noqa: E402


def sha(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def main():
    dev, stream, ctx = ob.open_context()
    R, raw = ob.rmat(ctx, dev, 16)
    A, t = ob.consolidated(ctx, dev, R)
    n = int(A.shape0)
    med = float(t[2].abs().median().item())

    def both(name, call):
        r = call(capi.SINK_COO)
        tup = ctx.fetch(r)
        d = call(capi.SINK_DIGEST)
        print(json.dumps({"call": name, "nnz": int(d.nnz), "hash": "%016x" % int(d.hash), "sum": float(d.sum).hex(),
                          "coo_nnz": int(r.nnz), "coo_sha": sha(*tup)}), flush=True)

    for name, pred, ip, dp in (("tril", capi.SELECT_TRIL, -1, 0.0), ("absge", capi.SELECT_ABS_GE, 0, med),
                               ("rowrel", capi.SELECT_ROW_REL, 0, 0.25), ("topk8", capi.SELECT_ROW_TOPK, 8, 0.0)):
        both("select " + name, lambda sink: ctx.select(A, pred, iparam=ip, dparam=dp, sink=sink))
    both("select raw tril", lambda sink: ctx.select(R, capi.SELECT_TRIL, iparam=-1, sink=sink))
    rng = np.random.default_rng(7)
    rows = rng.permutation(n)[: n // 2].astype(np.int32)
    cols = rng.integers(0, n, n // 2).astype(np.int32)
    both("extract perm rows, repeated cols", lambda sink: ctx.extract(A, rows, cols, sink=sink))
    both("extract ascending", lambda sink: ctx.extract(A, np.sort(rows), None, sink=sink))
    for op, comp, nm in ((capi.EMULT_TIMES, False, "TIMES"), (capi.EMULT_FIRST, False, "FIRST"), (capi.EMULT_FIRST, True, "FIRST|COMPLEMENT")):
        for path in (1, 2, 3):
            ctx.set_tuning("emult_path", path)
            both("emult %s A o A^T path %d" % (nm, path), lambda sink: ctx.emult(op, A, A, tB='T', alpha=1.5, complement=comp, sink=sink))
    ctx.set_tuning("emult_path", 0)
    both("add A + 2 A^T", lambda sink: ctx.add(A, A, 1.0, 2.0, tB='T', sink=sink))
    for op, nm in ((capi.REDUCE_SUM, "SUM"), (capi.REDUCE_DIAG, "DIAG"), (capi.REDUCE_COUNT, "COUNT")):
        idx, val = ctx.reduce(A, op)
        print(json.dumps({"call": "reduce " + nm, "nnz": int(len(idx)), "sha": sha(idx, val)}), flush=True)
    X = torch.from_numpy(rng.standard_normal((n, 4))).to(dev)
    Y = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.multiply_dense(A, X, Y)
    torch.cuda.synchronize()
    print(json.dumps({"call": "multiply_dense nrhs 4", "sha": sha(Y.cpu().numpy())}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
