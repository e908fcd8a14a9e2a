#!/usr/bin/env python3
"""bench.py -- nnz(C)/s of C = A*A on BASELINE.json's cfg2 (R-MAT scale-20, fp64,
~16M tuples) on N MI355X GPUs of one node, plus the dominant kernel's roofline
line; with --full (N=1) also the other configs and the CPU port of the
reference algorithm beside it.

    python bench.py --gpus 1 --steps K --warmup W
    python bench.py --gpus 1 --steps K --warmup W --full      (the headline, then the other configs and the CPU baseline)
    python bench.py --workload poisson|galerkin|rmat [--scale S] [--grid G]     (one other config as the headline)
    python bench.py ... --dump-outputs DIR      (the last timed step's result as DIR/<name>.npy, for comparing builds)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run does only what the headline needs: set up, warm up, time the
steps, dump if asked, print the line.  The roofline line comes from the timed
steps' own kernel timers, so it stays in a plain run.

One step = one pass of the hot path over the whole synthetic matrix:
  N = 1   spsamd_multiply(A, A) from the raw, device-resident COO tuples
          (device consolidate + symbolic + numeric) into the digest sink.
          With --full the JSON line's `other_configs` object carries, measured
          in the same run after the headline (fewer steps each): cfg3 (Poisson
          4096^2, digest and COO sinks), cfg5 (Galerkin R*A*R^T on 256^3, two
          chained COO multiplies), cfg4 on one GPU (R-MAT scale-23), cfg2 into
          the COO sink, the prepared-operand variants and the PCIe-inclusive
          host delivery rate; `cpu_baseline` carries the CPU port.
          --no-other-configs and --no-cpu-baseline drop either from --full.
  N > 1   strong scaling on the same matrix: every rank owns a contiguous row
          block of the raw tuples; a step = spsamd_dist_multiply (C ABI):
          consolidate the own block, exchange the needed B row panels with
          grouped ncclSend / ncclRecv (RCCL), multiply the block against its
          panel.  C stays row partitioned (no reduction).  The block
          boundaries are setup: a per-row cost estimate first, then --calibrate
          rounds of (run the step, gather every rank's local time, move the
          boundaries so the measured times come out equal); they are fixed
          before the warmup and timed steps.
The digest sink (count + value sum + index hash of the emitted tuples) is the
device analogue of the reference's ScalarAccumulator (accum.hpp:158-167):
nnz(C) ~ 9.7e9 tuples (155 GB) is never materialised in the headline run.
Inputs are generated in HBM before the timed region; nothing crosses PCIe
inside it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md)
PMC_FILE = os.path.join("profiles", "r03", "pmc_traffic.json")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=int, default=20, help="R-MAT scale (cfg2 = 20, cfg4 = 23)")
    ap.add_argument("--workload", choices=["rmat", "poisson", "galerkin"], default="rmat",
                    help="rmat: cfg2/cfg4 (the benchmarked line); poisson: cfg3, the 2-D 5-point stencil on a --grid x --grid "
                         "mesh; galerkin: cfg5, R*A*R^T on the 7-point Laplacian of a --grid^3 mesh (default 256)")
    ap.add_argument("--grid", type=int, default=0, help="mesh size of --workload poisson (cfg3 = 4096) / galerkin (cfg5 = 256)")
    ap.add_argument("--sink", choices=["digest", "coo"], default="digest", help="N=1: the sink of the timed multiply")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--prepared", action="store_true",
                    help="N=1: the operands are prepared once before the timed steps (spsamd_operand_prepare); not the headline, "
                         "which starts from the raw tuples every step")
    ap.add_argument("--full", action="store_true",
                    help="N=1, default workload: after the headline also measure the other configs and the CPU baseline "
                         "(off: the run does only what the headline needs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-other-configs", action="store_true", help="with --full: skip the other configs")
    ap.add_argument("--cpu-scale", type=int, default=15, help="R-MAT scale of the bounded CPU sample (scale 15: ~25 s on one core)")
    ap.add_argument("--calibrate", type=int, default=3,
                    help="N>1 setup: measure/rebalance rounds of the row-block boundaries (0: cost estimate only)")
    ap.add_argument("--rehearse-gloo", action="store_true",
                    help="N>1 rehearsal on ONE GPU: every rank uses cuda:0, collectives run over gloo on host copies "
                         "(exercises the multi-rank logic where only one GPU is available; not a measurement)")
    ap.add_argument("--dist-path", action="store_true",
                    help="with --gpus 1: run the row-block + all-to-allv path on a 1-rank group (rehearsal of the N>1 code)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy "
                         "(float64): the digest, or for the COO sink nnz(C) and a fixed seeded sample of C's tuples")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    return args


# ------------------------------------------------------------------------------------------ --dump-outputs

DUMP_MAX_BYTES = 64 << 20      # all files of one dump together
DUMP_BLOCK = 1024              # COO sink: C is sampled in runs of this many consecutive (row-major) tuples ...
DUMP_BLOCKS = 1024             # ... this many runs at most (1M tuples, 32 MB as four float64 arrays)
DUMP_SEED = 12345              # which runs: fixed, so that two builds are sampled at the same positions


def digest_arrays(nnz, vsum, vhash):
    """The digest sink's answer (count, value sum, index hash); the 64-bit hash as two exact 32-bit halves."""
    import numpy as np
    vhash = int(vhash)
    return {"nnz_c": np.array([int(nnz)], np.float64), "digest_sum": np.array([float(vsum)], np.float64),
            "digest_hash": np.array([vhash >> 32, vhash & 0xffffffff], np.float64)}


def coo_arrays(ctx, res):
    """A COO-sink result: nnz(C), its shape, and C's tuples -- all of them up to DUMP_BLOCK * DUMP_BLOCKS, beyond that
    DUMP_BLOCKS runs of DUMP_BLOCK consecutive tuples at seeded positions -- with the position of every sampled tuple."""
    import numpy as np
    n = int(res.nnz)
    nblk = -(-n // DUMP_BLOCK)
    if nblk <= DUMP_BLOCKS:
        blocks = np.arange(nblk, dtype=np.int64)
    else:
        blocks = np.sort(np.random.default_rng(DUMP_SEED).choice(nblk, DUMP_BLOCKS, replace=False))
    pos, rows, cols, vals = [], [], [], []
    for b in blocks.tolist():
        lo = b * DUMP_BLOCK
        cnt = min(DUMP_BLOCK, n - lo)
        pos.append(np.arange(lo, lo + cnt, dtype=np.int64))
        rows.append(ctx.to_host(res.idx0 + 4 * lo, cnt, np.int32))
        cols.append(ctx.to_host(res.idx1 + 4 * lo, cnt, np.int32))
        vals.append(ctx.to_host(res.val + 8 * lo, cnt, np.float64))

    def cat(parts):
        return np.concatenate(parts).astype(np.float64) if parts else np.zeros(0, np.float64)
    return {"nnz_c": np.array([n], np.float64), "c_shape": np.array([int(res.shape0), int(res.shape1)], np.float64),
            "c_pos": cat(pos), "c_row": cat(rows), "c_col": cat(cols), "c_val": cat(vals)}


def write_dump(dirname, arrays):
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise RuntimeError("--dump-outputs: %d bytes exceed the %d byte limit" % (total, DUMP_MAX_BYTES))
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), name
        np.save(os.path.join(dirname, name + ".npy"), a)


def cpu_baseline(scale, seed):
    """The CPU port of the reference algorithm (oracle/spsparse_oracle.c,
    orc_multiply_mm: sorted rows x sorted columns, leap-frog merge joins --
    multiply_sparse.hpp:192-246) timed on one host core on a bounded sample of
    the same workload.  Reported beside the GPU number, never the target.
    Also timed: the same port on cfg1, and the row-wise
    checker at one thread and at every host core."""
    os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")      # idle OpenMP workers sleep instead of spinning until exit
    from oracle import binding as orc
    from spsparse_amd import workloads as wl
    A = orc.Mat(*wl.rmat(scale, seed))
    t = time.time()
    i, j, v, _ = orc.multiply(A, A)
    dt = time.time() - t
    t = time.time()
    i2, _, _, _ = orc.multiply(A, A, rowwise=True)
    dt2 = time.time() - t
    assert len(i) == len(i2)
    # the honest "good CPU algorithm" figure: the row-wise checker as a streaming digest, rows handed out
    # dynamically to every host core this process may use, on a larger sample (R-MAT scale 18: 2.9e9 products)
    ncores = orc.host_threads(cap=256)
    A18 = orc.Mat(*wl.rmat(18, seed))
    t = time.time()
    d18 = orc.multiply_digest(A18, A18, nthreads=ncores)
    dt3 = time.time() - t
    a1, b1 = wl.random_rows(1000, 10, seed=1), wl.random_rows(1000, 10, seed=2)
    A1, B1 = orc.Mat(*a1), orc.Mat(*b1)
    t = time.time()
    c1 = orc.multiply(A1, B1)
    dt1 = time.time() - t
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"value": len(v) / dt, "unit": "nnz(C)/s", "cores": 1, "kind": "port",
            "sample": "R-MAT scale-%d A*A (same generator, %d tuples -> nnz(C)=%d) in %.1f s; the reference's "
                      "inner-product algorithm is Theta(rows*cols): extrapolated to scale-20 it needs days" % (scale, A.nnz, len(v), dt),
            "rowwise_port_value": len(v) / dt2,
            "rowwise_port_all_cores_value": d18.nnz / dt3, "rowwise_port_all_cores_products_per_s": d18.products / dt3,
            "rowwise_port_all_cores_sample": "R-MAT scale-18 A*A, streaming digest, dynamic row schedule, %d threads: nnz(C)=%d in %.2f s" % (ncores, d18.nnz, dt3),
            "host_cores": ncores, "cpu_model": model,
            "cfg1_value": len(c1[2]) / dt1, "cfg1_sample": "1k x 1k, 10 tuples per row, A*B: nnz(C)=%d in %.3f s" % (len(c1[2]), dt1)}


# ------------------------------------------------------------------------------------------ N = 1 workloads

class Workload:
    """Device-resident operands of one BASELINE config and its step."""

    def __init__(self, torch, capi, ctx, dev, kind, scale=20, grid=0, seed=1, sink="digest", prepared=False):
        self.torch, self.capi, self.ctx, self.kind = torch, capi, ctx, kind
        self.handles = []
        self.sink = capi.SINK_COO if sink == "coo" else capi.SINK_DIGEST
        self.sink_name = sink

        def bufs(m):
            return (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
                    torch.empty(m, dtype=torch.float64, device=dev))

        def ptrs(t):
            return [x.data_ptr() for x in t]

        if kind == "rmat":
            self.n, self.ne = 1 << scale, 16 << scale
            self.t = bufs(self.ne)
            ctx.gen_rmat(scale, seed, 0, self.ne, *ptrs(self.t))
            self.A = capi.device_coo(*ptrs(self.t), self.ne, (self.n, self.n))
            self.name = ("R-MAT scale-%d A*A (Graph500 a,b,c,d=0.57,0.19,0.19,0.05, edge factor 16, seed %d), fp64, "
                         "raw COO tuples resident in HBM, %s sink" % (scale, seed, sink))
            self.workspace = int(self.ne * 220) + (512 << 20)
        elif kind == "poisson":
            g = grid or 4096
            self.n, self.ne = g * g, 5 * g * g - 4 * g
            self.t = bufs(self.ne)
            ctx.gen_poisson2d(g, *ptrs(self.t))
            self.A = capi.device_coo(*ptrs(self.t), self.ne, (self.n, self.n))
            self.name = "2-D 5-point Poisson stencil on a %dx%d mesh, A*A, fp64, COO tuples resident in HBM, %s sink" % (g, g, sink)
            self.workspace = int(self.ne * 220) + (512 << 20)
        else:
            g = grid or 256
            nc = g // 2
            self.n = nc ** 3
            na = 7 * g ** 3 - 6 * g ** 2
            self.ne = na + g ** 3
            self.t = bufs(na)
            self.t2 = bufs(g ** 3)
            ctx.gen_laplace3d(g, *ptrs(self.t))
            ctx.gen_aggregation3d(g, *ptrs(self.t2))
            self.A = capi.device_coo(*ptrs(self.t), na, (g ** 3, g ** 3), sort0=0)
            self.R = capi.device_coo(*ptrs(self.t2), g ** 3, (nc ** 3, g ** 3), sort0=0)
            self.sink, self.sink_name = capi.SINK_COO, "coo"
            self.name = ("Galerkin triple product R*A*R^T, 7-point Laplacian on a %d^3 mesh, 2x2x2 aggregation, fp64: T = R*A into "
                         "the COO sink, C = T*R^T reading T in place (chained result buffers), COO sink" % g)
            self.workspace = int(na * 260) + (512 << 20)
        torch.cuda.synchronize()
        if prepared:
            # every operand prepared ONCE (spsamd_operand_prepare): what a caller that multiplies with the same matrices again and
            # again pays per product -- no inspection / consolidation / row pointers / window indices per step
            def prep(coo, transpose, role):
                h = capi.Operand(ctx, coo, transpose, role)
                self.handles.append(h)
                return h.coo
            if kind == "galerkin":
                self.Rt = prep(self.R, 'T', capi.AS_B)
                self.R = prep(self.R, '.', capi.AS_A)
                self.A = prep(self.A, '.', capi.AS_B)
            else:
                self.A = prep(self.A, '.', capi.AS_A | capi.AS_B)
            self.name += ", operands prepared once (spsamd_operand_prepare)"

    def step(self):
        """One pass; returns the list of spsamd_result of its multiplies (one, or two for galerkin)."""
        capi, ctx = self.capi, self.ctx
        if self.kind == "galerkin":
            rt = ctx.multiply(self.R, self.A, sink=capi.SINK_COO)
            rc = ctx.multiply(capi.result_operand(rt), getattr(self, "Rt", self.R), tB="T", sink=capi.SINK_COO)
            return [rt, rc]
        return [ctx.multiply(self.A, self.A, sink=self.sink, flags=getattr(self, "flags", 0))]

    def release(self):
        for h in self.handles:
            h.close()
        self.handles = []
        self.t = self.t2 = None
        self.torch.cuda.empty_cache()


def run_workload(torch, w, steps, warmup):
    """warmup + timed steps of one workload on one GPU; returns the summary dict and the per-step results."""
    # setup: size the library's workspace so that no timed step allocates device memory -- a first estimate, one
    # untimed sizing call, then one slab of what that call really used (the window indices of the heavy-row path
    # grow with rows x windows: 190 B per raw tuple at R-MAT scale 20, 380 B at scale 23)
    w.ctx.reserve(w.workspace)
    used = max(int(r.workspace_bytes) for r in w.step())
    w.ctx.reserve(max(w.workspace, int(used * 1.08) + (256 << 20)))
    for _ in range(warmup):
        w.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    results = [w.step() for _ in range(steps)]
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    last = results[-1]
    ms_step = elapsed / steps * 1e3
    nnz_c = int(last[-1].nnz)
    read_alg = sum(16 * int(r.nnz_a) + 12 * int(r.products) for r in last)
    write_alg = sum(16 * int(r.nnz) for r in last) if w.sink_name == "coo" else 0
    out = {
        "workload": w.name, "steps": steps, "warmup": warmup, "ms_per_step": ms_step,
        "nnz_c_per_s": nnz_c / (ms_step * 1e-3),
        "n": w.n, "raw_tuples": w.ne,
        "nnz_a": [int(r.nnz_a) for r in last], "nnz_b": [int(r.nnz_b) for r in last],
        "products": [int(r.products) for r in last], "nnz_c": [int(r.nnz) for r in last],
        "read_alg_bytes": read_alg, "read_alg_GBps": read_alg / (ms_step * 1e-3) / 1e9,
        "read_alg_frac_of_hbm_peak": read_alg / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBPS,
        "read_write_alg_GBps": (read_alg + write_alg) / (ms_step * 1e-3) / 1e9,
        "stage_ms": [{"consolidate": r.ms_consolidate, "symbolic": r.ms_symbolic, "numeric": r.ms_numeric, "light": r.ms_light,
                      "mid": r.ms_mid, "heavy_hash_cells": r.ms_heavy - r.ms_dense, "heavy_dense_cells": r.ms_dense,
                      "total_device": r.ms_total} for r in last],
        "window": int(last[0].window), "workspace_GB": max(int(r.workspace_bytes) for r in last) / 1e9,
    }
    if w.sink_name == "digest":
        out["digest"] = {"sum": float(last[0].sum), "hash": "%016x" % int(last[0].hash)}
    return out, results


def pcie_delivery(torch, capi, ctx, dev, scale, seed):
    """PCIe-inclusive host delivery of a COO result (never `value`): R-MAT scale-`scale` A*A, host COO in ->
    spsamd_multiply -> spsamd_result_fetch into host arrays; nnz(C)/s end to end."""
    import numpy as np
    from spsparse_amd import workloads as wl
    a = wl.rmat(scale, seed)
    s, keep = capi.host_coo(*a)
    ctx.multiply(s, s, sink=capi.SINK_COO)           # warm: workspace, output buffers
    t0 = time.perf_counter()
    res = ctx.multiply(s, s, sink=capi.SINK_COO)
    t1 = time.perf_counter()
    gi, gj, gv = ctx.fetch(res)
    t2 = time.perf_counter()
    return {"sample": "R-MAT scale-%d A*A, host operands, COO sink fetched into host arrays" % scale, "nnz_c": int(res.nnz),
            "multiply_with_h2d_ms": (t1 - t0) * 1e3, "fetch_ms": (t2 - t1) * 1e3,
            "fetch_GBps": int(res.nnz) * 16 / (t2 - t1) / 1e9, "end_to_end_nnz_c_per_s": int(res.nnz) / (t2 - t0)}


def spawn_ranks(args):
    """`python bench.py --gpus N` outside torch.distributed.run: start the N ranks as fresh child processes
    (nothing in THIS process has touched the GPU or imported torch), relay rank 0's JSON line and the launcher's
    return code.  Never a re-exec: the children are ordinary subprocesses of a parent that stays GPU-free."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in p.stdout:
        if ln.startswith("{"):
            line = ln.rstrip("\n")
        else:
            sys.stderr.write(ln)
    rc = p.wait()
    if line is not None:
        print(line, flush=True)
    if rc == 0 and line is None:
        sys.stderr.write("bench.py: the ranks ended without a result line\n")
        rc = 1
    sys.exit(rc)


def main():
    args = parse()
    if args.dump_outputs and args.workload == "galerkin" and (args.gpus > 1 or args.dist_path):
        raise SystemExit("--dump-outputs: the sharded Galerkin step leaves C's tuples spread over the ranks; dump it with --gpus 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)
    # dmabuf IPC for RCCL: must be in the environment before the HIP runtime starts
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    from spsparse_amd import capi
    from spsparse_amd import dist as sd

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d does not match WORLD_SIZE %d" % (args.gpus, world))
    if args.rehearse_gloo:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.dist_path
    coll_dev = torch.device("cpu") if args.rehearse_gloo else dev      # where the collectives' tensors live
    if use_dist:
        if args.rehearse_gloo:
            dist.init_process_group("gloo")
        elif world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        else:
            dist.init_process_group("nccl", device_id=dev)

    # one explicit HIP stream for everything: torch tensor ops, RCCL collectives and the
    # library's kernels stay ordered on it (torch's default stream is the NULL handle,
    # which the C ABI reads as "create a private stream")
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    ctx = capi.Context(local_rank, stream.cuda_stream)
    scale, seed = args.scale, args.seed

    if not use_dist:
        line = single_gpu(args, torch, capi, ctx, dev, stream)
        print(json.dumps(line), flush=True)
        ctx.close()
        return

    if args.rehearse_gloo:
        dd = capi.Dist(ctx, rank, world, transport=sd.host_transport(ctx, world))
    else:
        # the communicator is the library's own, created from a unique id that rank 0 hands out through torch.distributed
        uid = [capi.Dist.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        dd = capi.Dist(ctx, rank, world, unique_id=uid[0])

    def barrier():
        dist.barrier()
        torch.cuda.synchronize()

    if args.workload == "galerkin":
        line = galerkin_sharded(args, torch, dist, capi, sd, ctx, dd, dev, coll_dev, rank, world, barrier)
        if rank == 0:
            print(json.dumps(line), flush=True)
        dd.close()
        ctx.close()
        dist.destroy_process_group()
        return
    if args.workload == "poisson":
        g = args.grid or 4096
        n, ne = g * g, 5 * g * g - 4 * g
        wname = "2-D 5-point Poisson stencil on a %dx%d mesh, A*A, fp64, COO tuples resident in HBM, digest sink" % (g, g)
    else:
        n, ne = 1 << scale, 16 << scale
        wname = ("R-MAT scale-%d A*A (Graph500 a,b,c,d=0.57,0.19,0.19,0.05, edge factor 16, seed %d), fp64, "
                 "raw COO tuples resident in HBM, digest sink" % (scale, seed))

    def gen_all():
        t0 = torch.empty(ne, dtype=torch.int32, device=dev)
        t1 = torch.empty(ne, dtype=torch.int32, device=dev)
        tv = torch.empty(ne, dtype=torch.float64, device=dev)
        if args.workload == "poisson":
            ctx.gen_poisson2d(args.grid or 4096, t0.data_ptr(), t1.data_ptr(), tv.data_ptr())
        else:
            ctx.gen_rmat(scale, seed, 0, ne, t0.data_ptr(), t1.data_ptr(), tv.data_ptr())
        return t0, t1, tv

    def consolidated(coo):
        """device consolidate -> torch tensors (row, col, val)   (setup only)"""
        r = ctx.consolidate(coo, 0)
        m = int(r.nnz)
        o0 = torch.empty(m, dtype=torch.int32, device=dev)
        o1 = torch.empty(m, dtype=torch.int32, device=dev)
        ov = torch.empty(m, dtype=torch.float64, device=dev)
        ctx.memcpy(o0.data_ptr(), r.idx0, m * 4)
        ctx.memcpy(o1.data_ptr(), r.idx1, m * 4)
        ctx.memcpy(ov.data_ptr(), r.val, m * 8)
        return o0, o1, ov

    raw0, raw1, rawv = gen_all()
    torch.cuda.synchronize()
    # setup: pre-size the library's workspace (about 170 B per raw tuple at these sizes) so that
    # no timed step -- not even the first one when --warmup 0 -- allocates device memory
    ctx.reserve(int(ne * 220) + (512 << 20))
    # setup (untimed): contiguous row blocks equal in estimated time, identical on every rank ...
    c0, c1, cv = consolidated(capi.device_coo(raw0.data_ptr(), raw1.data_ptr(), rawv.data_ptr(), ne, (n, n)))
    rowlen = torch.bincount(c0.long(), minlength=n)
    P = sd.row_products(c0, c1, rowlen, n)
    cost = sd.row_cost(P)
    cost_prefix = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(cost, 0)])
    bounds = sd.product_balanced_bounds(cost, world)
    del c0, c1, cv, P, rowlen, cost

    # the step itself lives behind the C ABI (spsamd_dist_multiply): consolidate the own block, exchange the needed
    # B row panels with grouped ncclSend / ncclRecv, multiply.

    def take_block(b):
        keep = (raw0 >= b[rank]) & (raw0 < b[rank + 1])
        return raw0[keep].contiguous(), raw1[keep].contiguous(), rawv[keep].contiguous()

    def run_block(blk):
        """One step on this rank's block; also returns the device time of its local part (the block product,
        without the exchange, where a rank also waits for the slowest one)."""
        blk0, blk1, blkv = blk
        Ab = capi.device_coo(blk0.data_ptr(), blk1.data_ptr(), blkv.data_ptr(), blk0.numel(), (n, n))
        res, st = dd.multiply(Ab, None, bounds_now[0], sink=capi.SINK_DIGEST)
        return res, int(st.remote_tuples), float(res.ms_total)

    # ... then corrected by measurement: run the step, gather every rank's local time, move the
    # boundaries so that the measured times come out equal (sd.rebalance_bounds), repeat.
    bounds_now = [bounds]
    calib = []
    for _ in range(max(0, args.calibrate)):
        blk = take_block(bounds_now[0])
        run_block(blk)
        local_ms = min(run_block(blk)[2] for _ in range(3))        # best of three: the timer noise is about 1 ms
        mine = torch.tensor([local_ms], dtype=torch.float64, device=coll_dev)
        every = [torch.empty(1, dtype=torch.float64, device=coll_dev) for _ in range(world)]
        dist.all_gather(every, mine)
        times = [float(x[0]) for x in every]
        calib.append([round(x, 2) for x in times])
        bounds_now[0] = sd.rebalance_bounds(bounds_now[0], cost_prefix, times, min_gain=0.015)
        del blk
    bounds = bounds_now[0]
    block = take_block(bounds)
    del raw0, raw1, rawv, cost_prefix
    torch.cuda.empty_cache()

    def step():
        res, remote, _ = run_block(block)
        return res, remote

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    results = []
    for _ in range(args.steps):
        results.append(step())
    barrier()
    elapsed = time.perf_counter() - t0

    res, remote = results[-1]
    tmax = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = float(tmax[0])
    stats = torch.tensor([res.nnz_a, res.products, remote], dtype=torch.int64, device=coll_dev)
    dist.all_reduce(stats)
    nnz_a, products, remote_total = [int(x) for x in stats.tolist()]
    nnz_c, vsum, vhash = sd.reduce_digest(int(res.nnz), float(res.sum), int(res.hash), coll_dev)

    if rank == 0:
        if args.dump_outputs:
            write_dump(args.dump_outputs, digest_arrays(nnz_c, vsum, vhash))
        ms_step = elapsed / args.steps * 1e3
        line = headline(args, world, wname, n, ne, nnz_a, products, nnz_c, vsum, vhash, ms_step, elapsed,
                        [r[0] for r in results], remote_total, calib,
                        "%d row blocks (per-row cost estimate, then %d measure/rebalance rounds) + all-to-allv of B row panels" % (world, len(calib)))
        print(json.dumps(line), flush=True)
    dd.close()
    ctx.close()
    dist.destroy_process_group()


def galerkin_sharded(args, torch, dist, capi, sd, ctx, dd, dev, coll_dev, rank, world, barrier):
    """cfg5 on N ranks (BASELINE: 2): the Galerkin triple product R*A*R^T of the 7-point Laplacian on a g^3 mesh, 2x2x2
    aggregation, cut along z planes: rank q owns the coarse planes [zc_q, zc_q+1) -- its rows of R, T and C -- and the
    fine planes under them -- its rows of A and its tuples of R^T.  T = R*A needs no remote row of A (the fine cells of
    an aggregate lie in the rank's own planes); C = T*R^T needs the R^T rows of one fine plane on either side (SURVEY
    8e).  Both products are spsamd_dist_multiply; T is chained from the first into the second in place."""
    g = args.grid or 256
    nc = g // 2
    na = 7 * g ** 3 - 6 * g ** 2
    nr = g ** 3

    def bufs(m):
        return (torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.int32, device=dev),
                torch.empty(m, dtype=torch.float64, device=dev))
    ta, tr = bufs(na), bufs(nr)
    ctx.gen_laplace3d(g, *[x.data_ptr() for x in ta])
    ctx.gen_aggregation3d(g, *[x.data_ptr() for x in tr])
    torch.cuda.synchronize()
    zc = [nc * q // world for q in range(world + 1)]                  # coarse planes per rank
    bounds_c = [z * nc * nc for z in zc]                             # rows of R / T / C
    bounds_f = [2 * z * g * g for z in zc]                           # rows of A = inner index of R*A; columns of R = inner index of T*R^T

    def take(t, dim, lo, hi):
        keep = (t[dim] >= lo) & (t[dim] < hi)
        return tuple(x[keep].contiguous() for x in t)
    Rrows = take(tr, 0, bounds_c[rank], bounds_c[rank + 1])          # A_block of R*A
    Arows = take(ta, 0, bounds_f[rank], bounds_f[rank + 1])          # B_block of R*A: op(B) = A, rows = fine cells
    Rcols = take(tr, 1, bounds_f[rank], bounds_f[rank + 1])          # B_block of T*R^T: op(B) = R^T, rows = fine cells = R's columns
    del ta, tr
    torch.cuda.empty_cache()
    shapeA, shapeR = (g ** 3, g ** 3), (nc ** 3, g ** 3)

    def coo(t, shape, sort0=0):
        return capi.device_coo(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[0].numel(), shape, sort0)
    Rb, Ab, Rc = coo(Rrows, shapeR), coo(Arows, shapeA), coo(Rcols, shapeR, sort0=-1)
    ctx.reserve(int((na + nr) // world * 300) + (512 << 20))

    def step(sink2=capi.SINK_COO):
        rt, st1 = dd.multiply(Rb, Ab, bounds_f, sink=capi.SINK_COO)
        rc, st2 = dd.multiply(capi.result_operand(rt), Rc, bounds_f, tB="T", sink=sink2)
        return rt, rc, int(st1.remote_tuples) + int(st2.remote_tuples)

    step()
    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    results = [step() for _ in range(args.steps)]
    barrier()
    elapsed = time.perf_counter() - t0
    tmax = torch.tensor([elapsed], dtype=torch.float64, device=coll_dev)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    elapsed = float(tmax[0])
    rt, rc, remote = results[-1]
    # untimed: the same second product into the digest sink, for the whole-job digest of C
    _, rd, _ = step(capi.SINK_DIGEST)
    stats = torch.tensor([rt.nnz_a, rt.products, rt.nnz, rc.products, rc.nnz, remote], dtype=torch.int64, device=coll_dev)
    dist.all_reduce(stats)
    nnz_r, p1, nnz_t, p2, nnz_c, remote_total = [int(x) for x in stats.tolist()]
    cnt, vsum, vhash = sd.reduce_digest(int(rd.nnz), float(rd.sum), int(rd.hash), coll_dev)
    assert cnt == nnz_c
    ms_step = elapsed / args.steps * 1e3
    read_alg = 16 * nnz_r + 12 * p1 + 16 * nnz_t + 12 * p2
    return {
        "metric": "nnz(C)/s for C=R*A*R^T (two chained SpGEMMs)", "value": nnz_c * args.steps / elapsed, "unit": "nnz(C)/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step, "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {
            "workload": "Galerkin triple product R*A*R^T, 7-point Laplacian on a %d^3 mesh, 2x2x2 aggregation, fp64, cut along z planes: "
                        "T = R*A (no remote rows), C = T*R^T reading T in place (one-plane halo of R^T), COO sinks" % g,
            "parallelism": "%d row blocks of R / T / C at coarse z planes, A and R^T at the fine planes under them + all-to-allv of "
                           "needed B row panels (spsamd_dist_multiply with 'T' for R^T)" % world,
            "sink": "coo", "sink_flags": 0,
            "nnz_r": nnz_r, "nnz_t": nnz_t, "nnz_c": nnz_c, "products": [p1, p2], "remote_panel_tuples": remote_total,
            "digest": {"sum": vsum, "hash": "%016x" % vhash},
            "read_alg_GBps": read_alg / (ms_step * 1e-3) / 1e9,
            "read_alg_frac_of_hbm_peak": read_alg / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBPS,
        },
    }


def roofline_of(args, world, results, scale_is_cfg2):
    """Dominant kernel of rank 0 = the numeric kernel with the largest duration (ties within 3 %: the one with more
    algorithmic bytes), timed with HIP events on the library's stream in every step.  Algorithmic bytes of one launch = 12 B per scalar product it
    processes + 16 B per A tuple of its rows."""
    res = results[-1]

    def avg(f):
        return sum(f(r) for r in results) / len(results)
    t_heavy = max(1, res.products_heavy)
    p_win = res.products_heavy - res.products_dense - res.products_tiles - res.products_direct     # windowed k_hash (rows with > 256 A tuples)

    def tup(p):                                     # A tuples attributed in proportion to the products
        return res.tuples_heavy * p / t_heavy
    kernels = [
        ("k_dense", avg(lambda r: r.ms_dense), res.products_dense, tup(res.products_dense)),
        ("k_bm_tiles|k_hash_tiles2", avg(lambda r: r.ms_tiles), res.products_tiles, tup(res.products_tiles)),
        ("k_direct_tiles", avg(lambda r: r.ms_direct), res.products_direct, tup(res.products_direct)),
        ("k_hash(window cells)", avg(lambda r: r.ms_heavy - r.ms_dense - r.ms_tiles - r.ms_direct), p_win, tup(p_win)),
        ("k_hash(rows)", avg(lambda r: r.ms_mid), res.products_mid, res.tuples_mid),
        ("k_light", avg(lambda r: r.ms_light), res.products_light, res.tuples_light),
    ]
    # dominant = longest; kernels within 3 % of the longest count as tied (k_dense and the tile kernel took 32.5 and 32.2 ms
    # of a cfg2 step in round 2; 28.1 and 31.9 since round 3) and the tie goes to the one that moves more algorithmic bytes, so that the headline figure does not
    # flip between two kernels with the run-to-run noise.  all_kernels lists every kernel either way.
    t_max = max(k[1] for k in kernels)
    name, ms_kernel, k_prod, k_tup = max((k for k in kernels if k[1] >= 0.97 * t_max), key=lambda k: 16 * k[3] + 12 * k[2])
    alg_bytes = int(16 * k_tup + 12 * k_prod)
    achieved = alg_bytes / (ms_kernel * 1e-3) / 1e9 if ms_kernel > 0 else 0.0
    # HBM-side bytes per launch: bench.py cannot run the profiler on itself, so this is the figure of the
    # committed rocprofv3 --pmc passes of this same command (file and commit named beside it); null when no
    # pass covers the kernel.  It is a constant of that profiled run, NOT a measurement of this run.
    traffic, source = None, None
    try:
        with open(os.path.join(ROOT, PMC_FILE)) as f:
            pmc = json.load(f)
        if scale_is_cfg2 and world == 1 and name in pmc["kernels"]:
            traffic = pmc["kernels"][name]["traffic_bytes_per_launch"]
            source = "%s (rocprofv3 --pmc passes of `%s`, build %s; constant of that run)" % (
                PMC_FILE, pmc.get("command", "python bench.py"), pmc.get("commit", "?"))
    except (OSError, KeyError, ValueError):
        traffic = None
    # (the kernel that moves the most algorithmic bytes, named beside the longest one: since round 3 they are two kernels)
    big = max(kernels, key=lambda k: 16 * k[3] + 12 * k[2])
    big_bytes = 16 * big[3] + 12 * big[2]
    return {"bound": "hbm", "kernel": name, "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic, "traffic_source": source,
            "alg_bytes_per_launch": alg_bytes, "ms_per_launch": ms_kernel,
            "most_bytes_kernel": {"kernel": big[0], "ms_per_launch": big[1], "alg_bytes_per_launch": int(big_bytes),
                                  "frac": big_bytes / (big[1] * 1e-3) / 1e9 / HBM_PEAK_GBPS if big[1] > 0 else None},
            "all_kernels": {k[0]: {"ms": k[1], "products": int(k[2]),
                                   "frac": (16 * k[3] + 12 * k[2]) / (k[1] * 1e-3) / 1e9 / HBM_PEAK_GBPS if k[1] > 0 else None} for k in kernels}}


def headline(args, world, wname, n, ne, nnz_a, products, nnz_c, vsum, vhash, ms_step, elapsed, results, remote_total, calib, par):
    res = results[-1]
    return {
        "metric": "nnz(C)/s for C=A*A SpGEMM",
        "value": nnz_c * args.steps / elapsed,
        "unit": "nnz(C)/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_step,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": wname,
            "n": n, "raw_tuples": ne, "nnz_a": nnz_a, "products": products, "nnz_c": nnz_c,
            "parallelism": par,
            "sink": args.sink if world == 1 else "digest", "sink_flags": 0,
            "remote_panel_tuples": remote_total,
            "calibration_local_ms": calib,
            "digest": {"sum": vsum, "hash": "%016x" % vhash},
            "read_alg_GBps": (16 * nnz_a + 12 * products) / (ms_step * 1e-3) / 1e9,
            "read_alg_frac_of_hbm_peak": (16 * nnz_a + 12 * products) / (ms_step * 1e-3) / 1e9 / HBM_PEAK_GBPS,
            "products_per_s": products / (ms_step * 1e-3),
            "stage_ms_rank0": {"consolidate": res.ms_consolidate, "symbolic": res.ms_symbolic, "numeric": res.ms_numeric,
                               "light": res.ms_light, "mid": res.ms_mid, "heavy_hash_cells": res.ms_heavy - res.ms_dense,
                               "heavy_dense_cells": res.ms_dense},
            "rows_rank0": {"light": res.rows_light, "mid": res.rows_mid, "heavy": res.rows_heavy,
                           "hash_cells": res.cells_hash, "dense_cells": res.cells_dense},
        },
        "roofline": roofline_of(args, world, results, args.workload == "rmat" and args.scale == 20),
    }


def single_gpu(args, torch, capi, ctx, dev, stream):
    """N = 1: the headline workload, then (--full on the default workload only) the other configs and the CPU baseline
    in the same process."""
    w = Workload(torch, capi, ctx, dev, args.workload, args.scale, args.grid, args.seed, args.sink, prepared=args.prepared)
    summary, results = run_workload(torch, w, args.steps, args.warmup)
    last = results[-1]
    if args.dump_outputs:
        # before anything else runs on ctx: a later COO multiply may reuse the buffers of the last step's result
        c = last[-1]
        write_dump(args.dump_outputs, digest_arrays(c.nnz, c.sum, c.hash) if w.sink == capi.SINK_DIGEST else coo_arrays(ctx, c))
    flat = [r for step in results for r in step] if w.kind == "galerkin" else [step[0] for step in results]
    nnz_a, products, nnz_c = sum(summary["nnz_a"]), sum(summary["products"]), summary["nnz_c"][-1]
    elapsed = summary["ms_per_step"] * 1e-3 * args.steps
    dsum, dhash = float(last[-1].sum), int(last[-1].hash)
    if w.kind == "galerkin":
        # untimed: the second product once more into the digest sink, so that the line carries C's digest like the others
        rt = ctx.multiply(w.R, w.A, sink=capi.SINK_COO)
        rd = ctx.multiply(capi.result_operand(rt), w.R, tB="T", sink=capi.SINK_DIGEST)
        assert int(rd.nnz) == nnz_c
        dsum, dhash = float(rd.sum), int(rd.hash)
    line = headline(args, 1, w.name, w.n, w.ne, nnz_a, products, nnz_c,
                    dsum, dhash, summary["ms_per_step"], elapsed,
                    [step[-1] for step in results] if w.kind == "galerkin" else flat, 0, None, "1 GPU")
    if w.kind == "galerkin":
        line["metric"] = "nnz(C)/s for C=R*A*R^T (two chained SpGEMMs)"
        line["config"]["multiplies"] = summary
    if w.sink_name == "coo":
        line["config"]["read_write_alg_GBps"] = summary["read_write_alg_GBps"]
    line["config"]["workspace_GB"] = summary["workspace_GB"]
    w.release()
    ctx.close()                                   # the headline's workspace goes back before the other configs run
    default_line = args.workload == "rmat" and args.scale == 20 and args.sink == "digest" and not args.prepared
    if args.full and default_line and not args.no_other_configs:
        others = {}

        def other(key, kind, steps, warmup, **kw):
            c2 = capi.Context(dev.index, stream.cuda_stream)           # fresh workspace per config
            try:
                w2 = Workload(torch, capi, c2, dev, kind, **kw)
                others[key] = run_workload(torch, w2, steps, warmup)[0]
                w2.release()
            except Exception as e:                                      # a failing extra config must not lose the headline
                others[key] = {"error": repr(e)}
            finally:
                c2.close()
                torch.cuda.empty_cache()

        other("cfg3_poisson4096_digest", "poisson", 10, 2, grid=4096)
        other("cfg3_poisson4096_coo", "poisson", 10, 2, grid=4096, sink="coo")
        other("cfg5_galerkin256_coo", "galerkin", 5, 1, grid=256)
        other("cfg2_rmat20_coo_sink", "rmat", 2, 1, scale=20, seed=args.seed, sink="coo")
        other("cfg4_rmat23_one_gpu_digest", "rmat", 2, 1, scale=23, seed=args.seed)
        # the same products with their operands prepared once (never `value`: the headline starts from the raw tuples every step)
        other("cfg2_rmat20_digest_prepared", "rmat", 5, 2, scale=20, seed=args.seed, prepared=True)
        other("cfg3_poisson4096_digest_prepared", "poisson", 10, 2, grid=4096, prepared=True)
        other("cfg5_galerkin256_coo_prepared", "galerkin", 5, 1, grid=256, prepared=True)
        if "ms_per_step" in others.get("cfg2_rmat20_digest_prepared", {}):
            line["config"]["prepared_b_ms_per_step"] = others["cfg2_rmat20_digest_prepared"]["ms_per_step"]
        try:
            c3 = capi.Context(dev.index, stream.cuda_stream)
            others["pcie_inclusive_host_delivery"] = pcie_delivery(torch, capi, c3, dev, 17, args.seed)
            c3.close()
        except Exception as e:
            others["pcie_inclusive_host_delivery"] = {"error": repr(e)}
        line["other_configs"] = others
        # (the driver's parser keeps `config` and drops other top-level keys: the other configs' two figures go there too)
        line["config"]["other_configs"] = {k: {"ms_per_step": round(v["ms_per_step"], 3),
                                               "read_alg_frac": round(v["read_alg_frac_of_hbm_peak"], 4) if "read_alg_frac_of_hbm_peak" in v else None}
                                           for k, v in others.items() if isinstance(v, dict) and "ms_per_step" in v}
        coo = others.get("cfg2_rmat20_coo_sink", {})
        if "ms_per_step" in coo:
            line["config"]["coo_sink_ms_per_step"] = coo["ms_per_step"]
            line["config"]["coo_sink_nnz_c_per_s"] = coo["nnz_c_per_s"]
    if args.full and default_line and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline(args.cpu_scale, args.seed)
    return line


if __name__ == "__main__":
    main()
