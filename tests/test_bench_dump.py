"""bench.py --dump-outputs: what the last timed step returned, as .npy files.  The CPU half checks the sampling of a
COO result and the size limit against a stand-in context; the GPU half runs bench.py and holds the dump to the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeResult:
    """A COO result of n tuples whose device arrays are stand-ins: tuple p is (p // 7, p % 7, p / 2)."""
    def __init__(self, n):
        self.nnz, self.shape0, self.shape1 = n, n // 7 + 1, 7
        self.idx0, self.idx1, self.val = 1 << 44, 2 << 44, 3 << 44


class _FakeCtx:
    def __init__(self, n):
        self.n, self.reads = n, 0

    def to_host(self, ptr, count, dtype):
        base = ptr >> 44 << 44
        first = (ptr - base) // np.dtype(dtype).itemsize
        assert 0 <= first and first + count <= self.n, "read outside the result"
        self.reads += 1
        p = np.arange(first, first + count, dtype=np.int64)
        return {1 << 44: p // 7, 2 << 44: p % 7, 3 << 44: p / 2}[base].astype(dtype)


@pytest.mark.parametrize("n", [0, 1, 5000, bench.DUMP_BLOCK * bench.DUMP_BLOCKS, 10 ** 10 + 3])
def test_coo_sample_is_fixed_in_bounds_and_under_the_limit(n, tmp_path):
    a = bench.coo_arrays(_FakeCtx(n), _FakeResult(n))
    pos = a["c_pos"].astype(np.int64)
    assert a["nnz_c"].tolist() == [n]
    assert pos.size == min(n, bench.DUMP_BLOCK * bench.DUMP_BLOCKS)
    assert np.all(np.diff(pos) > 0) and (pos.size == 0 or (pos[0] >= 0 and pos[-1] < n))
    if n > 0:
        assert n - 1 in pos or n > bench.DUMP_BLOCK * bench.DUMP_BLOCKS
    assert np.array_equal(a["c_row"], pos // 7) and np.array_equal(a["c_col"], pos % 7) and np.array_equal(a["c_val"], pos / 2)
    again = bench.coo_arrays(_FakeCtx(n), _FakeResult(n))
    assert all(np.array_equal(a[k], again[k]) for k in a)
    bench.write_dump(str(tmp_path), a)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(k + ".npy" for k in a)
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= bench.DUMP_MAX_BYTES
    for f in files:
        assert np.load(os.path.join(tmp_path, f)).dtype == np.float64


def test_digest_hash_is_stored_exactly():
    h = 0xfedcba9876543210
    a = bench.digest_arrays(12, 0.5, h)
    hi, lo = (int(x) for x in a["digest_hash"])
    assert (hi << 32 | lo) == h and a["nnz_c"].tolist() == [12] and a["digest_sum"].tolist() == [0.5]


def test_dump_limit_is_enforced(tmp_path):
    with pytest.raises(RuntimeError, match="limit"):
        bench.write_dump(str(tmp_path / "d"), {"x": np.zeros(bench.DUMP_MAX_BYTES // 8 + 1)})
    assert not os.path.exists(tmp_path / "d")


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def _bench(args, timeout=280):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-cpu-baseline", "--no-other-configs"] + args,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_bench_dump_matches_the_oracle(tmp_path):
    """R-MAT scale 12 A*A through bench.py into both sinks: the digest and the sampled COO tuples of the last timed step
    equal the oracle's product; --steps sets the number of timed steps."""
    from oracle import binding as orc
    from spsparse_amd import workloads as wl
    a = wl.rmat(12, seed=1)
    A = orc.Mat(*a)
    wi, wj, wv, shape = orc.multiply(A, A, rowwise=True, nthreads=4)
    cnt, vs, h = orc.digest(wi, wj, wv)

    d = tmp_path / "digest"
    line = _bench(["--scale", "12", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    hi, lo = (int(x) for x in np.load(d / "digest_hash.npy"))
    assert np.load(d / "nnz_c.npy").tolist() == [cnt] and (hi << 32 | lo) == h
    assert abs(float(np.load(d / "digest_sum.npy")[0]) - vs) <= 1e-12 * np.abs(wv).sum()

    c = tmp_path / "coo"
    line = _bench(["--scale", "12", "--sink", "coo", "--steps", "2", "--warmup", "0", "--dump-outputs", str(c)])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert np.load(c / "nnz_c.npy").tolist() == [len(wv)] and np.load(c / "c_shape.npy").tolist() == list(shape)
    pos = np.load(c / "c_pos.npy").astype(np.int64)
    assert pos.size == min(len(wv), bench.DUMP_BLOCK * bench.DUMP_BLOCKS) and np.all(np.diff(pos) > 0)
    assert np.array_equal(np.load(c / "c_row.npy"), wi[pos]) and np.array_equal(np.load(c / "c_col.npy"), wj[pos])
    gv = np.load(c / "c_val.npy")
    assert np.max(np.abs(gv - wv[pos]) / np.abs(wv[pos])) <= 1e-12
