"""bench.py --full: a plain run measures the headline alone; the other configs and the CPU baseline run only with --full.
The control flow of single_gpu() is driven with stand-ins for torch, the library and the workloads, so no GPU is needed."""
import sys
import types

import pytest

import bench


class _Res:
    nnz, sum, hash = 10, 1.5, 7


class _Workload:
    def __init__(self, torch, capi, ctx, dev, kind, scale=20, grid=0, seed=1, sink="digest", prepared=False):
        self.kind, self.sink_name = kind, sink
        self.sink = capi.SINK_COO if sink == "coo" else capi.SINK_DIGEST
        self.name, self.n, self.ne = kind, 4, 8

    def release(self):
        pass


class _Context:
    def __init__(self, *a):
        pass

    def close(self):
        pass


def _run(monkeypatch, argv):
    calls = {"workloads": [], "cpu_baseline": 0, "pcie_delivery": 0}

    def run_workload(torch, w, steps, warmup):
        calls["workloads"].append((w.kind, w.sink_name, steps, warmup))
        summary = {"ms_per_step": 2.0, "nnz_c_per_s": 5e3, "nnz_a": [3], "products": [4], "nnz_c": [10],
                   "read_alg_frac_of_hbm_peak": 0.1, "read_write_alg_GBps": 1.0, "workspace_GB": 0.5}
        return summary, [[_Res()] for _ in range(steps)]

    def cpu_baseline(scale, seed):
        calls["cpu_baseline"] += 1
        return {"value": 1.0}

    def pcie_delivery(*a):
        calls["pcie_delivery"] += 1
        return {"nnz_c": 1}

    monkeypatch.setattr(bench, "Workload", _Workload)
    monkeypatch.setattr(bench, "run_workload", run_workload)
    monkeypatch.setattr(bench, "headline", lambda *a: {"config": {}})
    monkeypatch.setattr(bench, "cpu_baseline", cpu_baseline)
    monkeypatch.setattr(bench, "pcie_delivery", pcie_delivery)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"] + argv)
    args = bench.parse()
    torch = types.SimpleNamespace(cuda=types.SimpleNamespace(empty_cache=lambda: None))
    capi = types.SimpleNamespace(SINK_COO=1, SINK_DIGEST=2, Context=_Context)
    line = bench.single_gpu(args, torch, capi, _Context(), types.SimpleNamespace(index=0),
                            types.SimpleNamespace(cuda_stream=0))
    return line, calls


@pytest.mark.parametrize("dump", [False, True])
@pytest.mark.parametrize("steps,warmup", [(5, 1), (3, 0)])
def test_plain_run_measures_the_headline_alone(monkeypatch, tmp_path, steps, warmup, dump):
    argv = ["--steps", str(steps), "--warmup", str(warmup)] + (["--dump-outputs", str(tmp_path / "d")] if dump else [])
    line, calls = _run(monkeypatch, argv)
    assert not bench.parse().full
    assert calls["workloads"] == [("rmat", "digest", steps, warmup)]
    assert calls["cpu_baseline"] == 0 and calls["pcie_delivery"] == 0
    assert "other_configs" not in line and "cpu_baseline" not in line and "other_configs" not in line["config"]
    assert (tmp_path / "d" / "digest_hash.npy").exists() == dump


def test_full_run_adds_the_other_configs_and_the_cpu_baseline(monkeypatch):
    line, calls = _run(monkeypatch, ["--full", "--steps", "4", "--warmup", "1"])
    assert calls["workloads"][0] == ("rmat", "digest", 4, 1)
    assert len(calls["workloads"]) == 9 and calls["pcie_delivery"] == 1 and calls["cpu_baseline"] == 1
    assert set(line["other_configs"]) == {"cfg3_poisson4096_digest", "cfg3_poisson4096_coo", "cfg5_galerkin256_coo",
                                          "cfg2_rmat20_coo_sink", "cfg4_rmat23_one_gpu_digest", "cfg2_rmat20_digest_prepared",
                                          "cfg3_poisson4096_digest_prepared", "cfg5_galerkin256_coo_prepared",
                                          "pcie_inclusive_host_delivery"}
    assert line["cpu_baseline"] == {"value": 1.0}


@pytest.mark.parametrize("skip,workloads,cpu", [("--no-other-configs", 1, 1), ("--no-cpu-baseline", 9, 0)])
def test_full_run_drops_what_is_skipped(monkeypatch, skip, workloads, cpu):
    line, calls = _run(monkeypatch, ["--full", skip])
    assert len(calls["workloads"]) == workloads and calls["cpu_baseline"] == cpu


def test_full_run_of_another_workload_is_its_headline_alone(monkeypatch):
    line, calls = _run(monkeypatch, ["--full", "--scale", "16"])
    assert calls["workloads"] == [("rmat", "digest", 5, 1)] and calls["cpu_baseline"] == 0
    assert "other_configs" not in line and "cpu_baseline" not in line
