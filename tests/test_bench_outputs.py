"""bench.py's plain run and --dump-outputs: the result line of a plain run holds the headline and nothing of --full, and the
dumped arrays are what the last timed step computed -- the solution, checked against a direct solve of the oracle system,
with its iteration count and relative residual."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import fedd_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("two_level_variant", "spmv_back_to_back", "cfg2_one_gpu", "per_gpu_share_n8", "cfg5_share_one_gpu",
             "cfg4_one_gpu", "p2_cube", "cpu_baseline", "gpu_over_cpu", "self_check")
DUMPED = ["gmres_iterations.npy", "relres.npy", "solution.npy", "solution_global_ids.npy"]


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)     # bench sets it on import: restored afterwards
    import bench
    return bench


def test_dump_sample_is_fixed_and_bounded(bench):
    assert np.array_equal(bench.dump_index(1000), np.arange(1000))
    n = 3 * bench.DUMP_MAX_ENTRIES
    idx = bench.dump_index(n)
    assert idx.size == bench.DUMP_MAX_ENTRIES and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(idx, bench.dump_index(n))
    assert 2 * 8 * idx.size <= 64 * 2 ** 20                   # values and ids as float64


def test_dump_sample_gathers_by_global_id(bench):
    n = 50
    idx = np.array([1, 7, 8, 20, 49])
    x = np.arange(n) * 0.5
    out = np.zeros(idx.size)
    for gid in (np.arange(0, n, 2), np.arange(1, n, 2)[::-1]):      # two owners, one of them in reverse order
        pos, val = bench.sample_of(idx, gid, x[gid])
        out[pos] = val
    np.testing.assert_array_equal(out, x[idx])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _check_dump(d, out, M):
    assert sorted(os.listdir(out)) == DUMPED
    arrs = {f[:-4]: np.load(os.path.join(out, f)) for f in DUMPED}
    assert all(v.dtype == np.float64 for v in arrs.values())
    n = (M + 1) ** 3
    np.testing.assert_array_equal(arrs["solution_global_ids"], np.arange(n))
    assert arrs["gmres_iterations"][0] == d["config"]["gmres_iterations"]
    assert arrs["relres"][0] == d["config"]["relres"] <= 1e-8
    A, b, _, _, _ = fo.laplace_problem(fo.build_mesh_structured(3, 1, M))
    xd = fo.direct_solve(A, b)
    assert np.abs(arrs["solution"] - xd).max() <= 1e-6 * np.abs(xd).max()


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_step(fedd_lib, tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--global-cells", "20",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config",
                "roofline", "kernels"):
        assert key in d
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "DoF/s" and d["dtype"] == "f64" and d["higher_is_better"]
    assert d["value"] == pytest.approx(21 ** 3 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in d]
    _check_dump(d, str(out), 20)


@pytest.mark.gpu
def test_bench_n2_rehearsal_dumps_the_gathered_solution(fedd_lib, tmp_path):
    """two ranks on one GPU over gloo: rank 0 gathers the owned entries of both ranks by global id"""
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1",
           "--warmup", "0", "--global-cells", "20", "--rehearse-one-gpu", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and not [k for k in FULL_ONLY if k in d]
    _check_dump(d, str(out), 20)
