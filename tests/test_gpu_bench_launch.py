"""The N > 1 entry paths of bench.py on the one-GPU box: the 8-GPU scaling run is the
driver's, so what can be shown here is that every way of starting it reaches the timed region and
prints one JSON line -- bench.py launching its own ranks, the driver's torch.distributed.run form, both
scaling modes, and the RCCL (`nccl`) branch executed once with a single rank."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = ["--steps", "6", "--warmup", "2", "--ramp-ms", "5", "--no-cpu", "--no-extra", "--no-secondary", "--no-e2e"]


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GAMS_BENCH_BACKEND",
              "GAMS_BENCH_FORCE_DIST"):
        env.pop(k, None)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env.update(extra or {})
    return env


def _one_json_line(res):
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def _bench(args, extra_env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=_env(extra_env),
                          capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize("workload,scale,scaling", [("Atha", "0.05", "weak"), ("GRCh38-step10", "0.01", "strong")])
def test_bench_self_launch_two_ranks_on_one_gpu(workload, scale, scaling):
    """`python bench.py --gpus 2` (no launcher, no WORLD_SIZE): two ranks share the one device, so the
    barrier and the reductions go over gloo (chosen by bench.py because devices < ranks)."""
    out = _one_json_line(_bench(["--gpus", "2", "--workload", workload, "--scale", scale] + QUICK))
    assert out["n_gpus"] == 2 and out["scaling"] == scaling and out["steps"] == 6
    assert out["value"] > 0 and out["unit"] == "windows/s"
    per_step = out["config"]["windows_per_step"]
    assert all(w > 0 for w in per_step)
    if scaling == "strong":
        assert "LPT-sharded x2" in out["config"]["sharding"]


def test_bench_one_rank_through_rccl():
    """The nccl branch -- init_process_group('nccl', device_id=...), barrier, all_reduce MAX / SUM on
    cuda tensors -- executed on an MI355X with one rank, started the way the driver starts N ranks."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr", "127.0.0.1", "--master-port", "29547", os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--workload", "Atha", "--scale", "0.05"] + QUICK
    res = subprocess.run(cmd, env=_env({"GAMS_BENCH_FORCE_DIST": "1", "GAMS_BENCH_BACKEND": "nccl"}),
                         capture_output=True, text=True, timeout=900)
    out = _one_json_line(res)
    assert out["n_gpus"] == 1 and out["value"] > 0
    assert out["config"]["collectives"].startswith("nccl")


def test_bench_n1_launcher_path_equals_direct_path():
    """N = 1 through torch.distributed.run does the same work as `python bench.py`: same windows per step,
    same peaks, and a rate in the same range (both time 40 steps of a 6-Mb genome)."""
    args = ["--gpus", "1", "--workload", "Atha", "--scale", "0.05", "--steps", "40", "--warmup", "5",
            "--no-cpu", "--no-extra", "--no-secondary"]
    direct = _one_json_line(_bench(args))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
           "--master-addr", "127.0.0.1", "--master-port", "29548", os.path.join(ROOT, "bench.py")] + args
    launched = _one_json_line(subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=900))
    assert launched["config"]["windows_per_step"] == direct["config"]["windows_per_step"]
    assert launched["config"]["peaks_per_step"] == direct["config"]["peaks_per_step"]
    assert 0.5 < launched["value"] / direct["value"] < 2.0


def test_bench_plain_line_dump_outputs_and_full(tmp_path):
    """A plain run's line is the headline only; --dump-outputs writes the peak records of the LAST timed step, the
    same in two runs with the same arguments; --full adds the roofline, CPU, end-to-end and secondary blocks."""
    import numpy as np

    args = ["--gpus", "1", "--workload", "Atha", "--scale", "0.05", "--steps", "7", "--warmup", "2", "--ramp-ms", "5"]
    a = _one_json_line(_bench(args + ["--dump-outputs", str(tmp_path / "a")]))
    b = _one_json_line(_bench(args + ["--dump-outputs", str(tmp_path / "b")]))
    for k in ("roofline", "cpu_baseline", "parity_vs_oracle", "end_to_end", "extra", "secondary", "pass_with_peaks_ms"):
        assert k not in a
    assert a["steps"] == 7 and a["unit"] == "windows/s" and a["higher_is_better"] is True and a["dtype"] == "u8"
    # the ramp runs a multiple of the 3 batches, so the timed steps start at batch 2 % 3 and the last one is 8 % 3
    w = a["config"]["windows_per_step"]
    assert a["value"] * a["ms_per_step"] * 1e-3 == pytest.approx(sum(w[(2 + i) % 3] for i in range(7)) / 7, rel=1e-9)
    fields = ("ctg", "window", "gc_count", "signal")
    got = {f: np.load(tmp_path / "a" / f"peaks_{f}.npy") for f in fields}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == sorted(f"peaks_{f}.npy" for f in fields)
    assert all(v.dtype == np.float64 and v.size == a["config"]["peaks_per_step"][8 % 3] > 0 for v in got.values())
    assert set(np.unique(got["signal"])) <= {-1.0, 1.0} and np.all(np.diff(got["ctg"]) >= 0)
    for f in fields:
        assert np.array_equal(got[f], np.load(tmp_path / "b" / f"peaks_{f}.npy"))

    full = _one_json_line(_bench(args + ["--full"]))
    assert full["config"]["windows_per_step"] == w and full["config"]["peaks_per_step"] == a["config"]["peaks_per_step"]
    assert full["roofline"]["launch_ms"] > 0 and full["parity_vs_oracle"] is True and full["cpu_baseline"]["value"] > 0
    assert full["pass_with_peaks_ms"] > 0 and "error" not in full["end_to_end"] and "error" not in full["secondary"]
