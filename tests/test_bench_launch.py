"""bench.py's N-rank launch path.

`python bench.py --gpus N` with N > 1 and no launcher around it starts torch.distributed.run
as a child process, before any GPU call, and relays rank 0's JSON line; every rank checks
that WORLD_SIZE equals --gpus.  The CPU tests run here (no GPU: the ranks must refuse and the
parent must return their failure); the GPU test rehearses two ranks on the one-GPU box over
gloo and reads the --full line.  A plain one-GPU run times the headline only and, with
--dump-outputs, writes the last timed launch's outputs.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR",
                        "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    env.update(OMP_NUM_THREADS="2", **kw)
    return env


def test_gpus_n_without_launcher_spawns_ranks_and_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-only check of the launcher's failure path")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--no-variants", "--no-cpu-baseline"], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode != 0
    assert "launching 2 ranks" in r.stderr
    assert "torch.distributed.run" in r.stderr and "--nproc-per-node 2" in r.stderr
    assert "2 ranks on this node need 2 GPUs, 0 visible" in r.stderr
    assert r.stdout.strip() == ""  # no JSON line from a failed run


def test_world_size_must_equal_gpus():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "1", "--warmup", "0",
                        "--no-variants", "--no-cpu-baseline"], cwd=ROOT,
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "--gpus 4 but the launcher started WORLD_SIZE=2" in r.stderr


@pytest.mark.gpu
def test_bench_gpus_2_gloo_rehearsal_reports_two_ranks():
    """Two ranks sharing cuda:0 over gloo, launched by bench.py itself."""
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "2", "--steps", "5", "--warmup", "2",
                        "--full", "--no-cpu-baseline", "--no-train"], cwd=ROOT,
                       env=_env(DPAC_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0"),
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [s for s in r.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 8192
    assert out["dist"]["world"] == 2 and out["dist"]["backend"] == "gloo"
    assert out["dist"]["launcher"] == "torch.distributed.run"
    assert out["value"] > 0 and out["roofline"]["frac"] > 0
    assert out["dist"]["note"].startswith("ranks share a GPU")
    # strong scaling: the global batch stays 4096, split 2048 + 2048
    st = out["strong_scaling"]
    assert st["scaling"] == "strong" and st["global_batch"] == 4096
    assert st["batch_per_gpu"] == 2048 and st["batch_per_rank"] == [2048, 2048]
    assert st["value"] > 0 and st["ms_per_step"] > 0 and 0 < st["roofline"]["frac"] < 1
    assert st["roofline"]["peak"] == 2 * 8000.0
    sp = out["speedup_vs_1"]
    assert sp["one_gpu_value"] > 0
    assert abs(sp["weak"] - out["value"] / sp["one_gpu_value"]) < 1e-9 * sp["weak"]
    assert abs(sp["strong"] - st["value"] / sp["one_gpu_value"]) < 1e-9 * sp["strong"]
    print("gloo rehearsal line:", json.dumps({k: out[k] for k in ("value", "n_gpus", "ms_per_step",
                                                                  "speedup_vs_1")}))


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` measures the headline alone (everything else needs
    --full), K sets the timed steps, and --dump-outputs writes what the last timed launch wrote:
    launch K - 1 = 2 runs over buffer set 2, so the files equal that set's outputs from the same
    launch in this process, bit for bit, on the sampled trajectories."""
    import numpy as np
    import torch

    import bench
    from deeppde_actorcritic_amd import _lib
    from deeppde_actorcritic_amd import equation as peq

    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [s for s in r.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "traj-steps/s" and line["higher_is_better"]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "f32" and line["full"] is False
    assert line["ms_per_step"] > 0
    B, N, d = bench.B_PER_GPU, bench.HORIZON, bench.DIM
    assert abs(line["value"] - B * N / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for key in ("variants", "cpu_baseline", "strong_scaling", "speedup_vs_1"):
        assert key not in line
    assert "variants" not in r.stderr and "cpu_baseline" not in r.stderr

    assert sorted(os.listdir(out_dir)) == ["coef.npy", "dt.npy", "x.npy"]
    got = {k: np.load(out_dir / f"{k}.npy") for k in ("x", "dt", "coef")}
    idx = bench.dump_sample_index(B, 4)
    keep = len(idx)
    assert keep == 2048 and len(np.unique(idx)) == keep and idx.min() >= 0 and idx.max() < B
    assert got["x"].shape == (N + 1, keep, d) and got["dt"].shape == got["coef"].shape == (keep, N)
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6

    torch.cuda.set_device(0)
    eqp = peq.LQR(bench.lqr_config()).params()
    rs = bench.RolloutSets(_lib.load(), eqp, _lib.SCHEME_ADAPTIVE, torch.float32, B, N, d, 0, 3)
    rs.launcher(3)(2)
    torch.cuda.synchronize()
    _, _, x, dt, coef = rs.sets[2]
    np.testing.assert_array_equal(got["x"], x.cpu().numpy()[:, idx])
    np.testing.assert_array_equal(got["dt"], dt.cpu().numpy()[idx])
    np.testing.assert_array_equal(got["coef"], coef.cpu().numpy()[idx])
