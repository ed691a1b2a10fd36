"""bench.py's N>1 code path (one process per rank, barrier + max-over-ranks timing, whole-job aggregate, ATE
all-reduce) exercised with 2 ranks on ONE GPU through gloo -- the driver's real multi-GPU run uses RCCL."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_ranks_on_one_gpu():
    """`python bench.py --gpus 2` with no launcher around it: bench.py re-executes itself as two ranks (here both on device 0,
    gloo; the driver's node gives every rank its own GPU and RCCL)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(BENCH_DIST_BACKEND="gloo", BENCH_DEVICE_OVERRIDE="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                       # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 4
    assert abs(d["value"] - 2 * 64 * 4 / (d["ms_per_step"] * 4e-3)) / d["value"] < 1e-6
    # which kernel is the longest with two ranks sharing one GPU varies (k_feature, or the one-workgroup-per-trajectory Cholesky
    # when the other rank's per-track kernel holds the CUs): frac is the utilisation on the FLOP the kernel executes (a number,
    # <= 1 by construction); the reference algorithm's FLOP over the same time stays under alg_equivalent_ratio and is never below it
    rf = d["roofline"]
    assert rf["bound"] in ("valu", "mfma", "hbm") and rf["alg_equivalent_ratio"] > 0
    assert 0 < rf["frac"] <= 1 and rf["frac"] == rf["executed_frac"]
    assert abs(rf["achieved"] / rf["peak"] - rf["frac"]) < 1e-9
    assert rf["executed_frac"] <= rf["alg_equivalent_ratio"] * (1 + 1e-9)
    # PMC counters only when the passes ran on the kernel sources this run was built from
    assert (rf["traffic"] is None) == bool(rf["traffic_source"]["stale"])
    assert d["ate_m"] < 0.05 and len(d["ate_per_sequence_m"]) == 1
    assert d["repeats"]["windows"] >= 3 and d["repeats"]["values"][0] == d["value"]
    # the headline is SURVEY.md 8d's metric: inputs uploaded inside the timed region; the resident-input rate sits beside it
    assert d["inputs"].startswith("uploaded per frame") and d["upload"]["bytes_per_step_per_gpu"] > 1e6
    assert d["resident_inputs"]["median"] > 0 and len(d["resident_inputs"]["values"]) >= 3


@pytest.mark.gpu
def test_cfg4_monte_carlo_mode_reports_per_sequence_ate():
    """bench.py --config cfg4: 5 synthetic sequences x noise seeds, EuRoC intrinsics (anisotropic noise), per-sequence ATE
    through shard.ate_local / ate_allreduce, the CPU oracle's ATE beside the HIP path's on sampled trajectories."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cfg4", "--steps", "4", "--warmup", "1", "--repeats", "1",
           "--no-early-accept-pass", "--no-upload-pass", "--cpu-seconds", "5", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["name"] == "cfg4" and d["config"]["sequences"] == 5 and d["config"]["trajectories_per_gpu"] == 128
    assert len(d["ate_per_sequence_m"]) == 5 and max(d["ate_per_sequence_m"]) < 0.1
    # anisotropic noise: the device runs the reference's literal R_n = Q_1^T R_o Q_1 construction (kernels_literal.hip);
    # `ate_vs_ref_m` is against the oracle's restatement of it, the pre-whitened (GLS) restatement is reported beside it
    assert d["ate_vs_ref_is"].startswith("literal") and d["ate_vs_ref_m"] < 1e-3 and d["ate_vs_ref_whitened_m"] < 1e-2
    assert abs(d["ate_ref_m"] - d["ate_hip_sample_m"]) < 1e-2
    assert d["cpu_baseline"]["kind"] in ("reference", "port")


@pytest.mark.gpu
def test_cfg2_single_trajectory_latency_config_runs():
    """bench.py --config cfg2 (BASELINE.json configs[1]: 10-camera window, 50 tracks, double, ONE trajectory): a C++ caller over
    the drop-in shim, one propagate() + getImuState() per IMU sample, the reference's stage names; the reference's own source
    in double on one core beside it; the state at the end of the run against the oracle at 1e-6."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cfg2", "--steps", "10", "--warmup", "3", "--repeats", "2", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["config"]["name"] == "cfg2" and d["dtype"] == "f64" and d["n_gpus"] == 1 and d["steps"] == 10
    assert d["value"] > 0 and abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6
    assert set(d["latency_us"]["stage_mean"]) >= {"imu_prop", "msckf_augment_state", "msckf_update", "msckf_add_features", "msckf_marginalize", "msckf_prune_empty_states"}
    assert d["roofline"]["peak"] == 78.6 and 0 < d["roofline"]["frac"] < 1
    assert d["cpu_baseline"]["kind"] in ("reference", "port") and d["cpu_baseline"]["cores"] == 1
    assert d["parity"]["shim_run_vs_oracle_state_rel"] < 1e-6 and max(d["parity"]["capi_run_vs_oracle"].values()) < 1e-6


@pytest.mark.gpu
def test_eight_rank_rehearsal_on_one_device():
    """The driver's 8-GPU launch cannot be tried from here (one GPU per box): eight ranks share device 0 instead (gloo, 8
    trajectories each), which exercises what an 8-rank node does to the HOST -- 8 x (uploading thread + 4 enqueue threads) on
    disjoint cores taken from LOCAL_RANK, eight scenario pools, the max-over-ranks timing and the per-sequence ATE all-reduce
    -- and, with every rank given the same seeds, that all ranks end in the same bits.  Not a scaling measurement."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(BENCH_DIST_BACKEND="gloo", BENCH_DEVICE_OVERRIDE="0", BENCH_SAME_SEEDS="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--trajectories", "8", "--steps", "3", "--warmup", "1", "--repeats", "2",
           "--no-cpu-baseline", "--no-early-accept-pass", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1500)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["ranks_seen"] == list(range(8)) and d["ranks_bit_identical_for_equal_seeds"] is True
    assert abs(d["value"] - 8 * 8 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-6
    assert d["config"]["host_affinity"] is None or len(d["config"]["host_affinity"]) == 5


def _plain(args, tmp, name):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp / name)],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), tmp / name


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` (no --full): the result line's headline fields, K timed steps behind
    ms_per_step, nothing of what --full adds, and --dump-outputs: what the timed path computed, float32 / float64, under
    64 MB, identical from run to run.  A run longer than the scenario's SCENARIO_STEPS_MAX distinct steps times its steps
    in windows, each from the same filter states: the last step's outputs are those of a run of one window."""
    import numpy as np
    import bench
    d, a = _plain(["--gpus", "1", "--steps", "5", "--warmup", "2"], tmp_path, "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d
    assert d["steps"] == 5 and d["warmup"] == 2 and d["unit"] == "updates/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - 64 * 5 / (d["ms_per_step"] * 5e-3)) / d["value"] < 1e-6
    assert not set(d) & {"roofline", "repeats", "cpu_baseline", "other_configs", "ate_m", "resident_inputs"}
    files = sorted(p.name for p in a.iterdir())
    assert files == sorted(n + ".npy" for n in d["dumped_outputs"]) and "covariance.npy" in files and "imu_state.npy" in files
    assert sum(p.stat().st_size for p in a.iterdir()) <= 64 << 20
    arrs = {p.stem: np.load(p) for p in a.iterdir()}
    assert all(x.dtype in (np.float32, np.float64) for x in arrs.values())
    assert arrs["imu_state"].shape == (64, 29) and np.all(np.isfinite(arrs["covariance"])) and np.all(arrs["gate_stats"][:, 4] > 0)
    _, b = _plain(["--gpus", "1", "--steps", "5", "--warmup", "2"], tmp_path, "b")
    for n, x in arrs.items():
        assert np.array_equal(x, np.load(b / (n + ".npy"))), n
    # windows: 2 x SCENARIO_STEPS_MAX steps = two windows over the same frames, against one window (8 trajectories)
    m = bench.SCENARIO_STEPS_MAX
    d1, one = _plain(["--steps", str(m), "--warmup", "1", "--trajectories", "8"], tmp_path, "one")
    d2, two = _plain(["--steps", str(2 * m), "--warmup", "1", "--trajectories", "8"], tmp_path, "two")
    assert d1["timed_windows"]["windows"] == 1 and d2["timed_windows"]["windows"] == 2 and d2["steps"] == 2 * m
    for n in d1["dumped_outputs"]:
        assert np.array_equal(np.load(one / (n + ".npy")), np.load(two / (n + ".npy"))), n
