"""The scenarios of tests/test_gpu_ragged_imu.py are worth comparing, and the new entries exist: without a GPU.

On the CPU oracle alone every non-skipped cell of the ragged-IMU batch updates on every full-window frame (so the GPU module
compares real updates, also right after the 1-, 17- and 33-sample cells and on the frames that have no sample at all), the
resampling keeps what a frame's ten samples integrate, and the count schedule reaches what the issue names: every boundary of
k_propagate's groups of 16, differing counts on every frame, one sequence that pauses and one that ends early."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
import ragged_imu as R
from msckf_mono_amd import scenario as sc

NEW = ("msckf_hip_scenario_set_cell", "msckf_hip_propagate_range_counts", "msckf_hip_frame_log_metrics_ranges")


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def test_the_new_entries_are_declared_bound_and_exported():
    from msckf_mono_amd import capi
    hdr = open(os.path.join(H.ROOT, "include", "msckf_hip.h")).read()
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in capi.SYMBOLS and re.search(r" T %s\b" % name, exported), name
    for method in ("propagate_range_counts", "frame_log_metrics_ranges"):
        assert callable(getattr(capi.Batch, method))
    assert "skip" in capi.Batch.scenario_set.__code__.co_varnames
    assert re.search(r"MSCKF_HIP_CELL_SKIP\s*=\s*%d\b" % capi.CELL_SKIP, hdr)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]], ids=["plain", "sanitized"])
def test_the_cell_rule_alone(tmp_path, flags):
    """host_lists.h states what a cell may carry once (cell_refusal); a stand-alone program checks it, also under the address
    and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "cell_rule_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, os.path.join(H.ROOT, "tests", "cpp", "cell_rule_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "cell rule ok" in run.stdout, run.stdout + run.stderr


@pytest.mark.parametrize("k", [0, 1, 3, 5, 8, 9, 10, 11, 12, 15, 16, 17, 20, 32, 33])
def test_resampling_keeps_the_interval_and_the_mean_reading(k):
    rd = sc.Trajectory(2, 5, 6, 10, 8).imu_for_frame(3)
    out = R.resample(rd, k)
    assert out.shape == (k, 7)
    if k == 0:
        return
    assert np.isclose(out[:, 6].sum(), rd[:, 6].sum(), rtol=1e-14, atol=0) and np.all(out[:, 6] > 0)
    # the dT-weighted mean reading is the ten samples' (equal dT there): what a first-order integrator sees is unchanged
    w = out[:, 6] / out[:, 6].sum()
    assert np.allclose(w @ out[:, :6], rd[:, :6].mean(0), rtol=1e-12, atol=1e-14)
    if k == 10:
        assert np.array_equal(out, rd)
    if k == 20:
        assert np.array_equal(out[::2, :6], rd[:, :6]) and np.allclose(out[:, 6], rd[0, 6] / 2, rtol=1e-15)


@pytest.mark.parametrize("zeros", ["last", "rotating"])
def test_the_count_schedule_reaches_what_it_is_there_for(zeros):
    rs = R.RaggedImuSet(zeros=zeros)
    assert rs.B == 7 and rs.B % 3 != 0 and sorted(set(rs.N)) == [6, 15] and rs.nf == rs.n_cap + 4 and rs.K == 33
    used = set()
    for f in range(rs.nf):
        row = [rs.counts[b][rs.local[b][f]] for b in range(rs.B) if not rs.skipped(b, f)]
        assert len(set(row)) >= 4, (f, row)                      # the counts differ within every frame
        used |= set(row)
    assert {0, 1, 15, 16, 17, 32, 33} <= used and max(used) == rs.K
    b, frames = R.MID_SKIP
    assert [f for f in range(rs.nf) if rs.skipped(b, f)] == list(frames) and rs.N[b] == 15
    assert [f for f in range(rs.nf) if rs.skipped(R.TAIL_SKIP, f)] == list(range(rs.nf - 5, rs.nf))
    assert all(not rs.skipped(t, f) for t in range(rs.B) if t not in (b, R.TAIL_SKIP) for f in range(rs.nf))
    # the tail-skipped trajectory reaches its full window before it stops; mixed drop flags meet skipped cells
    assert rs.n_local(R.TAIL_SKIP) > rs.N[R.TAIL_SKIP]
    for t in range(rs.B):
        zero_at = [j for j in range(rs.n_local(t)) if rs.counts[t][j] == 0]
        if zeros == "last":
            assert zero_at == ([rs.n_local(t) - 1] if t in R.ZERO_LAST else []), (t, zero_at)
        else:
            # an empty cell hands its ten samples on: the next cell resamples twenty
            for j in zero_at:
                if j + 1 < rs.nf:
                    assert np.isclose(rs.rd[t][j + 1][:, 6].sum(), 2 * sc.IMU_PER_FRAME / sc.IMU_RATE, rtol=1e-12)


def test_every_cell_of_the_ragged_imu_batch_updates_on_the_oracle(po):
    """m_rows > 0 and n_passed > 0 on every full-window frame of every non-skipped cell, and no weaker than the same
    trajectories on ten equal samples per image"""
    rs, eq = R.RaggedImuSet(), R.RaggedImuSet(equal=True)
    for b in range(rs.B):
        o, oe = rs.oracle(po, po.F64, b), eq.oracle(po, po.F64, b)
        least, least_eq, n_full = None, None, 0
        for f in range(rs.nf):
            eq.oracle_cell(oe, b, f)
            if eq.full(b, f):
                least_eq = min(least_eq or 10 ** 9, oe.lastStats()["n_passed"])
            if rs.skipped(b, f):
                continue
            rs.oracle_cell(o, b, f)
            j = rs.local[b][f]
            if rs.full(b, j):
                s = o.lastStats()
                assert s["m_rows"] > 0 and s["n_passed"] > 0, (b, f, j, rs.counts[b][j], s)
                least = min(least or 10 ** 9, s["n_passed"])
                n_full += 1
        assert n_full >= 3 and least >= least_eq > 0, (b, n_full, least, least_eq)
        assert np.all(np.isfinite(o.getCovariance()))
        # an empty last cell: the oracle's IMU state is the one before that frame's augment, the update still ran
        if b in R.ZERO_LAST:
            assert rs.counts[b][rs.n_local(b) - 1] == 0 and rs.full(b, rs.n_local(b) - 1)


def test_the_lockstep_twin_is_the_plain_ragged_set():
    """equal = True: ten samples per cell, the Trajectory's own, nobody skipped -- what msckf_hip_scenario_set can express"""
    eq = R.RaggedImuSet(equal=True)
    assert eq.K == sc.IMU_PER_FRAME
    for b in range(eq.B):
        assert eq.local[b] == list(range(eq.nf))
        for j in range(eq.nf):
            assert np.array_equal(eq.rd[b][j], eq.trajs[b].imu_for_frame(j))
