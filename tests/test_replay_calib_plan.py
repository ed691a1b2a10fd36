"""The host side of the Monte-Carlo replay's calibration model (csrc/replay_plan.h, CALIB: the two records, their refusals and
lifetime, and the inline functions the kernels compile) as a stand-alone host program, without a device."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

FLAGS = [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]]
N_ROWS, N_REC = 300, 3
SEED_ROW, SEED_NOISE, SEED_IMU_REC, SEED_OBS, SEED_CAM_REC = 1234, 555, 99, 4321, 98


@pytest.fixture(scope="module", params=FLAGS, ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("replay_calib") / "replay_calib_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-o", path, os.path.join(H.ROOT, "tests", "cpp", "replay_calib_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return path


def test_the_calibration_records_their_refusals_and_lifetime(exe):
    """every refusal with its code and text in the stated order, a refused call leaves the previous record in force, the records
    stay through both assigns, a fault record, a timing record and a commit, alloc clears them; which records are trivial; the
    identity and zero records return the values' bits; the clamp at its exact thresholds and rint at exact ties"""
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "replay calib ok" in run.stdout, run.stdout + run.stderr


def _centred(seed, i, scale):
    return (sc.replay_uniform(seed, np.asarray(i, dtype=np.uint64)) - 0.5) * scale


def _imu_record(j):
    i = np.arange(27)
    diag = (i < 18) & ((i % 9) % 4 == 0)
    ic = np.zeros(31)
    ic[:27] = np.where(diag, 1.0, 0.0) + _centred(SEED_IMU_REC, 31 * j + i, np.where(i < 18, 0.02, 2e-3))
    u = sc.replay_uniform(SEED_IMU_REC, np.asarray(31 * j + np.arange(27, 31), dtype=np.uint64))
    if j >= 1:
        ic[27], ic[28] = 0.5 + u[0] * 0.3, 8.0 + u[1] * 4.0
    if j == 2:
        ic[29], ic[30] = 1e-4 * (1.0 + u[2]), 1e-2 * (1.0 + u[3])
    return ic


def _hex(tokens):
    return np.array([float.fromhex(t) for t in tokens])


def test_the_imu_functions_are_the_twins_bit_for_bit(exe):
    """300 rows under three records (matrices alone, with saturation, with saturation and quantisation): calib_imu's c and
    calib_out's value and clip mask, printed as hex doubles, against scenario.replay_imu_calib_row / replay_imu_calib_out"""
    run = subprocess.run([exe, "imu"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("imu ")]
    assert len(lines) == N_ROWS
    n = np.arange(N_ROWS)
    idx = 6 * n[:, None] + np.arange(6)[None, :]
    v = _centred(SEED_ROW, idx, np.array([2.0] * 3 + [30.0] * 3))
    noise = _centred(SEED_NOISE, idx, 0.1)
    clipped_rows = quantised = 0
    for j in range(N_REC):
        ic = _imu_record(j)
        rows = n[n % N_REC == j]
        c = sc.replay_imu_calib_row(v[rows], ic)
        out, clipped = sc.replay_imu_calib_out(c + noise[rows], ic)
        mask = (clipped.astype(np.int64) << np.arange(6)).sum(1)
        for k, r in enumerate(rows):
            ln = lines[r]
            assert int(ln[1]) == r
            assert np.array_equal(_hex(ln[2:8]), c[k]), (r, "c")
            assert np.array_equal(_hex(ln[8:14]), out[k]), (r, "out")
            assert int(ln[14]) == mask[k], (r, "mask")
        clipped_rows += int(clipped.any(1).sum())
        quantised += int((out != (c + noise[rows])).any(1).sum()) if j == 2 else 0
        if j == 0:
            assert not clipped.any() and np.array_equal(out, c + noise[rows])
    assert clipped_rows > 50 and quantised == N_ROWS // N_REC


def test_the_camera_map_is_the_twins_bit_for_bit(exe):
    """300 entries under three records with all eight fields non-zero: calib_cam against scenario.replay_cam_calib"""
    run = subprocess.run([exe, "cam"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("cam ")]
    assert len(lines) == N_ROWS
    n = np.arange(N_ROWS)
    xy = _centred(SEED_OBS, 2 * n[:, None] + np.arange(2)[None, :], 1.2)
    got = np.array([_hex(ln[2:4]) for ln in lines])
    scale = np.array([0.01, 0.01, 0.01, 0.01, 0.2, 0.05, 2e-3, 2e-3])
    for j in range(N_REC):
        cc = _centred(SEED_CAM_REC, 8 * j + np.arange(8), scale)
        assert np.all(cc != 0.0)
        rows = n % N_REC == j
        want = sc.replay_cam_calib(xy[rows], cc)
        assert np.array_equal(got[rows], want), j
        assert np.all(want != xy[rows])
