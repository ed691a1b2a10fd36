"""The host side of the Monte-Carlo replay's Q_imu model (csrc/replay_plan.h, MODEL: chol_psd, the model's assignment record and
its refusals, the walk_planned flag, the model tag) as a stand-alone host program, without a device."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

FLAGS = [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]]
MATRICES = ("diagonal", "dense_spd", "zero_walk", "rank_deficient", "small_exact", "negative_pivot")


@pytest.fixture(scope="module", params=FLAGS, ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("replay_model") / "replay_model_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-o", path, os.path.join(H.ROOT, "tests", "cpp", "replay_model_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return path


def test_the_model_plan_alone(exe):
    """chol_psd at literal matrices (diagonal, dense, zero walk blocks, a rank-one block, a negative pivot, the tolerance on
    either side), every refusal of the model's assignment with its code, text and order, walk_planned falling on set_cell,
    commit and either assignment, and the model tag switching back and forth"""
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "replay model ok" in run.stdout, run.stdout + run.stderr


def test_the_factor_is_the_twins_bit_for_bit(exe):
    """L of every literal matrix, printed in hexfloat, against scenario.replay_noise_factor of the printed Q: equal bits, and
    the negative pivot refused on both sides"""
    run = subprocess.run([exe, "factor"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = {(ln.split()[0], ln.split()[1]): ln.split()[2:] for ln in run.stdout.splitlines()}
    assert sorted(name for kind, name in rows if kind == "Q") == sorted(MATRICES)
    dense = 0
    for name in MATRICES:
        Q = np.array([float.fromhex(x) for x in rows[("Q", name)]]).reshape(12, 12).T          # printed column-major
        if rows[("L", name)] == ["refused"]:
            assert name == "negative_pivot"
            with pytest.raises(ValueError, match="not positive semi-definite"):
                sc.replay_noise_factor(Q)
            continue
        L = np.array([float.fromhex(x) for x in rows[("L", name)]]).reshape(12, 12).T
        twin = sc.replay_noise_factor(Q)
        assert np.array_equal(L, twin), name
        assert not np.triu(L, 1).any(), name
        sym = 0.5 * (Q + Q.T)
        assert np.max(np.abs(L @ L.T - sym)) <= 1e-15 * max(1.0, np.abs(sym).max()), name
        dense += np.count_nonzero(np.tril(L, -1)) > 30
    assert dense == 1
