"""The host side of the Monte-Carlo replay's fault model (csrc/replay_plan.h, FAULTS: the fault record, its refusals, the
sub-seed, the rule on a track) as a stand-alone host program, without a device."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

FLAGS = [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]]


@pytest.fixture(scope="module", params=FLAGS, ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("replay_faults") / "replay_faults_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-o", path, os.path.join(H.ROOT, "tests", "cpp", "replay_faults_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return path


def test_the_fault_record_alone(exe):
    """every refusal with its code and text in the stated order, a refused call leaves the previous record in force, the record
    stays through replay_assign, replay_assign_q and a commit, alloc clears it; the rule on a track against its definition"""
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "replay faults ok" in run.stdout, run.stdout + run.stderr


def test_fault_seed_is_the_twins(exe):
    """fault_seed(s, f) of the header against scenario.replay_fault_seed at the three values the program also asserts at compile
    time, and at a few more that wrap"""
    pairs = [(0x0, 0), (0xC0FFEE00, 7), (0xFFFFFFFFFFFFFFFF, 199), (0x9E3779B97F4A7C15, 1), (0x123456789ABCDEF0, 65535)]
    args = [x for s, f in pairs for x in ("%x" % s, str(f))]
    run = subprocess.run([exe, "seed"] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("seed ")]
    assert len(lines) == len(pairs)
    for (s, f), (_, hs, hf, hv) in zip(pairs, lines):
        assert (int(hs, 16), int(hf)) == (s, f)
        assert int(hv, 16) == sc.replay_fault_seed(s, f), (hs, hf)
    assert [int(ln[3], 16) for ln in lines[:3]] == [0xb39eedfc2740d498, 0xf41882913a46030b, 0xdbf3bb1f8a55d8db]


def test_the_rule_on_a_track_is_the_twins(exe):
    """track_faults (what the two device reductions call) against scenario.replay_fault_code on single tracks that start at
    entry e0 of a cell: the twin draws the whole cell, the header only the track's entries"""
    seed, frame = 0xC0FFEE03, 11
    for e0, M, pm, po in ((0, 5, 0.3, 0.5), (12, 2, 0.6, 0.2), (7, 1, 1.0, 1.0), (3, 6, 1.0, 0.4), (40, 9, 0.5, 0.0), (0, 0, 0.5, 0.5)):
        run = subprocess.run([exe, "track", "%x" % seed, str(frame), str(e0), str(M), repr(pm), repr(po)], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        draws = [d[e0:] for d in sc.replay_fault_draws(seed, frame, e0 + M)]
        code = sc.replay_fault_code([M], draws, pm, po)
        assert run.stdout.split() == ["track", str(int((code == sc.FAULT_MISSED).sum())), str(int((code == sc.FAULT_OUTLIER).sum()))], (e0, M, pm, po)
        assert M - int((code == sc.FAULT_MISSED).sum()) >= min(M, 2)
    assert np.array_equal(sc.replay_fault_code([3], ([0.0, 0.0, 0.9], [1.0] * 3, [0.0] * 3), 0.5, 0.5), [0, 0, 0])      # 3 - 2 < 2: loses none
    assert np.array_equal(sc.replay_fault_code([3], ([0.0, 0.6, 0.9], [0.0] * 3, [0.0] * 3), 0.5, 0.5), [2, 1, 1])
