"""The host side of the Monte-Carlo replay's timing model (csrc/replay_plan.h, TIMING: the record, its refusals, the image table
of a sequence, the stencil rule, the preconditions of the shift) as a stand-alone host program, without a device."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

FLAGS = [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]]


@pytest.fixture(scope="module", params=FLAGS, ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("replay_timing") / "replay_timing_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-o", path, os.path.join(H.ROOT, "tests", "cpp", "replay_timing_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return path


def test_the_timing_record_the_table_and_the_preconditions(exe):
    """every refusal with its code and text in the stated order, a refused call leaves the previous record in force, the record
    stays through both assigns, a fault record and a commit, alloc clears it; the hand-traced image table; each precondition of
    the shift with the sequence, frame and track it names, only under a non-zero record"""
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "replay timing ok" in run.stdout, run.stdout + run.stderr


# the program's hand-traced sequence, for the twin: per frame None (skipped) or (readings [k][7], n_drop)
def _cell(dTs, drop):
    rd = np.zeros((len(dTs), 7))
    rd[:, 6] = dTs
    return rd, drop


HAND = [_cell([0.01, 0.02], 0), None, _cell([], 0), _cell([0.01, 0.01, 0.01], 2), _cell([0.04], 0), _cell([0.02, 0.03], 1), _cell([0.05], 0)]


def test_the_image_table_is_the_twins_and_the_hand_trace(exe):
    """the header's table of the hand-traced sequence (a skipped cell, an image without samples, drops of 2 and 1) against
    scenario.replay_image_table, the times bit for bit, and against the trace written out"""
    run = subprocess.run([exe, "table"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    img = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("image ")]
    base = [int(ln.split()[2]) for ln in run.stdout.splitlines() if ln.startswith("base ")]
    time, frame_of, tbase = sc.replay_image_table(HAND)
    assert [int(r[3]) for r in img] == list(frame_of) == [0, 2, 3, 4, 5, 6]
    assert np.array_equal(np.array([float(r[2]) for r in img]), time)
    assert base == list(tbase) == [0, 0, 0, 0, 2, 2, 3]
    assert time[0] == time[1] == 0.01 + 0.02 and np.allclose(time, [0.03, 0.03, 0.06, 0.10, 0.15, 0.20], rtol=1e-15, atol=0)
    # the window is a suffix of the images: slot s of frame f is image base[f] + s, the frame's own image the last
    W = [1, 0, 2, 3, 2, 3, 3]
    for f, c in enumerate(HAND):
        if c is not None:
            assert frame_of[tbase[f] + W[f] - 1] == f


def test_timing_seed_and_stencil_are_the_twins():
    """the literal sub-seeds the program asserts at compile time, and the stencil rule at the places it asserts"""
    want = {0x0: 0x61a685ffc80a8140, 0xC0FFEE00: 0x398ed654c613a63f, 0xFFFFFFFFFFFFFFFF: 0xec159351af424190}
    for s, v in want.items():
        assert int(sc.replay_mix(s, sc.REPLAY_TIMING_STREAM)) == v
    assert sc.REPLAY_TIMING_STREAM == (1 << 63) + 2 != sc.REPLAY_FAULT_STREAM
    assert [sc.replay_timing_stencil(l, 6) for l in range(6)] == [(0, 3), (0, 3), (1, 3), (2, 3), (3, 3), (3, 3)]
    assert [sc.replay_timing_stencil(l, 3) for l in range(3)] == [(0, 3)] * 3
    assert sc.replay_timing_stencil(1, 2) == (0, 2) and sc.replay_timing_stencil(0, 1) == (0, 1)
