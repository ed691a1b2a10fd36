"""The Monte-Carlo replay's host side (csrc/replay_plan.h: the integer part of the random stream, the sequence store, the
assignment, every frame's bases and block size, the refusals) as a stand-alone host program, without a device."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import replay_lab as RL
from msckf_mono_amd import scenario as sc

FLAGS = [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]]


@pytest.fixture(scope="module", params=FLAGS, ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("replay_plan") / "replay_plan_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-o", path, os.path.join(H.ROOT, "tests", "cpp", "replay_plan_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return path


def test_the_replay_plan_alone(exe):
    """the integer part at literal values (compile time and run time), a small plan -- frames without an entry, a sequence with
    F == f_cap tracks beside one with none, a skipped sequence cell, a second assignment, a patched cell -- with its bases,
    sizes and the ordinary FrameLayout behind them, and every refusal with its code, text and order"""
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "replay plan ok" in run.stdout, run.stdout + run.stderr


def test_mix_and_uniform_are_splitmix64_bit_for_bit(exe):
    """mix(seed, i) and U(seed, i) of the header against scenario.SplitMix64 itself (one generator per value, advanced by hand:
    a stream cannot be asked for value 2^64 - 2 by drawing), for seeds and indices that include index 0 and seed + (i + 1) gamma
    wrapping past 2^64; and the twin's replay_mix / replay_uniform against the same"""
    run = subprocess.run([exe, "mix"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [ln.split() for ln in run.stdout.splitlines() if ln.startswith("mix ")]
    assert len(lines) == 64
    wrapped = 0
    for _, s, i, v, u in lines:
        seed, idx = int(s, 16), int(i, 16)
        rng = sc.SplitMix64(seed)
        rng.ctr = idx                                  # the next value drawn is value idx
        assert int(rng.u64(1)[0]) == int(v, 16), (s, i)
        rng.ctr = idx
        assert float(rng.uniform(1)[0]) == float.fromhex(u), (s, i)
        assert int(sc.replay_mix(seed, idx)) == int(v, 16) and float(sc.replay_uniform(seed, idx)) == float.fromhex(u), (s, i)
        wrapped += seed + (idx + 1) * 0x9E3779B97F4A7C15 >= 1 << 64
    assert any(int(i, 16) == 0 for _, _, i, _, _ in lines) and wrapped > 32


def test_bases_and_block_sizes_of_the_common_shape(exe, tmp_path):
    """the header's per-frame bases (a prefix sum of entries(seq_of[b], f) over the non-monotone seq_of), expanded entries and
    block sizes at the common shape against numpy and the layout rule written out here: the first three frames hold no entry,
    the two sequences' counts differ from frame 4 on, so every trajectory's base differs from its neighbours'"""
    seqs = RL.sequences()
    path = str(tmp_path / "cells.txt")
    with open(path, "w") as fh:
        fh.write("%d %d %d %d %d %d %d\n" % (len(seqs), RL.NF, sc.IMU_PER_FRAME, RL.B, RL.F_CAP, RL.M_CAP, RL.N_CAP))
        fh.write(" ".join(str(s) for s in RL.SEQ_OF) + "\n")
        for f in range(RL.NF):
            for s, tr in enumerate(seqs):
                fr = tr.frames[f]
                fh.write(" ".join(str(int(x)) for x in [f, s, len(fr["M"])] + list(fr["M"]) + list(fr["slots"])) + "\n")
    run = subprocess.run([exe, "plan", path], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = [ln.split() for ln in run.stdout.splitlines()]
    frames = [r for r in rows if r[0] == "frame"]
    assert len(frames) == RL.NF

    def up(x, a=256):
        return (x + a - 1) // a * a

    def block_bytes(nf, esz):          # [rd | n | drop | k | M | off | slots | obs], each at a 256-byte offset
        o = 0
        for per in (7 * sc.IMU_PER_FRAME * esz, 4, 4, 4, 4 * RL.F_CAP, 4 * RL.F_CAP):
            o = up(o + RL.B * per)
        return up(up(o + 4 * nf) + 2 * nf * esz)

    largest, differing = 0, 0
    for f, r in enumerate(frames):
        cnt = [int(seqs[s].frames[f]["M"].sum()) for s in RL.SEQ_OF]
        base = np.concatenate([[0], np.cumsum(cnt)])
        assert [int(x) for x in r[1:5]] == [f, int(base[-1]), block_bytes(int(base[-1]), 4), block_bytes(int(base[-1]), 8)], f
        assert [int(x) for x in r[5:]] == [int(x) for x in base[:-1]], f
        largest = max(largest, int(base[-1]))
        differing += len(set(cnt)) > 1
        if f < 3:
            assert base[-1] == 0
    assert differing >= 8
    assert [int(x) for x in rows[-1][1:]] == [largest, block_bytes(largest, 4), block_bytes(largest, 8)] and rows[-1][0] == "largest"
