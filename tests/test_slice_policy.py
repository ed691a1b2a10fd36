"""The slice policy of the frame loops (msckf_mono_amd/csrc/slice_policy.h) as a stand-alone host program: how many slices a
request runs on how many hardware queues, and what the text of GPU_MAX_HW_QUEUES parses to, without a device.
tests/cpp/slice_policy_host.cpp holds the checks; it is built plain and under the address and undefined-behaviour sanitizers
and run directly."""
import os
import subprocess

import pytest

import helpers as H

SRC = os.path.join(H.ROOT, "tests", "cpp", "slice_policy_host.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]}


def build_policy_program(directory, flags=("-O2",)):
    exe = os.path.join(str(directory), "slice_policy_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(flags) + ["-o", exe, SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def policy_table(exe):
    """(requested, B, process budget, streamed) -> slices, for the cases of tests/test_gpu_slice_policy.py"""
    out = subprocess.run([exe, "--table"], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr
    table = {}
    for line in out.stdout.splitlines():
        left, n = line.split(" : ")
        table[tuple(int(x) for x in left.split())] = int(n)
    return table


@pytest.mark.parametrize("flags", list(FLAGS))
def test_slice_policy_header_alone(tmp_path, flags):
    exe = build_policy_program(tmp_path, FLAGS[flags])
    env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0 and run.stdout.strip() == "slice policy ok", (run.returncode, run.stdout, run.stderr)


def test_the_table_of_the_gpu_cases(tmp_path):
    t = policy_table(build_policy_program(tmp_path))
    assert len(t) == 24
    for (req, B, budget, streamed), n in t.items():
        assert 1 <= n <= min(req, B)
        if budget == 8:
            assert n == min(req, B)          # queues are plentiful: the count is the request, as before there was a policy
    assert t[(4, 8, 4, 1)] < 4 and t[(4, 8, 4, 0)] < 4      # 4 slices do not fit the runtime's default of 4 queues
