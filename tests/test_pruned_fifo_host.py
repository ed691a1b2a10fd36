"""The pruned-state log's host mirror (host_lists.h, PrunedFifo) as a stand-alone host program: which image's camera a record
is, without a device."""
import os
import subprocess

import pytest

import helpers as H


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]], ids=["plain", "sanitized"])
def test_the_pruned_fifo_alone(tmp_path, flags):
    """an augment pushes the frame's ordinal, a drop pops the oldest into the stored records' ordinals until the capacity is
    reached, a window that changed behind the log's back holds unknown states; also under the address and
    undefined-behaviour sanitizers"""
    exe = str(tmp_path / "pruned_fifo_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, os.path.join(H.ROOT, "tests", "cpp", "pruned_fifo_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "pruned fifo ok" in run.stdout, run.stdout + run.stderr
