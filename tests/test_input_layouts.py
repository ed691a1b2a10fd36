"""The staged input layouts (input_layouts.h: the single-call work-list block and its rules, the readings chunk, the scenario's
host store, a frame's sections resident and streamed) as a stand-alone host program: what the kernels read, without a device."""
import os
import subprocess

import pytest

import helpers as H


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]], ids=["plain", "sanitized"])
def test_the_input_layouts_alone(tmp_path, flags):
    """the section offsets of a streamed frame block and the single-call block at their spot cases, the work-list rules with
    their codes, texts and order, the readings chunks with and without counts, and every track of a small scenario read the
    way wl_first does through the resident arrays and through the frame blocks, before and after a patch; every block a heap
    block of exactly the size the header asked for, also under the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "input_layouts_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, os.path.join(H.ROOT, "tests", "cpp", "input_layouts_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "input layouts ok" in run.stdout, run.stdout + run.stderr
