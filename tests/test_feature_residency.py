"""Why k_feature_pair is built for four wavefronts per SIMD (msckf_mono_amd/csrc/update_routes.h: PAIR_WAVES_PER_SIMD and
feature_pair_residency), from a stand-alone host program without a device: sixteen wavefronts' LDS fits a compute unit at every
window length the kernel takes, a slice of 32 trajectories x 200 tracks fits the chip's slots in one residency at four
wavefronts per SIMD and does not at three."""
import os
import re
import subprocess

import pytest

import helpers as H

SRC = os.path.join(H.ROOT, "tests", "cpp", "feature_residency_host.cpp")
KERNELS = os.path.join(H.ROOT, "msckf_mono_amd", "csrc", "kernels_feature.hip")
COMPUTE_UNITS = 256          # MI355X
SLICE = (32, 200)            # the headline run's slice: trajectories, tracks per trajectory


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("residency") / "feature_residency_host")
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    out = subprocess.run([exe, str(SLICE[0]), str(SLICE[1]), str(COMPUTE_UNITS)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr
    return [dict(t.split("=") for t in l.split() if "=" in t) for l in out.stdout.splitlines()]


def test_sixteen_wavefronts_of_lds_fit_a_compute_unit(lines):
    head, rows = lines[0], [l for l in lines if "lm" in l]
    assert int(head["waves_per_simd"]) == 4 and int(head["simds_per_cu"]) == 4
    assert [int(r["lm"]) for r in rows] == list(range(2, int(head["m_reg"]) + 1))
    for r in rows:
        assert int(r["waves_per_cu"]) == 16 and r["same_as_launch"] == "1", r
        assert 16 * int(r["lds"]) <= int(head["feature_lds"]) and r["lds_fits"] == "1", r
    assert int(rows[-1]["lds"]) == 8952      # 30 cameras: 16 x 8 952 B = 143 KB of the 160 KB


def test_a_slice_fits_one_residency_at_four_wavefronts_per_simd_and_not_at_three(lines):
    four, three = [l for l in lines if "wavefronts" in l]
    waves = SLICE[0] * (SLICE[1] // 2)       # two tracks per wavefront
    assert int(four["waves_per_simd"]) == 4 and int(three["waves_per_simd"]) == 3
    assert int(four["wavefronts"]) == int(three["wavefronts"]) == waves == 3200
    assert int(four["slots"]) == COMPUTE_UNITS * 16 == 4096 and four["one_residency"] == "1"
    assert int(three["slots"]) == COMPUTE_UNITS * 12 == 3072 and three["one_residency"] == "0"


def test_the_kernel_reads_the_constant():
    src = open(KERNELS).read()
    att = re.findall(r"amdgpu_waves_per_eu\(([^()]*)\)\)\)\s*void k_feature_pair\(", src)
    assert att == ["routes::PAIR_WAVES_PER_SIMD, routes::PAIR_WAVES_PER_SIMD"], att
