"""CPU-side checks of the map log's boundary (msckf_hip_map_log_*, kernels_log.hip): the six entries are declared, bound
and exported, the code object holds both kernels, the record's field table covers its eight scalars, and
scenario.landmark_csr lays the ground-truth landmarks out cell by cell."""
import os
import re
import subprocess

import numpy as np
import pytest

from msckf_mono_amd import scenario as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["msckf_hip_map_log_" + s for s in ("enable", "reset", "frames", "counts", "read", "metrics")]


@pytest.fixture(scope="module")
def hip_lib():
    from msckf_mono_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi


def test_the_six_entries_are_declared_bound_and_exported(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "msckf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(msckf_hip_[a-z_0-9]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (msckf_hip_[a-z_0-9]+)", out))
    L = hip_lib.lib()
    for s in NAMES:
        assert s in declared, s
        assert s in hip_lib.SYMBOLS, s
        assert s in exported and hasattr(L, s), s
    for m in ("map_log_enable", "map_log_reset", "map_log_frames", "map_log_counts", "map_log_read", "map_log_metrics"):
        assert callable(getattr(hip_lib.Batch, m)), m


def test_the_code_object_contains_both_kernels(hip_lib):
    data = open(hip_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"k_map_log" in data and b"k_map_metrics" in data


def test_the_field_table_covers_the_record_without_overlap(hip_lib):
    assert sorted(hip_lib.MAP_LOG_FIELDS) == sorted(["p", "gamma", "frame", "track", "flags", "M"])
    hit = np.zeros(8, dtype=int)
    for sl in hip_lib.MAP_LOG_FIELDS.values():
        hit[sl] += 1
    assert np.array_equal(hit, np.ones(8, dtype=int)), hit
    assert hip_lib.MAP_LOG_FIELDS["p"] == slice(0, 3)


def test_landmark_csr_lays_the_cells_out_frame_by_frame():
    """two trajectories with different track counts, frames [2, 7): the window has fewer than four cameras on frames 0..2, so
    the range starts with an empty cell"""
    trajs = [sc.Trajectory(2, 300, 8, 5, 7), sc.Trajectory(2, 301, 8, 9, 7)]
    f0, f1, B = 2, 7, 2
    xyz, off = sc.landmark_csr(trajs, f0, f1)
    assert off.shape == ((f1 - f0) * B + 1,) and off[0] == 0 and np.all(np.diff(off) >= 0)
    assert xyz.shape == (off[-1], 3) and xyz.dtype == np.float64
    for k in range(f0, f1):
        for b, tr in enumerate(trajs):
            cell = (k - f0) * B + b
            assert off[cell + 1] - off[cell] == len(tr.frames[k]["M"]), (k, b)
            assert np.array_equal(xyz[off[cell]:off[cell + 1]], tr.landmarks[k]), (k, b)
    assert off[1] == 0 and off[-1] == 4 * (5 + 9)      # frame 2: Nw = 3, no tracks; frames 3..6: F tracks each
    e_xyz, e_off = sc.landmark_csr(trajs, 3, 3)
    assert e_xyz.shape == (0, 3) and np.array_equal(e_off, [0])
