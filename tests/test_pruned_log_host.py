"""CPU-side checks of the pruned-state log's boundary (msckf_hip_pruned_log_*, kernels_log.hip): the six entries are declared,
bound, exported and documented, the code object holds both kernels, the record's field table covers its 32 scalars, the
numpy reference of the pose error that the GPU tests use inverts the filter's own injection (np_oracle.update_quat), and
shard.ate_from_pruned_metrics adds sums and counts per sequence."""
import os
import re
import subprocess

import numpy as np
import pytest

import np_oracle
import pruned_log_ref as R
from msckf_mono_amd import scenario as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SUFFIXES = ("enable", "reset", "frames", "counts", "read", "metrics")
NAMES = ["msckf_hip_pruned_log_" + s for s in SUFFIXES]


@pytest.fixture(scope="module")
def hip_lib():
    from msckf_mono_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi


def test_header_binding_library_and_integration_name_the_same_six_entries(hip_lib):
    hdr = open(os.path.join(ROOT, "include", "msckf_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(msckf_hip_pruned_log_[a-z_0-9]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", hip_lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (msckf_hip_pruned_log_[a-z_0-9]+)", out))
    bound = set(s for s in hip_lib.SYMBOLS if s.startswith("msckf_hip_pruned_log_"))
    assert declared == exported == bound == set(NAMES), (declared, exported, bound)
    L = hip_lib.lib()
    for s in SUFFIXES:
        assert hasattr(L, "msckf_hip_pruned_log_" + s) and callable(getattr(hip_lib.Batch, "pruned_log_" + s)), s
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    row = next(ln for ln in doc.splitlines() if ln.startswith("| `msckf_hip_pruned_log_enable"))
    assert all("_" + s in row for s in SUFFIXES[1:]) and "k_pruned_log" in row and "k_pruned_metrics" in row, row
    for s in SUFFIXES:
        assert "bt.pruned_log_" + s + "(" in doc, s


def test_the_code_object_contains_both_kernels(hip_lib):
    data = open(hip_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"k_pruned_log" in data and b"k_pruned_metrics" in data


def test_the_field_table_covers_the_record_without_overlap(hip_lib):
    assert hip_lib.PRUNED_LOG_STRIDE == 32 and len(hip_lib.PRUNED_LOG_METRICS) == 10
    hit = np.zeros(32, dtype=int)
    for sl in hip_lib.PRUNED_LOG_FIELDS.values():
        hit[sl] += 1
    assert np.array_equal(hit, np.ones(32, dtype=int)), hit
    f = hip_lib.PRUNED_LOG_FIELDS
    assert f["q"] == slice(0, 4) and f["p"] == slice(4, 7) and f["frame"] == slice(7, 8) and f["cov"] == slice(8, 29)
    P = np.arange(27.0 * 27).reshape(27, 27)
    P = P + P.T
    assert np.array_equal(R.block6(R.triangle(P, 1)), P[21:27, 21:27])      # row by row, entries (r, c) with r <= c


def test_the_pose_error_inverts_the_filters_own_injection():
    """100 seeded random q_gt and e_th with |e_th| from 1e-3 to 0.3 rad: q = update_quat(e_th) * q_gt gives e_th back to 1e-12
    (update_quat's quaternion is exactly unit below |e_th| = 2, so the inversion is exact up to rounding), whichever sign
    the estimate's quaternion carries; the opposite sign and the opposite multiplication order miss by more than 1e-4 at
    0.3 rad."""
    rng = np.random.default_rng(20240611)
    worst = 0.0
    for i, mag in enumerate(np.geomspace(1e-3, 0.3, 100)):
        q_gt = rng.normal(size=4); q_gt /= np.linalg.norm(q_gt)
        e = rng.normal(size=3); e *= mag / np.linalg.norm(e)
        q_hat = np_oracle.qmul(np_oracle.update_quat(e), q_gt)
        for sign in (1.0, -1.0):
            got = R.angle_error(sign * q_hat, q_gt)
            worst = max(worst, float(np.abs(got - e).max()))
            assert np.allclose(got, e, rtol=0, atol=1e-12), (i, mag, got, e)
    print("pose error vs update_quat: worst |e_th - e| %.2e" % worst)
    e = np.array([0.3, 0.0, 0.0]) @ sc.quat_to_rot(q_gt)                      # 0.3 rad about a generic axis
    q_hat = np_oracle.qmul(np_oracle.update_quat(e), q_gt)
    assert np.abs(R.angle_error(q_hat, q_gt) - e).max() < 1e-12
    assert np.abs(-R.angle_error(q_hat, q_gt) - e).max() > 1e-4               # the opposite sign
    wrong = R.qmul(R.qinv(q_gt), q_hat)                                        # the opposite order: q_gt^-1 * q
    assert np.abs(-2.0 * wrong[1:4] / np.linalg.norm(wrong) * np.sign(wrong[0]) - e).max() > 1e-4


def test_numpy_metrics_on_a_hand_made_log():
    """two matched records (one with a block that has no Cholesky factor), one outside the ordinal range, one unmatched"""
    gt = np.zeros((3, 1, 7)); gt[:, 0, 0] = 1.0; gt[:, 0, 4] = [0.0, 1.0, 2.0]
    rec = np.zeros((4, 32)); rec[:, 0] = 1.0
    rec[:, 8:29] = R.triangle(np.eye(21) * 4.0, 0)
    rec[0, 4:7], rec[0, 7] = [0.0, 0.3, 0.4], 3
    rec[1, 4:7], rec[1, 7] = [1.0, 0.0, 2.0], 4
    rec[1, 8:29] = R.triangle(-np.eye(21), 0)
    rec[2, 7] = 9
    rec[3, 7] = 5
    out, _ = R.numpy_metrics(rec, [0, 1, 2, 7], 0, 3, 6, gt)
    assert np.allclose(out, [3, 2, 0.25 + 4.0, 2.0, 0, 0, 0.25 / 4.0, 1, 1, 1], rtol=1e-15, atol=0), out


def test_ate_from_pruned_metrics_adds_sums_and_counts_per_sequence():
    from msckf_mono_amd import shard
    m = np.zeros((3, 10))
    m[:, 0], m[:, 1], m[:, 2], m[:, 4] = [5, 6, 7], [4, 6, 2], [16.0, 6.0, 8.0], [0.04, 0.06, 0.02]
    acc = shard.ate_from_pruned_metrics(m, [1, 0, 1], 2)
    assert np.array_equal(acc, [[6.0, 6.0], [24.0, 6.0]])                     # matched records count, not the records in range
    assert np.allclose(shard.ate_allreduce(acc), [1.0, 2.0])
    ang = shard.ate_from_pruned_metrics(m, [1, 0, 1], 2, angle=True)
    assert np.allclose(ang, [[0.06, 6.0], [0.06, 6.0]]) and np.allclose(shard.ate_allreduce(ang), [0.1, 0.1])
    both = shard.ate_from_pruned_metrics(m[:1], [0], 1) + shard.ate_from_pruned_metrics(m[1:], [0, 0], 1)
    assert np.array_equal(both, shard.ate_from_pruned_metrics(m, [0, 0, 0], 1))   # ranks combine by addition
