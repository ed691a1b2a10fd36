"""The host side of the full-state NEES log, without a device: the numpy twin scenario.nees_record against an independent
solve on the double oracle's states, the condition of the inputs the GPU bar rests on, what a wrong definition would move, the
initial error drawn from P0, csrc/nees_plan.h as a stand-alone host program, and the binding.  Shapes and bounds:
tests/nees_lab.py."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import nees_lab as NL
import replay_model_lab as ML
from msckf_mono_amd import capi
from msckf_mono_amd import scenario as sc

FLAGS = [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]]


@pytest.fixture(scope="module")
def small(oracle_lib):
    return NL.small_records(oracle_lib)


@pytest.fixture(scope="module")
def replay(oracle_lib):
    return NL.replay_records(oracle_lib)


def _truth(r):
    return NL.with_walk(r["truth16"], r["walk"][r["f"] + 1]) if "walk" in r else r["truth16"]


def _rel(x, ref):
    return np.abs(x - ref) / np.maximum(np.abs(ref), 1e-300)     # (a bias column is exactly zero before the first update)


# ------------------------------------------------------------------------------------------------ 1. the twin
def test_the_twin_against_an_independent_solve(small, replay):
    """scenario.nees_record (the kernel's form: Cholesky of the correlation matrix column by column, a riding forward solve, a
    3 x 3 Cholesky per block) against z^T solve(C, z) and e_k^T solve(P_kk, e_k) by numpy's LU on every record of both
    geometries: rtol gpu_bar(kappa(C)); no record is flagged.  The error-state angle against the plain quaternion product:
    the plain product cancels down to e_th from numbers of size 1, so it is held to 4 eps absolute."""
    worst = 0.0
    for r in small + replay:
        cols, not_pd = sc.nees_record(r["imu16"], r["P"], _truth(r))
        e = sc.nees_error(r["imu16"], _truth(r))
        ref = NL.solve_columns(e, r["P"])
        bar = NL.gpu_bar(NL.corr_cond(r["P"]))
        assert not not_pd and np.all(cols >= 0) and cols[0] > 0, (r["b"], r["f"])      # (before the first update the bias errors are zero)
        worst = max(worst, float(np.max(np.abs(cols - ref) / np.maximum(ref, 1e-300))) / bar)
        assert np.all(np.abs(cols - ref) <= bar * ref), (r["b"], r["f"], cols, ref, bar)
        assert np.max(np.abs(e[:3] - NL.plain_error_angle(r["imu16"][:4], _truth(r)[:4]))) <= 4 * 2.0 ** -52, (r["b"], r["f"])
    print("twin vs independent solve, worst difference over its bar: %.3g" % worst)


def test_the_twin_flags_what_has_no_factor():
    """a non-positive diagonal entry, and an indefinite matrix with a positive diagonal: zeros and flag 1"""
    r = dict(imu16=sc.Trajectory(2, 300, 8, 0, 1).imu0[:16])
    P = np.diag(np.arange(1.0, 16.0))
    assert not sc.nees_record(r["imu16"], P, r["imu16"])[1]
    bad = P.copy(); bad[7, 7] = -7.0
    cols, flag = sc.nees_record(r["imu16"], bad, r["imu16"])
    assert flag and not cols.any()
    bad = P.copy(); bad[0, 4] = bad[4, 0] = 3.0                  # |P_04| > sqrt(P_00 P_44): no factor, and block 0 alone has one
    cols, flag = sc.nees_record(r["imu16"], bad, r["imu16"])
    assert flag and not cols.any()
    bad = P.copy(); bad[0, 1] = 2.0                              # only the upper triangle is read: block 0 loses its factor
    assert sc.nees_record(r["imu16"], bad, r["imu16"])[1]
    low = P.copy(); low[1, 0] = 2.0
    assert not sc.nees_record(r["imu16"], low, r["imu16"])[1]


# ------------------------------------------------------------------------------------------------ 2. the condition the bar rests on
def test_the_condition_of_every_record_of_the_lab(small, replay):
    """100 kappa(C) 2^-53 <= 1e-6 on every record of both geometries, so that the GPU test's bar means something"""
    kappa = np.array([NL.corr_cond(r["P"]) for r in small + replay])
    print("kappa(C): SMALL %.3g .. %.3g, replay %.3g .. %.3g" % (kappa[:len(small)].min(), kappa[:len(small)].max(), kappa[len(small):].min(), kappa[len(small):].max()))
    assert np.all(NL.gpu_bar(kappa) <= NL.COND_LIMIT), kappa.max()


# ------------------------------------------------------------------------------------------------ 3. mutants
@pytest.mark.parametrize("name, mutant, column", [("diagonal_only", NL.diagonal_only, 0), ("swapped_bg_v", NL.swapped_bg_v, 0),
                                                   ("swapped_bg_v", NL.swapped_bg_v, 2), ("opposite_angle", NL.opposite_angle, 0)])
def test_a_wrong_definition_moves_a_column_by_ten_bars(small, replay, name, mutant, column):
    """NEES from the diagonal alone, b_g and v swapped in e, e_th with the opposite sign: at every frame from 1 on of both
    geometries the named column moves by at least 10 gpu_bar(kappa(C))"""
    least = np.inf
    for r in small + replay:
        if r["f"] < 1:
            continue
        e = sc.nees_error(r["imu16"], _truth(r))
        ref, got = NL.solve_columns(e, r["P"]), mutant(e, r["P"])
        ratio = _rel(got[column], ref[column]) / NL.gpu_bar(NL.corr_cond(r["P"]))
        least = min(least, ratio)
        assert ratio >= 10.0, (name, r["b"], r["f"], ratio)
    print("%s column %d: moved by at least %.3g bars" % (name, column, least))


@pytest.mark.parametrize("name", ["no_walk", "row_f"])
def test_a_wrong_walk_row_moves_the_bias_columns_by_ten_bars(replay, name):
    """The walk not added, or row f in place of row f + 1, on the trajectories whose Q_imu has walk blocks (0 and 2): columns 0,
    2 and 4 each move by at least 10 gpu_bar(kappa(C)) at every frame from 1 on -- for row f, at every such frame whose cell has
    samples (a cell with k = 0 and a skipped cell leave the walk where it was: rows f and f + 1 are equal there)"""
    least, seen = np.inf, 0
    for r in replay:
        f, W = r["f"], r["walk"]
        if r["b"] == 1 or f < 1:
            continue
        wrong = r["truth16"] if name == "no_walk" else NL.with_walk(r["truth16"], W[f])
        if name == "row_f" and np.array_equal(W[f], W[f + 1]):
            assert ML.k_of(ML.SEQ_OF[r["b"]], f) <= 0
            continue
        ref = NL.solve_columns(sc.nees_error(r["imu16"], _truth(r)), r["P"])
        got = NL.solve_columns(sc.nees_error(r["imu16"], wrong), r["P"])
        ratio = _rel(got[[0, 2, 4]], ref[[0, 2, 4]]) / NL.gpu_bar(NL.corr_cond(r["P"]))
        least, seen = min(least, float(ratio.min())), seen + 1
        assert np.all(ratio >= 10.0), (name, r["b"], f, ratio)
    assert seen >= 2 * (NL.NF_REPLAY - 4)
    print("%s: columns 0, 2, 4 moved by at least %.3g bars" % (name, least))


def test_replay_bias_gt_is_the_truth_the_walk_rows_give(replay):
    """scenario.replay_bias_gt on the twin's walks is with_walk(row f + 1): what the device adds under add_walk"""
    nf = NL.NF_REPLAY
    paths = [ML._paths(nf)[s] for s in ML.SEQ_OF]
    gt = sc.replay_bias_gt(paths, np.stack([ML.twin_walk(nf, b) for b in range(ML.B)], axis=1))
    for r in replay:
        t = _truth(r)
        assert np.array_equal(gt[r["f"], r["b"]], np.concatenate([t[4:7], t[10:13]]))


# ------------------------------------------------------------------------------------------------ 4. the initial error
def test_the_initial_error_is_drawn_from_p0_and_comes_back_out():
    """e0 = L0 z with z the first 15 normals of the sub-seed mix(seed, 2^63) and L0 = chol_psd(P0): L0 L0^T = P0, another seed
    another draw, a semi-definite P0 draws zero where it is zero.  perturbed_imu29 puts e0 in: the additive parts come back
    to one rounding of the sum (half an ulp of the perturbed value: (x + e) - x is exact once x + e is rounded), e_th within
    |e_th|^3 / 8 (buildUpdateQuat normalises); the null-space anchors are the perturbed values."""
    tr = NL.small_trajs()[0]
    P0 = np.diag(np.asarray(tr.cfg["P0_diag"], dtype=np.float64))
    P0[3:6, 6:9] = P0[6:9, 3:6] = 2e-3 * np.eye(3)
    L0 = sc.chol_psd(P0, "P0")
    assert np.max(np.abs(L0 @ L0.T - P0)) <= 1e-15 * P0.max()
    z = sc.replay_pairs(int(sc.replay_mix(77, 2 ** 63)), 8).reshape(-1)[:15]
    e0 = sc.replay_initial_error(77, P0)
    assert np.allclose(e0, L0 @ z, rtol=0, atol=8 * 2.0 ** -53 * np.abs(L0) @ np.abs(z))
    assert not np.array_equal(e0, sc.replay_initial_error(78, P0))
    assert int(sc.replay_mix(77, 2 ** 63)) not in [int(s) for f in range(4096) for s in sc.replay_subseeds(77, f)]
    semi = P0.copy(); semi[12:, :] = 0.0; semi[:, 12:] = 0.0
    assert not sc.replay_initial_error(77, semi)[12:].any()
    assert np.array_equal(sc.replay_noise_factor(ML.q_dense()), sc.chol_psd(ML.q_dense()))
    for scale in (1.0, 30.0):                                      # |e_th| about 3e-3 and 0.1 rad
        e = e0.copy(); e[:3] *= scale
        s = sc.perturbed_imu29(tr.imu0, e)
        back = sc.nees_error(s[:16], tr.imu0[:16])
        assert np.all(np.abs(back[3:] - e[3:]) <= 0.5 * np.spacing(np.abs(s[4:16]))), scale
        th = np.linalg.norm(e[:3])
        assert np.linalg.norm(back[:3] - e[:3]) <= th ** 3 / 8 + 4 * 2.0 ** -52, (scale, back[:3] - e[:3])
        assert np.array_equal(s[19:23], s[0:4]) and np.array_equal(s[23:26], s[7:10]) and np.array_equal(s[26:29], s[13:16])
        assert np.array_equal(s[16:19], tr.imu0[16:19]) and abs(np.linalg.norm(s[:4]) - 1.0) <= 2.0 ** -52


def test_the_truth_table_of_a_batch():
    """scenario.imu_state_gt: [frames][B][16] = q_IG b_g v b_a p of gt_frames and the constant biases, unit quaternions"""
    trajs = NL.small_trajs()
    t = sc.imu_state_gt(trajs, 3, 9)
    assert t.shape == (6, len(trajs), 16)
    for b, tr in enumerate(trajs):
        assert np.array_equal(t[:, b, 0:4], tr.gt_frames["q_IG"][3:9]) and np.array_equal(t[:, b, 13:16], tr.gt_frames["p"][3:9])
        assert np.array_equal(t[:, b, 7:10], tr.gt_frames["v"][3:9])
        assert np.all(t[:, b, 4:7] == tr.b_g) and np.all(t[:, b, 10:13] == tr.b_a)
    assert np.max(np.abs(np.linalg.norm(t[..., :4], axis=-1) - 1.0)) <= 1e-12


# ------------------------------------------------------------------------------------------------ 5. csrc/nees_plan.h on its own
@pytest.fixture(scope="module", params=FLAGS, ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("nees_plan") / "nees_plan_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-o", path, os.path.join(H.ROOT, "tests", "cpp", "nees_plan_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return path


def test_the_plan_alone(exe):
    """the strides, and every refusal of truth_set, the reserve, the read and the ensemble with its code, text and order"""
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "nees plan ok" in run.stdout, run.stdout + run.stderr


def test_the_column_table_is_the_bindings(exe):
    """the header's column table against capi.NEES_LOG_FIELDS / NEES_ENSEMBLE_FIELDS and the flag bits"""
    run = subprocess.run([exe, "--columns"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = {ln.split()[0]: ln.split()[1:] for ln in run.stdout.splitlines()}
    rec = dict(zip(rows["record"][1::2], map(int, rows["record"][2::2])))
    assert int(rows["record"][0]) == capi.NEES_LOG_STRIDE == 8
    assert capi.NEES_LOG_FIELDS["nees"] == slice(rec["nees"], rec["nees"] + 1) and capi.NEES_LOG_FIELDS["nees_theta"].start == rec["blocks"]
    assert capi.NEES_LOG_FIELDS["frame"].start == rec["frame"] and capi.NEES_LOG_FIELDS["flags"].start == rec["flags"]
    assert [capi.NEES_LOG_FIELDS[k].start for k in ("nees_theta", "nees_b_g", "nees_v", "nees_b_a", "nees_p")] == list(range(rec["blocks"], rec["frame"]))
    assert rows["flag"] == ["not_pd", str(capi.NEES_FLAG_NOT_PD), "skipped", str(capi.NEES_FLAG_SKIPPED), "stat_err", str(capi.NEES_FLAG_STAT_ERR)]
    ens = dict(zip(rows["ensemble"][1::2], map(int, rows["ensemble"][2::2])))
    assert int(rows["ensemble"][0]) == capi.NEES_ENSEMBLE_STRIDE == 14
    f = capi.NEES_ENSEMBLE_FIELDS
    assert (f["n"].start, f["n_flagged"].start, f["sum"], f["sum_sq"]) == (ens["n"], ens["flagged"], slice(ens["sum"], ens["sum_sq"]), slice(ens["sum_sq"], 14))
    assert rows["truth"] == ["16", "walk", "6"]


# ------------------------------------------------------------------------------------------------ 6. the binding
def test_the_binding_has_the_new_entries():
    for name in ("truth_set", "nees_log_enable", "nees_log_reset", "nees_log_count", "nees_log_read", "nees_log_ensemble"):
        assert callable(getattr(capi.Batch, name, None)), name
    for name in ("msckf_hip_truth_set", "msckf_hip_nees_log_enable", "msckf_hip_nees_log_reset", "msckf_hip_nees_log_count", "msckf_hip_nees_log_read",
                 "msckf_hip_nees_log_ensemble"):
        assert name in capi.SYMBOLS, name
    assert len(capi.NEES_LOG_FIELDS) == 8 and sorted(s.start for s in capi.NEES_LOG_FIELDS.values()) == list(range(8))
