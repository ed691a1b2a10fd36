"""The aligned trajectory error without a device: the numpy twin trajeval against an SVD, a brute-force scan and known transforms
written here, the hand cases of tests/traj_lab.py and what makes them sensitive, csrc/traj_plan.h as a stand-alone host program
(plain and under the address and undefined-behaviour sanitizers) against the twin on the bar of traj_lab, and the binding."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import traj_lab as TL
from msckf_mono_amd import asl
from msckf_mono_amd import capi
from msckf_mono_amd import scenario as sc
from msckf_mono_amd import trajeval as te

FLAGS = [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]]
LD = np.longdouble


@pytest.fixture(scope="module")
def cases():
    return TL.hand_cases()


def _col(c, name):
    b = c["name"].index(name)
    return c["est"][c["r0b"][b]:c["r1b"][b], b], c["gt"][c["r0b"][b]:c["r1b"][b], b]


def _kabsch(p, g, fix=True):
    """R minimising sum |g_c - R p_c|^2 by the SVD of sum g_c p_c^T; fix: the determinant fix-up that makes it a rotation"""
    pc, gc = p - p.mean(0), g - g.mean(0)
    U, _, Vt = np.linalg.svd(gc.T @ pc)
    D = np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) if fix else np.eye(3)
    return U @ D @ Vt


# ------------------------------------------------------------------------------------------------ 1. the twin is right
def test_se3_is_kabsch_with_the_determinant_fix(cases):
    """every hand case with a unique minimiser: Horn's quaternion gives the rotation of the SVD with the fix-up (4e-13: two
    eigen-decompositions of well-separated problems), det R = 1, and t = gbar - R pbar"""
    seen = 0
    for name in cases["name"]:
        est, gt = _col(cases, name)
        row = te.align(est, gt, te.ALIGN_SE3)
        R = row[1:10].reshape(3, 3)
        assert abs(np.linalg.det(R) - 1.0) < 1e-14 and np.max(np.abs(R @ R.T - np.eye(3))) < 1e-14, name
        if len(est) < 3 or row[13] < 1e-3:
            continue
        seen += 1
        p, g = est[:, 4:7], gt[:, 4:7]
        assert np.max(np.abs(R - _kabsch(p, g))) < (4e-13 if name != "c" else 1e-9), (name, R, _kabsch(p, g))
        assert np.max(np.abs(row[10:13] - (g.mean(0) - R @ p.mean(0)))) <= 1e-9 * max(1.0, np.abs(g).max()), name
        e = p @ R.T + row[10:13] - g
        assert abs(row[14] - np.sum(e * e)) <= 1e-6 * row[14] + (1e-3 if name == "c" else 0.0), name
    assert seen >= 8


def test_the_reflection_case_is_one(cases):
    """(b): the plain SVD, without the fix-up, gives det = -1; the twin's R is the rotation of the fixed SVD"""
    est, gt = _col(cases, "b")
    assert np.linalg.det(_kabsch(est[:, 4:7], gt[:, 4:7], fix=False)) < -0.999
    row = te.align(est, gt, te.ALIGN_SE3)
    assert abs(np.linalg.det(row[1:10].reshape(3, 3)) - 1.0) < 1e-14 and row[13] > 0.1


def test_yaw_against_a_scan_of_theta(cases):
    """the criterion sum |g_c - Rz(theta) p_c|^2 scanned over 20001 angles: none is below the twin's by more than rounding, and
    the best of the scan lies within one step of the twin's theta (modulo 2 pi)"""
    th = np.linspace(-np.pi, np.pi, 20001)
    for name in ("a129", "a64", "b", "e+1", "e-1", "g"):
        est, gt = _col(cases, name)
        row = te.align(est, gt, te.ALIGN_YAW)
        R = row[1:10].reshape(3, 3)
        assert R[2, 2] == 1.0 and not R[2, :2].any() and not R[:2, 2].any(), name
        pc, gc = est[:, 4:7] - est[:, 4:7].mean(0), gt[:, 4:7] - gt[:, 4:7].mean(0)
        c, s = np.cos(th)[:, None], np.sin(th)[:, None]
        cost = np.sum((gc[None, :, 0] - (c * pc[None, :, 0] - s * pc[None, :, 1])) ** 2 + (gc[None, :, 1] - (s * pc[None, :, 0] + c * pc[None, :, 1])) ** 2, axis=1) + np.sum((gc[:, 2] - pc[:, 2]) ** 2)
        assert cost.min() >= row[14] * (1 - 1e-12) - 1e-12, (name, cost.min(), row[14])
        d = th[np.argmin(cost)] - np.arctan2(R[1, 0], R[0, 0])
        assert abs((d + np.pi) % (2 * np.pi) - np.pi) <= 1.01 * (th[1] - th[0]), name
        assert 0.0 < row[13] <= 1.0


def test_yaw_next_to_plus_and_minus_pi(cases):
    """(e): theta = +-(pi - 1e-9) comes back with its sign, the two rows mirror each other, no jump in R"""
    for name, sign in (("e+1", 1.0), ("e-1", -1.0)):
        est, gt = _col(cases, name)
        R = te.align(est, gt, te.ALIGN_YAW)[1:10].reshape(3, 3)
        assert R[0, 0] < -0.999 and abs(R[1, 0]) < 0.05
    clean = TL.helix()
    for sign in (1.0, -1.0):
        R0 = TL.rot_z(sign * (np.pi - 1e-9))
        row = te.align(te.transformed(clean, R0.T, -R0.T @ TL.T0), clean, te.ALIGN_YAW)
        assert np.sign(row[4]) == sign and np.max(np.abs(row[1:10].reshape(3, 3) - R0)) < 1e-14      # R[1, 0] = sin theta


@pytest.mark.parametrize("mode, R0", [(te.ALIGN_YAW, TL.R_YAW), (te.ALIGN_SE3, TL.R_GENERAL), (te.ALIGN_SE3, TL.R_YAW)])
def test_a_known_transform_comes_back_attitudes_included(mode, R0):
    """a noise-free estimate in a frame that is off by (R0, t0): R = R0, t = t0, zero position AND zero attitude error -- the latter
    pins the quaternion convention (the aligned attitude is C(q) R^T, R's quaternion is Hamilton, g ~ R p + t); mode 0 sees the
    offset in both"""
    gt = TL.helix()
    est = te.transformed(gt, R0.T, -R0.T @ TL.T0)
    row = te.align(est, gt, mode)
    assert np.max(np.abs(row[1:10].reshape(3, 3) - R0)) < 1e-14 and np.max(np.abs(row[10:13] - TL.T0)) < 1e-13
    assert row[0] == TL.N_REC and row[13] > 0.5
    assert row[14] < 1e-26 and row[15] < 1e-14 and row[17] < 1e-28 and row[18] < 1e-14, row[14:19]
    raw = te.align(est, gt, te.ALIGN_NONE)
    assert raw[14] == raw[19] == row[19] and raw[14] > 100.0 and raw[17] > 1.0 and np.array_equal(raw[1:10], np.eye(3).ravel()) and not raw[10:14].any()
    # the opposite convention would leave an attitude error of the size of R0's angle
    wrong = te.error_angle(te.quat_mul(est[:, 0:4], sc.rot_to_quat(R0)[None, :]), gt[:, 0:4])
    assert np.sqrt(np.sum(wrong * wrong, axis=1)).min() > 0.5


def test_rpe_does_not_see_a_global_transform(cases):
    """the rows of rpe are unchanged (to rounding of the transform itself) when the ground truth is moved by a global SE(3)
    transform; the pair counts are n - lag, zero for a lag beyond the trajectory; a perfect estimate has zero error"""
    est, gt = _col(cases, "a129")
    a = te.rpe(est, gt, TL.LAGS)
    b = te.rpe(est, te.transformed(gt, TL.R_GENERAL, np.array([10.0, -20.0, 5.0])), TL.LAGS)
    assert np.array_equal(a[:, 0], [128, 127, 124, 65, 0]) and not a[4].any()
    assert np.all(a[:4, 1:] > 0) and np.allclose(a, b, rtol=1e-9, atol=0)
    assert np.max(np.abs(te.rpe(gt, gt, TL.LAGS))[:, 1:]) < 1e-28
    far_e, far_g = _col(cases, "c")
    assert np.all(te.rpe(far_e, far_g, (1, 5))[:, 1] > 0)


def test_the_flat_cases(cases):
    """(f) yaw mode without horizontal extent, n <= 1, identical points: R = I and cond = 0 exactly; (d) collinear under SE(3): cond ~ 0
    and the criterion's value is that of any minimiser"""
    est, gt = _col(cases, "f")
    for dtype in (np.float64, LD):
        row = te.align(est, gt, te.ALIGN_YAW, dtype)
        assert np.array_equal(row[1:10], np.eye(3).ravel()) and row[13] == 0, dtype
        assert np.array_equal(np.asarray(row[10:12], dtype=np.float64), [1.5 + 0.75, -2.25 - 4.0])
    for name in ("a0", "a1"):
        for mode in (1, 2):
            row = te.align(*_col(cases, name), mode)
            assert np.array_equal(row[1:10], np.eye(3).ravel()) and row[13] == 0 and row[14] == 0
    est, gt = _col(cases, "d")
    row = te.align(est, gt, te.ALIGN_SE3)
    assert row[13] < 1e-12
    s_e, s_g = est[:, 5] - est[:, 5].mean(), (gt[:, 4:7] - gt[:, 4:7].mean(0)) @ np.array([0.6, 0.0, 0.8])
    assert abs(row[14] - np.sum((s_e - s_g) ** 2)) < 1e-12


def test_a_raw_moment_pass_two_misses_the_bar_on_the_far_helix(cases):
    """(c): the twin with pass 2 expanded from raw moments, held to the bar like a device result, fails on R and on sum |e|^2 by
    orders of magnitude; the centred float64 twin is the bar's own yardstick and the hand cases' other trajectories do not notice"""
    b = cases["name"].index("c")
    sl = slice(b, b + 1)
    est, gt, r0b, r1b = cases["est"][:, sl], cases["gt"][:, sl], cases["r0b"][sl], cases["r1b"][sl]
    scale = TL.scales(est, gt, r0b, r1b)
    for mode in (te.ALIGN_YAW, te.ALIGN_SE3):
        ld, f64 = TL.twin_align(est, gt, r0b, r1b, mode, LD), TL.twin_align(est, gt, r0b, r1b, mode, np.float64)
        raw = TL.twin_align(est, gt, r0b, r1b, mode, np.float64, centred=False)
        with pytest.raises(AssertionError):
            TL.check_align(raw, f64, ld, scale, "raw moments")
        got, own = TL.align_distance(raw, ld, scale), TL.align_distance(f64, ld, scale)
        print("mode %d: raw-moment R off by %.3g (centred %.3g), sum |e|^2 by %.3g (centred %.3g)" % (mode, got["R"][0], own["R"][0], got["sum_sq"][0], own["sum_sq"][0]))
        assert got["R"][0] > 1e6 * TL.MULTIPLE_R * max(own["R"][0], TL.floor_of(scale)[0])


def test_the_float64_twin_against_the_longdouble_twin(cases):
    """the yardstick itself on every hand case and mode: the float64 twin's scaled distance from the longdouble twin is below 1e-9
    on every aligned column wherever R is unique or flat (1e-13 on R where three noisy points leave cond at 4e-3; 8e-11 on t and the
    lengths of the far helix, a million metres on an extent of 3), and longdouble is the wider type here"""
    assert np.finfo(LD).eps < 2.0 ** -60
    scale = TL.scales(cases["est"], cases["gt"], cases["r0b"], cases["r1b"])
    for mode in (0, 1, 2):
        ld = TL.twin_align(cases["est"], cases["gt"], cases["r0b"], cases["r1b"], mode, LD)
        f64 = TL.twin_align(cases["est"], cases["gt"], cases["r0b"], cases["r1b"], mode, np.float64)
        TL.check_align(f64, f64, ld, scale, "f64 twin", multiple=1.0)
        d = TL.align_distance(f64, ld, scale)
        unique = np.array(ld[:, 13] > TL.COND_FLOOR) | np.array(ld[:, 13] == 0)
        print("mode %d: float64 twin's distance per group:" % mode, {k: "%.2g" % v[unique].max() for k, v in d.items()})
        # (the unaligned sums of the far helix are of size 1e15 on an extent of 1e3: their rounding is not small on this scale)
        assert all(v[unique].max() < 1e-9 for k, v in d.items() if mode and k != "raw")
    rl, r64 = TL.twin_rpe(cases["est"], cases["gt"], cases["r0b"], cases["r1b"], TL.LAGS, LD), TL.twin_rpe(cases["est"], cases["gt"], cases["r0b"], cases["r1b"], TL.LAGS, np.float64)
    assert all(v.max() < 1e-9 for v in TL.rpe_distance(r64, rl, scale).values())


# ------------------------------------------------------------------------------------------------ 2. csrc/traj_plan.h on its own
@pytest.fixture(scope="module", params=FLAGS, ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("traj_plan") / "traj_plan_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-o", path, os.path.join(H.ROOT, "tests", "cpp", "traj_plan_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return path


def test_the_plan_alone(exe):
    """the strides, every refusal with its code, text and place in the order, and the flat rules of the closing maths"""
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "traj plan ok" in run.stdout, run.stdout + run.stderr


def test_the_column_table_is_the_bindings(exe):
    run = subprocess.run([exe, "--columns"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = {ln.split()[0]: ln.split()[1:] for ln in run.stdout.splitlines()}
    al = dict(zip(rows["align"][1::2], map(int, rows["align"][2::2])))
    assert int(rows["align"][0]) == capi.ALIGN_STRIDE == te.ALIGN_ROW == 20
    f = capi.ALIGN_FIELDS
    assert (f["n"].start, f["R"], f["t"], f["cond"].start) == (al["n"], slice(al["R"], al["t"]), slice(al["t"], al["cond"]), al["cond"])
    assert [f[k].start for k in ("sum_sq_err", "max_err", "final_err", "sum_sq_ang_err", "max_ang_err", "sum_sq_err_unaligned")] == \
        [al[k] for k in ("sum_sq", "max", "last", "sum_sq_ang", "max_ang", "raw")]
    assert sorted(s.start for s in f.values()) == [0, 1, 10, 13, 14, 15, 16, 17, 18, 19] and {k: s.start for k, s in TL.GROUPS.items()} == al
    rp = dict(zip(rows["rpe"][1::2], map(int, rows["rpe"][2::2])))
    assert int(rows["rpe"][0]) == capi.RPE_STRIDE == te.RPE_ROW == 4 and rp["max_lags"] == capi.RPE_MAX_LAGS == 8
    assert [capi.RPE_FIELDS[k].start for k in ("n_pairs", "sum_sq_trans_err", "sum_sq_ang_err", "max_trans_err")] == [rp[k] for k in ("pairs", "sum_sq", "sum_sq_ang", "max")]
    assert rows["mode"] == ["none", str(capi.ALIGN_NONE), "yaw", str(capi.ALIGN_YAW), "se3", str(capi.ALIGN_SE3), "pose", "7"]
    assert (te.ALIGN_NONE, te.ALIGN_YAW, te.ALIGN_SE3) == (capi.ALIGN_NONE, capi.ALIGN_YAW, capi.ALIGN_SE3)


def test_the_closing_maths_of_the_header_against_the_twin(exe, cases):
    """R, t and cond of every hand case and aligned mode from the header (the text the kernel runs: Jacobi in double) on the float64
    twin's pass-2 sums, held to the longdouble closing of the same sums on traj_lab's bar: R on 1, t on the extent, R and t only
    where cond exceeds the floor, the flat cases exactly"""
    lines, want = [], []
    est, gt, r0b, r1b = cases["est"], cases["gt"], cases["r0b"], cases["r1b"]
    for mode in (te.ALIGN_YAW, te.ALIGN_SE3):
        for b in range(est.shape[1]):
            p, g = est[r0b[b]:r1b[b], b, 4:7], gt[r0b[b]:r1b[b], b, 4:7]
            n = len(p)
            pbar, gbar = (p.sum(0) / n, g.sum(0) / n) if n else (np.zeros(3), np.zeros(3))
            pc, gc = p - pbar, g - gbar
            S, sp, sg = (pc[:, :, None] * gc[:, None, :]).sum(0), (pc * pc).sum(0), (gc * gc).sum(0)
            sums = (S, sp.sum(), sg.sum(), sp[0] + sp[1], sg[0] + sg[1])
            lines.append(" ".join(["%d" % mode, repr(float(n))] + [repr(float(x)) for x in np.concatenate([pbar, gbar, S.ravel(), sums[1:]])]))
            both = []
            for dtype in (np.float64, LD):
                R, q, t, cond = te.closing(mode, n, pbar.astype(dtype), gbar.astype(dtype), S.astype(dtype), *[dtype(x) for x in sums[1:]], dtype=dtype)
                row = np.zeros(20, dtype=dtype); row[0], row[1:10], row[10:13], row[13] = n, R.ravel(), t, cond
                both.append(row)
            want.append(both)
    run = subprocess.run([exe, "--close"], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    out = np.array([[float(x) for x in ln.split()] for ln in run.stdout.splitlines()])
    assert out.shape == (len(lines), 17)
    rows = np.zeros((len(lines), 20)); rows[:, 1:14] = out[:, :13]; rows[:, 0] = [w[0][0] for w in want]
    f64, ld = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
    scale = TL.scales(est, gt, r0b, r1b) * 2
    worst = TL.check_align(rows, f64, ld, scale, "header")
    print("header vs longdouble closing, largest d / max(d(float64 twin), floor):", {k: "%.2g" % worst[k] for k in ("R", "t", "cond")})
    q = out[:, 13:17]
    assert np.max(np.abs(np.linalg.norm(q, axis=1) - 1.0)) < 1e-15 and np.all(q[:, 0] >= 0)
    assert np.max(np.abs(te.quat_rot(q).reshape(-1, 9) - out[:, :9])) < 1e-15                  # the quaternion printed is R's
    nb = est.shape[1]
    f = cases["flat_yaw"][0]
    assert np.array_equal(out[f, :9], np.eye(3).ravel()) and out[f, 12] == 0                    # (f) in yaw mode: flat
    assert out[nb + cases["name"].index("d"), 12] < 1e-12                                       # (d) under SE(3): not unique


# ------------------------------------------------------------------------------------------------ 3. the pieces around it
def test_poses_of_a_batch():
    trajs = [sc.Trajectory(2, 300 + b, 8, 40, 6) for b in range(2)]
    g = te.gt_pose7(trajs, 1, 5)
    assert g.shape == (4, 2, 7)
    for b, tr in enumerate(trajs):
        assert np.array_equal(g[:, b, 0:4], tr.gt_frames["q_IG"][1:5]) and np.array_equal(g[:, b, 4:7], tr.gt_frames["p"][1:5])
    assert np.array_equal(te.pose7_from_truth16(np.arange(32.0).reshape(2, 16)), [[0, 1, 2, 3, 13, 14, 15], [16, 17, 18, 19, 29, 30, 31]])
    moved = te.transformed(g, TL.R_GENERAL, TL.T0)
    assert np.allclose(moved[..., 4:7], g[..., 4:7] @ TL.R_GENERAL.T + TL.T0, rtol=0, atol=1e-14)
    assert np.allclose(te.quat_rot(moved[..., 0:4]), te.quat_rot(g[..., 0:4]) @ TL.R_GENERAL.T, rtol=0, atol=1e-14)
    assert np.max(np.abs(np.linalg.norm(moved[..., 0:4], axis=-1) - 1.0)) < 1e-15


def test_asl_ate_aligned():
    """asl.ate_aligned on a synthetic run: mode 0 is asl.ate; a run whose frame is off by a yaw and a shift (what the stand-still
    initialisation gives) has a large unaligned ATE and, in modes 1 and 2, the ATE of its noise"""
    rng = np.random.default_rng(5)
    gt7 = TL.helix(60)
    t = (np.arange(61) * 50_000_000).astype(np.int64)
    ds = dict(gt=dict(t=t, p=np.concatenate([gt7[:1, 4:7], gt7[:, 4:7]]), q_IG=np.concatenate([gt7[:1, 0:4], gt7[:, 0:4]])))
    est = TL.estimate_of(gt7, TL.R_YAW, TL.T0, rng, sigma_p=0.01)
    out = []
    for k in range(60):
        s = np.zeros(29); s[0:4], s[13:16] = est[k, 0:4], est[k, 4:7]
        out.append((int(t[k]), s))
    plain = asl.ate(out, ds)
    a0, row0 = asl.ate_aligned(out, ds, 0)
    assert abs(a0 - plain[0]) <= 1e-12 * plain[0] and row0[0] == plain[2] == 60 and plain[0] > 1.0
    for mode in (1, 2):
        a, row = asl.ate_aligned(out, ds, mode)
        assert a < 0.03 and abs(row[19] - plain[1]) <= 1e-12 * plain[1] and row[13] > 0.1
        assert np.max(np.abs(row[1:10].reshape(3, 3) - TL.R_YAW)) < 0.02


def test_the_binding_has_the_new_entries():
    for name in ("frame_log_align", "frame_log_rpe", "traj_align", "traj_rpe"):
        assert callable(getattr(capi.Batch, name, None)), name
        assert "msckf_hip_" + name in capi.SYMBOLS, name
