"""The aligned trajectory error on the device (msckf_hip_frame_log_align / _rpe, msckf_hip_traj_align / _rpe; kernels_traj.hip)
against the longdouble twin msckf_mono_amd.trajeval on the bar of tests/traj_lab.py: the hand cases, the frame log of
test_gpu_frame_log.py's SMALL geometry under known per-trajectory transforms of the ground truth, the cross-checks between the
four calls and frame_log_metrics, that an alignment removes the transform, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import traj_lab as TL
from msckf_mono_amd import scenario as sc
from msckf_mono_amd import trajeval as te
from test_gpu_frame_log import SMALL, _logged_run

pytestmark = pytest.mark.gpu

LD = np.longdouble
MODES = (te.ALIGN_NONE, te.ALIGN_YAW, te.ALIGN_SE3)
LOG_LAGS = (1, 2, 5, 16, 64)                    # 17 frames: 16 leaves one pair, 64 none
R0B = np.array([0, 1, 2, 0, 3, 0], dtype=np.int32)
R1B = np.array([17, 16, 9, 17, 12, 5], dtype=np.int32)


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as mod
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def cases():
    return TL.hand_cases()


@pytest.fixture(scope="module")
def small_trajs():
    g = SMALL
    return [sc.Trajectory(2, 300 + b, g["N"], g["F"], g["nf"]) for b in range(g["B"])]


@pytest.fixture(scope="module")
def handle(capi):
    bt = capi.Batch(1, 8, 8, 8, capi.F64)
    yield bt
    bt.close()


def _transform_of(b, mode):
    """the known transform of trajectory b's ground truth: a yaw for the yaw alignment, a general rotation for SE(3)"""
    yaw = TL.rot_z(0.4 + 0.9 * b)
    R0 = yaw if mode != te.ALIGN_SE3 else yaw @ TL.rot_x(0.3 - 0.2 * b) @ TL.rot_z(-0.5 * b)
    return R0, np.array([2.0 + b, -3.0, 0.5 * b])


def _moved(gt, mode):
    out = gt.copy()
    for b in range(gt.shape[1]):
        R0, t0 = _transform_of(b, mode)
        out[:, b] = te.transformed(gt[:, b], R0, t0)
    return out


def _twins(est, gt, r0b, r1b, mode):
    return TL.twin_align(est, gt, r0b, r1b, mode, np.float64), TL.twin_align(est, gt, r0b, r1b, mode, LD)


def _show(tag, worst):
    print("%s: largest d(device) / max(d(float64 twin), n 2^-52) per column group: %s" % (tag, {k: "%.2g" % v for k, v in worst.items()}))


# ------------------------------------------------------------------------------------------------ 1. the hand cases
@pytest.mark.parametrize("mode", MODES)
def test_hand_cases_align(handle, cases, mode):
    """traj_align on the 15 hand trajectories of one 129-record array (record counts 0 .. 129, the reflection, the far helix,
    the collinear path, yaw next to +-pi, vertical motion, flipped quaternion signs) in one launch, against the longdouble twin;
    the flat cases give R = I and cond = 0 exactly, a rotation comes out everywhere; the same bits on a second call"""
    est, gt, r0b, r1b = cases["est"], cases["gt"], cases["r0b"], cases["r1b"]
    dev = handle.traj_align(est, gt, mode, r0b, r1b)
    assert np.array_equal(dev, handle.traj_align(est, gt, mode, r0b, r1b))
    f64, ld = _twins(est, gt, r0b, r1b, mode)
    _show("hand cases, mode %d" % mode, TL.check_align(dev, f64, ld, TL.scales(est, gt, r0b, r1b), "hand cases mode %d" % mode))
    assert np.array_equal(dev[:, 0], r1b - r0b)
    R = dev[:, 1:10].reshape(-1, 3, 3)
    assert np.max(np.abs(np.linalg.det(R) - 1.0)) < 1e-14 and np.max(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3))) < 1e-14
    flat = [cases["name"].index(k) for k in ("a0", "a1")] + (cases["flat_yaw"] if mode == te.ALIGN_YAW else [])
    for b in (range(len(dev)) if mode == te.ALIGN_NONE else flat):
        assert np.array_equal(dev[b, 1:10], np.eye(3).ravel()) and dev[b, 13] == 0, (mode, cases["name"][b])
    if mode == te.ALIGN_SE3:
        assert dev[cases["name"].index("d"), 13] < 1e-12 and dev[cases["name"].index("b"), 13] > 0.1
    if mode == te.ALIGN_NONE:
        assert np.array_equal(dev[:, 14], dev[:, 19]) and not dev[:, 10:14].any()
    g = cases["name"].index("g")                  # flipped quaternion signs: the attitude error is the frame offset's (0.47 rad) or,
    assert dev[g, 18] < (0.1 if mode == te.ALIGN_SE3 else 1.0)      # aligned, the noise's -- never pi


def test_hand_cases_rpe(handle, cases):
    """traj_rpe with lags (1, 2, 5, 64, 200) on the hand cases: the pair counts are max(n - lag, 0) exactly -- none at all for the lag
    of 200 --, the sums against the longdouble twin; the same bits on a second call"""
    est, gt, r0b, r1b = cases["est"], cases["gt"], cases["r0b"], cases["r1b"]
    dev = handle.traj_rpe(est, gt, TL.LAGS, r0b, r1b)
    assert dev.shape == (est.shape[1], len(TL.LAGS), 4) and np.array_equal(dev, handle.traj_rpe(est, gt, TL.LAGS, r0b, r1b))
    assert np.array_equal(dev[:, :, 0], np.maximum((r1b - r0b)[:, None] - np.array(TL.LAGS)[None, :], 0)) and not dev[:, 4].any()
    f64, ld = TL.twin_rpe(est, gt, r0b, r1b, TL.LAGS, np.float64), TL.twin_rpe(est, gt, r0b, r1b, TL.LAGS, LD)
    _show("hand cases, rpe", TL.check_rpe(dev, f64, ld, TL.scales(est, gt, r0b, r1b), "hand cases rpe"))
    assert np.all(dev[cases["name"].index("a129"), :4, 1:] > 0)


# ------------------------------------------------------------------------------------------------ 2. - 4. the frame log
@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_frame_log_against_the_twin(capi, handle, small_trajs, dtype_name):
    """SMALL geometry (N 8, F 40, B 6, 17 frames).  The ground truth of trajeval.gt_pose7 is moved by a known transform per
    trajectory (a yaw for mode 1, a general rotation for mode 2, the yaw for mode 0).
    (2) frame_log_align / frame_log_rpe against the twin on frame_log_read's records, whole range and unequal per-trajectory ranges.
    (3) traj_align / traj_rpe on the read-back agree with the frame-log calls on the same bar; mode 0's column 19 and
        frame_log_metrics' sum |e|^2 agree on it; a second call gives the same bits.
    (4) modes 1 and 2 remove the transform: the aligned sum |e|^2 is at most the unaligned one against the untransformed truth (the
        minimum is no larger than the criterion at (R0, t0); 1e-12 relative for the moved truth's rounding to double), and
        R is R0 composed with the twin's residual alignment of the untransformed problem -- to the bar, plus what rounding the
        moved truth to double can turn R by: n 2^-52 (1 + |t0| / extent) / cond."""
    g = SMALL
    nf, B = g["nf"], g["B"]
    bt = _logged_run(capi, small_trajs, dtype_name, streams=2)
    arr, _ = bt.frame_log_read()
    est = te.pose7_from_truth16(arr[:, :, 0:16])
    gt = te.gt_pose7(small_trajs, 0, nf)
    whole0, whole1 = np.zeros(B, dtype=np.int32), np.full(B, nf, dtype=np.int32)
    for mode in MODES:
        moved = _moved(gt, mode)
        for tag, r0b, r1b in (("whole", None, None), ("ranges", R0B, R1B)):
            a0, a1 = (whole0, whole1) if r0b is None else (r0b, r1b)
            dev = bt.frame_log_align(0, nf, moved, mode, r0b, r1b)
            assert np.array_equal(dev, bt.frame_log_align(0, nf, moved, mode, r0b, r1b))
            f64, ld = _twins(est, moved, a0, a1, mode)
            scale = TL.scales(est, moved, a0, a1)
            _show("frame log %s %s mode %d" % (dtype_name, tag, mode), TL.check_align(dev, f64, ld, scale, (dtype_name, tag, mode)))
            assert np.array_equal(dev[:, 0], a1 - a0)
            TL.check_align(handle.traj_align(est, moved, mode, r0b, r1b), f64, ld, scale, (dtype_name, tag, mode, "traj_align"))
            if r0b is None and mode != te.ALIGN_NONE:                                                       # (4)
                base = bt.frame_log_align(0, nf, gt, te.ALIGN_NONE)
                assert np.all(dev[:, 14] <= base[:, 19] * (1 + 1e-12)), (dev[:, 14], base[:, 19])
                assert np.all(base[:, 19] < 1e-2 * dev[:, 19])                   # (the transform is what the unaligned error sees)
                resid = TL.twin_align(est, gt, a0, a1, mode, LD)
                own = TL.align_distance(f64, ld, scale)["R"]
                for b in range(B):
                    R0, t0 = _transform_of(b, mode)
                    n, _, ext = scale[b]
                    bar = TL.MULTIPLE_R * max(own[b], n * 2.0 ** -52) + n * 2.0 ** -52 * (1 + np.linalg.norm(t0) / ext) / float(ld[b, 13])
                    d = np.max(np.abs(dev[b, 1:10].reshape(3, 3) - R0 @ np.array(resid[b, 1:10], dtype=np.float64).reshape(3, 3)))
                    assert d <= bar, (dtype_name, mode, b, d, bar)
            if mode == te.ALIGN_NONE:                                                                        # (3)
                m = bt.frame_log_metrics(0, nf, moved[:, :, 4:7]) if r0b is None else bt.frame_log_metrics_ranges(r0b, r1b, moved[:, :, 4:7])
                col = np.array(ld[:, 19], dtype=np.float64)
                own = TL.align_distance(f64, ld, scale)["raw"]
                d = np.abs(m[:, 1] - col) / np.array([s[1] for s in scale])
                assert np.all(d <= TL.MULTIPLE * np.maximum(own, TL.floor_of(scale))), (d, own)
                assert np.array_equal(m[:, 0], dev[:, 0])
        for tag, r0b, r1b in (("whole", None, None), ("ranges", R0B, R1B)):
            a0, a1 = (whole0, whole1) if r0b is None else (r0b, r1b)
            dev = bt.frame_log_rpe(0, nf, moved, LOG_LAGS, r0b, r1b)
            assert np.array_equal(dev, bt.frame_log_rpe(0, nf, moved, LOG_LAGS, r0b, r1b))
            assert np.array_equal(dev[:, :, 0], np.maximum((a1 - a0)[:, None] - np.array(LOG_LAGS)[None, :], 0))
            f64, ld = TL.twin_rpe(est, moved, a0, a1, LOG_LAGS, np.float64), TL.twin_rpe(est, moved, a0, a1, LOG_LAGS, LD)
            scale = TL.scales(est, moved, a0, a1)
            _show("frame log %s %s rpe (truth moved as for mode %d)" % (dtype_name, tag, mode), TL.check_rpe(dev, f64, ld, scale, (dtype_name, tag, "rpe")))
            TL.check_rpe(handle.traj_rpe(est, moved, LOG_LAGS, r0b, r1b), f64, ld, scale, (dtype_name, tag, "traj_rpe"))
    # a sub-range of the records, the ground truth indexed from its first record
    dev = bt.frame_log_align(3, 11, _moved(gt, te.ALIGN_SE3)[3:11], te.ALIGN_SE3)
    f64, ld = _twins(est[3:11], _moved(gt, te.ALIGN_SE3)[3:11], np.zeros(B, dtype=np.int32), np.full(B, 8, dtype=np.int32), te.ALIGN_SE3)
    TL.check_align(dev, f64, ld, TL.scales(est[3:11], _moved(gt, te.ALIGN_SE3)[3:11], np.zeros(B, dtype=np.int32), np.full(B, 8, dtype=np.int32)), "sub-range")
    bt.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_in_order(capi, small_trajs):
    """every refusal of the four calls with its text, in traj_plan.h's order (a later fault does not mask an earlier one); each leaves
    the handle running and the log untouched: the records read back as before, and the next call answers"""
    g = SMALL
    nf, B = g["nf"], g["B"]
    bt = _logged_run(capi, small_trajs, "f32")
    before, _ = bt.frame_log_read()
    gt = te.gt_pose7(small_trajs, 0, nf)
    est = te.pose7_from_truth16(before[:, :, 0:16])
    good = bt.frame_log_align(0, nf, gt, 1)
    nan = gt.copy(); nan[4, 2, 5] = np.nan; nan[6, 1, 0] += 1e-3          # not finite, and a norm that is off: finite comes first
    off = gt.copy(); off[6, 1, 0] += 1e-3
    lo, hi, out_hi = [0] * B, [nf] * B, [nf] * (B - 1) + [nf + 1]

    def refused(text, fn, *a, **kw):
        with pytest.raises(capi.HipError, match=r"\(-22\).*" + text):
            fn(*a, **kw)

    refused("record range beyond the records written", bt.frame_log_align, 0, nf + 1, np.concatenate([nan, nan[:1]]), 7)
    refused("record range beyond the records written", bt.frame_log_rpe, 0, nf + 1, np.concatenate([nan, nan[:1]]), [0])
    refused("mode is 0", bt.frame_log_align, 0, nf, nan, 3, lo, out_hi)
    refused("mode is 0", bt.traj_align, est, nan, -1, lo, out_hi)
    refused("between 1 and 8 lags", bt.frame_log_rpe, 0, nf, nan, list(range(1, 10)), lo, out_hi)
    refused("between 1 and 8 lags", bt.traj_rpe, est, nan, [], lo, out_hi)
    refused("a lag is at least 1 record", bt.frame_log_rpe, 0, nf, nan, [1, 0], lo, out_hi)
    refused("a lag is at least 1 record", bt.traj_rpe, est, nan, [-2], lo, out_hi)
    for fn, args in ((bt.frame_log_align, (0, nf, nan, 1)), (bt.frame_log_rpe, (0, nf, nan, [1])), (bt.traj_align, (est, nan, 2)), (bt.traj_rpe, (est, nan, [1]))):
        refused(r"lies outside \[r0, r1\)", fn, *args, lo, out_hi)
        refused(r"lies outside \[r0, r1\)", fn, *args, [0, 0, 5, 0, 0, 0], [nf, nf, 4, nf, nf, nf])
        refused("entry not finite", fn, *args, lo, hi)
        refused("entry not finite", fn, *args)
        refused("quaternion norm off by more than 1e-6", fn, *(args[:-2] + (off,) + args[-1:]))
    refused(r"lies outside \[r0, r1\)", bt.frame_log_align, 2, nf, nan[2:], 1, [1] + [2] * (B - 1), hi)
    # what the binding checks before the call, through the C entry points: null pointers first, one range without the other
    L, dp, ip = bt.L, C.POINTER(C.c_double), C.POINTER(C.c_int)
    o = np.zeros((B, 20)); gp, op = nan.ctypes.data_as(dp), o.ctypes.data_as(dp)
    i0 = np.array(lo, dtype=np.int32); one = np.array([1], dtype=np.int32)
    assert L.msckf_hip_frame_log_align(bt.h, 0, nf + 1, None, None, None, 9, op) == -22 and b"null argument" in L.msckf_hip_last_error()
    assert L.msckf_hip_frame_log_rpe(bt.h, 0, nf, None, None, gp, None, 0, op) == -22 and b"null argument" in L.msckf_hip_last_error()
    assert L.msckf_hip_traj_align(bt.h, nf, B, None, gp, None, None, 9, op) == -22 and b"null argument" in L.msckf_hip_last_error()
    assert L.msckf_hip_traj_rpe(bt.h, nf, B, gp, gp, None, None, one.ctypes.data_as(ip), 1, None) == -22 and b"null argument" in L.msckf_hip_last_error()
    assert L.msckf_hip_frame_log_align(bt.h, 0, nf, i0.ctypes.data_as(ip), None, gp, 1, op) == -22 and b"both or neither" in L.msckf_hip_last_error()
    assert L.msckf_hip_traj_rpe(bt.h, nf, B, gp, gp, None, i0.ctypes.data_as(ip), one.ctypes.data_as(ip), 1, op) == -22 and b"both or neither" in L.msckf_hip_last_error()
    assert L.msckf_hip_traj_align(bt.h, -1, B, gp, gp, None, None, 9, op) == -22 and b"pose arrays" in L.msckf_hip_last_error()
    assert L.msckf_hip_traj_align(bt.h, nf, 0, gp, gp, None, None, 9, op) == -22 and b"pose arrays" in L.msckf_hip_last_error()
    # the handle runs on and the log is as it was
    assert bt.frame_log_count() == nf and np.array_equal(bt.frame_log_read()[0], before)
    assert np.array_equal(bt.frame_log_align(0, nf, gt, 1), good)
    assert bt.frame_log_align(5, 5, gt[5:5], 2).shape == (B, 20) and not bt.frame_log_rpe(5, 5, gt[5:5], [1]).any()      # an empty range: zeros
    assert bt.traj_align(est[:, :2], gt[:, :2], 2).shape == (2, 20)                                                       # n_traj is free of B
    bt.close()
