"""The numpy twin of the replay's calibration model (scenario.replay_imu_calib_row, replay_imu_calib_out, replay_cam_calib,
replay_expand_calibrated, replay_calib_counts and the record builders), without a device, and the margins of the lab assignment
(tests/replay_calib_lab.py) that let tests/test_gpu_replay_calib.py demand exact clip masks, counts and quantised values."""
import numpy as np

import replay_calib_lab as CL
import replay_faults_lab as FLB
import replay_lab as RL
from msckf_mono_amd import scenario as sc

EUROC = (458.654, 457.296, 367.215, 248.375)


def test_identity_records_return_the_values_bits():
    ident, zeros = sc.imu_calib_identity(), np.zeros(8)
    assert np.array_equal(ident, sc.imu_calib_record()) and np.array_equal(zeros, sc.cam_calib_record())
    for s, tr in enumerate(RL.sequences()):
        for f in range(RL.NF):
            rd, obs = tr.imu_for_frame(f), tr.frames[f]["obs"]
            assert np.array_equal(sc.replay_imu_calib_row(rd[:, :6], ident), rd[:, :6]), (s, f)
            out, clipped = sc.replay_imu_calib_out(rd[:, :6], ident)
            assert np.array_equal(out, rd[:, :6]) and not clipped.any()
            assert np.array_equal(sc.replay_cam_calib(obs, zeros), obs), (s, f)
    # ... and the composed twin under no records is the twin without calibration, bit for bit
    tr = RL.sequences()[1]
    for f in (0, 9):
        c = sc.replay_expand_calibrated(tr, f, RL.SEEDS[0], sigma4=RL.SIGMA)
        rd, obs = sc.replay_expand(tr, f, RL.SEEDS[0], RL.SIGMA)
        assert np.array_equal(c["rd"], rd) and np.array_equal(c["obs"], obs) and not c["clip"].any() and not c["code"].any()
        assert np.array_equal(c["rd_cal"], tr.imu_for_frame(f)[:, :6]) and np.array_equal(c["obs_cal"], tr.frames[f]["obs"])


def test_a_gyro_scale_error_scales_the_integrated_rotation():
    """a cell of k samples at a constant rate under T_g = (1 + eps) I: the integrated rotation sum_i c_i dT_i is (1 + eps) times
    the sequence's.  Each c is one rounded product (the two other products are exact zeros), so it is within 2^-53 of
    (1 + eps) omega; the two sums of k terms of one sign each carry at most (k - 1) 2^-53: the bar is (k + 1) 2^-52"""
    k, eps = 40, 3e-3
    omega = np.array([0.31, -0.12, 0.05])
    rd = np.concatenate([np.tile(omega, (k, 1)), np.tile([0.1, 9.8, 0.2], (k, 1)), np.full((k, 1), 0.005)], 1)
    c = sc.replay_imu_calib_row(rd[:, :6], sc.imu_calib_record(scale_g=eps))
    assert np.array_equal(c[:, 3:], rd[:, 3:6])                   # T_a = I: the accelerometer's bits
    rot, rot0 = (c[:, :3] * rd[:, 6:7]).sum(0), (rd[:, :3] * rd[:, 6:7]).sum(0)
    assert np.all(np.abs(rot / rot0 - (1.0 + eps)) <= (k + 1) * 2.0 ** -52)
    # g-sensitivity adds G a to the rate, misalignment mixes the axes
    g = sc.replay_imu_calib_row(rd[:, :6], sc.imu_calib_record(g_sens=1e-4))
    assert np.allclose(g[:, :3] - rd[:, :3], 1e-4 * rd[:, 3:6].sum(1, keepdims=True), rtol=1e-9, atol=0)
    m = sc.replay_imu_calib_row(rd[:, :6], sc.imu_calib_record(misalign_a=[1e-3, 0, 0, 0, 0, 0]))
    assert np.allclose(m[:, 3] - rd[:, 3], 1e-3 * rd[:, 4], rtol=1e-9, atol=0) and np.array_equal(m[:, 4:6], rd[:, 4:6])


def test_clamp_and_rint_at_exact_thresholds_and_ties():
    ic = sc.imu_calib_record(sat_g=0.25, sat_a=9.0)
    x = np.array([[0.25, -0.25, np.nextafter(0.25, 1.0), 0.3, 9.0, -12.0], [np.nextafter(-0.25, -1.0), 0.0, 0.1, np.nextafter(9.0, 10.0), -9.0, 8.9]])
    out, clipped = sc.replay_imu_calib_out(x, ic)
    assert np.array_equal(out, [[0.25, -0.25, 0.25, 0.3, 9.0, -9.0], [-0.25, 0.0, 0.1, 9.0, -9.0, 8.9]])
    assert np.array_equal(clipped, [[False, False, True, False, False, True], [True, False, False, True, False, False]])
    # ties go to the even multiple; the steps are powers of two, so quotient and product are exact
    ic = sc.imu_calib_record(lsb_g=0.25, lsb_a=0.5)
    x = np.array([[0.125, 0.375, 0.625, 0.75, 1.25, 1.2500000000000002], [-0.375, -0.125, 0.0, -0.75, -1.25, 0.24]])
    out, clipped = sc.replay_imu_calib_out(x, ic)
    assert np.array_equal(out, [[0.0, 0.5, 0.5, 1.0, 1.0, 1.5], [-0.5, -0.0, 0.0, -1.0, -1.0, 0.0]]) and not clipped.any()
    assert np.signbit(out[1, 1]) and not np.signbit(out[1, 2])
    # saturation first, then quantisation
    out, clipped = sc.replay_imu_calib_out(np.full((1, 6), 1.0), sc.imu_calib_record(sat_g=0.3, lsb_g=0.25))
    assert np.array_equal(out[0], [0.25] * 3 + [1.0] * 3) and np.array_equal(clipped[0], [True] * 3 + [False] * 3)


def _radtan(x, k1, k2, p1, p2):
    r2 = (x ** 2).sum(-1)
    rad = 1.0 + k1 * r2 + k2 * r2 * r2
    xy = x[:, 0] * x[:, 1]
    return np.stack([x[:, 0] * rad + 2 * p1 * xy + p2 * (r2 + 2 * x[:, 0] ** 2), x[:, 1] * rad + p1 * (r2 + 2 * x[:, 1] ** 2) + 2 * p2 * xy], -1)


def _through_both(x, true, assumed):
    """project normalised points with the true calibration, undistort the pixels with the assumed one by fixed-point iteration"""
    px = _radtan(x, *true[4:]) * np.array(true[0:2]) + np.array(true[2:4])
    y = (px - np.array(assumed[2:4])) / np.array(assumed[0:2])
    u = y.copy()
    for _ in range(60):
        u = y - (_radtan(u, *assumed[4:]) - u)
    return u


def test_cam_calib_from_intrinsics_is_first_order():
    """an independent path: the lab's observations projected with the true pinhole-radtan calibration and undistorted with the
    assumed one.  Both calibrations lie within the perturbation of an undistorted pinhole camera (the replay's coordinates are
    rectified ones): then the Jacobian of the assumed undistortion is I + O(perturbation) and the record's residual is second
    order.  Measured at the lab's magnitudes (the record of trajectory 4): printed, and written in DESIGN section 4.13; halving
    the perturbation at least halves it (a second-order residual quarters)"""
    x = np.concatenate([tr.frames[f]["obs"] for tr in RL.sequences() for f in range(RL.NF)])
    assert len(x) > 400 and np.abs(x).max() > 0.3
    e_u, e_v, d_u, d_v, k1, k2, p1, p2 = CL.CAMCAL[4]
    f_u, f_v, c_u, c_v = EUROC
    res = []
    for h in (1.0, 0.5, 0.25):
        assumed = (f_u, f_v, c_u, c_v, -h * k1, h * k2, -h * p1, 0.5 * h * p2)                 # a residual distortion of its own
        true = (f_u * (1 + h * e_u), f_v * (1 + h * e_v), c_u + h * d_u * f_u, c_v + h * d_v * f_v, assumed[4] + h * k1, assumed[5] + h * k2, assumed[6] + h * p1, assumed[7] + h * p2)
        rec = sc.cam_calib_from_intrinsics(true, assumed)
        assert np.allclose(rec, h * CL.CAMCAL[4], rtol=1e-9, atol=1e-18)
        first = np.abs(sc.replay_cam_calib(x, rec) - x).max()
        res.append(float(np.abs(_through_both(x, true, assumed) - sc.replay_cam_calib(x, rec)).max()))
        assert res[-1] < 0.02 * first                                # second order against first order
    print("residual of the first-order camera record at 1, 1/2, 1/4 of the lab's perturbation: %.3g %.3g %.3g (normalised units)" % tuple(res))
    assert res[1] <= 0.5 * res[0] and res[2] <= 0.5 * res[1]
    # an assumed calibration without distortion: the record is the exact map, to rounding
    assumed = (f_u, f_v, c_u, c_v, 0.0, 0.0, 0.0, 0.0)
    true = (f_u * (1 + e_u), f_v * (1 + e_v), c_u + d_u * f_u, c_v + d_v * f_v, k1, k2, p1, p2)
    assert np.abs(_through_both(x, true, assumed) - sc.replay_cam_calib(x, sc.cam_calib_from_intrinsics(true, assumed))).max() < 1e-15


def _pre_clamp(f, b, model):
    """the lab sample values of trajectory b on frame f before saturation and quantisation, [k][6]"""
    tr = RL.sequences()[RL.SEQ_OF[b]]
    rd = tr.imu_for_frame(f).copy()
    rd[:, :6] = sc.replay_imu_calib_row(rd[:, :6], CL.IMUCAL[b])
    if model:
        L, scale, sigma_uv, walks = CL.model()
        return sc.replay_model_cell(rd, np.zeros((0, 2)), f, CL.SEEDS[b], L, scale, sigma_uv, walks[b][f])[0][:, :6]
    return sc.replay_cell(rd, np.zeros((0, 2)), f, CL.SEEDS[b], RL.SIGMA)[0][:, :6]


def test_lab_margins():
    """what the device tests' exact masks, counts and quantised values rest on, with nothing excluded: under either noise model no
    lab sample's pre-clamp value lies within 1e-9 x its noise scale of +-sat, and none lies within that distance of a
    quantisation tie (a device value differs from the twin's by rounding errors of the noise alone, some 1e-14 of that scale)"""
    nearest_sat, nearest_tie, samples = np.inf, np.inf, 0
    for model in (False, True):
        noise = CL.model_noise_scale() if model else CL.NOISE_SIGMA4
        for b in range(RL.B):
            ic = CL.IMUCAL[b]
            for f in range(RL.NF):
                x = _pre_clamp(f, b, model)
                samples += len(x)
                for cols, sat, lsb in ((slice(0, 3), ic[27], ic[29]), (slice(3, 6), ic[28], ic[30])):
                    v = x[:, cols]
                    if sat > 0.0:
                        nearest_sat = min(nearest_sat, float((np.abs(np.abs(v) - sat) / noise[cols]).min()))
                        v = np.minimum(np.maximum(v, -sat), sat)
                    if lsb > 0.0:
                        q = v / lsb
                        nearest_tie = min(nearest_tie, float((np.abs(np.abs(q - np.floor(q)) - 0.5) * lsb / noise[cols]).min()))
    print("lab margins over %d samples: nearest +-sat %.3g, nearest tie %.3g (in units of the noise scale)" % (samples, nearest_sat, nearest_tie))
    assert samples == 2 * RL.B * RL.NF * sc.IMU_PER_FRAME
    assert nearest_sat > 1e-9 and nearest_tie > 1e-9
    # the lab clips a visible share on both saturating trajectories and nothing elsewhere
    for model in (False, True):
        c = CL.counts(model)
        assert np.all(c[:, 0] == RL.NF * sc.IMU_PER_FRAME) and c[2, 7] > 30 and c[4, 7] > 20 and not c[[0, 1, 3], 1:].any()
        assert np.array_equal(CL.counts(model, 0, 7) + CL.counts(model, 7, RL.NF), c)


def test_the_composed_twin_and_the_counts_agree():
    """replay_expand_calibrated's clip masks add up to replay_calib_counts; the camera map is applied before noise and faults,
    which keep their draws: codes, survivors and slots are those of the faulted twin without calibration"""
    for model in (False, True):
        pop = np.zeros((RL.B, 8), dtype=np.int64)
        for b in range(RL.B):
            for f in range(RL.NF):
                m = CL.twin_cell(f, b, model)["clip"]
                pop[b] += np.concatenate([[len(m)], ((m[:, None] >> np.arange(6)) & 1).sum(0), [int((m != 0).sum())]])
        assert np.array_equal(pop, CL.counts(model))
    for b in (3, 4):
        c = CL.twin_cell(9, b, fault4=FLB.FAULT4)
        p = FLB.twin_cell(9, b)
        assert np.array_equal(c["code"], p["code"]) and np.array_equal(c["Mp"], p["Mp"]) and np.array_equal(c["slots"], p["slots"])
        kept = c["code"] == sc.FAULT_KEPT
        assert kept.any() and not np.array_equal(c["obs"], p["obs"])
        # a kept entry's noise is the same draw on the mapped value: the difference is the map's own displacement
        plain = CL.twin_cell(9, b, imucal=None, camcal=None)
        moved = (c["obs_cal"] - plain["obs_cal"])
        nofault = CL.twin_cell(9, b)
        assert np.allclose(nofault["obs"] - plain["obs"], moved, rtol=0, atol=1e-15)


def test_record_builders():
    ic = sc.imu_calib_record(scale_g=[1e-3, 2e-3, 3e-3], misalign_g=[1, 2, 3, 4, 5, 6], scale_a=-1e-3, misalign_a=0.5, g_sens=np.arange(9.0), sat_g=1, sat_a=2, lsb_g=3, lsb_a=4)
    assert ic.shape == (31,)
    assert np.array_equal(ic[0:9].reshape(3, 3), [[1.001, 1, 2], [3, 1.002, 4], [5, 6, 1.003]])
    assert np.array_equal(ic[9:18].reshape(3, 3), [[0.999, 0.5, 0.5], [0.5, 0.999, 0.5], [0.5, 0.5, 0.999]])
    assert np.array_equal(ic[18:27], np.arange(9.0)) and np.array_equal(ic[27:], [1, 2, 3, 4])
    assert np.array_equal(sc.cam_calib_record(1, 2, 3, 4, 5, 6, 7, 8), np.arange(1.0, 9.0))
    # the extrinsic error: its own sub-seed, one draw per seed, no kernel involved
    assert sc.REPLAY_EXTRINSIC_STREAM == (1 << 63) + 3 and sc.REPLAY_EXTRINSIC_STREAM not in (sc.REPLAY_FAULT_STREAM, sc.REPLAY_TIMING_STREAM, 1 << 63)
    cfg = sc.filter_config(RL.N)
    cam12 = np.array([cfg["c_u"], cfg["c_v"], cfg["f_u"], cfg["f_v"], 0.0] + list(cfg["q_CI"]) + list(cfg["p_C_I"]))
    assert np.array_equal(sc.perturbed_cam12(cam12, 5, 0.0, 0.0)[[0, 1, 2, 3, 4, 9, 10, 11]], cam12[[0, 1, 2, 3, 4, 9, 10, 11]])
    assert np.allclose(sc.perturbed_cam12(cam12, 5, 0.0, 0.0), cam12, rtol=0, atol=1e-15)
    a, a2, b = sc.perturbed_cam12(cam12, 5, 2e-3, 1e-3), sc.perturbed_cam12(cam12, 5, 2e-3, 1e-3), sc.perturbed_cam12(cam12, 6, 2e-3, 1e-3)
    assert np.array_equal(a, a2) and not np.array_equal(a, b) and np.array_equal(a[:5], cam12[:5])
    assert abs(np.linalg.norm(a[5:9]) - 1.0) < 1e-15
    angle = np.linalg.norm(sc.error_angle(a[5:9], cam12[5:9]))
    n = sc.replay_pairs(int(sc.replay_mix(5, sc.REPLAY_EXTRINSIC_STREAM)), 3).reshape(6)
    assert np.isclose(angle, 2e-3 * np.linalg.norm(n[:3]), rtol=1e-5) and np.allclose(a[9:12] - cam12[9:12], 1e-3 * n[3:], rtol=0, atol=1e-15)
