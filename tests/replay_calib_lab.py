"""The shared shapes of the replay's calibration tests (tests/test_replay_calib_inputs.py on the CPU, tests/test_gpu_replay_calib.py
on the device): the common shape of tests/replay_lab.py -- two noise-free sequences, five trajectories, 16 frames -- with one IMU
and one camera calibration record per trajectory, and the twin's cells alone or composed with the lab's faults and timing.

The lab assignment: identity records | matrices only (scale, misalignment, g-sensitivity; a focal-length error) | saturation
low enough to clip a visible share of the samples | quantisation (a 16-bit gyro at +-250 deg/s, an accelerometer at 1 mg;
residual radial distortion) | everything, with a camera record whose eight fields are all non-zero.

The saturation levels sit just above the sequences' own values (gyro x stays near 0.34 rad/s on path 1 and 0.47 on path 0,
accelerometer x near 9.8 m/s^2), so that the noise carries a share of the samples over them on either sensor: 62 and 43 of a
trajectory's 160 samples clip under sigma4.  tests/test_replay_calib_inputs.py asserts the margins the device tests rest on: no
pre-clamp value within 1e-9 of its noise scale of +-sat or of a quantisation tie, under both noise models."""
import functools

import numpy as np

import replay_faults_lab as FLB
import replay_lab as RL
import replay_timing_lab as TL
from msckf_mono_amd import scenario as sc

SEEDS = FLB.SEEDS
G_SENS = 2e-4 * np.array([[1.0, -0.5, 0.3], [0.4, 1.2, -0.7], [-0.2, 0.6, 0.9]])      # rad/s per m/s^2
LSB_G, LSB_A = np.deg2rad(250.0) / 32768.0, 9.80665e-3
IMUCAL = np.stack([
    sc.imu_calib_identity(),
    sc.imu_calib_record(scale_g=[3e-3, -2e-3, 4e-3], misalign_g=[1e-3, -2e-3, 1.5e-3, 5e-4, -1e-3, 2e-3],
                        scale_a=[-5e-3, 2e-3, 3e-3], misalign_a=[-1e-3, 5e-4, 2e-3, -1.5e-3, 1e-3, -5e-4], g_sens=G_SENS),
    sc.imu_calib_record(sat_g=0.345, sat_a=9.85),
    sc.imu_calib_record(lsb_g=LSB_G, lsb_a=LSB_A),
    sc.imu_calib_record(scale_g=[-4e-3, 1e-3, 2e-3], misalign_g=2e-3, scale_a=[1e-3, -3e-3, 2e-3], misalign_a=-1e-3, g_sens=G_SENS.T,
                        sat_g=0.475, sat_a=9.85, lsb_g=LSB_G, lsb_a=LSB_A),
])
CAMCAL = np.stack([
    sc.cam_calib_record(),
    sc.cam_calib_record(e_u=4e-3, e_v=-3e-3),
    sc.cam_calib_record(),
    sc.cam_calib_record(k1=-8e-3, k2=2e-3),
    sc.cam_calib_record(e_u=-3e-3, e_v=2e-3, d_u=1.5 * FLB.PX, d_v=-2.0 * FLB.PX, k1=6e-3, k2=-1.5e-3, p1=3e-4, p2=-2e-4),
])
# the scale of one sample's noise per column under the two models the lab runs: sigma4's levels, and the Q_imu model's white rows
# at the lab's scale over the sequences' 5 ms step
NOISE_SIGMA4 = np.array([RL.SIGMA[0]] * 3 + [RL.SIGMA[1]] * 3)


def model_noise_scale():
    Q, scale, _ = FLB.model_of(0)
    d = np.diag(Q)
    dT = float(RL.sequences()[0].imu_for_frame(0)[0, 6])
    return scale * np.sqrt(np.concatenate([d[0:3], d[6:9]]) / dT)


@functools.lru_cache(maxsize=None)
def model():
    """the Q_imu model of the lab with every trajectory's walk table: (L, scale, sigma_uv, walks [B][frames + 1][6])"""
    Q, scale, sigma_uv = FLB.model_of(0)
    L = sc.replay_noise_factor(Q)
    walks = np.stack([sc.replay_walk(RL.sequences()[RL.SEQ_OF[b]], SEEDS[b], L, scale) for b in range(RL.B)])
    return L, scale, sigma_uv, walks


def twin_cell(f, b, use_model=False, imucal=IMUCAL, camcal=CAMCAL, fault4=None, timing4=None, delta=None, sigma=RL.SIGMA, seeds=SEEDS):
    """trajectory b's cell of frame f by the numpy twin under the records: scenario.replay_expand_calibrated's dict plus M (the
    sequence's) and drop.  fault4 / timing4: the whole assignments or None; delta: the entries' deltas where they are known"""
    s = RL.SEQ_OF[b]
    tr = RL.sequences()[s]
    kw = dict(imucal=None if imucal is None else imucal[b], camcal=None if camcal is None else camcal[b],
              fault4=None if fault4 is None else fault4[b], timing4=None if timing4 is None else timing4[b], delta=delta,
              table=TL.table(s) if timing4 is not None or delta is not None else None)
    if use_model:
        L, scale, _, walks = model()
        c = sc.replay_expand_calibrated(tr, f, seeds[b], model=(L, scale, sigma[2:], walks[b][f]), **kw)
    else:
        c = sc.replay_expand_calibrated(tr, f, seeds[b], sigma4=sigma, **kw)
    c["M"] = tr.frames[f]["M"]
    c["drop"] = 1 if RL.full(tr, f) else 0
    return c


def stage_replay(bt, imucal=IMUCAL, camcal=CAMCAL, fault4=None, timing4=None, use_model=False, sigma=RL.SIGMA, seeds=SEEDS):
    """replay_lab's sequences on handle bt under the sigma4 noise or the Q_imu model, committed, with the records set"""
    RL.stage_replay(bt, RL.SEQ_OF, seeds, sigma)
    if use_model:
        Q, scale, _ = FLB.model_of(0)
        bt.replay_assign_q(RL.SEQ_OF, seeds, Q, scale, sigma[2:])
    if fault4 is not None:
        bt.replay_set_faults(fault4)
    if timing4 is not None:
        bt.replay_set_timing(timing4)
    bt.replay_set_imu_calib(imucal)
    bt.replay_set_cam_calib(camcal)


def counts(use_model=False, f0=0, f1=RL.NF, imucal=IMUCAL):
    """scenario.replay_calib_counts of every trajectory, [B][8]"""
    out = []
    for b in range(RL.B):
        tr = RL.sequences()[RL.SEQ_OF[b]]
        if use_model:
            L, scale, _, _ = model()
            out.append(sc.replay_calib_counts(tr, SEEDS[b], imucal[b], f0, f1, model=(L, scale)))
        else:
            out.append(sc.replay_calib_counts(tr, SEEDS[b], imucal[b], f0, f1, sigma4=RL.SIGMA))
    return np.stack(out)
