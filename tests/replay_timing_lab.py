"""The shared shapes of the replay's timing tests (tests/test_replay_timing_inputs.py on the CPU, tests/test_gpu_replay_timing.py
on the device): the common shape of tests/replay_lab.py -- two noise-free sequences, five trajectories, 16 frames -- with one
timing record per trajectory, the twin's cells with and without faults, and the analytic observation at a shifted time.

The lab assignment: no timing | a 5 ms offset | rolling shutter alone (a 480-row sensor read in 30 ms behind EuRoC's cam0
intrinsics) | 1 ms of jitter alone | all three with a negative offset."""
import functools

import numpy as np

import replay_faults_lab as FLB
import replay_lab as RL
from msckf_mono_amd import scenario as sc

F_V, C_V, ROWS, T_READ = 457.296, 248.375, 480, 0.030
R_Y, Y_0 = T_READ * F_V / ROWS, (ROWS / 2 - C_V) / F_V
TIMING4 = np.array([
    [0.0, 0.0, 0.0, 0.0],
    [5e-3, 0.0, 0.0, 0.0],
    [0.0, R_Y, Y_0, 0.0],
    [0.0, 0.0, 0.0, 1e-3],
    [-3e-3, R_Y, Y_0, 1e-3],
])
ALL = np.array([5e-3, R_Y, Y_0, 1e-3])     # the record the sensitivity checks perturb
# the bar of the device comparison under noise and faults (replay_faults_lab.check_scalars): 1e-13 (sigma + rho) at the lab's
# largest noise and ring -- what a wrong rule has to exceed to be seen there; without noise the comparison is bit for bit
BAR = 1e-13 * (RL.SIGMA[2] + 30 * FLB.PX)


@functools.lru_cache(maxsize=None)
def table(s):
    """replay_image_table of sequence s (once; nobody writes to it)"""
    return sc.replay_image_table(RL.sequences()[s])


def delta_of(f, b, timing4=TIMING4, seeds=FLB.SEEDS):
    """the twin's delta of every entry of trajectory b's cell on frame f"""
    s = RL.SEQ_OF[b]
    fr = RL.sequences()[s].frames[f]
    _, frame_of, base = table(s)
    if not len(fr["obs"]):
        return np.zeros(0)
    return sc.replay_timing_delta(fr["obs"][:, 1], frame_of[base[f] + fr["slots"]], seeds[b], timing4[b])


def twin_cell(f, b, timing4=TIMING4, delta=None, fault4=None, seeds=FLB.SEEDS, model=None, sigma=RL.SIGMA):
    """trajectory b's cell of frame f by the numpy twin under the timing record (delta: the entries' deltas where they are known),
    as replay_faults_lab.twin_cell gives it: dict of rd, M, Mp, slots, obs, code, drop.  fault4 None: no faults.  model: None for
    the sigma4 noise `sigma`, or (L, scale, sigma_uv, w_start)"""
    s = RL.SEQ_OF[b]
    tr = RL.sequences()[s]
    f4 = np.zeros(4) if fault4 is None else fault4[b]
    if model is None:
        rd, Mp, slots, obs, code = sc.replay_expand_timed_faulted(tr, f, seeds[b], sigma, timing4[b], f4, delta, table(s))
    else:
        L, scale, sigma_uv, w_start = model
        rd, Mp, slots, obs, code = sc.replay_model_expand_timed_faulted(tr, f, seeds[b], L, scale, sigma_uv, timing4[b], f4, w_start, delta, table(s))
    return dict(rd=rd, M=tr.frames[f]["M"], Mp=Mp, slots=slots, obs=obs, code=code, drop=1 if RL.full(tr, f) else 0)


def stage_replay(bt, timing4=TIMING4, fault4=None, seeds=FLB.SEEDS, model=False, sigma=RL.SIGMA):
    """replay_lab's sequences on handle bt under the sigma4 noise or the Q_imu model, committed, with the timing (and fault) record set"""
    RL.stage_replay(bt, RL.SEQ_OF, seeds, sigma)
    if model:
        Q, scale, sigma_uv = FLB.model_of(0)
        bt.replay_assign_q(RL.SEQ_OF, seeds, Q, scale, sigma[2:])
    if fault4 is not None:
        bt.replay_set_faults(fault4)
    bt.replay_set_timing(timing4)


# ------------------------------------------------------------------------------------------------ the analytic observation
def exact_obs(tr, f, delta):
    """frame f's observations of the noise-free Trajectory tr with every entry exposed delta [n] seconds after its image's time:
    the frame's landmarks projected through the camera of scenario.ground_truth at the shifted time, [n][2]"""
    fr = tr.frames[f]
    if not len(fr["obs"]):
        return np.zeros((0, 2))
    img = f - (fr["Nw"] - 1 - fr["slots"])                       # slot Nw - 1 is frame f's own image
    t = tr.frame_times[img] + np.asarray(delta, dtype=np.float64)
    gt = sc.ground_truth(t, tr.path_id)
    C_CG = np.einsum("ij,nkj->nik", sc.quat_to_rot(tr.cfg["q_CI"]), gt["R_GI"])
    p_C = gt["p"] + np.einsum("nij,j->ni", gt["R_GI"], tr.cfg["p_C_I"])
    pts = np.repeat(tr.landmarks[f], fr["M"], axis=0)
    pc = np.einsum("nij,nj->ni", C_CG, pts - p_C)
    return pc[:, :2] / pc[:, 2:3]


def stencil_kind(M):
    """per entry of a cell with track lengths M: 0 a three-node interior entry, 1 a track end (the stencil pulled inside), 2 an
    entry of a two-node track, 3 a track of one"""
    kind = []
    for m in (int(x) for x in M):
        kind += [3] if m == 1 else [2, 2] if m == 2 else [1] + [0] * (m - 2) + [1]
    return np.array(kind, dtype=np.int64)
