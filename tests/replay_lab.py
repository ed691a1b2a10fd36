"""The common shape of the Monte-Carlo replay's tests (tests/test_replay_plan.py, tests/test_replay_inputs.py on the CPU,
tests/test_gpu_replay.py on the device): two noise-free sequences, five trajectories that replay them with their own seeds.

seq_of = [1, 0, 1, 1, 0] is non-monotone and the sequences' entry counts differ on most frames, so every trajectory's first
entry in the expanded block differs from what a copy of its sequence's would be.  sigma is scenario.Trajectory's own default
noise (imu_noise_scale = 0.05, obs_noise_px = 0.5 at filter_config's Q_imu and f_u)."""
import functools

import numpy as np

from msckf_mono_amd import scenario as sc

N, F, NF = 6, 8, 16
N_CAP = M_CAP = 6
F_CAP = 8
B = 5
SEQ_OF = [1, 0, 1, 1, 0]
SEEDS = [0xC0FFEE00 + b for b in range(B)]
SIGMA = (7.07e-3, 7.07e-2, 0.5 / 458.654, 0.5 / 458.654)      # sigma_g, sigma_a, sigma_u, sigma_v


@functools.lru_cache(maxsize=None)
def sequences():
    """the two noise-free sequences (built once; nobody writes to them)"""
    return tuple(sc.Trajectory(7, p, N, F, NF, imu_noise_scale=0.0, obs_noise_px=0.0, path_id=p) for p in (0, 1))


def full(tr, f):
    return tr.frames[f]["Nw"] == tr.N


def twin_cell(f, b, seq_of=SEQ_OF, seeds=SEEDS, sigma=SIGMA):
    """trajectory b's cell of frame f by the numpy twin: (readings [10][7], M, slots, obs [n][2], n_drop)"""
    tr = sequences()[seq_of[b]]
    rd, obs = sc.replay_expand(tr, f, seeds[b], sigma)
    fr = tr.frames[f]
    return rd, fr["M"], fr["slots"], obs, 1 if full(tr, f) else 0


def stage_replay(bt, seq_of=SEQ_OF, seeds=SEEDS, sigma=SIGMA):
    """the sequences as a replay on handle bt, assigned and committed"""
    seqs = sequences()
    bt.replay_alloc(len(seqs), NF, sc.IMU_PER_FRAME)
    for f in range(NF):
        for s, tr in enumerate(seqs):
            fr = tr.frames[f]
            bt.replay_set_cell(f, s, tr.imu_for_frame(f), fr["M"], fr["slots"], fr["obs"], 1 if full(tr, f) else 0)
    bt.replay_assign(seq_of, seeds, sigma)
    bt.replay_commit()


class NoisyTrajectory:
    """what helpers.oracle_frame reads of a trajectory (imu_for_frame, frame_times, frames), with the cells given"""

    def __init__(self, seq_traj, cells):
        self.cfg, self.imu0, self.frame_times, self.N = seq_traj.cfg, seq_traj.imu0, seq_traj.frame_times, seq_traj.N
        self.gt_frames = seq_traj.gt_frames
        self._rd = [np.asarray(c[0]) for c in cells]
        self.frames = [dict(Nw=seq_traj.frames[f]["Nw"], M=np.asarray(c[1]), slots=np.asarray(c[2]), obs=np.asarray(c[3])) for f, c in enumerate(cells)]

    def imu_for_frame(self, f):
        return self._rd[f]


def twin_trajectory(b):
    return NoisyTrajectory(sequences()[SEQ_OF[b]], [twin_cell(f, b) for f in range(NF)])
