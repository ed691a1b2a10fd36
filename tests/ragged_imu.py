"""Scenarios with their own IMU sample count per (frame, trajectory) cell and sequences of unequal length, shared by
tests/test_ragged_imu_scenarios.py (CPU: the oracle alone updates on them) and tests/test_gpu_ragged_imu.py.

scenario.Trajectory hands every frame ten equal IMU samples.  `resample` turns them into k samples over the same interval, so
that the oracle and the device integrate the same motion from the same k readings.  A cell with k = 0 propagates nothing: its
camera state is cloned from the unpropagated state, 50 ms of motion (6 cm, 1.2 degrees) away from where the image was taken,
and the oracle alone then gates out every track that observes that camera.  So in the set that is compared with the oracle
(zeros = "last") an empty cell is a trajectory's LAST frame, whose camera no track observes: the update of that frame is a real
one.  The set for the bit comparisons (zeros = "rotating") has its empty cells mid-run and hands their ten samples on to the
trajectory's next frame.  A trajectory whose sequence has no image on a frame is skipped there: its own frame counter stands
still, so its work-lists keep their camera slots."""
import numpy as np

import helpers as H
from msckf_mono_amd import scenario as sc

PATTERN = [10, 9, 11, 5, 17, 1, 20, 10, 12, 8, 33, 10]      # what a 200 Hz IMU against a 20 Hz camera with drops looks like
BOUNDARY = [1, 15, 0, 16, 17, 32, 33]                        # around k_propagate's groups of 16 samples (the empty cell's samples go to a 16)
COUNTS = PATTERN + BOUNDARY                                   # 19 counts: one per frame of the ragged batch, rotated per trajectory
NONZERO = [c for c in COUNTS if c]
ZERO_LAST = (0, 4, 5)                                         # zeros = "last": the trajectories whose last frame has no sample (windows 6, 6, 15)
K_CAP = max(COUNTS)

# (window, tracks per frame) per trajectory: 6 cameras = the one-launch update, 15 = the chain of kernels; B = 7 is no multiple
# of the slice count 3 (slices start at trajectories 0, 2, 4)
SPECS = [(6, 9, ""), (15, 20, ""), (6, 12, ""), (15, 16, ""), (6, 7, ""), (15, 24, ""), (6, 10, "")]
MID_SKIP = (1, (3, 4))        # trajectory 1 has no image on frames 3 and 4, then resumes
TAIL_SKIP = 4                 # trajectory 4's sequence ends five frames early
FULL_Q = 2                    # the trajectory that carries an off-diagonal Q_imu in the `full_q` variant


def resample(rd, k):
    """the readings rd [n][7] (omega a dT) as k readings over the same interval.  k <= n: n samples in k contiguous groups, each
    group one sample with the mean reading and the summed dT; k > n: every sample in equal parts, dT divided.  k = 0: none."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 7)
    n = len(rd)
    if k == 0:
        return np.zeros((0, 7))
    if k <= n:
        out = []
        for idx in np.array_split(np.arange(n), k):
            g = rd[idx]
            out.append(np.concatenate([g[:, :6].mean(0), [g[:, 6].sum()]]))
        return np.array(out)
    parts = [k // n + (1 if i < k % n else 0) for i in range(n)]
    out = []
    for r, p in zip(rd, parts):
        out += [np.concatenate([r[:6], [r[6] / p]])] * p
    return np.array(out)


def correlated(diag, seed, lo=0.3, hi=0.6):
    """SPD matrix with the given diagonal and off-diagonal entries of lo .. hi of the geometric mean of their diagonal entries"""
    rng = np.random.default_rng(seed)
    n = len(diag)
    c = rng.uniform(np.sqrt(lo), np.sqrt(hi), n) * rng.choice([-1.0, 1.0], n)
    R = np.outer(c, c)
    np.fill_diagonal(R, 1.0)
    s = np.sqrt(np.asarray(diag, dtype=np.float64))
    return R * np.outer(s, s)


class RaggedImuSet(H.RaggedSet):
    """helpers.RaggedSet whose cells carry their own sample count, with two trajectories of shorter sequences.
    local[b][f]: trajectory b's own frame index on global frame f, or None where it is skipped; rd[b][j]: the readings of its
    frame j; counts[b][j] = len(rd[b][j]).  equal = True: ten samples in every cell, nobody skipped (the lockstep twin).
    zeros: where the empty cells are (module docstring).
    full_q: trajectory FULL_Q is initialised with a whole Q_imu (no oracle for it: bit comparisons only)."""

    def __init__(self, seed0=1500, equal=False, full_q=False, zeros="last"):
        n_cap = max(s[0] for s in SPECS)
        super().__init__(0, seed0=seed0, specs=SPECS, n_cap=n_cap)
        nf, B = self.nf, self.B
        self.K = sc.IMU_PER_FRAME if equal else K_CAP
        self.full_q = full_q
        if full_q:
            N, F, _ = SPECS[FULL_Q]
            base = sc.filter_config(N)
            self.trajs[FULL_Q] = sc.Trajectory(2, seed0 + FULL_Q, N, F, nf, cfg=sc.filter_config(N, Q_imu=correlated(base["Q_imu_diag"], 77)))
            self.frames[FULL_Q] = [dict(f) for f in self.trajs[FULL_Q].frames]
        self.local = []
        for b in range(B):
            loc, j = [], 0
            for f in range(nf):
                skipped = not equal and ((b == MID_SKIP[0] and f in MID_SKIP[1]) or (b == TAIL_SKIP and f >= nf - 5))
                loc.append(None if skipped else j)
                j += 0 if skipped else 1
            self.local.append(loc)
        self.rd, self.counts = [], []
        for b, tr in enumerate(self.trajs):
            rds, carried = [], np.zeros((0, 7))
            for j in range(nf):
                if equal:
                    k = sc.IMU_PER_FRAME
                elif zeros == "rotating":
                    k = COUNTS[(j + 3 * b) % len(COUNTS)]
                else:
                    k = 0 if (b in ZERO_LAST and j == self.n_local(b) - 1) else NONZERO[(j + 3 * b) % len(NONZERO)]
                have = np.concatenate([carried, tr.imu_for_frame(j)])
                rds.append(resample(have, k))
                carried = have if k == 0 else np.zeros((0, 7))
            self.rd.append(rds)
            self.counts.append([len(r) for r in rds])

    def skipped(self, b, f):
        return self.local[b][f] is None

    def n_local(self, b):
        return sum(1 for j in self.local[b] if j is not None)

    def cell(self, b, f):
        """(readings, M, slots, obs, n_drop, skip) of trajectory b on global frame f"""
        j = self.local[b][f]
        if j is None:
            return np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), 0, True
        fr = self.frames[b][j]
        return self.rd[b][j], fr["M"], fr["slots"], fr["obs"], 1 if self.full(b, j) else 0, False

    def oracle_cell(self, o, b, f):
        """global frame f on trajectory b's oracle: nothing where it is skipped; else its k samples (none: it only augments),
        augmentState, the update when it is handed tracks, the drop when its window is full"""
        j = self.local[b][f]
        if j is None:
            return
        tr, fr = self.trajs[b], self.frames[b][j]
        if len(self.rd[b][j]):
            o.propagate(self.rd[b][j])
        o.augmentState(j, tr.frame_times[j])
        if len(fr["M"]):
            o.setTracks(fr["M"], fr["slots"], fr["obs"])
            o.marginalize()
        if self.full(b, j):
            o.dropOldest(1)

    def stage(self, bt, K=None, only=None):
        """the cells as a scenario of capacity K (default: the largest count) on handle bt; only = b: a handle of ONE trajectory
        that holds trajectory b's cells"""
        bt.scenario_alloc(self.nf, self.K if K is None else K)
        for f in range(self.nf):
            for b in (range(self.B) if only is None else [only]):
                rd, M, slots, obs, drop, skip = self.cell(b, f)
                bt.scenario_set(f, b if only is None else 0, rd, M, slots, obs, drop, skip=skip)
        bt.scenario_commit()

    def solo_batch(self, capi, dtype, b):
        bt = capi.Batch(1, self.n_cap, self.f_cap, self.m_cap, dtype)
        bt.initialize(0, self.trajs[b].cfg, self.trajs[b].imu0)
        return bt
