"""Shared helpers for the parity tests: drive the CPU oracle and the HIP path with the same seeded inputs
and measure the parity metric of SURVEY.md section 8c."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import np_oracle  # noqa: E402  (oracle/ is on the path now)


def quat_angle(q, qref):
    """rotation angle of q (x) qref^-1 for (w,x,y,z) quaternions (atan2 form: accurate near zero)"""
    q = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    r = np.asarray(qref, dtype=np.float64) / np.linalg.norm(qref)
    rc = np.array([r[0], -r[1], -r[2], -r[3]])
    w = q[0] * rc[0] - q[1:] @ rc[1:]
    v = q[0] * rc[1:] + rc[0] * q[1:] + np.cross(q[1:], rc[1:])
    return float(2 * np.arctan2(np.linalg.norm(v), abs(w)))


def rel(x, ref, floor=1e-3):
    return float(np.linalg.norm(np.asarray(x) - np.asarray(ref)) / max(np.linalg.norm(ref), floor))


def state_errors(imu, imu_ref, cams, cams_ref, P, P_ref):
    """dict of the parity metrics: relative L2 per vector field, rotation angle for attitudes, relative
    Frobenius norm for the covariance (full and IMU block)."""
    e = dict(
        q=quat_angle(imu[0:4], imu_ref[0:4]), bg=rel(imu[4:7], imu_ref[4:7]), v=rel(imu[7:10], imu_ref[7:10]),
        ba=rel(imu[10:13], imu_ref[10:13]), p=rel(imu[13:16], imu_ref[13:16]),
        P=rel(P, P_ref, 1e-30), Pii=rel(P[:15, :15], P_ref[:15, :15], 1e-30))
    if len(cams_ref):
        e["cam_q"] = max(quat_angle(a[:4], b[:4]) for a, b in zip(cams, cams_ref))
        e["cam_p"] = max(rel(a[4:7], b[4:7]) for a, b in zip(cams, cams_ref))
    return e


def worst(e):
    return max(e.values())


def oracle_frame(o, tr, k, N):
    o.propagate(tr.imu_for_frame(k))
    o.augmentState(k, tr.frame_times[k])
    fr = tr.frames[k]
    if len(fr["M"]):
        o.setTracks(fr["M"], fr["slots"], fr["obs"])
        o.marginalize()
    if o.getNumCamStates() == N:
        o.dropOldest(1)


def device_frame(batch, b, tr, k, N):
    batch.propagate_range(b, 1, tr.imu_for_frame(k))
    batch.augment_range(b, 1)
    fr = tr.frames[k]
    batch.set_tracks(b, fr["M"], fr["slots"], fr["obs"])
    if len(fr["M"]):
        batch.marginalize_range(b, 1)
    if batch.num_cam_states(b) == N:
        batch.drop_oldest_range(b, 1, 1)


def copy_oracle_to_device(o, batch, b):
    """teacher forcing: device state + covariance <- oracle"""
    cams, _ = o.getCamStates()
    batch.set_covariance(b, o.getCovariance())
    batch.set_imu_state(b, o.getImuState())
    for i, c in enumerate(cams):
        batch.set_cam_pose(b, i, c)
    batch.set_num_residualized(b, o.numResidualized())


def check_tracks(td, to, ok, prec, tr, fr, o, k):
    """Per-track parity of the triangulated point and of the gate statistic (rows of last_tracks: motion_ok tri_valid
    gate_pass included gamma p_f_G).  Double: 1e-6 on both.  Float: the point is the result of an iterative solve whose
    depth error scales with depth^2 / baseline, so it is held (i) through what the filter uses it for -- its
    reprojection in every camera of the track agrees with the oracle's point to 1e-4 normalized units (0.05 px) -- and
    (ii) directly to 2e-3 of its depth; gamma to 1e-3 relative + 1e-3 absolute, and WITHOUT the absolute term where the
    oracle's gamma exceeds 0.05 (the absolute term is for the short tracks of quiet scenarios, gamma ~ 1e-2).
    Flags, for EVERY track and at the track's own index: motion_ok; tri_valid where the motion check passed; gate_pass and
    included (device column 3; the oracle stacks exactly the tracks that pass its gate) where a Jacobian was formed, and
    neither set elsewhere."""
    assert len(td) == len(to), (k, len(td), len(to))
    mo = to[:, 0] > 0
    assert np.array_equal(td[:, 0] > 0, mo), (k, "motion_ok", np.nonzero((td[:, 0] > 0) != mo)[0])
    assert np.array_equal((td[:, 1] > 0) & mo, (to[:, 1] > 0) & mo), (k, "tri_valid", np.nonzero(((td[:, 1] > 0) != (to[:, 1] > 0)) & mo)[0])
    jac = mo & (to[:, 1] > 0)
    want = jac & (to[:, 2] > 0)
    assert np.array_equal(td[:, 2] > 0, want), (k, "gate_pass", np.nonzero((td[:, 2] > 0) != want)[0])
    assert np.array_equal(td[:, 3] > 0, want), (k, "included", np.nonzero((td[:, 3] > 0) != want)[0])
    if prec == "f64":
        assert np.allclose(td[ok, 5:8], to[ok, 5:8], rtol=0, atol=1e-6), k
        assert np.allclose(td[ok, 4], to[ok, 4], rtol=1e-6, atol=1e-9), k
        return
    cams, _ = o.getCamStates()
    off = np.concatenate([[0], np.cumsum(fr["M"])])
    for t in np.nonzero(ok)[0]:
        sl = fr["slots"][off[t]:off[t + 1]]
        pd, pr = td[t, 5:8], to[t, 5:8]
        worst_rp, depth = 0.0, 1e9
        for s in sl:
            R = q_to_rot(cams[s, :4])
            a, b = R @ (pd - cams[s, 4:7]), R @ (pr - cams[s, 4:7])
            worst_rp = max(worst_rp, float(np.abs(a[:2] / a[2] - b[:2] / b[2]).max()))
            depth = min(depth, float(b[2]))
        assert worst_rp < 1e-4, (k, t, worst_rp)
        assert np.linalg.norm(pd - pr) < 2e-3 * max(depth, 1.0), (k, t, pd, pr, depth)
    assert np.allclose(td[ok, 4], to[ok, 4], rtol=1e-3, atol=1e-3), (k, np.abs(td[ok, 4] - to[ok, 4]).max())
    big = ok & (to[:, 4] > 0.05)
    assert np.allclose(td[big, 4], to[big, 4], rtol=1e-3, atol=0), (k, "gamma", np.nonzero(big & (np.abs(td[:, 4] - to[:, 4]) > 1e-3 * np.abs(to[:, 4])))[0])


def q_to_rot(q):
    """Eigen toRotationMatrix of (w,x,y,z)"""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def copy_device_to_oracle(batch, b, o):
    """teacher forcing the other way: oracle state + covariance <- device trajectory b (the oracle's window is built by
    replaying augmentState, then overwritten)"""
    cams, ids = batch.cam_states(b)
    while o.getNumCamStates() < len(cams):
        o.augmentState(int(ids[o.getNumCamStates()]) if len(ids) else 0, 0.0)
    o.setImuState(batch.imu_state(b))
    for i, c in enumerate(cams):
        o.setCamPose(i, c)
    o.setCovariance(batch.covariance(b))
    o.setNumResidualized(batch.num_residualized(b))


# ----------------------------------------------------------------------------------- ragged batches (tests/test_gpu_ragged.py)
STAT_KEYS = ("n_tracks", "n_motion_rejected", "n_tri_rejected", "n_gate_rejected", "n_passed", "m_rows")

# (window N_b, tracks per frame F_b, kind) per trajectory of the two ragged handles: the window sizes straddle the one-launch
# update's limit (14 | 15 cameras) and, on the second handle, the single-level factorizations' (31 | 33).  Kinds:
#   "dense"  every track spans the window, and on full-window frames track 0 also sees the newest camera: length N_b = m_cap
#   "idle"   F = 0 on every frame: never updates          "gaps"  handed an empty track list on every third frame
#   "gated"  on GATED_FRAME its observations carry 20 px of noise (test_all_tracks_gated_out_leaves_state_untouched's scenario)
RAGGED = {
    1: dict(n_cap=32, specs=[(5, 7, ""), (9, 24, ""), (14, 40, ""), (15, 33, ""), (21, 52, ""), (27, 60, ""), (32, 6, "dense"),
                             (10, 0, "idle"), (12, 20, "gaps"), (8, 24, "gated")]),
    2: dict(n_cap=40, specs=[(6, 9, ""), (14, 36, ""), (15, 28, ""), (31, 60, ""), (33, 44, ""), (40, 5, "dense"),
                             (11, 0, "idle"), (13, 22, "gaps"), (7, 30, "gated")]),
}
GATED_FRAME = 12


class RaggedSet:
    """The trajectories of one ragged handle: trajs[b] (scenario.Trajectory built for its own window N[b]), frames[b][k] the
    work-list trajectory b is handed on frame k, and the handle's capacities (n_cap = max N_b, f_cap = max F_b, m_cap = n_cap)."""

    def __init__(self, handle, seed0=500, nf=None, specs=None, n_cap=None):
        from msckf_mono_amd import scenario as sc
        r = RAGGED[handle] if handle else dict(n_cap=n_cap, specs=specs)
        self.specs = list(r["specs"])
        self.B = len(self.specs)
        self.N = [s[0] for s in self.specs]
        self.n_cap = r["n_cap"]
        self.m_cap = self.n_cap
        self.f_cap = max(max(s[1] for s in self.specs), 1)
        self.nf = nf if nf is not None else self.n_cap + 4
        assert max(self.N) <= self.n_cap
        self.trajs, self.frames = [], []
        for b, (N, F, kind) in enumerate(self.specs):
            tr = sc.Trajectory(2, seed0 + b, N, F, self.nf, dense_tracks=(kind == "dense"))
            fl = [dict(f) for f in tr.frames]
            if kind == "gaps":
                for k in range(1, self.nf, 3):
                    fl[k] = dict(Nw=fl[k]["Nw"], M=np.zeros(0, np.int32), slots=np.zeros(0, np.int32), obs=np.zeros((0, 2)))
            elif kind == "gated":
                noisy = sc.Trajectory(2, seed0 + b, N, F, self.nf, obs_noise_px=20.0)      # same seed: same motion and landmarks
                fl[GATED_FRAME] = dict(noisy.frames[GATED_FRAME])
            elif kind == "dense":
                for k in range(self.nf):
                    fl[k] = self._with_newest_camera(tr, k, fl[k], N)
            self.trajs.append(tr)
            self.frames.append(fl)

    @staticmethod
    def _with_newest_camera(tr, k, fr, N):
        """track 0 of a full-window frame, when it spans slots 0 .. N - 2, extended by its (noise-free) observation in the
        camera this frame's augmentState adds: a track of N observations"""
        if fr["Nw"] != N or not len(fr["M"]) or fr["M"][0] != N - 1:
            return fr
        pc = tr.C_CG[k] @ (tr.landmarks[k][0] - tr.p_C[k])
        if pc[2] <= 0.5:
            return fr
        M = fr["M"].copy()
        slots = np.insert(fr["slots"], M[0], N - 1).astype(np.int32)
        obs = np.insert(fr["obs"], M[0], pc[:2] / pc[2], axis=0)
        M[0] += 1
        return dict(Nw=fr["Nw"], M=M, slots=slots, obs=obs)

    def updating(self, b):
        return self.specs[b][1] > 0

    def full(self, b, k):
        return self.frames[b][k]["Nw"] == self.N[b]

    def imu(self, k):
        return np.stack([tr.imu_for_frame(k) for tr in self.trajs])

    def batch(self, capi, dtype):
        bt = capi.Batch(self.B, self.n_cap, self.f_cap, self.m_cap, dtype)
        for b, tr in enumerate(self.trajs):
            bt.initialize(b, tr.cfg, tr.imu0)
        return bt

    def oracle(self, po, dtype, b):
        o = po.Oracle(dtype, po.LEAN)
        o.initialize(self.trajs[b].cfg, self.trajs[b].imu0)
        return o

    def oracle_frame(self, o, b, k):
        """frame k of trajectory b on its oracle: propagate, augmentState, the update when it is handed tracks, the drop when
        its own window is full"""
        tr, fr = self.trajs[b], self.frames[b][k]
        o.propagate(tr.imu_for_frame(k))
        o.augmentState(k, tr.frame_times[k])
        if len(fr["M"]):
            o.setTracks(fr["M"], fr["slots"], fr["obs"])
            o.marginalize()
        if self.full(b, k):
            o.dropOldest(1)

    def device_frame(self, bt, k, only=None):
        """frame k through the per-call API, every device stage ONE launch sequence over the whole range: propagate_range and
        marginalize_range over (0, B); set_tracks per trajectory; the drop per trajectory, when its own window is full.
        only = b: trajectory b alone is active -- its neighbours are propagated, but get no camera state and no tracks."""
        act = range(self.B) if only is None else [only]
        bt.propagate_range(0, self.B, self.imu(k))
        if only is None:
            bt.augment_range(0, self.B)
        else:
            bt.augment_range(only, 1)
        for b in act:
            fr = self.frames[b][k]
            bt.set_tracks(b, fr["M"], fr["slots"], fr["obs"])
        bt.marginalize_range(0, self.B)
        for b in act:
            if self.full(b, k):
                bt.drop_oldest_range(b, 1, 1)

    def stage_scenario(self, bt):
        """the same frames as a resident scenario, the drop flag per trajectory from its own window"""
        from msckf_mono_amd import scenario as sc
        bt.scenario_alloc(self.nf, sc.IMU_PER_FRAME)
        for k in range(self.nf):
            for b, tr in enumerate(self.trajs):
                fr = self.frames[b][k]
                bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if self.full(b, k) else 0)
        bt.scenario_commit()


def snapshot(bt, b, strict=True):
    """everything a test compares bit for bit: IMU state, camera states, covariance, window size, statistics"""
    st = bt.last_stats(b, strict=strict)
    return bt.imu_state(b), bt.cam_states(b)[0], bt.covariance(b), bt.num_cam_states(b), {k: st[k] for k in STAT_KEYS + ("r_rows",)}


def same_bits(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3] and x[4] == y[4]


# ------------------------------------------------------ state kernels (tests/test_state_inputs.py, tests/test_gpu_state_kernels.py)
def cov_scaled_err(P, P_ref):
    """max_ij |P_ij - Pref_ij| / sqrt(Pref_ii Pref_jj): every entry against the scale of ITS row and column, so that an error in a
    small block (a camera's six columns, one sample's process noise) is not hidden under the norm of the whole matrix"""
    P, P_ref = np.asarray(P, dtype=np.float64), np.asarray(P_ref, dtype=np.float64)
    s = np.sqrt(np.diag(P_ref))
    return float(np.max(np.abs(P - P_ref) / np.outer(s, s)))


def imu_state_err(x, ref):
    """worst of the attitude angle and the relative error of v and p (the fields a propagate moves) of two IMU-29 states, and
    of their null-space anchors"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return max(quat_angle(x[0:4], ref[0:4]), rel(x[7:10], ref[7:10]), rel(x[13:16], ref[13:16]),
               quat_angle(x[19:23], ref[19:23]), rel(x[23:26], ref[23:26]), rel(x[26:29], ref[26:29]))


# Process noise and covariance scale of the state-kernel inputs.  With scenario.filter_config's Q_imu_diag one sample adds
# Q dT ~ 1e-4 * 0.005 to a P_II diagonal of 1e-5 .. 1e-2: a lost sample is 1e-8 of ||P||.  Here every diagonal entry of P_II that
# takes process noise (theta, b_g, v, b_a) starts at STATE_P_OVER_Q = 0.1 s times its Q_imu entry, so that one sample adds
# dT / 0.1 s of it: 2.5e-2 at the shortest dT of the families (0.0025 s), never below the 1e-3 the tests need (checked on the
# CPU in tests/test_state_inputs.py; the dT = 0 samples of `jitter` add nothing by definition).
STATE_Q_DIAG = [4e-3] * 3 + [4e-4] * 3 + [4e-2] * 3 + [4e-3] * 3
STATE_P_OVER_Q = 0.1
STATE_P_IMU_DIAG = [STATE_P_OVER_Q * q for q in STATE_Q_DIAG] + [1e-2] * 3
STATE_P_CAM_DIAG = [1e-3] * 3 + [1e-2] * 3
STATE_FAMILIES = ("nominal", "still", "fast", "jitter", "mixed")
STATE_JITTER_DT = (0.0025, 0.005, 0.01, 0.02)
STATE_JITTER_ZERO_AT = (5, 20)     # samples of `jitter` with dT = 0 exactly (finite in both references: test_state_inputs.py)
STATE_FAST_ANGLE = 0.5             # |omega - b_g| dT of the `fast` samples [rad]


def _state_sample(kind, rng, bg, k, fast_angle):
    """one reading of family `kind`: omega(3) a(3) dT"""
    u = rng.normal(3)
    u /= np.linalg.norm(u)
    acc = 3.0 * rng.normal(3) + np.array([0.0, 0.0, 9.81])
    jit = STATE_JITTER_DT[int(rng.integers(1, len(STATE_JITTER_DT))[0])]
    dT = 0.005
    if kind == "still":
        om = bg.copy()                                  # omega - b_g = 0 exactly (in float too: both round the same way)
    elif kind == "fast":
        om = bg + u * (fast_angle / dT)
    elif kind == "jitter":
        dT = 0.0 if k in STATE_JITTER_ZERO_AT else jit
        om = bg + 0.4 * u
    else:
        om = bg + 0.4 * u + 0.01 * rng.normal(3)
    return np.concatenate([om, acc, [dT]])


def state_inputs(case, seed, K=40, fast_angle=STATE_FAST_ANGLE):
    """(imu29, cfg, readings [K][7]) of reading family `case` (STATE_FAMILIES), from scenario.SplitMix64(seed) alone.  `mixed`
    cycles through the four other families and has a `still` and a `fast` sample on each side of index 16 (14, 15 | 17, 18);
    sample 16 itself is a nominal one of 0.01 s."""
    from msckf_mono_amd import scenario as sc
    assert case in STATE_FAMILIES
    rng = sc.SplitMix64(0x57A7E000 + 7919 * int(seed) + STATE_FAMILIES.index(case))
    q = rng.normal(4)
    q = q / np.linalg.norm(q) * (1.0 if q[0] >= 0 else -1.0)
    bg, v, ba, p = 0.01 * rng.normal(3), rng.normal(3), 0.05 * rng.normal(3), 2.0 * rng.normal(3)
    imu = np.concatenate([q, bg, v, ba, p, sc.GRAVITY, q, v, p])
    cfg = sc.filter_config(64)
    cfg["Q_imu_diag"] = list(STATE_Q_DIAG)
    cfg["P0_diag"] = list(STATE_P_IMU_DIAG)
    cfg["max_cam_states"] = 63
    fixed = {14: "still", 15: "fast", 16: "nominal", 17: "fast", 18: "still"}
    rd = np.zeros((K, 7))
    for k in range(K):
        kind = case if case != "mixed" else fixed.get(k, STATE_FAMILIES[k % 4])
        rd[k] = _state_sample(kind, rng, bg, k, fast_angle)
        if case == "mixed" and k == 16:
            rd[k, 6] = 0.01
    return imu, cfg, rd


def state_spd(ncam, seed):
    """random symmetric positive definite covariance of a window of ncam camera states: a random correlation matrix (Wishart,
    2 D degrees of freedom) scaled to the diagonals STATE_P_IMU_DIAG / STATE_P_CAM_DIAG"""
    from msckf_mono_amd import scenario as sc
    D = 15 + 6 * ncam
    rng = sc.SplitMix64(0xC0FA0000 + 104729 * int(seed) + ncam)
    A = rng.normal(2 * D * D).reshape(D, 2 * D)
    C = A @ A.T
    d = np.sqrt(np.diag(C))
    s = np.sqrt(np.array(STATE_P_IMU_DIAG + STATE_P_CAM_DIAG * ncam))
    P = C / np.outer(d, d) * np.outer(s, s)
    return (P + P.T) / 2


def state_cam_poses(ncam, seed):
    """ncam distinct camera poses q_CG(4, unit) p_C_G(3)"""
    from msckf_mono_amd import scenario as sc
    rng = sc.SplitMix64(0xCA3E0000 + int(seed))
    q = rng.normal(4 * ncam).reshape(ncam, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= np.where(q[:, :1] >= 0, 1.0, -1.0)
    return np.concatenate([q, 3.0 * rng.normal(3 * ncam).reshape(ncam, 3)], 1)


def oracle_window(o, cfg, imu, P, poses):
    """oracle `o` holding the IMU state, the len(poses) camera states and the covariance given"""
    o.initialize(cfg, imu)
    for i in range(len(poses)):
        o.augmentState(i, 0.0)
    o.setImuState(imu)
    for i, c in enumerate(poses):
        o.setCamPose(i, c)
    o.setCovariance(P)
    return o


def device_window(bt, b, cfg, imu, P, poses):
    """the same on trajectory b of a device batch (set_covariance, set_imu_state, set_cam_pose)"""
    bt.initialize(b, cfg, imu)
    bt.set_covariance(b, P)                 # (sets the window size with it)
    bt.set_imu_state(b, imu)
    for i, c in enumerate(poses):
        bt.set_cam_pose(b, i, c)


class TwinMutant(np_oracle.NpMSCKF):
    """oracle/np_oracle.NpMSCKF (the numpy/scipy twin) with a block propagate and, optionally, ONE deliberate mistake -- applied
    to this reference only, never to the code under test -- to show that inputs and metric can see it:
      "a"  no G Q G^T dT for sample 16 of a call        "b"  sample 16's null-space patch anchored at the state before sample 0
      "c"  the last camera's six P_IC columns are left unmultiplied        "d"  p advanced with the NEW velocity
    P / ncam: start from this covariance with ncam camera states; a config's whole "Q_imu" is used when it has one."""

    def __init__(self, cfg, imu, mutation=None, P=None, ncam=0):
        super().__init__(cfg, imu)
        assert mutation in (None, "a", "b", "c", "d")
        self.mutation = mutation
        if "Q_imu" in cfg:
            self.Q = np.array(cfg["Q_imu"], dtype=np.float64)
        if "P0" in cfg:
            self.P = np.array(cfg["P0"], dtype=np.float64)
        for i in range(ncam):
            self.augment(i)
        if P is not None:
            self.P = np.array(P, dtype=np.float64)

    def propagate_block(self, rds):
        rds = np.asarray(rds, dtype=np.float64).reshape(-1, 7)
        start = (self.q.copy(), self.v.copy(), self.p.copy())
        for k, rd in enumerate(rds):
            Q, keep = self.Q, None
            if self.mutation == "a" and k == 16:
                self.Q = np.zeros_like(Q)
            if self.mutation == "b" and k == 16:
                self.q_null, self.v_null, self.p_null = (x.copy() for x in start)
            if self.mutation == "c" and self.P.shape[0] > 15:
                keep = self.P[:15, -6:].copy()
            p_old = self.p.copy()
            self.propagate(rd)
            self.Q = Q
            if keep is not None:
                self.P[:15, -6:] = keep
                self.P[-6:, :15] = keep.T
            if self.mutation == "d":
                self.p = p_old + self.v * float(rd[6])
                self.p_null = self.p.copy()
