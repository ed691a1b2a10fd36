"""Seeded synthetic IMU + feature-track scenarios for the batched MSCKF core.

The reference consumes (a) IMU samples `imuReading{omega, a, dT}` (types.h:78-84, produced at 200 Hz by
datasets/asl_readers.cpp:181-206) and (b) per-image lists of undistorted *normalized* feature
coordinates with ids (corner_detector.cpp:320-439 -> MSCKF::update/addFeatures, msckf.h:215,302).  No
EuRoC data exists in this image, so this module generates both from an analytic trajectory:

  p(t) = [3 cos 0.4t, 3 sin 0.4t, 0.5 sin 0.8t] m, camera looking radially outwards (good parallax),
  small roll/pitch wobble, EuRoC cam0 extrinsics (euroc/MH_03_kalibr.yaml:5-9), 200 Hz IMU, 20 Hz camera.

Everything is driven by a counter-based splitmix64 stream so that a (config, trajectory) pair always
yields the same data on any machine: seed = 0x5EED0000 + 1000*config + trajectory.

Steady-state window (what BASELINE.json's configs are quoted on): at update time the filter holds
exactly N camera states; each frame F tracks end (last observation in the previous frame, slot N-2) and
span slots [N-1-M_j, N-2] with M_j = 3 + (rng mod (N-3)); after the update the oldest state is pruned.
"""
import numpy as np

_MASK = np.uint64(0xFFFFFFFFFFFFFFFF)
_GAMMA = np.uint64(0x9E3779B97F4A7C15)

# Kalibr T_cam_imu for EuRoC cam0 (reference euroc/MH_03_kalibr.yaml:5-9)
T_CAM_IMU = np.array([
    [0.0148655429818, -0.999880929698, 0.00414029679422, -0.021640145497],
    [0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768],
    [-0.0257744366974, 0.00375618835797, 0.999660727178, 0.009810730590],
    [0.0, 0.0, 0.0, 1.0]])
EUROC_INTRINSICS = (458.654, 457.296, 367.215, 248.375)  # f_u f_v c_u c_v (MH_03_kalibr.yaml:13)
GRAVITY = np.array([0.0, 0.0, -9.81])                    # datasets/asl_msckf.cpp:154
IMU_RATE, CAM_RATE = 200, 20
IMU_PER_FRAME = IMU_RATE // CAM_RATE


class SplitMix64:
    """Counter-based splitmix64: value i of the stream is mix(seed + (i+1)*gamma)."""

    def __init__(self, seed):
        self.seed = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
        self.ctr = 0

    def u64(self, n):
        with np.errstate(over="ignore"):
            i = np.arange(self.ctr + 1, self.ctr + n + 1, dtype=np.uint64)
            z = self.seed + i * _GAMMA
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        self.ctr += n
        return z

    def uniform(self, n):
        return (self.u64(n) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)

    def normal(self, n):
        m = (n + 1) // 2
        u1 = 1.0 - self.uniform(m)
        u2 = self.uniform(m)
        r = np.sqrt(-2.0 * np.log(u1))
        return np.concatenate([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)])[:n]

    def integers(self, n, mod):
        return (self.u64(n) % np.uint64(mod)).astype(np.int64)


# ------------------------------------------------------------------ Monte-Carlo replay: the numpy twin of csrc/replay_plan.h
# The noise a replay adds on the device is a pure function of (seed, frame, index); include/msckf_hip.h states it, this is its
# twin.  The integer part (replay_mix, replay_uniform) agrees with the host and device code bit for bit; ln, sqrt, cos and sin
# are numpy's.  Two noise models: four white levels (replay_noise / replay_cell / replay_expand), or the filter's Q_imu with its
# bias random walks (replay_noise_factor / replay_model_* / replay_walk / replay_bias_gt, further down).
def replay_mix(seed, i):
    """value i (0-based; an int or an array) of SplitMix64(seed), as uint64"""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + (np.asarray(i, dtype=np.uint64) + np.uint64(1)) * _GAMMA
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def replay_uniform(seed, i):
    """U(seed, i) = (mix(seed, i) >> 11) 2^-53, in [0, 1)"""
    return (replay_mix(seed, i) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def replay_pairs(seed, n):
    """pairs 0 .. n - 1 of sub-seed `seed`, [n][2]: (r cos(2 pi u2), r sin(2 pi u2)), u1 = 1 - U(seed, 2 j), u2 = U(seed, 2 j + 1)"""
    j = np.arange(n, dtype=np.uint64)
    u1 = 1.0 - replay_uniform(seed, np.uint64(2) * j)
    u2 = replay_uniform(seed, np.uint64(2) * j + np.uint64(1))
    r = np.sqrt(-2.0 * np.log(u1))
    return np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], -1)


def replay_subseeds(seed, frame):
    """(s_imu, s_obs) of a trajectory's seed on a frame: mix(seed, 2 f), mix(seed, 2 f + 1)"""
    return int(replay_mix(seed, 2 * int(frame))), int(replay_mix(seed, 2 * int(frame) + 1))


def replay_noise(seed, frame, K, k, n_entries):
    """unit-variance noise of one cell: (imu [K][6], rows from k on zero: g_x g_y g_z a_x a_y a_z of sample i from the pairs
    3 i, 3 i + 1, 3 i + 2 of s_imu; obs [n_entries][2]: (n_u, n_v) of entry e from pair e of s_obs)"""
    s_imu, s_obs = replay_subseeds(seed, frame)
    imu = np.zeros((K, 6))
    k = max(int(k), 0)                       # (a skipped cell's count is -1)
    imu[:k] = replay_pairs(s_imu, 3 * k).reshape(k, 6)
    return imu, replay_pairs(s_obs, n_entries).reshape(n_entries, 2)


def replay_cell(readings, obs, frame, seed, sigma4, K=None):
    """a noise-free cell (readings [k][7], obs [n][2]) as trajectory `seed` sees it on `frame` with sigma4 = (sigma_g, sigma_a,
    sigma_u, sigma_v): (readings [K][7] with rows from k on zero, obs [n][2]), in double"""
    rd = np.asarray(readings, dtype=np.float64).reshape(-1, 7)
    ob = np.asarray(obs, dtype=np.float64).reshape(-1, 2)
    k = len(rd)
    K = k if K is None else int(K)
    imu, nz = replay_noise(seed, frame, K, k, len(ob))
    sg, sa, su, sv = (float(x) for x in sigma4)
    out = np.zeros((K, 7))
    out[:k] = rd
    out[:, 0:3] += sg * imu[:, 0:3]
    out[:, 3:6] += sa * imu[:, 3:6]
    return out, ob + np.array([su, sv]) * nz


def replay_expand(seq_traj, frame, seed, sigma4):
    """frame `frame` of the noise-free Trajectory seq_traj (imu_noise_scale = 0, obs_noise_px = 0) with the replay's noise:
    (readings [IMU_PER_FRAME][7], obs [n][2]); M and slots are the sequence's own"""
    return replay_cell(seq_traj.imu_for_frame(frame), seq_traj.frames[frame]["obs"], frame, seed, sigma4)


# ---- the Q_imu model (csrc/replay_plan.h, MODEL; include/msckf_hip.h, msckf_hip_replay_assign_q): correlated noise drawn from
# the filter's own 12 x 12 Q_imu (noise order n_g n_wg n_a n_wa) and the two bias random walks.  Every sum below is formed in the
# order the header states, one rounded operation after the other, so that given the same draws the device's bits are these.
REPLAY_PSD_TOL = 1e-12


def chol_psd(A, what="Q"):
    """L = chol_psd(0.5 (A + A^T)), [n][n] lower triangular, as replay_plan.h forms it: column by column, d = A_cc - sum_j L_cj^2
    (ascending j); d < -1e-12 max_diag raises ValueError, |d| <= 1e-12 max_diag leaves the column zero"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    A = 0.5 * (A + A.T)
    top = max(0.0, float(np.max(np.diag(A))))
    L = np.zeros((n, n))
    for c in range(n):
        s = 0.0
        for j in range(c):
            s = s + L[c, j] * L[c, j]
        d = A[c, c] - s
        if d < -REPLAY_PSD_TOL * top:
            raise ValueError("%s is not positive semi-definite" % what)
        if abs(d) <= REPLAY_PSD_TOL * top:
            continue
        p = np.sqrt(d)
        L[c, c] = p
        for r in range(c + 1, n):
            t = 0.0
            for j in range(c):
                t = t + L[r, j] * L[c, j]
            L[r, c] = (A[r, c] - t) / p
    return L


def replay_noise_factor(Q):
    """L = chol_psd(0.5 (Q + Q^T)), [12][12] lower triangular: the factor of the Q_imu model's noise"""
    return chol_psd(np.asarray(Q, dtype=np.float64).reshape(12, 12))


def replay_model_draws(seed, frame, k, L, pairs_per_sample=6):
    """w [k][12] of a cell's samples: z[i] = pairs 6 i .. 6 i + 5 of s_imu, w_r = sum_{c <= r} L_rc z_c with c ascending from 0.0"""
    k = max(int(k), 0)
    s_imu = replay_subseeds(seed, frame)[0]
    j = (np.uint64(pairs_per_sample) * np.arange(k, dtype=np.uint64))[:, None] + np.arange(6, dtype=np.uint64)[None, :]
    u1 = 1.0 - replay_uniform(s_imu, np.uint64(2) * j)
    u2 = replay_uniform(s_imu, np.uint64(2) * j + np.uint64(1))
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)], -1).reshape(k, 12)
    L = np.asarray(L, dtype=np.float64)
    w = np.zeros((k, 12))
    for row in range(12):
        a = np.zeros(k)
        for c in range(row + 1):
            a = a + L[row, c] * z[:, c]
        w[:, row] = a
    return w


def replay_model_increments(dT, w, scale):
    """(noise [k][6] on omega and a, delta [k][6] of the gyro and accelerometer bias) of samples with steps dT [k] and draws
    w [k][12]: (scale w) / sqrt(dT) of rows 0:3, 6:9 and (scale w) sqrt(dT) of rows 3:6, 9:12; both zero where dT <= 0"""
    dT = np.asarray(dT, dtype=np.float64)
    ok = dT > 0.0
    sq = np.sqrt(np.where(ok, dT, 1.0))[:, None]
    sw = float(scale) * w
    noise = np.where(ok[:, None], sw[:, [0, 1, 2, 6, 7, 8]] / sq, 0.0)
    delta = np.where(ok[:, None], sw[:, [3, 4, 5, 9, 10, 11]] * sq, 0.0)
    return noise, delta


def replay_model_cell(readings, obs, frame, seed, L, scale, sigma_uv, w_start, K=None):
    """a noise-free cell (readings [k][7], obs [n][2]) as trajectory `seed` sees it on `frame` under the model, the walk standing
    at w_start [6] when the frame begins: (readings [K][7] with rows from k on zero, obs [n][2], w_end [6] = the walk after the
    cell's k samples, Wstart of the next frame)"""
    rd = np.asarray(readings, dtype=np.float64).reshape(-1, 7)
    ob = np.asarray(obs, dtype=np.float64).reshape(-1, 2)
    k = len(rd)
    K = k if K is None else int(K)
    noise, delta = replay_model_increments(rd[:, 6], replay_model_draws(seed, frame, k, L), scale)
    P = np.zeros((k + 1, 6))
    for i in range(k):
        P[i + 1] = P[i] + delta[i]
    w_start = np.asarray(w_start, dtype=np.float64)
    out = np.zeros((K, 7))
    out[:k] = rd
    out[:k, :6] = (rd[:, :6] + (w_start + P[:k])) + noise
    nz = replay_pairs(replay_subseeds(seed, frame)[1], len(ob))
    return out, ob + np.array([float(sigma_uv[0]), float(sigma_uv[1])]) * nz, w_start + P[k]


def _replay_cells(seq_traj_or_cells):
    if hasattr(seq_traj_or_cells, "imu_for_frame"):
        return [seq_traj_or_cells.imu_for_frame(f) for f in range(seq_traj_or_cells.n_frames)]
    return [np.zeros((0, 7)) if c is None else np.asarray(c, dtype=np.float64).reshape(-1, 7) for c in seq_traj_or_cells]


def replay_walk(seq_traj_or_cells, seed, L, scale):
    """Wstart [frames + 1][6] of a trajectory that replays a noise-free Trajectory, or a list of per-frame readings [k][7] (None
    or empty: a skipped cell or one without samples): Wstart[0] = 0, Wstart[f + 1] = Wstart[f] + P(f, k_f)"""
    cells = _replay_cells(seq_traj_or_cells)
    W = np.zeros((len(cells) + 1, 6))
    for f, rd in enumerate(cells):
        W[f + 1] = replay_model_cell(rd, np.zeros((0, 2)), f, seed, L, scale, (0.0, 0.0), W[f])[2]
    return W


def replay_model_expand(seq_traj, frame, seed, L, scale, sigma_uv, w_start=None):
    """frame `frame` of the noise-free Trajectory seq_traj under the model: (readings [IMU_PER_FRAME][7], obs [n][2]);
    w_start: the frame's row of replay_walk (computed here when not given)"""
    if w_start is None:
        w_start = replay_walk(seq_traj, seed, L, scale)[frame]
    return replay_model_cell(seq_traj.imu_for_frame(frame), seq_traj.frames[frame]["obs"], frame, seed, L, scale, sigma_uv, w_start)[:2]


def replay_imu_sums(seq_traj_or_cells, seed, f0, f1, sigma4=None, model=None, dtype=np.float64):
    """msckf_hip_replay_imu_sums for one trajectory: [8] = samples, sum omega (3), sum a (3), sum dT over the frames [f0, f1) of a
    noise-free Trajectory or a list of per-frame readings [k][7] (None: a skipped cell), each sample as the expansion stores it:
    replay_cell's rows under sigma4 = (sigma_g, sigma_a, ., .), or replay_model_cell's under model = (L, scale) on the walk of
    replay_walk, rounded to `dtype` (the handle's scalar) and summed in double.  The order of the sum is numpy's, not the
    device's: the two agree to the summation bound, not to the bit."""
    cells = _replay_cells(seq_traj_or_cells)
    if (sigma4 is None) == (model is None):
        raise ValueError("one of sigma4 and model")
    W = None if model is None else replay_walk(cells, seed, model[0], model[1])
    out = np.zeros(8)
    for f in range(int(f0), int(f1)):
        rd = cells[f]
        if not len(rd):
            continue
        if model is None:
            rows = replay_cell(rd, np.zeros((0, 2)), f, seed, sigma4)[0]
        else:
            rows = replay_model_cell(rd, np.zeros((0, 2)), f, seed, model[0], model[1], (0.0, 0.0), W[f])[0]
        rows = rows.astype(dtype).astype(np.float64)
        out[0] += len(rows)
        out[1:8] += rows.sum(0)
    return out


def replay_bias_gt(trajs, walks):
    """the true b_g, b_a at each frame-log record: [frames][B][6] = trajs[b]'s constant biases + walks[f + 1][b] (walks
    [frames + 1][B][6]: Batch.replay_walk() or the stacked replay_walk of each trajectory), to take bias errors and bias NEES
    from frame_log_read by"""
    walks = np.asarray(walks, dtype=np.float64)
    const = np.stack([np.concatenate([tr.b_g, tr.b_a]) for tr in trajs])
    return const[None, :, :] + walks[1:]


# ---- seeded front-end faults (csrc/replay_plan.h, FAULTS; include/msckf_hip.h, msckf_hip_replay_set_faults): missed
# observations and outliers per trajectory, fault4 = (p_miss, p_out, rho_u, rho_v), on top of either noise model
REPLAY_FAULT_STREAM = (1 << 63) + 1
FAULT_KEPT, FAULT_OUTLIER, FAULT_MISSED = 0, 1, 2


def replay_fault_seed(seed, frame):
    """s_flt = mix(mix(seed, 2^63 + 1), frame): frames use mix(seed, 2 f) and mix(seed, 2 f + 1), replay_initial_error uses
    mix(seed, 2^63); no frame index reaches either"""
    return int(replay_mix(int(replay_mix(seed, REPLAY_FAULT_STREAM)), int(frame)))


def replay_fault_draws(seed, frame, n_entries):
    """(u_miss, u_out, u_ang), each [n_entries]: entry e of the sequence cell takes U(s_flt, 3 e), U(s_flt, 3 e + 1), U(s_flt, 3 e + 2)"""
    s = replay_fault_seed(seed, frame)
    e = np.uint64(3) * np.arange(int(n_entries), dtype=np.uint64)
    return replay_uniform(s, e), replay_uniform(s, e + np.uint64(1)), replay_uniform(s, e + np.uint64(2))


def replay_fault_code(M, draws, p_miss, p_out):
    """per entry of a cell with track lengths M (entries in sequence order): FAULT_MISSED where u_miss < p_miss -- unless the
    track would keep fewer than two observations, then it loses none -- else FAULT_OUTLIER where u_out < p_out, else FAULT_KEPT"""
    u_miss, u_out = np.asarray(draws[0]), np.asarray(draws[1])
    code = np.zeros(len(u_miss), dtype=np.int32)
    o = 0
    for m in (int(x) for x in M):
        miss = u_miss[o:o + m] < float(p_miss)
        if m - int(miss.sum()) < 2:
            miss = np.zeros(m, dtype=bool)
        code[o:o + m] = np.where(miss, FAULT_MISSED, np.where(u_out[o:o + m] < float(p_out), FAULT_OUTLIER, FAULT_KEPT))
        o += m
    assert o == len(code)
    return code


def replay_fault_cell(M, slots, obs_noisy, code, u_ang, rho_u, rho_v):
    """what the faulted expansion writes for a cell whose noisy coordinates are obs_noisy [n][2]: (M' = survivors per track,
    slots [n], obs [n][2]) with every track's range a stable partition -- survivors in sequence order, then the missed entries
    in sequence order -- and the outliers displaced by (rho_u cos a, rho_v sin a), a = the rounded product 2 pi u_ang"""
    M = np.asarray(M, dtype=np.int32)
    slots = np.asarray(slots, dtype=np.int32)
    code = np.asarray(code)
    ob = np.array(obs_noisy, dtype=np.float64).reshape(-1, 2)
    a = 6.283185307179586 * np.asarray(u_ang, dtype=np.float64)
    out = code == FAULT_OUTLIER
    ob[out, 0] = ob[out, 0] + float(rho_u) * np.cos(a[out])
    ob[out, 1] = ob[out, 1] + float(rho_v) * np.sin(a[out])
    order, Mp, o = [], np.zeros_like(M), 0
    for t, m in enumerate(int(x) for x in M):
        miss = code[o:o + m] == FAULT_MISSED
        order += list(o + np.nonzero(~miss)[0]) + list(o + np.nonzero(miss)[0])
        Mp[t] = m - int(miss.sum())
        o += m
    order = np.asarray(order, dtype=np.int64)
    return Mp, slots[order], ob[order]


def replay_fault_survivors(M, Mp, slots, obs):
    """the survivors of replay_fault_cell's (or the device's) partitioned cell, compact: (M', slots, obs) with no slack -- what a
    caller without slack (the CPU oracle, an ordinary scenario) is handed"""
    M, Mp = np.asarray(M, dtype=np.int64), np.asarray(Mp, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(M)])[:len(M)]
    keep = np.concatenate([np.arange(o, o + m) for o, m in zip(off, Mp)]).astype(np.int64) if len(M) else np.zeros(0, np.int64)
    return Mp.astype(np.int32), np.asarray(slots)[keep], np.asarray(obs).reshape(-1, 2)[keep]


def _replay_faulted(frame, seed, M, slots, obs, fault4):
    p_miss, p_out, rho_u, rho_v = (float(x) for x in fault4)
    draws = replay_fault_draws(seed, frame, len(obs))
    code = replay_fault_code(M, draws, p_miss, p_out)
    return replay_fault_cell(M, slots, obs, code, draws[2], rho_u, rho_v) + (code,)


def replay_expand_faulted(seq_traj, frame, seed, sigma4, fault4):
    """replay_expand with faults: (readings, M', slots, obs, code) in the expanded block's partition order"""
    rd, obs = replay_expand(seq_traj, frame, seed, sigma4)
    fr = seq_traj.frames[frame]
    return (rd,) + _replay_faulted(frame, seed, fr["M"], fr["slots"], obs, fault4)


def replay_model_expand_faulted(seq_traj, frame, seed, L, scale, sigma_uv, fault4, w_start=None):
    """replay_model_expand with faults: (readings, M', slots, obs, code) in the expanded block's partition order"""
    rd, obs = replay_model_expand(seq_traj, frame, seed, L, scale, sigma_uv, w_start)
    fr = seq_traj.frames[frame]
    return (rd,) + _replay_faulted(frame, seed, fr["M"], fr["slots"], obs, fault4)


# ---- the camera's clock (csrc/replay_plan.h, TIMING; include/msckf_hip.h, msckf_hip_replay_set_timing): time offset, per-image
# jitter and rolling-shutter readout per trajectory, timing4 = (t_d, r_y, y_0, sigma_j), on top of either noise model and of the
# faults.  Every operation below is one rounded double operation in the header's order: given the same delta the device's bits
# are these.
REPLAY_TIMING_STREAM = (1 << 63) + 2


def replay_image_table(cells):
    """the image table of a sequence: (time [images], frame_of [images], base [frames]).  cells: a noise-free Trajectory (its
    frames drop one state once the window is full), or per frame None (a skipped cell) or (readings [k][7], n_drop).  T = 0,
    ord = 0, W = 0; every cell that is not skipped adds its dT in order to T, then ord += 1, W += 1, time[ord - 1] = T,
    frame_of[ord - 1] = f, base[f] = ord - W, W -= n_drop; camera slot s of frame f's cell is image base[f] + s"""
    if hasattr(cells, "imu_for_frame"):
        tr = cells
        cells = [(tr.imu_for_frame(f), 1 if tr.frames[f]["Nw"] == tr.N else 0) for f in range(tr.n_frames)]
    T, ord_, W = np.float64(0.0), 0, 0
    time, frame_of, base = [], [], np.zeros(len(cells), dtype=np.int32)
    for f, c in enumerate(cells):
        if c is not None:
            for dT in np.asarray(c[0], dtype=np.float64).reshape(-1, 7)[:, 6]:
                T = T + dT
            ord_ += 1
            W += 1
            time.append(T)
            frame_of.append(f)
        base[f] = ord_ - W
        if c is not None:
            W -= int(c[1])
    return np.array(time, dtype=np.float64), np.array(frame_of, dtype=np.int32), base


def replay_timing_jitter(seed, image_frames):
    """g(q) for the frames q of some images: the first component of pair q of the sub-seed mix(seed, 2^63 + 2)"""
    s = int(replay_mix(seed, REPLAY_TIMING_STREAM))
    q = np.asarray(image_frames, dtype=np.uint64)
    u1 = 1.0 - replay_uniform(s, np.uint64(2) * q)
    u2 = replay_uniform(s, np.uint64(2) * q + np.uint64(1))
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)


def replay_timing_delta(y, image_frames, seed, timing4):
    """delta [n] of entries with sequence values y [n] on images taken at the frames image_frames [n] (frame_of[base + slot]):
    (t_d + r_y (y - y_0)) + sigma_j g(frame); sigma_j == 0: no draw"""
    t_d, r_y, y_0, s_j = (np.float64(x) for x in timing4)
    y = np.asarray(y, dtype=np.float64)
    g = replay_timing_jitter(seed, image_frames) if s_j != 0.0 else np.zeros(len(y))
    return (t_d + r_y * (y - y_0)) + s_j * g


def replay_timing_stencil(l, M):
    """(first node, node count) of entry l of a track of M entries: M < 3 the whole track, else l0 = min(max(l - 1, 0), M - 3)"""
    return (0, M) if M < 3 else (min(max(l - 1, 0), M - 3), 3)


def replay_timing_shift(M, slots, obs, time, base_f, delta, stencil=replay_timing_stencil):
    """the cell's coordinates [n][2] with every entry moved along its own track to time[base_f + slot] + delta: Lagrange weights
    over the stencil's nodes, times taken relative to the entry's own; delta == 0 and tracks of one entry: the value itself"""
    ob = np.asarray(obs, dtype=np.float64).reshape(-1, 2)
    out = ob.copy()
    tm = np.asarray(time, dtype=np.float64)[int(base_f) + np.asarray(slots, dtype=np.int64)] if len(ob) else np.zeros(0)
    delta = np.asarray(delta, dtype=np.float64)
    o = 0
    for m in (int(x) for x in M):
        for l in range(m):
            dl = delta[o + l]
            l0, n = stencil(l, m)
            if n < 2 or dl == 0.0:
                continue
            d = [tm[o + l0 + j] - tm[o + l] for j in range(n)]
            acc = None
            for j in range(n):
                others = [i for i in range(n) if i != j]
                num, den = dl - d[others[0]], d[j] - d[others[0]]
                for i in others[1:]:
                    num, den = num * (dl - d[i]), den * (d[j] - d[i])
                p = (num / den) * ob[o + l0 + j]
                acc = p if acc is None else acc + p
            out[o + l] = acc
        o += m
    assert o == len(ob)
    return out


def _replay_timed_obs(seq_traj, frame, seed, timing4, delta, table):
    fr = seq_traj.frames[frame]
    time, frame_of, base = replay_image_table(seq_traj) if table is None else table
    if delta is None:
        delta = replay_timing_delta(fr["obs"][:, 1], frame_of[base[frame] + fr["slots"]], seed, timing4) if len(fr["obs"]) else np.zeros(0)
    return replay_timing_shift(fr["M"], fr["slots"], fr["obs"], time, base[frame], delta)


def replay_expand_timed(seq_traj, frame, seed, sigma4, timing4, delta=None, table=None):
    """replay_expand under the timing record: every coordinate moved along its track before the noise is added.  delta [n]: the
    entries' deltas when they are known (the device's), else replay_timing_delta's; table: replay_image_table(seq_traj)"""
    return replay_cell(seq_traj.imu_for_frame(frame), _replay_timed_obs(seq_traj, frame, seed, timing4, delta, table), frame, seed, sigma4)


def replay_model_expand_timed(seq_traj, frame, seed, L, scale, sigma_uv, timing4, w_start=None, delta=None, table=None):
    """replay_model_expand under the timing record"""
    if w_start is None:
        w_start = replay_walk(seq_traj, seed, L, scale)[frame]
    obs = _replay_timed_obs(seq_traj, frame, seed, timing4, delta, table)
    return replay_model_cell(seq_traj.imu_for_frame(frame), obs, frame, seed, L, scale, sigma_uv, w_start)[:2]


def replay_expand_timed_faulted(seq_traj, frame, seed, sigma4, timing4, fault4, delta=None, table=None):
    """replay_expand_timed with faults: (readings, M', slots, obs, code) in the expanded block's partition order"""
    rd, obs = replay_expand_timed(seq_traj, frame, seed, sigma4, timing4, delta, table)
    fr = seq_traj.frames[frame]
    return (rd,) + _replay_faulted(frame, seed, fr["M"], fr["slots"], obs, fault4)


def replay_model_expand_timed_faulted(seq_traj, frame, seed, L, scale, sigma_uv, timing4, fault4, w_start=None, delta=None, table=None):
    """replay_model_expand_timed with faults: (readings, M', slots, obs, code) in the expanded block's partition order"""
    rd, obs = replay_model_expand_timed(seq_traj, frame, seed, L, scale, sigma_uv, timing4, w_start, delta, table)
    fr = seq_traj.frames[frame]
    return (rd,) + _replay_faulted(frame, seed, fr["M"], fr["slots"], obs, fault4)


def replay_fault_counts(cells_M, seed, fault4, f0=0, f1=None):
    """msckf_hip_replay_fault_counts for one trajectory: cells_M[f] the track lengths of its sequence's cell on frame f (None or
    empty: no track); int64 [6] = entries, missed, outliers, tracks, tracks that lost an observation, tracks with an outlier"""
    f1 = len(cells_M) if f1 is None else int(f1)
    c = np.zeros(6, dtype=np.int64)
    for f in range(int(f0), f1):
        M = np.zeros(0, np.int64) if cells_M[f] is None else np.asarray(cells_M[f], dtype=np.int64)
        n = int(M.sum())
        code = replay_fault_code(M, replay_fault_draws(seed, f, n), fault4[0], fault4[1])
        o = 0
        c[0] += n; c[1] += int((code == FAULT_MISSED).sum()); c[2] += int((code == FAULT_OUTLIER).sum()); c[3] += len(M)
        for m in (int(x) for x in M):
            c[4] += bool((code[o:o + m] == FAULT_MISSED).any()); c[5] += bool((code[o:o + m] == FAULT_OUTLIER).any())
            o += m
    return c


def replay_gate_confusion(records, cells_M, seed, fault4, q0, q1, f0):
    """msckf_hip_map_log_fault_metrics for one trajectory: records [n][8] (map-log records: gamma 3, frame ordinal 4, track 5,
    flags 6, M 7), the record with ordinal q belonging to replay frame f0 + (q - q0); cells_M as in replay_fault_counts.
    float64 [8] = records in range, clean passed, clean rejected, contaminated passed, contaminated rejected, sum gamma and
    sum 2 M - 3 over the clean passed records without flag 4, unmatched (track index >= the cell's tracks)"""
    out = np.zeros(8)
    codes = {}
    for r in np.asarray(records, dtype=np.float64).reshape(-1, 8):
        q, trk, flags = int(r[4]), int(r[5]), int(r[6])
        if not q0 <= q < q1:
            continue
        out[0] += 1
        f = f0 + (q - q0)
        M = np.zeros(0, np.int64) if cells_M[f] is None else np.asarray(cells_M[f], dtype=np.int64)
        if trk >= len(M):
            out[7] += 1
            continue
        if f not in codes:
            codes[f] = replay_fault_code(M, replay_fault_draws(seed, f, int(M.sum())), fault4[0], fault4[1])
        o = int(M[:trk].sum())
        dirty = bool((codes[f][o:o + int(M[trk])] == FAULT_OUTLIER).any())
        ok = bool(flags & 1)
        out[1 + 2 * dirty + (not ok)] += 1
        if not dirty and ok and not flags & 4:
            out[5] += r[3]
            out[6] += 2.0 * r[7] - 3.0
    return out


# ---- calibration errors (csrc/replay_plan.h, CALIB; include/msckf_hip.h, msckf_hip_replay_set_imu_calib / _set_cam_calib): per
# trajectory an IMU record [31] = T_g, T_a, G (3 x 3 row-major each), sat_g, sat_a, lsb_g, lsb_a and a camera record
# (e_u, e_v, d_u, d_v, k1, k2, p1, p2), on top of either noise model, the faults and the timing.  Every operation below is one
# rounded double operation in the header's order: the device's noise-free bits are these.
REPLAY_EXTRINSIC_STREAM = (1 << 63) + 3
IMU_CAL, CAM_CAL = 31, 8


def imu_calib_identity():
    """the identity IMU record: T_g = T_a = I, everything else 0"""
    ic = np.zeros(IMU_CAL)
    ic[[0, 4, 8, 9, 13, 17]] = 1.0
    return ic


def replay_imu_calib_row(rd6, imucal):
    """c [k][6] of samples with the sequence values rd6 [k][6] (omega, a): c_a = T_a v_a, c_g = T_g v_g then + G v_a column by
    column -- the first product, then each further product added, every product and sum rounded"""
    v = np.asarray(rd6, dtype=np.float64).reshape(-1, 6)
    ic = np.asarray(imucal, dtype=np.float64)
    Tg, Ta, G = ic[0:9].reshape(3, 3), ic[9:18].reshape(3, 3), ic[18:27].reshape(3, 3)
    c = np.zeros_like(v)
    for r in range(3):
        a = Tg[r, 0] * v[:, 0]
        a = a + Tg[r, 1] * v[:, 1]
        a = a + Tg[r, 2] * v[:, 2]
        a = a + G[r, 0] * v[:, 3]
        a = a + G[r, 1] * v[:, 4]
        a = a + G[r, 2] * v[:, 5]
        c[:, r] = a
        a = Ta[r, 0] * v[:, 3]
        a = a + Ta[r, 1] * v[:, 4]
        a = a + Ta[r, 2] * v[:, 5]
        c[:, 3 + r] = a
    return c


def replay_imu_calib_out(x6, imucal):
    """saturation and quantisation of the values x6 [k][6] (noise included): (values, clipped [k][6] bool).  sat > 0:
    min(max(x, -sat), sat), clipped where x lay strictly outside [-sat, sat]; lsb > 0: lsb rint(x / lsb), rint to nearest even"""
    x = np.array(x6, dtype=np.float64).reshape(-1, 6)
    ic = np.asarray(imucal, dtype=np.float64)
    clipped = np.zeros(x.shape, dtype=bool)
    for cols, sat, lsb in ((slice(0, 3), ic[27], ic[29]), (slice(3, 6), ic[28], ic[30])):
        if sat > 0.0:
            clipped[:, cols] = (x[:, cols] < -sat) | (x[:, cols] > sat)
            x[:, cols] = np.minimum(np.maximum(x[:, cols], -sat), sat)
        if lsb > 0.0:
            x[:, cols] = lsb * np.rint(x[:, cols] / lsb)
    return x, clipped


def replay_cam_calib(obs, camcal):
    """the camera's residual map of the values obs [n][2] under camcal = (e_u, e_v, d_u, d_v, k1, k2, p1, p2), [n][2]"""
    ob = np.asarray(obs, dtype=np.float64).reshape(-1, 2)
    e_u, e_v, d_u, d_v, k1, k2, p1, p2 = (np.float64(t) for t in camcal)
    x, y = ob[:, 0], ob[:, 1]
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    rad = (1.0 + k1 * r2) + k2 * (r2 * r2)
    xd = (x * rad + (2.0 * p1) * xy) + p2 * (r2 + 2.0 * xx)
    yd = (y * rad + p1 * (r2 + 2.0 * yy)) + (2.0 * p2) * xy
    return np.stack([(xd + e_u * xd) + d_u, (yd + e_v * yd) + d_v], -1)


def replay_expand_calibrated(seq_traj, frame, seed, sigma4=None, model=None, imucal=None, camcal=None, timing4=None, fault4=None,
                             delta=None, table=None):
    """frame `frame` of the noise-free Trajectory seq_traj under the calibration records, composed with the timing shift (timing4,
    or the known deltas) before and the faults (fault4) after, as replay_expand_timed / replay_expand_faulted compose them.
    sigma4 for the white noise, or model = (L, scale, sigma_uv, w_start) for the Q_imu model.  dict of rd [K][7], rd_cal [K][6]
    (the noise-free c), clip [K] (6-bit masks), obs_cal [n][2] (mapped, noise-free, sequence order), Mp, slots, obs (partition
    order), code"""
    if (sigma4 is None) == (model is None):
        raise ValueError("one of sigma4 and model")
    fr = seq_traj.frames[frame]
    rd = np.array(seq_traj.imu_for_frame(frame), dtype=np.float64).reshape(-1, 7)
    ic = imu_calib_identity() if imucal is None else np.asarray(imucal, dtype=np.float64)
    cc = np.zeros(CAM_CAL) if camcal is None else np.asarray(camcal, dtype=np.float64)
    obs = np.asarray(fr["obs"], dtype=np.float64).reshape(-1, 2)
    if timing4 is not None or delta is not None:
        obs = _replay_timed_obs(seq_traj, frame, seed, timing4, delta, table)
    obs_cal = replay_cam_calib(obs, cc)
    cal = rd.copy()
    cal[:, :6] = replay_imu_calib_row(rd[:, :6], ic)
    if model is None:
        out, nobs = replay_cell(cal, obs_cal, frame, seed, sigma4)
    else:
        L, scale, sigma_uv, w_start = model
        if w_start is None:
            w_start = replay_walk(seq_traj, seed, L, scale)[frame]
        out, nobs = replay_model_cell(cal, obs_cal, frame, seed, L, scale, sigma_uv, w_start)[:2]
    out[:, :6], clipped = replay_imu_calib_out(out[:, :6], ic)
    clip = (clipped.astype(np.int32) << np.arange(6, dtype=np.int32)).sum(1).astype(np.int32)
    Mp, slots, fobs, code = _replay_faulted(frame, seed, fr["M"], fr["slots"], nobs, np.zeros(4) if fault4 is None else fault4)
    return dict(rd=out, rd_cal=cal[:, :6], clip=clip, obs_cal=obs_cal, Mp=Mp, slots=slots, obs=fobs, code=code)


def replay_calib_counts(seq_traj_or_cells, seed, imucal, f0, f1, sigma4=None, model=None):
    """msckf_hip_replay_calib_counts for one trajectory: int64 [8] = samples, gyro x y z clipped, accelerometer x y z clipped,
    samples with any component clipped, over the frames [f0, f1) of a noise-free Trajectory or a list of per-frame readings
    [k][7] (None: a skipped cell); sigma4 = (sigma_g, sigma_a, ., .) or model = (L, scale)"""
    cells = _replay_cells(seq_traj_or_cells)
    if (sigma4 is None) == (model is None):
        raise ValueError("one of sigma4 and model")
    ic = imu_calib_identity() if imucal is None else np.asarray(imucal, dtype=np.float64)
    W = None if model is None else replay_walk(cells, seed, model[0], model[1])
    out = np.zeros(8, dtype=np.int64)
    for f in range(int(f0), int(f1)):
        rd = cells[f]
        if not len(rd):
            continue
        cal = rd.copy()
        cal[:, :6] = replay_imu_calib_row(rd[:, :6], ic)
        if model is None:
            rows = replay_cell(cal, np.zeros((0, 2)), f, seed, sigma4)[0]
        else:
            rows = replay_model_cell(cal, np.zeros((0, 2)), f, seed, model[0], model[1], (0.0, 0.0), W[f])[0]
        clipped = replay_imu_calib_out(rows[:, :6], ic)[1]
        out[0] += len(rows)
        out[1:7] += clipped.sum(0)
        out[7] += int(clipped.any(1).sum())
    return out


def _small_matrix(scale, misalign):
    """diag(1 + scale) + the off-diagonal misalignment [6] = (xy, xz, yx, yz, zx, zy): row r picks up misalign * axis c"""
    T = np.diag(1.0 + np.broadcast_to(np.asarray(scale, dtype=np.float64), (3,)))
    m = np.broadcast_to(np.asarray(misalign, dtype=np.float64), (6,))
    T[0, 1], T[0, 2], T[1, 0], T[1, 2], T[2, 0], T[2, 1] = m
    return T


def imu_calib_record(scale_g=0.0, misalign_g=0.0, scale_a=0.0, misalign_a=0.0, g_sens=0.0, sat_g=0.0, sat_a=0.0, lsb_g=0.0, lsb_a=0.0):
    """an IMU record [31]: T = diag(1 + scale) + misalignment (scale a scalar or [3]; misalign a scalar or [6] = the off-diagonal
    entries xy, xz, yx, yz, zx, zy [rad]), G = g_sens (a scalar for every entry, or 3 x 3) [rad/s per m/s^2], saturation levels
    and quantisation steps (0: none)"""
    G = np.broadcast_to(np.asarray(g_sens, dtype=np.float64), (3, 3)) if np.ndim(g_sens) == 0 else np.asarray(g_sens, dtype=np.float64).reshape(3, 3)
    return np.concatenate([_small_matrix(scale_g, misalign_g).ravel(), _small_matrix(scale_a, misalign_a).ravel(), np.ravel(G),
                           [float(sat_g), float(sat_a), float(lsb_g), float(lsb_a)]])


def cam_calib_record(e_u=0.0, e_v=0.0, d_u=0.0, d_v=0.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0):
    """a camera record [8]: relative focal-length errors, principal-point errors over the focal length, residual radtan coefficients"""
    return np.array([e_u, e_v, d_u, d_v, k1, k2, p1, p2], dtype=np.float64)


def cam_calib_from_intrinsics(true, assumed):
    """the first-order record of a camera that IS `true` and is undistorted with `assumed`, each (f_u, f_v, c_u, c_v, k1, k2, p1,
    p2) of a pinhole-radtan model: e = f_true / f_assumed - 1, d = (c_true - c_assumed) / f_assumed, and the coefficient
    differences.  Exact to first order in the perturbation around an assumed calibration without distortion; around one with
    distortion delta the residual also has a cross term of the order perturbation x delta"""
    t, a = np.asarray(true, dtype=np.float64), np.asarray(assumed, dtype=np.float64)
    return np.array([t[0] / a[0] - 1.0, t[1] / a[1] - 1.0, (t[2] - a[2]) / a[0], (t[3] - a[3]) / a[1], t[4] - a[4], t[5] - a[5], t[6] - a[6], t[7] - a[7]])


def perturbed_cam12(cam12, seed, sigma_rot, sigma_trans):
    """a trajectory's own camera-IMU extrinsic error, for initialize (which takes the camera block per trajectory: no kernel is
    involved): cam12 = (c_u, c_v, f_u, f_v, b, q_CI [4], p_C_I [3]) with q_CI <- update_quat(sigma_rot n[0:3]) q_CI and
    p_C_I += sigma_trans n[3:6], n the pairs 0 .. 2 of the sub-seed mix(seed, 2^63 + 3) (2^63 .. 2^63 + 2 are taken by the
    initial error, the faults and the timing)"""
    out = np.array(cam12, dtype=np.float64)
    n = replay_pairs(int(replay_mix(seed, REPLAY_EXTRINSIC_STREAM)), 3).reshape(6)
    q = quat_mul(update_quat(float(sigma_rot) * n[0:3]), out[5:9])
    out[5:9] = q / np.linalg.norm(q)
    out[9:12] = out[9:12] + float(sigma_trans) * n[3:6]
    return out


def rot_to_quat(R):
    """Rotation matrix -> (w,x,y,z) such that Eigen's toRotationMatrix() gives R back."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    if q[0] < 0:
        q = -q
    return q / np.linalg.norm(q)


def quat_to_rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def camera_extrinsics():
    """(q_CI, p_C_I): C_CI rotates IMU-frame vectors into the camera frame; p_C_I = camera origin in IMU frame."""
    R = T_CAM_IMU[:3, :3]
    # re-orthonormalise the 12-digit Kalibr matrix
    U, _, Vt = np.linalg.svd(R)
    R = U @ Vt
    return rot_to_quat(R), -R.T @ T_CAM_IMU[:3, 3]


def filter_config(N, isotropic=True, feature_px=7.0, gn_px=7.0, Q_imu=None, P0=None):
    """Filter parameters: the effective EuRoC set of SURVEY.md section 5 with max_cam_states = N-1.
    Q_imu (12 x 12) / P0 (15 x 15): whole noiseParams::Q_imu / initial_imu_covar (types.h:90-91) in place of the diagonal
    ones; "Q_imu_diag" / "P0_diag" then hold their diagonals."""
    f_u, f_v, c_u, c_v = EUROC_INTRINSICS
    if isotropic:
        f_v = f_u
    q_CI, p_C_I = camera_extrinsics()
    w_var, dbg_var, a_var, dba_var = 1e-4, 3.6733e-5, 1e-2, 7e-2
    cfg = dict(
        c_u=c_u, c_v=c_v, f_u=f_u, f_v=f_v, b=0.0, q_CI=q_CI, p_C_I=p_C_I,
        u_var_prime=(feature_px / f_u) ** 2, v_var_prime=(feature_px / f_v) ** 2,
        Q_imu_diag=[w_var] * 3 + [dbg_var] * 3 + [a_var] * 3 + [dba_var] * 3,
        P0_diag=[1e-5] * 3 + [1e-2] * 3 + [1e-2] * 3 + [1e-2] * 3 + [1e-12] * 3,
        max_gn_cost_norm=(gn_px / f_u) ** 2, min_rcond=3e-12, translation_threshold=0.1,
        redundancy_angle_thresh=0.005, redundancy_distance_thresh=0.05,
        min_track_length=3, max_track_length=1000, max_cam_states=N - 1)
    if Q_imu is not None:
        cfg["Q_imu"] = np.array(Q_imu, dtype=np.float64).reshape(12, 12)
        cfg["Q_imu_diag"] = list(np.diag(cfg["Q_imu"]))
    if P0 is not None:
        cfg["P0"] = np.array(P0, dtype=np.float64).reshape(15, 15)
        cfg["P0_diag"] = list(np.diag(cfg["P0"]))
    return cfg


# ------------------------------------------------------------------ analytic trajectory
# path_id -> (radius [m], turn rate [rad/s], vertical amplitude [m], vertical rate [rad/s], roll/pitch wobble [rad], wobble rate)
# 0 is the SURVEY 8d path every config uses; 1..4 are the other "sequences" of the cfg4 Monte-Carlo stand-in
# (BASELINE.json configs[3] names EuRoC MH_01..MH_05, which are not on disk).
PATHS = [(3.0, 0.4, 0.5, 0.8, 0.10, 0.7), (4.0, 0.3, 0.8, 0.5, 0.08, 0.5), (2.5, 0.5, 0.3, 1.0, 0.12, 0.9),
         (3.5, 0.35, 0.6, 0.7, 0.05, 0.6), (5.0, 0.25, 1.0, 0.4, 0.10, 0.8)]


def _path(t, path_id=0):
    R, w, Az, wz, _, _ = PATHS[path_id]
    t = np.asarray(t, dtype=np.float64)
    p = np.stack([R * np.cos(w * t), R * np.sin(w * t), Az * np.sin(wz * t)], -1)
    v = np.stack([-R * w * np.sin(w * t), R * w * np.cos(w * t), Az * wz * np.cos(wz * t)], -1)
    a = np.stack([-R * w * w * np.cos(w * t), -R * w * w * np.sin(w * t), -Az * wz * wz * np.sin(wz * t)], -1)
    return p, v, a


def _attitude(t, path_id=0):
    """R_GI(t) [..,3,3] (IMU axes in world) and body angular rate omega(t)."""
    _, w0, _, _, wob, wr = PATHS[path_id]
    t = np.asarray(t, dtype=np.float64)
    th = w0 * t
    o = np.stack([np.cos(th), np.sin(th), np.zeros_like(th)], -1)       # outward  -> z_I (camera axis)
    up = np.broadcast_to(np.array([0.0, 0.0, 1.0]), o.shape)             # up       -> x_I
    tg = np.stack([-np.sin(th), np.cos(th), np.zeros_like(th)], -1)     # tangent  -> -y_I
    Rn = np.stack([up, -tg, o], -1)
    al, dal = wob * np.sin(wr * t), wob * wr * np.cos(wr * t)
    be, dbe = wob * np.sin(wr * t + 1.0), wob * wr * np.cos(wr * t + 1.0)
    ca, sa, cb, sb = np.cos(al), np.sin(al), np.cos(be), np.sin(be)
    z, one = np.zeros_like(t), np.ones_like(t)
    Rx = np.stack([np.stack([one, z, z], -1), np.stack([z, ca, -sa], -1), np.stack([z, sa, ca], -1)], -2)
    Ry = np.stack([np.stack([cb, z, sb], -1), np.stack([z, one, z], -1), np.stack([-sb, z, cb], -1)], -2)
    R = Rn @ Rx @ Ry
    w = w0 + dal
    omega = np.stack([cb * w, dbe, sb * w], -1)
    return R, omega


def ground_truth(t, path_id=0):
    """dict of p, v, q_IG (w,x,y,z), R_GI at times t."""
    p, v, a = _path(t, path_id)
    R, om = _attitude(t, path_id)
    R2 = R.reshape(-1, 3, 3)
    q = np.stack([rot_to_quat(Ri.T) for Ri in R2]).reshape(np.shape(t) + (4,))
    return dict(p=p, v=v, a=a, R_GI=R, omega=om, q_IG=q)


def imu29_from_gt(gt_at_t, b_g, b_a):
    """Pack the 29-double IMU state layout used across the C-ABIs: q_IG b_g v b_a p g q_null v_null p_null."""
    q, v, p = gt_at_t["q_IG"], gt_at_t["v"], gt_at_t["p"]
    return np.concatenate([q, b_g, v, b_a, p, GRAVITY, q, v, p])


def landmark_csr(trajs, f0, f1):
    """Ground-truth landmarks of the frames [f0, f1) of a batch, as Batch.map_log_metrics takes them: (gt_xyz [.][3], gt_off)
    with gt_off CSR over the cells (frame - f0) * B + b -- track t of trajectory b on frame k observes
    gt_xyz[gt_off[(k - f0) * B + b] + t] = trajs[b].landmarks[k][t]."""
    cells = [np.asarray(tr.landmarks[k], dtype=np.float64).reshape(-1, 3) for k in range(f0, f1) for tr in trajs]
    off = np.zeros(len(cells) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(c) for c in cells])
    xyz = np.concatenate(cells) if cells else np.zeros((0, 3))
    return np.ascontiguousarray(xyz), off


def camera_pose_gt(trajs, f0, f1):
    """Ground-truth camera poses of the frames [f0, f1) of a batch, as Batch.pruned_log_metrics takes them: [f1 - f0][B][7],
    q_CG (w, x, y, z) p_C_G of the camera that frame k's augmentState adds (trajs[b].C_CG[k], .p_C[k])."""
    out = np.zeros((max(f1 - f0, 0), len(trajs), 7))
    for k in range(f0, f1):
        for b, tr in enumerate(trajs):
            out[k - f0, b, 0:4], out[k - f0, b, 4:7] = rot_to_quat(tr.C_CG[k]), tr.p_C[k]
    return out


# ------------------------------------------------------------------ full-state NEES: the numpy twin of k_nees_log (csrc/kernels_log.hip)
def imu_state_gt(trajs, f0, f1):
    """The truth table of the frames [f0, f1) of a batch (or of a replay's sequences), as Batch.truth_set takes it:
    [f1 - f0][len(trajs)][16] = q_IG b_g v b_a p at the time of each frame's log record, from trajs[b].gt_frames and its constant
    biases (a replay adds its walk on the device: truth_set's add_walk)"""
    out = np.zeros((max(f1 - f0, 0), len(trajs), 16))
    for b, tr in enumerate(trajs):
        g = tr.gt_frames
        out[:, b, 0:4], out[:, b, 4:7], out[:, b, 7:10] = g["q_IG"][f0:f1], tr.b_g, g["v"][f0:f1]
        out[:, b, 10:13], out[:, b, 13:16] = tr.b_a, g["p"][f0:f1]
    return out


def quat_mul(a, b):
    """Hamilton product of (w, x, y, z) quaternions, Eigen's operator*"""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])


def update_quat(dtheta):
    """buildUpdateQuat (msckf.h:851-872): the unit quaternion (sqrt(1 - |dtheta / 2|^2), -dtheta / 2), normalised"""
    dq = 0.5 * np.asarray(dtheta, dtype=np.float64)
    cs = float(dq @ dq)
    q = np.concatenate([[1.0 if cs > 1.0 else np.sqrt(1.0 - cs)], -dq])
    return q / np.linalg.norm(q)


def error_angle(q, q_gt):
    """e_th with q = update_quat(e_th) * q_gt: -2 vec(q * q_gt^-1) / |q * q_gt^-1| with the sign of q that makes the scalar part
    non-negative, formed from the small difference s q - q_gt as the device forms it"""
    q, g = np.asarray(q, dtype=np.float64), np.asarray(q_gt, dtype=np.float64)
    s = -1.0 if q @ g < 0 else 1.0
    g_inv = np.concatenate([[g[0]], -g[1:]]) / (g @ g)
    u = quat_mul(s * q - g, g_inv)
    u[0] += 1.0
    return -2.0 * u[1:] / np.linalg.norm(u)


def nees_error(imu16, truth16):
    """e [15] = [e_th ; b_g - b_g* ; v - v* ; b_a - b_a* ; p - p*], the error state in P's own order"""
    x, g = np.asarray(imu16, dtype=np.float64), np.asarray(truth16, dtype=np.float64)
    return np.concatenate([error_angle(x[0:4], g[0:4]), x[4:16] - g[4:16]])


def _solve_sq(A, e):
    """|L^-1 e|^2 with A = L L^T by Cholesky, column by column; None when a pivot is not positive"""
    n = len(e)
    L, y = np.zeros((n, n)), np.zeros(n)
    for j in range(n):
        s = A[j, j] - L[j, :j] @ L[j, :j]
        if not s > 0.0:
            return None
        L[j, j] = np.sqrt(s)
        for r in range(j + 1, n):
            L[r, j] = (A[r, j] - L[r, :j] @ L[j, :j]) / L[j, j]
        y[j] = (e[j] - L[j, :j] @ y[:j]) / L[j, j]
    return float(y @ y)


def nees_record(imu16, P_II, truth16):
    """Columns 0..5 of a NEES log record and whether flag 1 is set, as k_nees_log forms them: the 15-state NEES through the
    correlation matrix C = D^-1/2 P_II D^-1/2 (D = diag P_II, C's diagonal exactly 1), NEES = |L^-1 D^-1/2 e|^2 with C = L L^T, then
    the NEES of the 3 x 3 diagonal blocks th, b_g, v, b_a, p through a Cholesky factorisation of each.  P_II's upper triangle
    is read.  A diagonal entry or a pivot that is not positive: (zeros, True)."""
    e = nees_error(imu16, truth16)
    U = np.triu(np.asarray(P_II, dtype=np.float64)[:15, :15])
    P = U + np.triu(U, 1).T
    d = np.diag(P)
    if not np.all(d > 0.0):
        return np.zeros(6), True
    s = 1.0 / np.sqrt(d)
    C = P * s[:, None] * s[None, :]
    np.fill_diagonal(C, 1.0)
    cols = [_solve_sq(C, e * s)] + [_solve_sq(P[o:o + 3, o:o + 3], e[o:o + 3]) for o in range(0, 15, 3)]
    if any(c is None for c in cols):
        return np.zeros(6), True
    return np.array(cols), False


def replay_initial_error(seed, P0):
    """e0 [15] ~ N(0, P0) of a trajectory's seed: z = the first 15 normals of replay_pairs(replay_mix(seed, 2^63), 8) (a sub-seed no
    frame index reaches: frames use mix(seed, 2 f) and mix(seed, 2 f + 1)), e0 = L0 z with L0 = chol_psd(P0), each row summed
    in ascending column order"""
    P0 = np.asarray(P0, dtype=np.float64)
    n = P0.shape[0]
    z = replay_pairs(int(replay_mix(seed, 2 ** 63)), (n + 1) // 2).reshape(-1)[:n]
    L0 = chol_psd(P0, "P0")
    e0 = np.zeros(n)
    for r in range(n):
        a = 0.0
        for c in range(r + 1):
            a = a + L0[r, c] * z[c]
        e0[r] = a
    return e0


def perturbed_imu29(imu29, e0):
    """imu29 moved by the error state e0 [15] (th b_g v b_a p): q <- update_quat(e_th) * q, the rest additive; the null-space
    anchors q_null, v_null, p_null are set to the perturbed values, as imu29_from_gt sets them to the state"""
    s, e0 = np.array(imu29, dtype=np.float64), np.asarray(e0, dtype=np.float64)
    s[0:4] = quat_mul(update_quat(e0[0:3]), s[0:4])
    s[4:16] = s[4:16] + e0[3:15]
    s[19:23], s[23:26], s[26:29] = s[0:4], s[7:10], s[13:16]
    return s


class Trajectory:
    """One seeded trajectory: IMU stream + per-frame ending-track work-lists."""

    def __init__(self, config_id, traj_idx, N, F, n_frames, cfg=None, t0=0.0, imu_noise_scale=0.05,
                 obs_noise_px=0.5, dense_tracks=False, first_timed_window_only=False, depth_range=(2.0, 10.0), path_id=0):
        self.N, self.F, self.n_frames = N, F, n_frames
        self.depth_range = depth_range   # landmark depth in the mid-track camera; (2, 10) m = SURVEY 8d, larger = low parallax
        self.t0 = t0
        self.cfg = cfg if cfg is not None else filter_config(N)
        self.seed = 0x5EED0000 + 1000 * config_id + traj_idx
        rng = SplitMix64(self.seed)
        self.dT = 1.0 / IMU_RATE
        self.b_g = np.full(3, 0.002)
        self.b_a = np.full(3, 0.02)
        # IMU sample i covers [t0 + i dT, t0 + (i+1) dT); frame k is taken after IMU samples [10(k-1)+... ]
        n_imu = n_frames * IMU_PER_FRAME
        ti = t0 + np.arange(n_imu) * self.dT
        self.path_id = path_id
        gt = ground_truth(ti + 0.5 * self.dT, path_id)            # mid-interval sampling
        q = self.cfg["Q_imu_diag"]
        sg = imu_noise_scale * np.sqrt(q[0] / self.dT)
        sa = imu_noise_scale * np.sqrt(q[6] / self.dT)
        C_IG = np.swapaxes(gt["R_GI"], -1, -2)
        a_body = np.einsum("nij,nj->ni", C_IG, gt["a"] - GRAVITY)
        if "Q_imu" in self.cfg:
            # correlated gyro / accelerometer white noise: the [omega, a] block of Q_imu (noise order n_g n_wg n_a n_wa)
            sel = [0, 1, 2, 6, 7, 8]
            L = np.linalg.cholesky(np.asarray(self.cfg["Q_imu"], dtype=np.float64)[np.ix_(sel, sel)])
            n6 = (imu_noise_scale / np.sqrt(self.dT)) * (rng.normal(6 * n_imu).reshape(n_imu, 6) @ L.T)
            om = gt["omega"] + self.b_g + n6[:, :3]
            ac = a_body + self.b_a + n6[:, 3:]
        else:
            om = gt["omega"] + self.b_g + sg * rng.normal(3 * n_imu).reshape(n_imu, 3)
            ac = a_body + self.b_a + sa * rng.normal(3 * n_imu).reshape(n_imu, 3)
        self.readings = np.concatenate([om, ac, np.full((n_imu, 1), self.dT)], 1)   # [n_imu, 7]
        # frame k happens at time t0 + (k+1)*10*dT, i.e. after IMU samples [10k, 10k+10)
        self.frame_times = t0 + (np.arange(n_frames) + 1) * IMU_PER_FRAME * self.dT
        self.gt_frames = ground_truth(self.frame_times, path_id)
        self.gt0 = ground_truth(np.array(t0), path_id)
        self.imu0 = imu29_from_gt(self.gt0, self.b_g, self.b_a)
        q_CI, p_C_I = self.cfg["q_CI"], self.cfg["p_C_I"]
        C_CI = quat_to_rot(q_CI)
        R_GI = self.gt_frames["R_GI"]
        self.C_CG = np.einsum("ij,nkj->nik", C_CI, R_GI)                 # C_CI * R_GI^T
        self.p_C = self.gt_frames["p"] + np.einsum("nij,j->ni", R_GI, p_C_I)
        sig_obs = obs_noise_px / self.cfg["f_u"]
        self.frames = []
        self.landmarks = []
        for k in range(n_frames):
            Nw = min(k + 1, N)
            if Nw < 4 or F == 0:
                self.frames.append(dict(Nw=Nw, M=np.zeros(0, np.int32), slots=np.zeros(0, np.int32), obs=np.zeros((0, 2))))
                self.landmarks.append(np.zeros((0, 3)))
                continue
            if dense_tracks:
                M = np.full(F, Nw - 1, dtype=np.int64)
                rng.u64(F)
            else:
                M = 3 + rng.integers(F, Nw - 3)
            pts = self._sample_landmarks(rng, k, M)
            Mmax = Nw - 1
            ar = np.arange(Mmax)[None, :]
            mask = ar < M[:, None]
            fr = np.clip(k - M[:, None] + ar, 0, k - 1)               # frames k-M .. k-1 (padded)
            pc = np.einsum("fmij,fmj->fmi", self.C_CG[fr], pts[:, None, :] - self.p_C[fr])
            z = pc[..., :2] / pc[..., 2:3] + sig_obs * rng.normal(2 * F * Mmax).reshape(F, Mmax, 2)
            sl = (Nw - 1 - M[:, None]) + ar
            self.frames.append(dict(Nw=Nw, M=M.astype(np.int32), slots=sl[mask].astype(np.int32), obs=z[mask]))
            self.landmarks.append(pts)

    def _sample_landmarks(self, rng, k, M):
        """One landmark per track, visible (90 deg FOV, in front) in frames k-M_j..k-1, depth_range (default 2-10 m) deep."""
        F = len(M)
        pts = np.zeros((F, 3))
        todo = np.arange(F)
        spread = 0.6
        for attempt in range(400):
            n = len(todo)
            u = rng.uniform(3 * n).reshape(n, 3)
            mid = k - 1 - (M[todo] // 2)
            ax, ay = spread * (2 * u[:, 0] - 1), spread * (2 * u[:, 1] - 1)
            d = self.depth_range[0] + (self.depth_range[1] - self.depth_range[0]) * u[:, 2]
            pc = np.stack([d * np.tan(ax), d * np.tan(ay), d], -1)
            pw = np.einsum("nji,nj->ni", self.C_CG[mid], pc) + self.p_C[mid]
            Mt = M[todo]
            ar = np.arange(int(Mt.max()))[None, :]
            mask = ar < Mt[:, None]
            fr = np.clip(k - Mt[:, None] + ar, 0, k - 1)
            q = np.einsum("fmij,fmj->fmi", self.C_CG[fr], pw[:, None, :] - self.p_C[fr])
            vis = (q[..., 2] > 0.5) & (np.abs(q[..., 0]) < q[..., 2]) & (np.abs(q[..., 1]) < q[..., 2])
            ok = np.all(vis | ~mask, axis=1)
            pts[todo[ok]] = pw[ok]
            todo = todo[~ok]
            if len(todo) == 0:
                break
            if attempt % 8 == 7:
                spread = max(0.7 * spread, 0.05)
            if attempt % 40 == 39:
                # the camera sweeps ~23 deg/s: a landmark cannot stay inside a 90 deg field of view for much
                # more than ~2 s, so over-long tracks (windows > 40 frames) are shortened (in place)
                M[todo] = np.maximum(3, (3 * M[todo]) // 4)
                spread = 0.6
        if len(todo):
            raise RuntimeError("landmark sampling failed")
        return pts

    # ---- views
    def imu_for_frame(self, k):
        return self.readings[k * IMU_PER_FRAME:(k + 1) * IMU_PER_FRAME]

    def stream(self):
        """Per-frame (cur_obs, cur_ids, new_obs, new_ids) as the front-end would hand them to
        MSCKF::update / addFeatures (asl_msckf.cpp:252-279).  Track t of frame k' gets id 10000*k' + t."""
        per_frame = [dict(cur=([], []), new=([], [])) for _ in range(self.n_frames)]
        for kp, fr in enumerate(self.frames):
            o = 0
            for t, M in enumerate(fr["M"]):
                fid = 10000 * kp + t
                for i in range(M):
                    k = kp - M + i
                    kind = "new" if i == 0 else "cur"
                    per_frame[k][kind][0].append(fr["obs"][o + i])
                    per_frame[k][kind][1].append(fid)
                o += M
        return per_frame
