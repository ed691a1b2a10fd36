"""IMU and camera calibration errors of the Monte-Carlo replay on the device (msckf_hip_replay_set_imu_calib, _set_cam_calib,
_expand_calib, _calib_counts; csrc/replay_plan.h CALIB, k_replay_expand_calib, k_replay_calib_counts).

  1. the calibrated expansion against the numpy twin on the common shape under the lab assignment (tests/replay_calib_lab.py),
     both noise models: rd_cal and obs_cal bit for bit in double, clip exact, the stored values by
     replay_faults_lab.check_scalars at the noise scales, clipped and quantised components bit for bit (double) or rounded once
     (float); everything the records do not touch is what the same handle expands without them
  2. composition with the lab's faults, with its timing, and with both, against the twin composed the same way
  3. edges: the lane groups (m_cap 16 | 17 | 32 | 33 | 63) with camera record, faults and timing together; K = 31 | 32 | 33 | 65
     under the Q_imu model with every IMU field set, k < K and k = K, a skipped cell and a cell with k = 0
  4. the loop reads what the kernel wrote: the bits of run_frames on the compact survivors of the read-backs
  5. replay_imu_sums in its stated order against the read-back rows, bit for bit; replay_calib_counts against the twin, the
     popcounts of the clip masks, and over split ranges
  6. trivial records (NULL, identity, zeros), alone and beside faults and timing: the bits of a handle that never heard of
     calibration
  7. refusals and the lifetime of the records

The margins that let 1, 2 and 5 demand exact masks, counts and quantised values are asserted on the twin in
tests/test_replay_calib_inputs.py."""
import numpy as np
import pytest

import helpers as H
import replay_calib_lab as CL
import replay_faults_lab as FLB
import replay_lab as RL
import replay_timing_lab as TL
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu
PRECS = ("f32", "f64")
MODELS = pytest.mark.parametrize("model", (False, True), ids=["sigma4", "q_imu"])


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c_
    c_.lib()
    return c_


def _cd(capi, prec):
    return capi.F64 if prec == "f64" else capi.F32


def _batch(capi, prec):
    bt = capi.Batch(RL.B, RL.N_CAP, RL.F_CAP, RL.M_CAP, _cd(capi, prec))
    for b, s in enumerate(RL.SEQ_OF):
        tr = RL.sequences()[s]
        bt.initialize(b, tr.cfg, tr.imu0)
    return bt


def _replay_batch(capi, prec, model=False, fault4=None, timing4=None, imucal=CL.IMUCAL, camcal=CL.CAMCAL):
    bt = _batch(capi, prec)
    CL.stage_replay(bt, imucal, camcal, fault4, timing4, model)
    return bt


def _read(bt, f, b):
    ex = bt.replay_expand(f, b)
    ex["code"] = bt.replay_expand_faults(f, b)
    ex["delta"] = bt.replay_expand_timing(f, b)
    ex.update(bt.replay_expand_calib(f, b))
    return ex


def _results(bt):
    bt.sync()
    return dict(snap=[H.snapshot(bt, b) for b in range(bt.B)], log=bt.frame_log_read()[0])


def _same(x, y):
    assert len(x["snap"]) == len(y["snap"])
    for b, (p, q) in enumerate(zip(x["snap"], y["snap"])):
        assert H.same_bits(p, q), b
    assert np.array_equal(x["log"], y["log"])


def _once(prec, x):
    """a double as the handle stores it: itself, or rounded once to float"""
    x = np.asarray(x, dtype=np.float64)
    return x if prec == "f64" else x.astype(np.float32).astype(np.float64)


def _bits(mask):
    return (np.asarray(mask)[:, None] >> np.arange(6)) & 1


def _check_imu(prec, ex, tw, ic, noise, where, worst):
    """rd_cal and clip exact; the stored values at the noise scale; clipped and quantised components exact"""
    assert np.array_equal(ex["rd_cal"], tw["rd_cal"]), (where, "rd_cal")
    assert np.array_equal(ex["clip"], tw["clip"]), (where, "clip")
    FLB.check_scalars(prec, ex["rd"][:, :6], tw["rd"][:, :6], noise, where, worst)
    exact = _bits(tw["clip"]).astype(bool)
    exact[:, :3] |= ic[29] > 0.0
    exact[:, 3:] |= ic[30] > 0.0
    assert np.array_equal(ex["rd"][:, :6][exact], _once(prec, tw["rd"][:, :6][exact])), (where, "clipped or quantised")
    assert np.array_equal(ex["rd"][:, 6], _once(prec, tw["rd"][:, 6])), (where, "dT")


# ------------------------------------------------------------------------------------------- 1. the expansion against the twin
@MODELS
@pytest.mark.parametrize("prec", PRECS)
def test_calibrated_expansion_against_the_twin(capi, prec, model):
    bt = _replay_batch(capi, prec, model)
    reads = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
    counts = bt.replay_calib_counts()
    bt.replay_set_imu_calib(None)
    bt.replay_set_cam_calib(None)
    plain = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
    bt.close()
    noise = CL.model_noise_scale() if model else CL.NOISE_SIGMA4
    worst, wo, moved_rd, moved_obs, clipped = [0.0], [0.0], 0, 0, np.zeros(RL.B, dtype=np.int64)
    for f in range(RL.NF):
        for b in range(RL.B):
            ex, pl = reads[f][b], plain[f][b]
            tw = CL.twin_cell(f, b, model)
            _check_imu(prec, ex, tw, CL.IMUCAL[b], noise, (f, b), worst)
            assert np.array_equal(ex["obs_cal"], tw["obs_cal"]), (f, b, "obs_cal")
            FLB.check_scalars(prec, ex["obs"], tw["obs"], np.array(RL.SIGMA[2:]), (f, b), wo)
            for key in ("M", "off", "slots", "n", "drop", "k", "code", "delta"):
                assert np.array_equal(ex[key], pl[key]), (f, b, key)
            assert np.array_equal(ex["rd"][:, 6], pl["rd"][:, 6]) and np.array_equal(ex["rd"][ex["k"]:], pl["rd"][ex["k"]:]), (f, b)
            assert not pl["clip"].any() and not ex["code"].any() and not ex["delta"].any()
            seq = RL.sequences()[RL.SEQ_OF[b]]
            assert np.array_equal(pl["rd_cal"], seq.imu_for_frame(f)[:, :6]) and np.array_equal(pl["obs_cal"], seq.frames[f]["obs"]), (f, b)
            if b == 0:                                               # the lab's first trajectory has identity records
                assert np.array_equal(ex["rd"], pl["rd"]) and np.array_equal(ex["obs"], pl["obs"]), f
            moved_rd += int((ex["rd"] != pl["rd"]).any(axis=1).sum())
            moved_obs += int((ex["obs"] != pl["obs"]).any(axis=1).sum()) if len(ex["obs"]) else 0
            clipped[b] += int((ex["clip"] != 0).sum())
    assert moved_rd > 500 and moved_obs > 300
    assert clipped[2] > 30 and clipped[4] > 20 and not clipped[[0, 1, 3]].any()
    assert np.array_equal(counts[:, 7], clipped)
    print("worst |device - twin| / noise (%s, %s): imu %.3g, obs %.3g" % (prec, "q_imu" if model else "sigma4", worst[0], wo[0]))


# ------------------------------------------------------------------------------------------------------- 2. composition
@pytest.mark.parametrize("combo", ("faults", "timing", "both"))
@MODELS
@pytest.mark.parametrize("prec", PRECS)
def test_calibration_composes_with_faults_and_timing(capi, prec, model, combo):
    """the calibration records with replay_faults_lab's faults, replay_timing_lab's timing, and both: the mapped noise-free
    coordinates bit for bit against the twin at the device's delta, the stored ones at sigma + rho; survivors, partition order
    and codes are the twin's; the IMU rows are those without faults and timing"""
    fault4 = FLB.FAULT4 if combo in ("faults", "both") else None
    timing4 = TL.TIMING4 if combo in ("timing", "both") else None
    bt = _replay_batch(capi, prec, model, fault4, timing4)
    reads = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
    bt.close()
    noise = CL.model_noise_scale() if model else CL.NOISE_SIGMA4
    worst, wo, faults, shifted = [0.0], [0.0], 0, 0
    for f in range(RL.NF):
        for b in range(RL.B):
            ex = reads[f][b]
            if timing4 is None:
                assert not ex["delta"].any()
            else:
                want = TL.delta_of(f, b)
                assert np.all(np.abs(ex["delta"] - want) <= 1e-13 * TL.TIMING4[b, 3]) if TL.TIMING4[b, 3] else np.array_equal(ex["delta"], want), (f, b)
                shifted += int((ex["delta"] != 0.0).sum())
            tw = CL.twin_cell(f, b, model, fault4=fault4, timing4=timing4, delta=None if timing4 is None else ex["delta"])
            _check_imu(prec, ex, tw, CL.IMUCAL[b], noise, (f, b), worst)
            assert np.array_equal(ex["obs_cal"], tw["obs_cal"]), (f, b, "obs_cal")
            rho = np.zeros(2) if fault4 is None else fault4[b, 2:]
            FLB.check_scalars(prec, ex["obs"], tw["obs"], np.array(RL.SIGMA[2:]) + rho, (f, b), wo)
            Mp = np.zeros(RL.F_CAP, np.int32)
            Mp[:len(tw["Mp"])] = tw["Mp"]
            assert np.array_equal(ex["M"], Mp) and np.array_equal(ex["slots"], tw["slots"]) and np.array_equal(ex["code"], tw["code"]), (f, b)
            faults += int((ex["code"] != 0).sum())
    assert (faults > 300) == (fault4 is not None) and (shifted > 800) == (timing4 is not None)
    print("worst |device - twin| / scale (%s, %s, %s): imu %.3g, obs %.3g" % (prec, "q_imu" if model else "sigma4", combo, worst[0], wo[0]))


# ---------------------------------------------------------------------------------------------------------- 3. the edges
def _edge_sequence(m_cap):
    """tests/test_gpu_replay_timing.py's edge sequence, restated: one sequence of m_cap small frames for a handle of
    n_cap = m_cap, f_cap = 9, K = 2: per frame (readings [k][7], M, slots, obs).  No drops, so frame f's window holds f + 1 images
    and the last frame's all m_cap.  Image times are uneven (k = 1 or 2 samples of 3 .. 30 ms).  Frames before the last carry one
    or two tracks of two or three observations on scattered slots; the last frame carries tracks of 1, 2, 3, G - 1, G and m_cap
    observations where m_cap allows, and three more that start mid-window"""
    rng = sc.SplitMix64(0x71AE + m_cap)
    G = 16 if m_cap <= 16 else 32 if m_cap <= 32 else 64
    edge = sorted(set(m for m in (1, 2, 3, G - 1, G, m_cap) if m <= m_cap))

    def pick(W, m, start=0):
        room = W - start
        step = max(1, min(3, room // m))
        return (start + step * np.arange(m)).astype(np.int32)

    cells = []
    for f in range(m_cap):
        W = f + 1
        k = 1 + int(rng.integers(1, 2)[0])
        rd = np.concatenate([rng.normal(6 * k).reshape(k, 6), 0.003 + 0.027 * rng.uniform(k).reshape(k, 1)], 1)
        if f < m_cap - 1:
            tracks = [pick(W, m, int(rng.integers(1, W - m + 1)[0])) for m in ((2, 3) if f % 2 else (3,)) if m <= W]
        else:
            tracks = [pick(W, m, (W - m) // 2 if m < 4 else 0) for m in edge]
            tracks += [pick(W, m, W // 2) for m in (2, 3, 4)][:9 - len(edge)]
        M = np.array([len(t) for t in tracks], dtype=np.int32)
        slots = np.concatenate(tracks) if tracks else np.zeros(0, np.int32)
        cells.append((rd, M, slots, 2.0 * rng.uniform(2 * len(slots)).reshape(-1, 2) - 1.0))
    return cells, edge, G


def _hand_cell(rd, M, slots, obs, f, seed, sigma4, imucal, camcal, fault4, K, model=None):
    """a hand-made noise-free cell under the records by the twin's public pieces (obs: already shifted where timing applies):
    dict of rd [K][7], rd_cal [K][6], clip [K], obs_cal, Mp, slots, obs (partition order), code"""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 7)
    k = len(rd)
    cal = rd.copy()
    cal[:, :6] = sc.replay_imu_calib_row(rd[:, :6], imucal)
    obs_cal = sc.replay_cam_calib(obs, camcal)
    if model is None:
        trd, tobs = sc.replay_cell(cal, obs_cal, f, seed, sigma4, K=K)
    else:
        L, scale, sigma_uv, w_start = model
        trd, tobs = sc.replay_model_cell(cal, obs_cal, f, seed, L, scale, sigma_uv, w_start, K=K)[:2]
    trd[:k, :6], clipped = sc.replay_imu_calib_out(trd[:k, :6], imucal)
    rd_cal, clip = np.zeros((K, 6)), np.zeros(K, dtype=np.int32)
    rd_cal[:k] = cal[:, :6]
    clip[:k] = (clipped.astype(np.int32) << np.arange(6, dtype=np.int32)).sum(1)
    draws = sc.replay_fault_draws(seed, f, len(tobs))
    code = sc.replay_fault_code(M, draws, fault4[0], fault4[1])
    Mp, ps, po_ = sc.replay_fault_cell(M, slots, tobs, code, draws[2], fault4[2], fault4[3])
    return dict(rd=trd, rd_cal=rd_cal, clip=clip, obs_cal=obs_cal, Mp=Mp, slots=ps, obs=po_, code=code)


@pytest.mark.parametrize("m_cap", (16, 17, 32, 33, 63))
@pytest.mark.parametrize("prec", PRECS)
def test_calibrated_expansion_at_the_group_edges(capi, prec, m_cap):
    """G = 16 | 32 | 64 on both sides of each switch and the full wavefront, tracks of 1, 2, 3, G - 1, G and m_cap observations.
    Three trajectories on the one sequence: a camera record alone without pixel noise (the stored coordinates are the mapped
    ones, rounded once), camera record + faults + timing + noise, and everything at the seed 2^64 - 1 with an IMU record"""
    cells, edge, G = _edge_sequence(m_cap)
    assert edge[-1] == m_cap and {1, 2, 3} <= set(edge) and (G - 1 in edge or G - 1 > m_cap) and (G in edge or G > m_cap)
    seeds = [31, 32, 0xFFFFFFFFFFFFFFFF]
    sigma = np.array([[0.01, 0.1, 0.0, 0.0], [0.01, 0.1, 2e-3, 1e-3], [0.01, 0.1, 1e-3, 1e-3]])
    fault4 = np.array([[0.0, 0.0, 0.0, 0.0], [0.4, 0.4, 0.02, 0.01], [0.3, 0.2, 0.01, 0.02]])
    timing4 = np.array([[0.0, 0.0, 0.0, 0.0], [-6e-3, 0.03, 0.05, 2e-3], [4e-3, 0.02, -0.1, 0.0]])
    camcal = np.stack([CL.CAMCAL[4], CL.CAMCAL[4], CL.CAMCAL[3]])
    imucal = np.stack([sc.imu_calib_identity(), sc.imu_calib_identity(), sc.imu_calib_record(scale_g=2e-3, misalign_a=1e-3, g_sens=1e-4, sat_g=1.0, sat_a=1.5, lsb_g=1e-3, lsb_a=1e-2)])
    bt = capi.Batch(3, m_cap, 9, m_cap, _cd(capi, prec))
    bt.replay_alloc(1, m_cap, 2)
    for f, (rd, M, slots, obs) in enumerate(cells):
        bt.replay_set_cell(f, 0, rd, M, slots, obs, 0)
    bt.replay_assign([0, 0, 0], seeds, sigma)
    bt.replay_set_faults(fault4)
    bt.replay_set_timing(timing4)
    bt.replay_set_imu_calib(imucal)
    bt.replay_set_cam_calib(camcal)
    bt.replay_commit()
    time, frame_of, base = sc.replay_image_table([(c[0], 0) for c in cells])
    worst, wi, mapped, clipped = [0.0], [0.0], 0, 0
    for f in (5, m_cap // 2, m_cap - 1):
        rd, M, slots, obs = cells[f]
        start = 0
        for b in range(3):
            ex = _read(bt, f, b)
            want = sc.replay_timing_delta(obs[:, 1], frame_of[base[f] + slots], seeds[b], timing4[b])
            assert np.all(np.abs(ex["delta"] - want) <= 1e-13 * max(timing4[b, 3], 1e-300)) if timing4[b, 3] else np.array_equal(ex["delta"], want), (m_cap, f, b)
            moved = sc.replay_timing_shift(M, slots, obs, time, base[f], ex["delta"])
            tw = _hand_cell(rd, M, slots, moved, f, seeds[b], sigma[b], imucal[b], camcal[b], fault4[b], 2)
            Ms = np.zeros(9, np.int32)
            Ms[:len(M)] = M
            Mp = np.zeros(9, np.int32)
            Mp[:len(M)] = tw["Mp"]
            assert (ex["n"], ex["drop"], ex["k"]) == (len(M), 0, len(rd)), (m_cap, f, b)
            assert np.array_equal(ex["off"], start + np.concatenate([[0], np.cumsum(Ms)[:-1]])), (m_cap, f, b)
            assert np.array_equal(ex["M"], Mp) and np.array_equal(ex["slots"], tw["slots"]) and np.array_equal(ex["code"], tw["code"]), (m_cap, f, b)
            assert np.array_equal(ex["obs_cal"], tw["obs_cal"]), (m_cap, f, b)
            assert np.array_equal(ex["rd_cal"], tw["rd_cal"]) and np.array_equal(ex["clip"], tw["clip"]), (m_cap, f, b)
            FLB.check_scalars(prec, ex["rd"][:, :6], tw["rd"][:, :6], np.array([0.01] * 3 + [0.1] * 3), (m_cap, f, b), wi)
            if b == 0:
                assert np.array_equal(ex["obs"], _once(prec, tw["obs_cal"])), (m_cap, f, b)
                mapped += int((ex["obs"] != _once(prec, obs)).any(axis=1).sum())
            else:
                FLB.check_scalars(prec, ex["obs"], tw["obs"], sigma[b, 2:] + fault4[b, 2:], (m_cap, f, b), worst)
            clipped += int((ex["clip"] != 0).sum())
            start += len(slots)
    bt.close()
    assert mapped > m_cap and clipped > 0
    print("worst |device - twin| / scale (%s, m_cap %d, G %d): obs %.3g, imu %.3g" % (prec, m_cap, G, worst[0], wi[0]))


@pytest.mark.parametrize("K", (31, 32, 33, 65))
@pytest.mark.parametrize("prec", PRECS)
def test_model_tile_boundary_with_every_imu_field(capi, prec, K):
    """the Q_imu model's tiles of 32 samples on both sides of the boundary and beyond two tiles, every IMU field set: cells of
    k = K, k = K - 3, a skipped cell and a cell with k = 0, two trajectories with different records on one sequence"""
    rng = sc.SplitMix64(0xCA11B + K)
    ks = [K, K - 3, None, 0, K]
    cells = [None if k is None else np.concatenate([rng.normal(6 * k).reshape(k, 6) * np.array([0.5] * 3 + [4.0] * 3), np.full((k, 1), 0.005)], 1) for k in ks]
    seeds = [0xABCDEF01, 0xABCDEF02]
    imucal = np.stack([CL.IMUCAL[4].copy(), CL.IMUCAL[1].copy()])
    imucal[0, 27:] = (0.6, 5.0, CL.LSB_G, CL.LSB_A)
    imucal[1, 27:] = (0.0, 3.0, 1e-3, 0.0)
    Q, scale, sigma_uv = FLB.model_of(0)
    L = sc.replay_noise_factor(Q)
    bt = capi.Batch(2, 6, 4, 6, _cd(capi, prec))
    bt.replay_alloc(1, len(ks), K)
    none = np.zeros((0, 2))
    for f, rd in enumerate(cells):
        bt.replay_set_cell(f, 0, np.zeros((0, 7)) if rd is None else rd, [], [], none, 0, skip=rd is None)
    bt.replay_assign_q([0, 0], seeds, Q, scale, sigma_uv)
    bt.replay_set_imu_calib(imucal)
    bt.replay_commit()
    noise = CL.model_noise_scale()
    worst, clipped = [0.0], 0
    want_counts = np.stack([sc.replay_calib_counts(cells, seeds[b], imucal[b], 0, len(ks), model=(L, scale)) for b in range(2)])
    assert np.array_equal(bt.replay_calib_counts(), want_counts)
    rows = [[None] * len(ks) for _ in range(2)]
    for b in range(2):
        walk = sc.replay_walk(cells, seeds[b], L, scale)
        for f, rd in enumerate(cells):
            ex = _read(bt, f, b)
            assert ex["k"] == (-1 if rd is None else len(rd)) and ex["n"] == 0, (K, f, b)
            tw = _hand_cell(np.zeros((0, 7)) if rd is None else rd, [], [], none, f, seeds[b], None, imucal[b], np.zeros(8), np.zeros(4), K, model=(L, scale, sigma_uv, walk[f]))
            assert np.array_equal(ex["rd_cal"], tw["rd_cal"]) and np.array_equal(ex["clip"], tw["clip"]), (K, f, b)
            _check_imu(prec, ex, tw, imucal[b], noise, (K, f, b), worst)
            k = max(ex["k"], 0)
            assert not ex["rd"][k:].any() and not ex["clip"][k:].any()
            clipped += int((ex["clip"] != 0).sum())
            rows[b][f] = ex["rd"][:k]
    sums = bt.replay_imu_sums()
    bt.close()
    assert clipped == int(want_counts[:, 7].sum()) and clipped > K
    for b in range(2):
        assert np.array_equal(sums[b], _sums_in_order(rows[b], 0, len(ks))), (K, b)
    print("worst |device - twin| / noise (%s, K %d): %.3g" % (prec, K, worst[0]))


# --------------------------------------------------------------------------- 4. the loop reads what the kernel wrote, bit for bit
_READ, _ORD = {}, {}


def _readbacks(capi, prec):
    """every (frame, trajectory) under the lab's calibration, timing and fault assignments: once per dtype, never written to"""
    if prec not in _READ:
        bt = _replay_batch(capi, prec, False, FLB.FAULT4, TL.TIMING4)
        _READ[prec] = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
        bt.close()
    return _READ[prec]


def _ordinary(capi, prec):
    """run_frames(0, 16) on a second handle whose ordinary scenario holds the survivors of the read-backs, compact"""
    if prec not in _ORD:
        bt = _batch(capi, prec)
        bt.scenario_alloc(RL.NF, sc.IMU_PER_FRAME)
        for f, row in enumerate(_readbacks(capi, prec)):
            for b, ex in enumerate(row):
                M_seq = RL.sequences()[RL.SEQ_OF[b]].frames[f]["M"]
                Mp, slots, obs = FLB.survivors(dict(M=M_seq, Mp=ex["M"][:ex["n"]], slots=ex["slots"], obs=ex["obs"]))
                bt.scenario_set(f, b, ex["rd"][:ex["k"]], Mp, slots, obs, ex["drop"])
        bt.scenario_commit()
        bt.set_streams(1)
        bt.frame_log_enable(RL.NF)
        bt.run_frames(0, RL.NF)
        _ORD[prec] = _results(bt)
        bt.close()
    return _ORD[prec]


@pytest.mark.parametrize("slices", (1, 2, 4))
@pytest.mark.parametrize("cuts", ([(0, 16)], [(0, 5), (5, 16)]), ids=["one_call", "two_calls"])
@pytest.mark.parametrize("prec", PRECS)
def test_calibrated_replay_runs_the_bits_of_the_ordinary_run_on_the_readbacks(capi, prec, cuts, slices):
    want = _ordinary(capi, prec)
    bt = _replay_batch(capi, prec, False, FLB.FAULT4, TL.TIMING4)
    bt.set_streams(slices)
    bt.set_slices_exact(slices > 1)
    assert 1 <= bt.effective_streams() <= slices
    bt.frame_log_enable(RL.NF)
    for f0, f1 in cuts:
        bt.run_frames_replay(f0, f1)
    got = _results(bt)
    bt.close()
    assert got["log"].shape == (RL.NF, RL.B, 48) and min(s[4]["n_passed"] for s in got["snap"]) > 0
    _same(got, want)


# ------------------------------------------------------------------------------------------------- 5. sums and counts
def _sums_in_order(rows, f0, f1):
    """msckf_hip_replay_imu_sums' row from the read-back rows rows[f] ([k][7], as the handle stores them) in its stated order:
    lane l adds the frames f0 + l, f0 + l + 64, ... ascending and a frame's samples ascending onto its own eight doubles; the 64
    partial sums are combined by the balanced binary tree over the lanes"""
    lanes = np.zeros((64, 8))
    for f in range(f0, f1):
        for r in rows[f]:
            lanes[(f - f0) % 64, 0] += 1.0
            lanes[(f - f0) % 64, 1:] += r
    while len(lanes) > 1:
        lanes = lanes[0::2] + lanes[1::2]
    return lanes[0]


@MODELS
@pytest.mark.parametrize("prec", PRECS)
def test_sums_and_counts_under_the_records(capi, prec, model):
    bt = _replay_batch(capi, prec, model)
    reads = [[_read(bt, f, b) for f in range(RL.NF)] for b in range(RL.B)]
    ranges = ((0, RL.NF), (0, 7), (7, RL.NF), (3, 4), (5, 5))
    sums = {r: bt.replay_imu_sums(*r) for r in ranges}
    counts = {r: bt.replay_calib_counts(*r) for r in ranges}
    bt.replay_set_imu_calib(None)
    plain_sums, plain_counts = bt.replay_imu_sums(), bt.replay_calib_counts()
    bt.close()
    for b in range(RL.B):
        rows = [reads[b][f]["rd"][:reads[b][f]["k"]] for f in range(RL.NF)]
        for r in ranges:
            assert np.array_equal(sums[r][b], _sums_in_order(rows, *r)), (b, r)
            pop = np.zeros(8, dtype=np.int64)
            for f in range(*r):
                m = reads[b][f]["clip"][:reads[b][f]["k"]]
                pop += np.concatenate([[len(m)], _bits(m).sum(0), [int((m != 0).sum())]])
            assert np.array_equal(counts[r][b], pop), (b, r)
    for r in ranges:
        assert np.array_equal(counts[r], CL.counts(model, *r)), r
    assert np.array_equal(counts[(0, 7)] + counts[(7, RL.NF)], counts[(0, RL.NF)]) and not counts[(5, 5)].any()
    assert counts[(0, RL.NF)][2, 7] > 30 and counts[(0, RL.NF)][4, 7] > 20
    assert np.array_equal(plain_counts[:, 0], counts[(0, RL.NF)][:, 0]) and not plain_counts[:, 1:].any()
    assert np.array_equal(plain_sums[0], sums[(0, RL.NF)][0]) and not np.array_equal(plain_sums[1:, 1:7], sums[(0, RL.NF)][1:, 1:7])


# ------------------------------------------------------------------------------------------------- 6. trivial records
def _run(bt):
    bt.frame_log_enable(RL.NF)
    bt.run_frames_replay(0, RL.NF)
    return _results(bt)


_PLAIN = {}


def _plain(capi, prec, beside):
    """a handle that never heard of calibration, at the lab's seeds, alone or beside the lab's faults and timing"""
    if (prec, beside) not in _PLAIN:
        bt = _batch(capi, prec)
        RL.stage_replay(bt, RL.SEQ_OF, CL.SEEDS, RL.SIGMA)
        if beside:
            bt.replay_set_faults(FLB.FAULT4)
            bt.replay_set_timing(TL.TIMING4)
        cells = [[dict(bt.replay_expand(f, b), code=bt.replay_expand_faults(f, b), delta=bt.replay_expand_timing(f, b)) for b in range(RL.B)] for f in (4, 9)]
        _PLAIN[(prec, beside)] = (_run(bt), cells)
        bt.close()
    return _PLAIN[(prec, beside)]


@pytest.mark.parametrize("beside", (False, True), ids=["alone", "beside_faults_and_timing"])
@pytest.mark.parametrize("setting", ("null", "identity", "zeros"))
@pytest.mark.parametrize("prec", PRECS)
def test_trivial_records_are_the_handle_without_calibration(capi, prec, setting, beside):
    want, cells = _plain(capi, prec, beside)
    ic, cc = dict(null=(None, None), identity=(np.tile(sc.imu_calib_identity(), (RL.B, 1)), None), zeros=(None, np.zeros((RL.B, 8))))[setting]
    bt = _replay_batch(capi, prec, False, FLB.FAULT4 if beside else None, TL.TIMING4 if beside else None)
    bt.replay_set_imu_calib(ic)                                    # after non-trivial records: they must be gone
    bt.replay_set_cam_calib(cc)
    for i, f in enumerate((4, 9)):
        for b in range(RL.B):
            ex = _read(bt, f, b)
            assert not ex["clip"].any()
            for key in ("rd", "obs", "M", "off", "slots", "code", "delta"):
                assert np.array_equal(ex[key], cells[i][b][key]), (f, b, key)
    _same(_run(bt), want)
    bt.close()


# ------------------------------------------------------------------------------------------------- 7. refusals and lifetime
@pytest.mark.parametrize("prec", PRECS)
def test_refusals_leave_the_records_and_the_records_outlive_assignments(capi, prec):
    EINVAL = r"\(-22\)"
    bt = _batch(capi, prec)
    for rec in (CL.IMUCAL, None):
        with pytest.raises(capi.HipError, match=EINVAL + ".*no replay allocated"):
            bt.replay_set_imu_calib(rec)
    for rec in (CL.CAMCAL, None):
        with pytest.raises(capi.HipError, match=EINVAL + ".*no replay allocated"):
            bt.replay_set_cam_calib(rec)
    CL.stage_replay(bt)
    first = [_read(bt, 9, b) for b in range(RL.B)]
    assert first[4]["clip"].any() and not first[0]["clip"].any()
    for bad in (float("inf"), float("nan")):
        for col in (0, 13, 20, 27, 30):
            g = CL.IMUCAL.copy()
            g[4, col] = bad
            with pytest.raises(capi.HipError, match=EINVAL + ".*calibration values must be finite"):
                bt.replay_set_imu_calib(g)
        for col in range(8):
            g = CL.CAMCAL.copy()
            g[3, col] = bad
            with pytest.raises(capi.HipError, match=EINVAL + ".*calibration values must be finite"):
                bt.replay_set_cam_calib(g)
    for col in (27, 28, 29, 30):
        g = CL.IMUCAL.copy()
        g[1, col] = -1e-9
        with pytest.raises(capi.HipError, match=EINVAL + ".*saturation and quantisation must not be negative"):
            bt.replay_set_imu_calib(g)
    g[4, 3] = float("nan")                                         # the order: finite first
    with pytest.raises(capi.HipError, match=EINVAL + ".*calibration values must be finite"):
        bt.replay_set_imu_calib(g)
    with pytest.raises(capi.HipError, match=r"\(-7\).*output buffer too small"):
        d = np.zeros((bt.f_cap * bt.m_cap, 2))
        capi._chk(bt.L.msckf_hip_replay_expand_calib(bt.h, 9, 0, None, None, d.ctypes.data_as(capi._dp), 1))
    for r0, r1 in ((3, 2), (0, RL.NF + 1), (-1, 2)):
        with pytest.raises(capi.HipError, match=EINVAL + ".*frame range out of bounds"):
            bt.replay_calib_counts(r0, r1)
    assert capi._chk(bt.L.msckf_hip_replay_expand_calib(bt.h, 9, 1, None, None, None, bt.f_cap * bt.m_cap)) == len(first[1]["obs"])   # any pointer may be NULL

    def same_as_first():
        for b in range(RL.B):
            ex = _read(bt, 9, b)
            for key in ("rd_cal", "clip", "obs_cal", "obs", "rd", "M", "slots"):
                assert np.array_equal(ex[key], first[b][key]), (b, key)

    same_as_first()                                               # the refused calls left the records in force
    # the records survive assign_q followed by assign, fault and timing records that come and go, and a commit
    Q, scale, sigma_uv = FLB.model_of(0)
    bt.replay_assign_q(RL.SEQ_OF, CL.SEEDS, Q, scale, sigma_uv)
    ex = _read(bt, 9, 4)
    assert np.array_equal(ex["rd_cal"], first[4]["rd_cal"]) and np.array_equal(ex["obs_cal"], first[4]["obs_cal"]) and not np.array_equal(ex["rd"], first[4]["rd"])
    bt.replay_assign(RL.SEQ_OF, CL.SEEDS, RL.SIGMA)
    bt.replay_set_faults(FLB.FAULT4)
    bt.replay_set_timing(TL.TIMING4)
    ex = _read(bt, 9, 4)
    assert np.array_equal(ex["rd_cal"], first[4]["rd_cal"]) and np.array_equal(ex["clip"], first[4]["clip"]) and ex["code"].any() and ex["delta"].any()
    bt.replay_set_faults(None)
    bt.replay_set_timing(None)
    bt.replay_commit()
    same_as_first()
    # other records between two runs take effect, one record goes while the other stays, and replay_alloc clears both
    bt.replay_set_imu_calib(CL.IMUCAL[4])
    bt.replay_set_cam_calib(CL.CAMCAL[4])
    ex = _read(bt, 9, 0)
    assert ex["clip"].any() and not np.array_equal(ex["obs_cal"], first[0]["obs_cal"])
    bt.replay_set_imu_calib(None)
    ex = _read(bt, 9, 0)
    assert not ex["clip"].any() and np.array_equal(ex["rd_cal"], first[0]["rd_cal"]) and not np.array_equal(ex["obs_cal"], first[0]["obs_cal"])
    RL.stage_replay(bt, RL.SEQ_OF, CL.SEEDS, RL.SIGMA)
    for b in range(RL.B):
        ex = _read(bt, 9, b)
        seq = RL.sequences()[RL.SEQ_OF[b]]
        assert not ex["clip"].any() and np.array_equal(ex["rd_cal"], seq.imu_for_frame(9)[:, :6]) and np.array_equal(ex["obs_cal"], seq.frames[9]["obs"])
    bt.close()
