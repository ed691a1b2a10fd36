"""Camera time offset, timestamp jitter and rolling shutter of the Monte-Carlo replay on the device (msckf_hip_replay_set_timing,
msckf_hip_replay_image_table, msckf_hip_replay_expand_timing; csrc/replay_plan.h TIMING, k_replay_expand_timed).

  1. the timed expansion against the numpy twin on the common shape under the lab assignment (tests/replay_timing_lab.py), both
     noise models: delta to 1e-13 sigma_j (one draw) and bit for bit where sigma_j = 0; without pixel noise the coordinates are the
     twin's at the device's delta, bit for bit in double and rounded once in float; with pixel noise and faults they meet
     replay_faults_lab.check_scalars at sigma + rho; slots, M, off, codes and IMU rows are the un-timed expansion's
  2. the lane groups' edges: handles of m_cap 16 | 17 | 32 | 33 | 63 on sequences of m_cap small frames with uneven image times, a
     last frame with tracks of 1, 2, 3, G - 1, G and m_cap observations and tracks that start mid-window; expansions only
  3. the loop reads what the kernel wrote: the bits of run_frames on the compact survivors of the read-backs
  4. zero records (zeros, NULL, y_0 alone): the bits of a handle that never heard of timing
  5. refusals, the preconditions at commit, and the lifetime of the record"""
import numpy as np
import pytest

import helpers as H
import replay_faults_lab as FLB
import replay_lab as RL
import replay_timing_lab as TL
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu
PRECS = ("f32", "f64")
NO_PIXEL_NOISE = RL.SIGMA[:2] + (0.0, 0.0)


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


def _replay_batch(capi, prec, timing4=TL.TIMING4, fault4=None, model=False, sigma=RL.SIGMA):
    bt = _batch(capi, prec)
    TL.stage_replay(bt, timing4, fault4, FLB.SEEDS, model, sigma)
    return bt


def _read(bt, f, b):
    ex = bt.replay_expand(f, b)
    ex["code"] = bt.replay_expand_faults(f, b)
    ex["delta"] = bt.replay_expand_timing(f, b)
    return ex


def _results(bt):
    bt.sync()
    return dict(snap=[H.snapshot(bt, b) for b in range(bt.B)], log=bt.frame_log_read()[0])


def _same(x, y):
    assert len(x["snap"]) == len(y["snap"])
    for b, (p, q) in enumerate(zip(x["snap"], y["snap"])):
        assert H.same_bits(p, q), b
    assert np.array_equal(x["log"], y["log"])


def _check_delta(dev, twin, sigma_j, where, worst):
    """the project's rule for one draw: 1e-13 sigma_j in double (delta is a double on either handle); no draw: equal bits"""
    assert dev.shape == twin.shape, where
    if sigma_j == 0.0:
        assert np.array_equal(dev, twin), where
    elif dev.size:
        worst[0] = max(worst[0], float(np.abs(dev - twin).max() / sigma_j))
        assert np.all(np.abs(dev - twin) <= 1e-13 * sigma_j), (where, worst[0])


def _same_bits_or_rounded_once(prec, dev, twin, where):
    if prec == "f64":
        assert np.array_equal(dev, twin), (where, float(np.abs(dev - twin).max()) if dev.size else 0.0)
    else:
        assert np.array_equal(dev, twin.astype(np.float32).astype(np.float64)), where


# ------------------------------------------------------------------------------------------- 1. the expansion against the twin
@pytest.mark.parametrize("model", (False, True), ids=["sigma4", "q_imu"])
@pytest.mark.parametrize("prec", PRECS)
def test_timed_expansion_without_pixel_noise_is_the_twin_at_the_devices_delta(capi, prec, model):
    """every (frame, trajectory) under the lab assignment with sigma_u = sigma_v = 0 and no faults: the deltas, then the
    coordinates bit for bit (double) or rounded once (float) against the twin evaluated at the device's delta; everything else
    is what the same handle expands without the record"""
    bt = _replay_batch(capi, prec, model=model, sigma=NO_PIXEL_NOISE)
    reads = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
    bt.replay_set_timing(None)
    plain = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
    bt.close()
    worst, moved = [0.0], 0
    for f in range(RL.NF):
        for b in range(RL.B):
            ex, pl = reads[f][b], plain[f][b]
            _check_delta(ex["delta"], TL.delta_of(f, b), TL.TIMING4[b, 3], (f, b), worst)
            assert not pl["delta"].any() and not ex["code"].any()
            tw = TL.twin_cell(f, b, delta=ex["delta"], sigma=NO_PIXEL_NOISE)
            _same_bits_or_rounded_once(prec, ex["obs"], tw["obs"], (f, b))
            for key in ("rd", "M", "off", "slots", "code", "n", "drop", "k"):
                assert np.array_equal(ex[key], pl[key]), (f, b, key)
            moved += int((ex["obs"] != pl["obs"]).any(axis=1).sum()) if len(ex["obs"]) else 0
            if b == 0:
                assert np.array_equal(ex["obs"], pl["obs"])              # the lab's first trajectory has no record
    assert moved > 800
    print("worst |delta - twin| / sigma_j (%s, %s): %.3g" % (prec, "q_imu" if model else "sigma4", worst[0]))


@pytest.mark.parametrize("model", (False, True), ids=["sigma4", "q_imu"])
@pytest.mark.parametrize("prec", PRECS)
def test_timed_expansion_with_pixel_noise_and_faults_against_the_twin(capi, prec, model):
    """the lab's timing and fault assignments together: coordinates by replay_faults_lab.check_scalars at sigma + rho against the
    twin at the device's delta; survivors, partition order, codes and IMU rows are those of the faulted expansion without timing"""
    bt = _replay_batch(capi, prec, fault4=FLB.FAULT4, model=model)
    reads = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
    bt.replay_set_timing(None)
    plain = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
    bt.close()
    worst, wd, faults = [0.0], [0.0], 0
    for f in range(RL.NF):
        for b in range(RL.B):
            ex, pl = reads[f][b], plain[f][b]
            _check_delta(ex["delta"], TL.delta_of(f, b), TL.TIMING4[b, 3], (f, b), wd)
            tw = TL.twin_cell(f, b, delta=ex["delta"], fault4=FLB.FAULT4)
            FLB.check_scalars(prec, ex["obs"], tw["obs"], np.array(RL.SIGMA[2:]) + FLB.FAULT4[b, 2:], (f, b), worst)
            Mp = np.zeros(RL.F_CAP, np.int32)
            Mp[:len(tw["Mp"])] = tw["Mp"]
            assert np.array_equal(ex["M"], Mp) and np.array_equal(ex["slots"], tw["slots"]) and np.array_equal(ex["code"], tw["code"]), (f, b)
            for key in ("rd", "M", "off", "slots", "code", "n", "drop", "k"):
                assert np.array_equal(ex[key], pl[key]), (f, b, key)
            faults += int((ex["code"] != 0).sum())
    assert faults > 300
    print("worst |device - twin| / (sigma + rho) (%s, %s): %.3g; delta / sigma_j: %.3g" % (prec, "q_imu" if model else "sigma4", worst[0], wd[0]))


# ---------------------------------------------------------------------------------------------------------- 2. the group edges
def _edge_sequence(m_cap):
    """one sequence of m_cap small frames for a handle of n_cap = m_cap, f_cap = 9, K = 2: per frame (readings [k][7], M, slots,
    obs).  No drops, so frame f's window holds f + 1 images and the last frame's all m_cap.  Image times are uneven (k = 1 or 2
    samples of 3 .. 30 ms).  Frames before the last carry one or two tracks of two or three observations on scattered slots; the
    last frame carries tracks of 1, 2, 3, G - 1, G and m_cap observations where m_cap allows -- the long ones on consecutive slots,
    the short ones on scattered slots that start mid-window -- and three more that start mid-window"""
    rng = sc.SplitMix64(0x71AE + m_cap)
    G = 16 if m_cap <= 16 else 32 if m_cap <= 32 else 64
    edge = sorted(set(m for m in (1, 2, 3, G - 1, G, m_cap) if m <= m_cap))

    def pick(W, m, start=0):
        """m ascending slots of a window of W, from `start` on, scattered where there is room"""
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


@pytest.mark.parametrize("m_cap", (16, 17, 32, 33, 63))
@pytest.mark.parametrize("prec", PRECS)
def test_timed_expansion_at_the_group_edges(capi, prec, m_cap):
    """G = 16 | 32 | 64 on both sides of each switch and the full wavefront.  Three trajectories on the one sequence: timing alone
    without pixel noise (bit for bit at the device's delta), all of timing with noise and faults, jitter alone at the seed 2^64 - 1.
    The last frame, whose window reaches m_cap, and two earlier frames are read"""
    cells, edge, G = _edge_sequence(m_cap)
    assert edge[-1] == m_cap and {1, 2, 3} <= set(edge) and (G - 1 in edge or G - 1 > m_cap) and (G in edge or G > m_cap)
    last = cells[-1]
    assert int(last[2].max()) == m_cap - 1 and sum(1 for t in range(len(last[1])) if last[2][int(last[1][:t].sum())] > 0) >= 4
    seeds = [31, 32, 0xFFFFFFFFFFFFFFFF]
    sigma = np.array([[0.01, 0.1, 0.0, 0.0], [0.01, 0.1, 2e-3, 1e-3], [0.01, 0.1, 1e-3, 1e-3]])
    fault4 = np.array([[0.0, 0.0, 0.0, 0.0], [0.4, 0.4, 0.02, 0.01], [0.0, 0.0, 0.0, 0.0]])
    timing4 = np.array([[4e-3, 0.02, -0.1, 0.0], [-6e-3, 0.03, 0.05, 2e-3], [0.0, 0.0, 0.0, 1e-3]])
    bt = capi.Batch(3, m_cap, 9, m_cap, _cd(capi, prec))
    bt.replay_alloc(1, m_cap, 2)
    for f, (rd, M, slots, obs) in enumerate(cells):
        bt.replay_set_cell(f, 0, rd, M, slots, obs, 0)
    bt.replay_assign([0, 0, 0], seeds, sigma)
    bt.replay_set_faults(fault4)
    bt.replay_set_timing(timing4)
    bt.replay_commit()
    time, frame_of, base = sc.replay_image_table([(c[0], 0) for c in cells])
    dt, df, db = bt.replay_image_table(0)
    assert np.array_equal(dt, time) and np.array_equal(df, frame_of) and np.array_equal(db, base) and not base.any() and len(time) == m_cap
    worst, wd, shifted = [0.0], [0.0], 0
    for f in (5, m_cap // 2, m_cap - 1):
        rd, M, slots, obs = cells[f]
        start = 0
        for b in range(3):
            ex = _read(bt, f, b)
            want = sc.replay_timing_delta(obs[:, 1], frame_of[base[f] + slots], seeds[b], timing4[b])
            _check_delta(ex["delta"], want, timing4[b, 3], (m_cap, f, b), wd)
            moved = sc.replay_timing_shift(M, slots, obs, time, base[f], ex["delta"])
            tw = FLB.faulted_cell(rd, M, slots, moved, f, seeds[b], sigma[b], fault4[b], 2)
            Ms = np.zeros(9, np.int32)
            Ms[:len(M)] = M
            Mp = np.zeros(9, np.int32)
            Mp[:len(M)] = tw["Mp"]
            assert (ex["n"], ex["drop"], ex["k"]) == (len(M), 0, len(rd)), (m_cap, f, b)
            assert np.array_equal(ex["off"], start + np.concatenate([[0], np.cumsum(Ms)[:-1]])), (m_cap, f, b)
            assert np.array_equal(ex["M"], Mp) and np.array_equal(ex["slots"], tw["slots"]) and np.array_equal(ex["code"], tw["code"]), (m_cap, f, b)
            if b == 0:
                _same_bits_or_rounded_once(prec, ex["obs"], tw["obs"], (m_cap, f, b))
                shifted += int((ex["obs"] != obs.astype(np.float32 if prec == "f32" else np.float64)).any(axis=1).sum())
                assert np.array_equal(ex["obs"][M.cumsum()[M == 1] - 1], obs[M.cumsum()[M == 1] - 1].astype(np.float32 if prec == "f32" else np.float64))   # a track of one stays
            else:
                FLB.check_scalars(prec, ex["obs"], tw["obs"], sigma[b, 2:] + fault4[b, 2:], (m_cap, f, b), worst)
            start += len(slots)
    bt.close()
    assert shifted > m_cap
    print("worst |device - twin| / (sigma + rho) (%s, m_cap %d, G %d): %.3g; delta / sigma_j: %.3g" % (prec, m_cap, G, worst[0], wd[0]))


# --------------------------------------------------------------------------- 3. the loop reads what the kernel wrote, bit for bit
_READ, _ORD = {}, {}


def _readbacks(capi, prec):
    """every (frame, trajectory) under the lab's timing and fault assignments: once per dtype, never written to"""
    if prec not in _READ:
        bt = _replay_batch(capi, prec, fault4=FLB.FAULT4)
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


@pytest.mark.parametrize("slices", (1, 2))
@pytest.mark.parametrize("cuts", ([(0, 16)], [(0, 5), (5, 16)]), ids=["one_call", "two_calls"])
@pytest.mark.parametrize("prec", PRECS)
def test_timed_replay_runs_the_bits_of_the_ordinary_run_on_the_readbacks(capi, prec, cuts, slices):
    want = _ordinary(capi, prec)
    bt = _replay_batch(capi, prec, fault4=FLB.FAULT4)
    bt.set_streams(slices)
    bt.set_slices_exact(slices > 1)
    assert bt.effective_streams() == slices
    bt.frame_log_enable(RL.NF)
    for f0, f1 in cuts:
        bt.run_frames_replay(f0, f1)
    got = _results(bt)
    bt.close()
    assert got["log"].shape == (RL.NF, RL.B, 48) and min(s[4]["n_passed"] for s in got["snap"]) > 0
    _same(got, want)


# ------------------------------------------------------------------------------------------------- 4. zero records
def _run(bt):
    bt.frame_log_enable(RL.NF)
    bt.run_frames_replay(0, RL.NF)
    return _results(bt)


_PLAIN = {}


def _plain(capi, prec):
    """a handle that never heard of timing, at the lab's seeds"""
    if prec not in _PLAIN:
        bt = _batch(capi, prec)
        RL.stage_replay(bt, RL.SEQ_OF, FLB.SEEDS, RL.SIGMA)
        _PLAIN[prec] = (_run(bt), [[bt.replay_expand(f, b) for b in range(RL.B)] for f in (4, 9)])
        bt.close()
    return _PLAIN[prec]


@pytest.mark.parametrize("setting", ("zeros", "null", "y0_only"))
@pytest.mark.parametrize("prec", PRECS)
def test_no_timing_is_the_handle_without_timing(capi, prec, setting):
    want, cells = _plain(capi, prec)
    t4 = dict(zeros=np.zeros((RL.B, 4)), null=None, y0_only=np.array([[0.0, 0.0, 0.3, 0.0]] * RL.B))[setting]
    bt = _replay_batch(capi, prec)
    bt.replay_set_timing(t4)                                     # after a non-zero record: it must be gone
    for i, f in enumerate((4, 9)):
        for b in range(RL.B):
            ex = _read(bt, f, b)
            assert not ex["delta"].any() and not ex["code"].any()
            for key in ("rd", "obs", "M", "off", "slots"):
                assert np.array_equal(ex[key], cells[i][b][key]), (f, b, key)
    _same(_run(bt), want)
    bt.close()


# ------------------------------------------------------------------------------------------------- 5. refusals and lifetime
@pytest.mark.parametrize("prec", PRECS)
def test_refusals_leave_the_record_and_the_record_outlives_assignments(capi, prec):
    EINVAL = r"\(-22\)"
    bt = _batch(capi, prec)
    for rec in (TL.TIMING4, None):
        with pytest.raises(capi.HipError, match=EINVAL + ".*no replay allocated"):
            bt.replay_set_timing(rec)
    TL.stage_replay(bt)
    for s in range(2):
        for got, want in zip(bt.replay_image_table(s), TL.table(s)):
            assert np.array_equal(got, want), s
    first = [_read(bt, 9, b) for b in range(RL.B)]
    assert all(first[b]["delta"].any() for b in range(1, RL.B)) and not first[0]["delta"].any()
    for bad in (float("inf"), float("nan")):
        for col in range(4):
            g = TL.TIMING4.copy()
            g[4, col] = bad
            with pytest.raises(capi.HipError, match=EINVAL + ".*timing values must be finite"):
                bt.replay_set_timing(g)
    g = TL.TIMING4.copy()
    g[2, 3] = -1e-9
    with pytest.raises(capi.HipError, match=EINVAL + ".*jitter must not be negative"):
        bt.replay_set_timing(g)
    g[4, 1] = float("nan")                                        # the order: finite first
    with pytest.raises(capi.HipError, match=EINVAL + ".*timing values must be finite"):
        bt.replay_set_timing(g)
    with pytest.raises(capi.HipError, match=r"\(-7\).*output buffer too small"):
        d = np.zeros(bt.f_cap * bt.m_cap)
        capi._chk(bt.L.msckf_hip_replay_expand_timing(bt.h, 9, 0, d.ctypes.data_as(capi._dp), 1))

    def same_as_first():
        for b in range(RL.B):
            ex = _read(bt, 9, b)
            for key in ("delta", "obs", "rd", "M", "slots", "code"):
                assert np.array_equal(ex[key], first[b][key]), (b, key)

    same_as_first()                                               # the refused calls left the record in force
    # a precondition of the shift: a track whose slots descend is committed without a record's objection, refused under one
    tr = RL.sequences()[0]
    fr = tr.frames[5]
    bad_slots = fr["slots"].copy()
    bad_slots[:2] = bad_slots[1::-1]
    bt.replay_set_cell(5, 0, tr.imu_for_frame(5), fr["M"], bad_slots, fr["obs"], 1 if RL.full(tr, 5) else 0)
    with pytest.raises(capi.HipError, match=EINVAL + ".*timing: sequence 0, frame 5, track 0: camera slots do not ascend strictly"):
        bt.replay_commit()
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.replay_expand(9, 1)
    bt.replay_set_timing(None)
    bt.replay_commit()
    with pytest.raises(capi.HipError, match=EINVAL + ".*timing: sequence 0, frame 5, track 0: camera slots do not ascend strictly"):
        bt.replay_set_timing(TL.TIMING4)
    assert not bt.replay_expand_timing(9, 1).any()                # ... and the empty record stayed
    bt.replay_set_cell(5, 0, tr.imu_for_frame(5), fr["M"], fr["slots"], fr["obs"], 1 if RL.full(tr, 5) else 0)
    bt.replay_commit()
    bt.replay_set_timing(TL.TIMING4)
    same_as_first()
    # the record survives assign_q followed by assign, a fault record that comes and goes, and a commit
    Q, scale, sigma_uv = FLB.model_of(0)
    bt.replay_assign_q(RL.SEQ_OF, FLB.SEEDS, Q, scale, sigma_uv)
    assert np.array_equal(bt.replay_expand_timing(9, 4), first[4]["delta"])
    bt.replay_assign(RL.SEQ_OF, FLB.SEEDS, RL.SIGMA)
    bt.replay_set_faults(FLB.FAULT4)
    assert np.array_equal(bt.replay_expand_timing(9, 4), first[4]["delta"]) and bt.replay_expand_faults(9, 4).any()
    bt.replay_set_faults(None)
    bt.replay_commit()
    same_as_first()
    # another record between two runs takes effect, and replay_alloc clears it
    bt.replay_set_timing(TL.ALL)
    assert bt.replay_expand_timing(9, 0).any() and not np.array_equal(bt.replay_expand_timing(9, 4), first[4]["delta"])
    RL.stage_replay(bt, RL.SEQ_OF, FLB.SEEDS, RL.SIGMA)
    assert not any(bt.replay_expand_timing(9, b).any() for b in range(RL.B))
    bt.close()
