"""Seeded missed observations and outliers of the Monte-Carlo replay on the device (msckf_hip_replay_set_faults and its three
companions; csrc/replay_plan.h FAULTS, k_replay_expand_faults, k_replay_fault_counts, k_map_fault_metrics).

  1. the faulted expansion against the numpy twin on the common shape under the lab assignment (tests/replay_faults_lab.py), both
     noise models: n, drop, k, off the sequence's; M, slots (the whole range, partition order) and the codes equal; coordinates to
     1e-13 (sigma + rho) in double, one ulp of float32(twin) in float
  2. the lane groups' edges: handles of m_cap 16 | 17 | 32 | 33 | 63, tracks of 0, 1, 2, 3, G - 1, G and m_cap observations, nine
     tracks of two, a skipped cell and one without tracks, p_miss 0.5 | 1 | 0
  3. the loop reads what the kernel wrote: the bits of run_frames on the compact survivors of the read-backs
  4. parity with the oracle on the twin's survivors (1e-6 double free-running, 1e-3 float teacher-forced), per track
  5. the two reductions against the twin, and their refusals
  6. neutrality (zeros, NULL: the bits of a handle without faults) and lifetime of the record

Measured on an MI355X: worst |device - twin| / (sigma + rho) in double 2.55e-14 on the common shape under
both noise models and 5.05e-15 over the group-edge cells, against the bound 1e-13; the tests print the figure (-s)."""
import numpy as np
import pytest

import helpers as H
import replay_faults_lab as FLB
import replay_lab as RL
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu
PRECS = ("f32", "f64")


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c_
    c_.lib()
    return c_


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def _cd(capi, prec):
    return capi.F64 if prec == "f64" else capi.F32


def _batch(capi, prec):
    bt = capi.Batch(RL.B, RL.N_CAP, RL.F_CAP, RL.M_CAP, _cd(capi, prec))
    for b, s in enumerate(RL.SEQ_OF):
        tr = RL.sequences()[s]
        bt.initialize(b, tr.cfg, tr.imu0)
    return bt


def _replay_batch(capi, prec, fault4=FLB.FAULT4, seeds=FLB.SEEDS, model=False):
    bt = _batch(capi, prec)
    FLB.stage_replay(bt, fault4, seeds, model)
    return bt


def _read(bt, f, b):
    ex = bt.replay_expand(f, b)
    ex["code"] = bt.replay_expand_faults(f, b)
    return ex


_READ = {}


def _readbacks(capi, prec):
    """replay_expand + replay_expand_faults of every (frame, trajectory) under the lab assignment: once per dtype, never written to"""
    if prec not in _READ:
        bt = _replay_batch(capi, prec)
        _READ[prec] = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
        bt.close()
    return _READ[prec]


def _results(bt):
    bt.sync()
    return dict(snap=[H.snapshot(bt, b) for b in range(bt.B)], log=bt.frame_log_read()[0])


def _same(x, y):
    assert len(x["snap"]) == len(y["snap"])
    for b, (p, q) in enumerate(zip(x["snap"], y["snap"])):
        assert H.same_bits(p, q), b
    assert np.array_equal(x["log"], y["log"])


# ------------------------------------------------------------------------------------------- 1. the expansion against the twin
def _check_cell(prec, ex, tw, M_seq, base, n, drop, k, sigma_uv, fault4, where, worst):
    """one read-back against the twin's cell: integers, slots and codes equal, coordinates by the lab's rule at sigma + rho"""
    f_cap = len(ex["M"])
    assert (ex["n"], ex["drop"], ex["k"]) == (n, drop, k), where
    Ms, Mp = np.zeros(f_cap, np.int32), np.zeros(f_cap, np.int32)
    Ms[:len(M_seq)] = M_seq
    Mp[:len(M_seq)] = tw["Mp"]
    assert np.array_equal(ex["off"], base + np.concatenate([[0], np.cumsum(Ms)[:-1]])), where      # the sequence's lengths
    assert np.array_equal(ex["M"], Mp), (where, ex["M"], Mp)
    assert np.array_equal(ex["slots"], tw["slots"]), where
    assert np.array_equal(ex["code"], tw["code"]), where
    FLB.check_scalars(prec, ex["obs"], tw["obs"], np.array(sigma_uv) + np.array(fault4[2:]), where, worst)


@pytest.mark.parametrize("model", (False, True), ids=["sigma4", "q_imu"])
@pytest.mark.parametrize("prec", PRECS)
def test_faulted_expansion_of_the_common_shape_against_the_twin(capi, prec, model):
    """every (frame, trajectory) under the lab assignment.  Under sigma4 the readings are the twin's by the existing rule; under
    the Q_imu model they are the bits of the same handle's unfaulted expansion (faults never touch a reading)"""
    if model:
        bt = _replay_batch(capi, prec, model=True)
        reads = [[_read(bt, f, b) for b in range(RL.B)] for f in range(RL.NF)]
        bt.replay_set_faults(None)
        plain = [[bt.replay_expand(f, b) for b in range(RL.B)] for f in range(RL.NF)]
        bt.close()
    else:
        reads = _readbacks(capi, prec)
    worst, wrd, moved = [0.0], [0.0], 0
    for f in range(RL.NF):
        base = 0
        for b in range(RL.B):
            ex, tw = reads[f][b], FLB.twin_cell(f, b)
            if model:                                  # the twin's observations do not depend on the IMU model
                assert np.array_equal(ex["rd"], plain[f][b]["rd"]), (f, b)
            else:
                assert np.array_equal(ex["rd"][:, 6], tw["rd"][:, 6] if prec == "f64" else tw["rd"][:, 6].astype(np.float32).astype(np.float64)), (f, b)
                FLB.check_scalars(prec, ex["rd"][:, :6], tw["rd"][:, :6], np.array([RL.SIGMA[0]] * 3 + [RL.SIGMA[1]] * 3), (f, b), wrd)
            _check_cell(prec, ex, tw, tw["M"], base, len(tw["M"]), tw["drop"], sc.IMU_PER_FRAME, RL.SIGMA[2:], FLB.FAULT4[b], (f, b), worst)
            moved += int((tw["code"] != 0).sum())
            base += len(tw["slots"])
    assert moved > 300
    print("worst |device - twin| / (sigma + rho) (%s, %s): %.3g; readings / sigma: %.3g" % (prec, "q_imu" if model else "sigma4", worst[0], wrd[0]))


# ---------------------------------------------------------------------------------------------------------- 2. the group edges
def _edge_cells(m_cap):
    """S = 2 sequences x 4 frames for a handle of n_cap = m_cap, f_cap = 9 (no filter runs on it): per (frame, sequence)
    (readings [k][7], M, slots, obs, n_drop, skip).  The edge list -- tracks of 0, 1, 2, 3, G - 1, G and m_cap observations where
    m_cap allows, the longest last -- and nine tracks of two (every lane group of a wavefront at G = 16, more than one wavefront at
    G = 32 and 64) sit in both sequences on different frames; sequence 0 also has a skipped cell and one without tracks"""
    rng = sc.SplitMix64(0xFA17 + m_cap)
    G = 16 if m_cap <= 16 else 32 if m_cap <= 32 else 64
    edge = sorted(set(m for m in (0, 1, 2, 3, G - 1, G, m_cap) if m <= m_cap))

    def cell(k, counts):
        M = np.array(counts, dtype=np.int32)
        slots = np.concatenate([np.arange(m, dtype=np.int32) for m in counts]) if len(counts) else np.zeros(0, np.int32)
        rd = np.concatenate([rng.normal(6 * k).reshape(k, 6), np.full((k, 1), 0.005)], 1)
        return rd, M, slots, 2.0 * rng.uniform(2 * int(M.sum())).reshape(-1, 2) - 1.0, 0, False

    skipped = (np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), 0, True)
    seq0 = [cell(10, edge), cell(7, [2] * 9), skipped, cell(10, [])]
    seq1 = [cell(10, [2] * 9), cell(10, edge), cell(0, [5]), cell(10, [3, 3])]
    return [seq0, seq1], edge, G


@pytest.mark.parametrize("m_cap", (16, 17, 32, 33, 63))
@pytest.mark.parametrize("prec", PRECS)
def test_faulted_expansion_at_the_group_edges(capi, prec, m_cap):
    """G = 16 | 32 | 64 on both sides of each switch and the full wavefront; three trajectories with p_miss 0.5 | 1 | 0 and
    p_out = 0.5, two of them on the same sequence; everything equal to the twin as on the common shape"""
    seqs, edge, G = _edge_cells(m_cap)
    assert edge[-1] == m_cap and {0, 1, 2, 3} <= set(edge) and (G - 1 in edge or G - 1 > m_cap) and (G in edge or G > m_cap)
    seq_of, seeds, sigma = [0, 1, 0], [21, 22, 0xFFFFFFFFFFFFFFFF], (0.01, 0.1, 2e-3, 1e-3)
    fault4 = np.array([[0.5, 0.5, 0.02, 0.01], [1.0, 0.5, 0.01, 0.03], [0.0, 0.5, 0.05, 0.05]])
    bt = capi.Batch(3, m_cap, 9, m_cap, _cd(capi, prec))
    bt.replay_alloc(2, 4, 10)
    for f in range(4):
        for s in range(2):
            rd, M, slots, obs, drop, skip = seqs[s][f]
            bt.replay_set_cell(f, s, rd, M, slots, obs, drop, skip=skip)
    bt.replay_assign(seq_of, seeds, sigma)
    bt.replay_set_faults(fault4)
    bt.replay_commit()
    worst, wrd, shielded, shortened = [0.0], [0.0], 0, 0
    for f in range(4):
        base = 0
        for b in range(3):
            rd, M, slots, obs, drop, skip = seqs[seq_of[b]][f]
            ex = _read(bt, f, b)
            tw = FLB.faulted_cell(rd, M, slots, obs, f, seeds[b], sigma, fault4[b], 10)
            _check_cell(prec, ex, tw, M, base, len(M), 0, -1 if skip else len(rd), sigma[2:], fault4[b], (m_cap, f, b), worst)
            assert np.array_equal(ex["rd"][:, 6], tw["rd"][:, 6] if prec == "f64" else tw["rd"][:, 6].astype(np.float32).astype(np.float64))
            FLB.check_scalars(prec, ex["rd"][:, :6], tw["rd"][:, :6], np.array([sigma[0]] * 3 + [sigma[1]] * 3), (m_cap, f, b), wrd)
            o = 0
            for t, m in enumerate(int(x) for x in M):
                raw = int(tw["raw"][o:o + m].sum())
                shielded += raw > 0 and m - raw < 2 and tw["Mp"][t] == m         # the rule bit: raw misses, none applied
                shortened += tw["Mp"][t] < m
                o += m
            base += len(slots)
    bt.close()
    assert shielded > 0 and shortened > 0, (shielded, shortened)
    print("worst |device - twin| / (sigma + rho) (%s, m_cap %d, G %d): %.3g" % (prec, m_cap, G, worst[0]))


# --------------------------------------------------------------------------- 3. the loop reads what the kernel wrote, bit for bit
_ORD = {}


def _ordinary(capi, prec):
    """run_frames(0, 16) on a second handle whose ordinary scenario holds the SURVIVORS of the read-backs, compact, no slack"""
    if prec not in _ORD:
        bt = _batch(capi, prec)
        bt.scenario_alloc(RL.NF, sc.IMU_PER_FRAME)
        for f, row in enumerate(_readbacks(capi, prec)):
            for b, ex in enumerate(row):
                n = ex["n"]
                M_seq = RL.sequences()[RL.SEQ_OF[b]].frames[f]["M"]
                Mp, slots, obs = FLB.survivors(dict(M=M_seq, Mp=ex["M"][:n], slots=ex["slots"], obs=ex["obs"]))
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
def test_faulted_replay_runs_the_bits_of_the_ordinary_run_on_the_survivors(capi, prec, cuts, slices):
    """the slack behind a shortened track and the sequence's (conservative) maxslot change nothing: snapshots and frame-log
    records are those of run_frames on the compact survivors"""
    want = _ordinary(capi, prec)
    bt = _replay_batch(capi, prec)
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
    shortened = sum(int((ex["M"][:ex["n"]] < RL.sequences()[RL.SEQ_OF[b]].frames[f]["M"]).sum()) for f, row in enumerate(_readbacks(capi, prec)) for b, ex in enumerate(row))
    assert shortened > 50


# ------------------------------------------------------------------------------------------------------- 4. against the oracle
def _errs(bt, b, o):
    return H.state_errors(bt.imu_state(b), o.getImuState(), bt.cam_states(b)[0], o.getCamStates()[0], bt.covariance(b), o.getCovariance())


def _oracle_frame(o, tr, f):
    """helpers.oracle_frame, stopping before the prune: lastTracks still index the frame's camera slots"""
    o.propagate(tr.imu_for_frame(f))
    o.augmentState(f, tr.frame_times[f])
    fr = tr.frames[f]
    if len(fr["M"]):
        o.setTracks(fr["M"], fr["slots"], fr["obs"])
        o.marginalize()
        return o.lastTracks(), o.lastStats()
    return None, None


def _check_frame(bt, b, o, tr, f, prec, rows, st):
    sd = bt.last_stats(b)
    for key in H.STAT_KEYS:
        assert st[key] == sd[key], (f, b, key, st, sd)
    ok = (rows[:, 0] > 0) & (rows[:, 1] > 0)
    H.check_tracks(bt.last_tracks(b), rows, ok, prec, tr, tr.frames[f], o, (f, b))
    return sd


def test_faulted_replay_double_free_running_vs_oracle(capi, po):
    """double, free-running from the first frame on the TWIN's survivors under the lab assignment and its asserted margins:
    1e-6 on every field after every frame, equal statistics, every track's flags, point and gamma (helpers.check_tracks)"""
    trs = [FLB.survivor_trajectory(b) for b in range(RL.B)]
    bt = _replay_batch(capi, "f64")
    oracles = []
    for tr in trs:
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        oracles.append(o)
    rejected = 0
    for f in range(RL.NF):
        bt.run_frames_replay(f, f + 1)
        bt.sync()
        for b, (tr, o) in enumerate(zip(trs, oracles)):
            rows, st = _oracle_frame(o, tr, f)
            if rows is not None:
                sd = _check_frame(bt, b, o, tr, f, "f64", rows, st)
                rejected += sd["n_gate_rejected"]
                if tr.frames[f]["Nw"] == RL.N:
                    assert sd["n_passed"] > 0 and sd["m_rows"] > 0, (f, b, sd)
            if o.getNumCamStates() == RL.N:
                o.dropOldest(1)
            assert bt.num_cam_states(b) == o.getNumCamStates(), (f, b)
            err = _errs(bt, b, o)
            assert H.worst(err) < 1e-6, (f, b, err)
    bt.close()
    assert rejected > 10


def test_faulted_replay_float_teacher_forced_vs_oracle(capi, po):
    """float: before every frame each trajectory's state and covariance go device -> float oracle, both run the frame on the
    twin's survivors and agree to 1e-3 with equal statistics and per-track parity"""
    trs = [FLB.survivor_trajectory(b) for b in range(RL.B)]
    bt = _replay_batch(capi, "f32")
    passed = [0] * RL.B
    for f in range(RL.NF):
        oracles = []
        for b, tr in enumerate(trs):
            o = po.Oracle(po.F32, po.LEAN)
            o.initialize(tr.cfg, tr.imu0)
            H.copy_device_to_oracle(bt, b, o)
            oracles.append(o)
        bt.run_frames_replay(f, f + 1)
        bt.sync()
        for b, (tr, o) in enumerate(zip(trs, oracles)):
            rows, st = _oracle_frame(o, tr, f)
            if rows is not None:
                passed[b] += _check_frame(bt, b, o, tr, f, "f32", rows, st)["n_passed"]
            if o.getNumCamStates() == RL.N:
                o.dropOldest(1)
            err = _errs(bt, b, o)
            assert H.worst(err) < 1e-3, (f, b, err)
    assert min(passed) > 0, passed
    bt.close()


# ------------------------------------------------------------------------------------------------------------ 5. the reductions
@pytest.mark.parametrize("prec", PRECS)
def test_fault_counts_equal_the_twins(capi, prec):
    bt = _replay_batch(capi, prec)
    for f0, f1 in ((0, RL.NF), (3, 11), (7, 7)):
        got = bt.replay_fault_counts(f0, f1)
        assert got.dtype == np.int64 and np.array_equal(got, FLB.counts(FLB.FAULT4, f0=f0, f1=f1)), (f0, f1, got)
    assert bt.replay_fault_counts()[:, 1:3].sum() > 300
    bt.replay_set_faults(None)
    none = bt.replay_fault_counts()
    assert not none[:, [1, 2, 4, 5]].any() and np.array_equal(none[:, [0, 3]], FLB.counts(FLB.FAULT4)[:, [0, 3]])
    bt.close()


@pytest.mark.parametrize("prec", PRECS)
def test_map_log_fault_metrics_against_the_twin(capi, prec):
    """after a faulted run with the map log on, in two calls: the counts equal replay_gate_confusion on map_log_read, the two sums
    agree with numpy's, two calls give equal bits; a cut of the ordinals with its frame offset; and every refusal with its code"""
    EINVAL = r"\(-22\)"
    bt = _replay_batch(capi, prec)
    with pytest.raises(capi.HipError, match=EINVAL + ".*map log not enabled"):
        bt.map_log_fault_metrics(0, 0, 0)
    bt.map_log_enable(RL.NF * RL.F_CAP)
    bt.run_frames_replay(0, 6)
    bt.run_frames_replay(6, RL.NF)
    bt.sync()
    assert bt.map_log_frames() == RL.NF
    recs = [bt.map_log_read(b)[0] for b in range(RL.B)]
    rtol = 1e-12 if prec == "f64" else 1e-6
    for q0, q1, f0 in ((0, RL.NF, 0), (4, 12, 4)):
        got = bt.map_log_fault_metrics(q0, q1, f0)
        assert np.array_equal(got, bt.map_log_fault_metrics(q0, q1, f0))
        for b in range(RL.B):
            want = sc.replay_gate_confusion(recs[b], FLB.cells_M(b), FLB.SEEDS[b], FLB.FAULT4[b], q0, q1, f0)
            assert np.array_equal(got[b, [0, 1, 2, 3, 4, 7]], want[[0, 1, 2, 3, 4, 7]]), (q0, q1, b, got[b], want)
            assert np.allclose(got[b, 5:7], want[5:7], rtol=rtol, atol=0), (q0, q1, b, got[b], want)
    full = bt.map_log_fault_metrics(0, RL.NF, 0)
    print("gate confusion per trajectory (%s): records, clean pass / rej, contaminated pass / rej\n" % prec, full[:, :5])
    assert full[2, 3] >= 1 and full[3, 4] >= 1 and not full[:2, 3:5].any() and not full[:, 7].any()
    assert np.all(full[:, 0] == full[:, 1:5].sum(1))
    # contaminated tracks that were never triangulated: what the counts know and the log does not
    cnt = bt.replay_fault_counts()
    assert np.all(cnt[:, 5] - full[:, 3] - full[:, 4] >= 0)
    # a shifted frame offset recomputes other tracks' faults: the caller's statement matters
    assert not np.array_equal(bt.map_log_fault_metrics(4, 12, 3)[:, 1:5], bt.map_log_fault_metrics(4, 12, 4)[:, 1:5])
    # the refusals: ordinals, the frame range, the replay's state
    with pytest.raises(capi.HipError, match=EINVAL + ".*frame ordinal range beyond the ordinals handed out"):
        bt.map_log_fault_metrics(0, RL.NF + 1, 0)
    for bad in ((0, RL.NF, 1), (0, 4, -1), (0, 4, RL.NF - 3)):
        with pytest.raises(capi.HipError, match=EINVAL + ".*frame range out of bounds"):
            bt.map_log_fault_metrics(*bad)
    fr = RL.sequences()[0].frames[5]
    bt.replay_set_cell(5, 0, RL.sequences()[0].imu_for_frame(5), fr["M"], fr["slots"], fr["obs"], 1)      # un-commits
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.map_log_fault_metrics(0, RL.NF, 0)
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.replay_fault_counts()
    bt.replay_commit()
    assert np.array_equal(bt.map_log_fault_metrics(0, RL.NF, 0), full)
    bt.close()
    bt = _batch(capi, prec)
    bt.map_log_enable(8)
    bt.replay_alloc(2, RL.NF, sc.IMU_PER_FRAME)
    bt.replay_commit()
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not assigned"):
        bt.map_log_fault_metrics(0, 0, 0)
    bt.close()


# ------------------------------------------------------------------------------------------------- 6. neutrality and lifetime
def _run(bt):
    bt.frame_log_enable(RL.NF)
    bt.run_frames_replay(0, RL.NF)
    return _results(bt)


_PLAIN = {}


def _plain(capi, prec):
    """a handle that never heard of faults, at the lab's seeds"""
    if prec not in _PLAIN:
        bt = _batch(capi, prec)
        RL.stage_replay(bt, RL.SEQ_OF, FLB.SEEDS, RL.SIGMA)
        _PLAIN[prec] = (_run(bt), [[bt.replay_expand(f, b) for b in range(RL.B)] for f in (4, 9)])
        bt.close()
    return _PLAIN[prec]


@pytest.mark.parametrize("setting", ("zeros", "null", "radii_only"))
@pytest.mark.parametrize("prec", PRECS)
def test_no_fault_is_the_handle_without_faults(capi, prec, setting):
    want, cells = _plain(capi, prec)
    f4 = dict(zeros=np.zeros((RL.B, 4)), null=None, radii_only=np.array([[0.0, 0.0, 0.1, 0.2]] * RL.B))[setting]
    bt = _replay_batch(capi, prec, fault4=FLB.FAULT4)
    bt.replay_set_faults(f4)                                     # after a faulted record: it must be gone
    for i, f in enumerate((4, 9)):
        for b in range(RL.B):
            ex = _read(bt, f, b)
            assert not ex["code"].any()
            for key in ("rd", "obs", "M", "off", "slots"):
                assert np.array_equal(ex[key], cells[i][b][key]), (f, b, key)
    _same(_run(bt), want)
    bt.close()


@pytest.mark.parametrize("prec", PRECS)
def test_refusals_leave_the_record_and_the_record_outlives_assignments(capi, prec):
    """every refusal with its code; a refused call leaves the previous record in force; equal seeds and equal fault4 give equal
    bits and another p_miss other M; a new record between two runs takes effect; the record survives replay_assign_q followed by
    replay_assign, and replay_alloc clears it"""
    EINVAL = r"\(-22\)"
    bt = _batch(capi, prec)
    with pytest.raises(capi.HipError, match=EINVAL + ".*no replay allocated"):
        bt.replay_set_faults(FLB.FAULT4)
    with pytest.raises(capi.HipError, match=EINVAL + ".*no replay allocated"):
        bt.replay_set_faults(None)
    seeds = [77, 78, 77, 79, 78]
    f4 = np.array([[0.3, 0.2, 3 * FLB.PX, 3 * FLB.PX]] * RL.B)
    f4[3, 0] = 0.5
    FLB.stage_replay(bt, f4, seeds)
    for bad in (-1e-9, 1.5, float("nan")):
        for col in (0, 1):
            g = f4.copy()
            g[4, col] = bad
            with pytest.raises(capi.HipError, match=EINVAL + r".*fault probabilities must lie in \[0, 1\]"):
                bt.replay_set_faults(g)
    for bad in (-1e-9, float("inf"), float("nan")):
        g = f4.copy()
        g[0, 3] = bad
        g[4, 2] = bad
        with pytest.raises(capi.HipError, match=EINVAL + ".*fault radii must be finite and not negative"):
            bt.replay_set_faults(g)
    g = f4.copy()
    g[0, 2], g[4, 1] = -1.0, 2.0                                  # the order: probabilities first
    with pytest.raises(capi.HipError, match=EINVAL + ".*fault probabilities"):
        bt.replay_set_faults(g)
    with pytest.raises(capi.HipError, match=r"\(-7\).*output buffer too small"):
        cap = bt.f_cap * bt.m_cap
        code = np.zeros(cap, np.int32)
        capi._chk(bt.L.msckf_hip_replay_expand_faults(bt.h, 9, 0, code.ctypes.data_as(capi._ip), 1))
    # the refused calls left f4 in force; trajectories 0 and 2: same sequence, seed and record; 3: another p_miss on another seed
    first = [_read(bt, 9, b) for b in range(RL.B)]
    for b in range(RL.B):
        tw = FLB.twin_cell(9, b, f4, seeds)
        assert np.array_equal(first[b]["code"], tw["code"]) and np.array_equal(first[b]["M"][:len(tw["Mp"])], tw["Mp"]), b
    assert np.array_equal(first[0]["M"], first[2]["M"]) and np.array_equal(first[0]["obs"], first[2]["obs"])
    bt.frame_log_enable(RL.NF)
    bt.run_frames_replay(0, 8)
    # another p_miss between two runs: other M from here on, and it takes effect in the run
    f5 = f4.copy()
    f5[:, 0] = 0.6
    bt.replay_set_faults(f5)
    second = [_read(bt, 9, b) for b in range(RL.B)]
    assert any(not np.array_equal(first[b]["M"], second[b]["M"]) for b in range(RL.B))
    for b in range(RL.B):
        assert np.array_equal(second[b]["code"], FLB.twin_cell(9, b, f5, seeds)["code"]), b
    bt.run_frames_replay(8, RL.NF)
    got = _results(bt)
    assert H.same_bits(got["snap"][0], got["snap"][2]) and not np.array_equal(got["snap"][0][0], got["snap"][3][0])
    # the same two records on a fresh handle, both runs: the same bits (a pure function of seed, frame, index and the record)
    b2 = _batch(capi, prec)
    FLB.stage_replay(b2, f4, seeds)
    b2.frame_log_enable(RL.NF)
    b2.run_frames_replay(0, 8)
    b2.replay_set_faults(f5)
    b2.run_frames_replay(8, RL.NF)
    _same(_results(b2), got)
    # ... and f4 throughout gives others
    b2.close()
    b3 = _batch(capi, prec)
    FLB.stage_replay(b3, f4, seeds)
    assert not np.array_equal(_run(b3)["log"][8:], got["log"][8:])
    b3.close()
    # the record survives assign_q followed by assign, and a commit
    Q, scale, sigma_uv = FLB.model_of(0)
    bt.replay_assign_q(RL.SEQ_OF, seeds, Q, scale, sigma_uv)
    assert np.array_equal(bt.replay_expand_faults(9, 1), second[1]["code"])
    bt.replay_assign(RL.SEQ_OF, seeds, RL.SIGMA)
    bt.replay_commit()
    third = [_read(bt, 9, b) for b in range(RL.B)]
    for b in range(RL.B):
        for key in ("code", "M", "slots", "obs", "rd"):
            assert np.array_equal(third[b][key], second[b][key]), (b, key)
    # replay_alloc clears it
    RL.stage_replay(bt, RL.SEQ_OF, seeds, RL.SIGMA)
    assert not any(bt.replay_expand_faults(9, b).any() for b in range(RL.B))
    assert not bt.replay_fault_counts()[:, [1, 2]].any()
    bt.close()
