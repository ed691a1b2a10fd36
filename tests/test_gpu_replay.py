"""The Monte-Carlo replay on the device (msckf_hip_replay_*, msckf_hip_run_frames_replay; csrc/replay_plan.h, kernels_replay.hip):
noise-free sequences staged once, expanded per frame by k_replay_expand into the ordinary frame block with each trajectory's
own seeded noise.

  1. the expansion against the numpy twin (scenario.replay_*): integers and slots equal, scalars to 1e-13 sigma (double) /
     one float ulp (float), on the common shape (tests/replay_lab.py) and on cells with k = 7, k = 0, a skipped cell and
     entry counts around the kernel's chunk (REPLAY_CHUNK of csrc/dev_common.h, read from there)
  2. the frame loop reads what the kernel wrote: an ordinary scenario staged from the expansion's read-backs gives the same bits
     through run_frames, however the replay's call is cut and sliced
  3. parity with the oracle on the read-back inputs at the suite's bars (1e-6 double free-running, 1e-3 float teacher-forced)
  4. seeds and noise levels: equal ones give equal bits, another seed does not, no noise is the sequence itself, a new
     assignment between two runs takes effect
  5. the map log and the pruned-state log record the same as on the ordinary run
  6. every refusal of the header reaches HipError with its code

Measured on an MI355X: worst |device - twin| / sigma in double 5.09e-14 on the common shape and 5.55e-14
on the edge cells, against the bound 1e-13 -- one ulp of a coordinate in [0.25, 0.5) where the two libraries' noise differs in
its last bits; the tests print the figure (-s)."""
import os
import re

import numpy as np
import pytest

import helpers as H
import replay_lab as RL
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu
PRECS = ("f32", "f64")
CHUNK = int(re.search(r"constexpr int REPLAY_CHUNK = (\d+);", open(os.path.join(H.ROOT, "msckf_mono_amd", "csrc", "dev_common.h")).read()).group(1))


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


def _batch(capi, prec, seq_of=RL.SEQ_OF):
    bt = capi.Batch(len(seq_of), RL.N_CAP, RL.F_CAP, RL.M_CAP, _cd(capi, prec))
    for b, s in enumerate(seq_of):
        tr = RL.sequences()[s]
        bt.initialize(b, tr.cfg, tr.imu0)
    return bt


def _replay_batch(capi, prec, seq_of=RL.SEQ_OF, seeds=RL.SEEDS, sigma=RL.SIGMA):
    bt = _batch(capi, prec, seq_of)
    RL.stage_replay(bt, seq_of, seeds, sigma)
    return bt


def _cells_of(ex):
    """scenario_set's arguments of a replay_expand read-back"""
    k = max(ex["k"], 0)
    return ex["rd"][:k], ex["M"][:ex["n"]], ex["slots"], ex["obs"], ex["drop"]


_READ = {}


def _readbacks(capi, prec):
    """replay_expand of every (frame, trajectory) of the common shape: read once per dtype, shared, never written to"""
    if prec not in _READ:
        bt = _replay_batch(capi, prec)
        _READ[prec] = [[bt.replay_expand(f, b) for b in range(RL.B)] for f in range(RL.NF)]
        bt.close()
    return _READ[prec]


def _stage_ordinary(bt, cells):
    """cells[f][b] (replay_expand read-backs) as an ordinary resident scenario"""
    bt.scenario_alloc(len(cells), sc.IMU_PER_FRAME)
    for f, row in enumerate(cells):
        for b, ex in enumerate(row):
            rd, M, slots, obs, drop = _cells_of(ex)
            bt.scenario_set(f, b, rd, M, slots, obs, drop, skip=ex["k"] < 0)
    bt.scenario_commit()


def _enable_logs(bt, logs):
    bt.frame_log_enable(RL.NF)
    if logs:
        bt.map_log_enable(RL.NF * RL.F_CAP)
        bt.pruned_log_enable(RL.NF)


def _results(bt, logs):
    bt.sync()
    out = dict(snap=[H.snapshot(bt, b) for b in range(bt.B)], log=bt.frame_log_read()[0])
    if logs:
        out["map_counts"] = bt.map_log_counts()
        out["map"] = [bt.map_log_read(b)[0] for b in range(bt.B)]
        out["prn_counts"] = bt.pruned_log_counts()
        out["prn"] = [bt.pruned_log_read(b) for b in range(bt.B)]
    return out


_ORD = {}


def _ordinary(capi, prec, logs=False):
    """run_frames(0, 16) on the scenario staged from the read-backs, one stream: once per dtype and log setting"""
    if (prec, logs) not in _ORD:
        bt = _batch(capi, prec)
        _stage_ordinary(bt, _readbacks(capi, prec))
        bt.set_streams(1)
        _enable_logs(bt, logs)
        bt.run_frames(0, RL.NF)
        _ORD[(prec, logs)] = _results(bt, logs)
        bt.close()
    return _ORD[(prec, logs)]


def _same(x, y):
    assert len(x["snap"]) == len(y["snap"])
    for b, (p, q) in enumerate(zip(x["snap"], y["snap"])):
        assert H.same_bits(p, q), b
    assert np.array_equal(x["log"], y["log"])


# ------------------------------------------------------------------------------------------- 1. the expansion against the twin
def _check_scalars(prec, dev_rd, dev_obs, twin_rd, twin_obs, sigma, where, worst):
    """dev_* against the twin's doubles: dT equal (the rounded value), the rest to 1e-13 sigma (double) or one float ulp of
    float32(twin) (float); worst[0] collects the largest |device - twin| / sigma of the double comparison"""
    sg = np.array([sigma[0]] * 3 + [sigma[1]] * 3)
    so = np.array([sigma[2], sigma[3]])
    if prec == "f64":
        assert np.array_equal(dev_rd[:, 6], twin_rd[:, 6]), where
        for d, t, s in ((dev_rd[:, :6], twin_rd[:, :6], sg), (dev_obs, twin_obs, so)):
            if d.size:
                ratio = np.abs(d - t) / s
                worst[0] = max(worst[0], float(ratio.max()))
                assert np.all(np.abs(d - t) <= 1e-13 * s), (where, float(ratio.max()))
        return
    for d, t in ((dev_rd, twin_rd), (dev_obs, twin_obs)):
        t32 = t.astype(np.float32)
        assert np.array_equal(d, d.astype(np.float32).astype(np.float64)), where          # a float widened
        assert np.all(np.abs(d - t32.astype(np.float64)) <= np.spacing(np.abs(t32)).astype(np.float64)), where
    assert np.array_equal(dev_rd[:, 6], twin_rd[:, 6].astype(np.float32).astype(np.float64)), where


@pytest.mark.parametrize("prec", PRECS)
def test_expansion_of_the_common_shape_against_the_twin(capi, prec):
    """every (frame, trajectory): n, drop, k, M and slots are the sequence's, off is the sequence's rebased to the trajectory's
    first entry in the expanded block (a prefix sum over the non-monotone seq_of, recomputed here), readings and coordinates
    are the twin's"""
    reads = _readbacks(capi, prec)
    worst = [0.0]
    for f in range(RL.NF):
        base = 0
        for b in range(RL.B):
            ex = reads[f][b]
            rd, M, slots, obs, drop = RL.twin_cell(f, b)
            assert (ex["n"], ex["drop"], ex["k"]) == (len(M), drop, sc.IMU_PER_FRAME), (f, b)
            Mp = np.zeros(RL.F_CAP, np.int32)
            Mp[:len(M)] = M
            assert np.array_equal(ex["M"], Mp) and np.array_equal(ex["slots"], slots), (f, b)
            assert np.array_equal(ex["off"], base + np.concatenate([[0], np.cumsum(Mp)[:-1]])), (f, b)
            assert ex["obs"].shape == obs.shape and ex["rd"].shape == rd.shape
            _check_scalars(prec, ex["rd"], ex["obs"], rd, obs, RL.SIGMA, (f, b), worst)
            base += len(slots)
    print("worst |device - twin| / sigma (%s): %.3g" % (prec, worst[0]))


def _edge_cells():
    """S = 2 sequences x 6 frames for a handle of n_cap = m_cap = 32, f_cap = 9 (no filter runs on it): per (frame, sequence)
    (readings [k][7], M, slots, obs, n_drop, skip).  Sequence 0: k = 7; a skipped cell; CHUNK - 1, CHUNK and CHUNK + 1 entries;
    nothing.  Sequence 1: k = 0; then cells of five to nine entries, so that the trajectories' bases differ."""
    rng = sc.SplitMix64(0xED6E)

    def cell(k, counts):
        M = np.array(counts, dtype=np.int32)
        slots = np.concatenate([np.arange(m, dtype=np.int32) for m in counts]) if len(counts) else np.zeros(0, np.int32)
        rd = np.concatenate([rng.normal(6 * k).reshape(k, 6), np.full((k, 1), 0.005)], 1)
        return rd, M, slots, 2.0 * rng.uniform(2 * int(M.sum())).reshape(-1, 2) - 1.0, 0, False

    def split(n):
        return [32] * (n // 32) + ([n % 32] if n % 32 else [])

    skipped = (np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), 0, True)
    assert CHUNK + 1 <= 9 * 32
    seq0 = [cell(7, [3, 4]), skipped, cell(10, split(CHUNK - 1)), cell(10, split(CHUNK)), cell(10, split(CHUNK + 1)), cell(10, [])]
    seq1 = [cell(0, [5]), cell(10, [3, 3]), cell(10, [7]), cell(10, [4, 4]), cell(10, [9]), cell(10, [])]
    return [seq0, seq1]


@pytest.mark.parametrize("prec", PRECS)
def test_expansion_at_the_cell_and_chunk_edges(capi, prec):
    """a sequence cell with k = 7 (rows 7 .. 9 zero, dT of the others untouched), one with k = 0 (no reading at all), a skipped
    cell (k = -1, nothing), and cells of REPLAY_CHUNK - 1, REPLAY_CHUNK and REPLAY_CHUNK + 1 entries (the last lane of a
    workgroup's first pass, a full pass, one entry into the second workgroup), each replayed by three trajectories"""
    seqs = _edge_cells()
    seq_of, seeds, sigma = [1, 0, 0], [11, 12, 0xFFFFFFFFFFFFFFFF], (0.01, 0.1, 2e-3, 1e-3)
    bt = capi.Batch(3, 32, 9, 32, _cd(capi, prec))
    bt.replay_alloc(2, 6, 10)
    for f in range(6):
        for s in range(2):
            rd, M, slots, obs, drop, skip = seqs[s][f]
            bt.replay_set_cell(f, s, rd, M, slots, obs, drop, skip=skip)
    bt.replay_assign(seq_of, seeds, sigma)
    bt.replay_commit()
    worst = [0.0]
    for f in range(6):
        base = 0
        for b in range(3):
            rd, M, slots, obs, drop, skip = seqs[seq_of[b]][f]
            ex = bt.replay_expand(f, b)
            assert (ex["n"], ex["drop"], ex["k"]) == (len(M), 0, -1 if skip else len(rd)), (f, b)
            Mp = np.zeros(9, np.int32)
            Mp[:len(M)] = M
            assert np.array_equal(ex["M"], Mp) and np.array_equal(ex["slots"], slots), (f, b)
            assert np.array_equal(ex["off"], base + np.concatenate([[0], np.cumsum(Mp)[:-1]])), (f, b)
            trd, tobs = sc.replay_cell(rd, obs, f, seeds[b], sigma, K=10)
            assert not ex["rd"][len(rd):].any(), (f, b)
            _check_scalars(prec, ex["rd"], ex["obs"], trd, tobs, sigma, (f, b), worst)
            base += len(slots)
    assert [len(seqs[0][f][2]) for f in (2, 3, 4)] == [CHUNK - 1, CHUNK, CHUNK + 1]
    print("worst |device - twin| / sigma (%s): %.3g" % (prec, worst[0]))
    bt.close()


# --------------------------------------------------------------------------- 2. the loop reads what the kernel wrote, bit for bit
@pytest.mark.parametrize("slices", (1, 2))
@pytest.mark.parametrize("cuts", ([(0, 16)], [(0, 5), (5, 16)]), ids=["one_call", "two_calls"])
@pytest.mark.parametrize("prec", PRECS)
def test_replay_runs_the_bits_of_the_ordinary_run_on_its_read_backs(capi, prec, cuts, slices):
    """run_frames_replay against run_frames(0, 16) on a second handle whose ordinary scenario holds the expansion's read-backs:
    snapshot of every trajectory and every frame-log record, with one slice and with exactly two (trajectories 0, 1 | 2, 3, 4)"""
    want = _ordinary(capi, prec)
    bt = _replay_batch(capi, prec)
    bt.set_streams(slices)
    bt.set_slices_exact(slices > 1)
    assert bt.effective_streams() == slices
    _enable_logs(bt, False)
    for f0, f1 in cuts:
        bt.run_frames_replay(f0, f1)
    got = _results(bt, False)
    bt.close()
    assert got["log"].shape == (RL.NF, RL.B, 48) and min(s[4]["n_passed"] for s in got["snap"]) > 0
    _same(got, want)


# ------------------------------------------------------------------------------------------------------- 3. against the oracle
def _readback_trajectory(capi, prec, b):
    reads = _readbacks(capi, prec)
    return RL.NoisyTrajectory(RL.sequences()[RL.SEQ_OF[b]], [_cells_of(reads[f][b]) for f in range(RL.NF)])


def _errs(bt, b, o):
    return H.state_errors(bt.imu_state(b), o.getImuState(), bt.cam_states(b)[0], o.getCamStates()[0], bt.covariance(b), o.getCovariance())


def _stats_equal(bt, b, o, where):
    so, sd = o.lastStats(), bt.last_stats(b)
    for key in H.STAT_KEYS:
        assert so[key] == sd[key], (where, key, so, sd)
    return sd


def test_replay_double_free_running_vs_oracle(capi, po):
    """double, free-running from the first frame, frame by frame: 1e-6 against each trajectory's own oracle on the read-back
    inputs, equal statistics after every update, a passed track on every full-window frame"""
    trs = [_readback_trajectory(capi, "f64", b) for b in range(RL.B)]
    bt = _replay_batch(capi, "f64")
    oracles = []
    for tr in trs:
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        oracles.append(o)
    for f in range(RL.NF):
        bt.run_frames_replay(f, f + 1)
        bt.sync()
        for b, (tr, o) in enumerate(zip(trs, oracles)):
            H.oracle_frame(o, tr, f, RL.N)
            if len(tr.frames[f]["M"]):
                sd = _stats_equal(bt, b, o, (f, b))
                if tr.frames[f]["Nw"] == RL.N:
                    assert sd["n_passed"] > 0 and sd["m_rows"] > 0, (f, b, sd)
            assert bt.num_cam_states(b) == o.getNumCamStates(), (f, b)
            err = _errs(bt, b, o)
            assert H.worst(err) < 1e-6, (f, b, err)
    bt.close()


def test_replay_float_teacher_forced_vs_oracle(capi, po):
    """float: before every frame each trajectory's state and covariance go device -> float oracle, both run the frame on the
    read-back inputs and agree to 1e-3 with equal statistics"""
    trs = [_readback_trajectory(capi, "f32", b) for b in range(RL.B)]
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
            H.oracle_frame(o, tr, f, RL.N)
            if len(tr.frames[f]["M"]):
                passed[b] += _stats_equal(bt, b, o, (f, b))["n_passed"]
            err = _errs(bt, b, o)
            assert H.worst(err) < 1e-3, (f, b, err)
    assert min(passed) > 0, passed
    bt.close()


# --------------------------------------------------------------------------------------------------- 4. seeds and noise levels
@pytest.mark.parametrize("prec", PRECS)
def test_equal_seeds_equal_bits_and_another_seed_not(capi, prec):
    """trajectories 0, 2 and 3 replay sequence 1: 0 and 2 with the same seed and noise levels, 3 with another seed; 1 and 4
    replay sequence 0 with the same seed but other noise levels"""
    seeds = [77, 78, 77, 79, 78]
    sigma = np.tile(np.array(RL.SIGMA), (RL.B, 1))
    sigma[4] *= 0.5
    bt = _replay_batch(capi, prec, seeds=seeds, sigma=sigma)
    bt.run_frames_replay(0, RL.NF)
    bt.sync()
    snap = [H.snapshot(bt, b) for b in range(RL.B)]
    bt.close()
    assert H.same_bits(snap[0], snap[2])
    assert not np.array_equal(snap[0][0], snap[3][0]) and not np.array_equal(snap[1][0], snap[4][0])


@pytest.mark.parametrize("prec", PRECS)
def test_no_noise_is_the_sequence_replicated(capi, prec):
    """sigma = 0 for all: the bits of run_frames on an ordinary scenario that holds each trajectory's noise-free sequence"""
    bt = _replay_batch(capi, prec, sigma=(0.0, 0.0, 0.0, 0.0))
    bt.frame_log_enable(RL.NF)
    bt.run_frames_replay(0, RL.NF)
    got = _results(bt, False)
    bt.close()
    bo = _batch(capi, prec)
    bo.scenario_alloc(RL.NF, sc.IMU_PER_FRAME)
    for f in range(RL.NF):
        for b, s in enumerate(RL.SEQ_OF):
            tr = RL.sequences()[s]
            fr = tr.frames[f]
            bo.scenario_set(f, b, tr.imu_for_frame(f), fr["M"], fr["slots"], fr["obs"], 1 if RL.full(tr, f) else 0)
    bo.scenario_commit()
    bo.frame_log_enable(RL.NF)
    bo.run_frames(0, RL.NF)
    want = _results(bo, False)
    bo.close()
    _same(got, want)
    assert H.same_bits(got["snap"][0], got["snap"][2]) and H.same_bits(got["snap"][1], got["snap"][4])


@pytest.mark.parametrize("prec", PRECS)
def test_a_new_assignment_between_two_runs_takes_effect(capi, prec):
    """frames 0 .. 4 under the common assignment, then other seeds and noise levels for frames 5 .. 15: the bits of an ordinary
    scenario staged from the read-backs under each assignment, and not those of the common assignment throughout.  Then other
    sequences as well (the filters are not run on them: a trajectory does not change its path mid-run): every base moves"""
    seq_b, seeds_b, sigma_b = RL.SEQ_OF, [5, 4, 3, 2, 1], tuple(2.0 * s for s in RL.SIGMA)
    bt = _replay_batch(capi, prec)
    cells = [[bt.replay_expand(f, b) for b in range(RL.B)] for f in range(5)]
    bt.frame_log_enable(RL.NF)
    bt.run_frames_replay(0, 5)
    bt.replay_assign(seq_b, seeds_b, sigma_b)
    cells += [[bt.replay_expand(f, b) for b in range(RL.B)] for f in range(5, RL.NF)]
    bt.run_frames_replay(5, RL.NF)
    got = _results(bt, False)
    seq_c = [0, 1, 1, 0, 1]
    bt.replay_assign(seq_c, seeds_b, sigma_b)
    base = 0
    for b, s in enumerate(seq_c):
        ex, fr = bt.replay_expand(9, b), RL.sequences()[s].frames[9]
        assert ex["off"][0] == base and np.array_equal(ex["slots"], fr["slots"]) and np.array_equal(ex["M"], fr["M"]), b
        base += len(fr["slots"])
    bt.close()
    for b in range(RL.B):
        assert np.array_equal(cells[3][b]["obs"], _readbacks(capi, prec)[3][b]["obs"])
        assert not np.array_equal(cells[9][b]["rd"], _readbacks(capi, prec)[9][b]["rd"])
    bo = _batch(capi, prec)
    _stage_ordinary(bo, cells)
    bo.frame_log_enable(RL.NF)
    bo.run_frames(0, RL.NF)
    want = _results(bo, False)
    bo.close()
    _same(got, want)
    common = _ordinary(capi, prec)
    assert np.array_equal(got["log"][:5], common["log"][:5]) and not np.array_equal(got["log"][5:], common["log"][5:])


# --------------------------------------------------------------------------------------------------------------------- 5. logs
@pytest.mark.parametrize("prec", PRECS)
def test_map_log_and_pruned_log_of_the_replay_equal_the_ordinary_runs(capi, prec):
    """with the map log and the pruned-state log on (every prune then has its own launch): counts, records and augment ordinals
    of the replay, run in two calls on two slices, equal those of the ordinary run on the read-backs"""
    want = _ordinary(capi, prec, logs=True)
    bt = _replay_batch(capi, prec)
    bt.set_streams(2)
    bt.set_slices_exact(True)
    _enable_logs(bt, True)
    bt.run_frames_replay(0, 7)
    bt.run_frames_replay(7, RL.NF)
    assert bt.map_log_frames() == RL.NF and bt.pruned_log_frames() == RL.NF and bt.frame_log_count() == RL.NF
    got = _results(bt, True)
    bt.close()
    _same(got, want)
    for key in ("map_counts", "prn_counts"):
        assert all(np.array_equal(p, q) for p, q in zip(got[key], want[key])), key
    assert min(got["map_counts"][0]) > 0 and min(got["prn_counts"][0]) > 0
    for b in range(RL.B):
        assert np.array_equal(got["map"][b], want["map"][b]), b
        assert np.array_equal(got["prn"][b][0], want["prn"][b][0]) and np.array_equal(got["prn"][b][2], want["prn"][b][2]), b


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_every_refusal_reaches_the_caller_with_its_code(capi):
    EINVAL, E2BIG = r"\(-22\)", r"\(-7\)"
    tr = RL.sequences()[0]
    fr = tr.frames[5]
    bt = _batch(capi, "f32")
    # nothing allocated
    for call in (lambda: bt.replay_commit(), lambda: bt.replay_assign(RL.SEQ_OF, RL.SEEDS, RL.SIGMA)):
        with pytest.raises(capi.HipError, match=EINVAL + ".*no replay allocated"):
            call()
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.run_frames_replay(0, 0)
    for bad in ((0, 4, 10), (2, 0, 10), (2, 4, 0)):
        with pytest.raises(capi.HipError, match=EINVAL + ".*bad replay size"):
            bt.replay_alloc(*bad)
    bt.replay_alloc(2, RL.NF, sc.IMU_PER_FRAME)
    # a cell: its place, the work-list rules, the drop, the cell rule
    ok = (tr.imu_for_frame(5), fr["M"], fr["slots"], fr["obs"], 1)
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay cell out of range"):
        bt.replay_set_cell(RL.NF, 0, *ok)
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay cell out of range"):
        bt.replay_set_cell(0, 2, *ok)
    with pytest.raises(capi.HipError, match=E2BIG + ".*more tracks than f_cap"):
        bt.replay_set_cell(0, 0, ok[0], [3] * 9, np.tile([0, 1, 2], 9), np.zeros((27, 2)), 0)
    with pytest.raises(capi.HipError, match=E2BIG + ".*track longer than m_cap"):
        bt.replay_set_cell(0, 0, ok[0], [7], np.arange(7), np.zeros((7, 2)), 0)
    with pytest.raises(capi.HipError, match=EINVAL + ".*camera slot out of range"):
        bt.replay_set_cell(0, 0, ok[0], [3], [0, 1, 6], np.zeros((3, 2)), 0)
    with pytest.raises(capi.HipError, match=EINVAL + ".*camera slot repeated within a track"):
        bt.replay_set_cell(0, 0, ok[0], [3], [0, 1, 1], np.zeros((3, 2)), 0)
    with pytest.raises(capi.HipError, match=EINVAL + ".*negative n_drop"):
        bt.replay_set_cell(0, 0, ok[0], ok[1], ok[2], ok[3], -1)
    with pytest.raises(capi.HipError, match=EINVAL + ".*IMU sample count k exceeds"):
        bt.replay_set_cell(0, 0, np.zeros((11, 7)), ok[1], ok[2], ok[3], 0)
    with pytest.raises(capi.HipError, match=EINVAL + ".*a skipped cell carries"):
        bt.replay_set_cell(0, 0, ok[0], [], [], np.zeros((0, 2)), 0, skip=True)
    # the assignment
    with pytest.raises(capi.HipError, match=EINVAL + ".*seq_of names no sequence"):
        bt.replay_assign([1, 0, 2, 1, 0], RL.SEEDS, RL.SIGMA)
    with pytest.raises(capi.HipError, match=EINVAL + ".*seq_of names no sequence"):
        bt.replay_assign([1, 0, -1, 1, 0], RL.SEEDS, RL.SIGMA)
    for bad in (-1e-9, float("inf"), float("nan")):
        with pytest.raises(capi.HipError, match=EINVAL + ".*sigma must be finite and not negative"):
            bt.replay_assign(RL.SEQ_OF, RL.SEEDS, (RL.SIGMA[0], bad, RL.SIGMA[2], RL.SIGMA[3]))
    # a run: the range, the commit, the assignment -- in this order
    with pytest.raises(capi.HipError, match=EINVAL + ".*frame range out of bounds"):
        bt.run_frames_replay(0, RL.NF + 1)
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.run_frames_replay(0, RL.NF)
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.replay_expand(0, 0)
    bt.replay_commit()
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not assigned"):
        bt.run_frames_replay(0, RL.NF)
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not assigned"):
        bt.replay_expand(0, 0)
    bt.replay_assign(RL.SEQ_OF, RL.SEEDS, RL.SIGMA)
    for bad in ((-1, 3), (5, 4), (0, RL.NF + 1)):
        with pytest.raises(capi.HipError, match=EINVAL + ".*frame range out of bounds"):
            bt.run_frames_replay(*bad)
    for bad in ((RL.NF, 0), (0, RL.B), (-1, 0)):
        with pytest.raises(capi.HipError, match=EINVAL + ".*replay cell out of range"):
            bt.replay_expand(*bad)
    # a staged replay is no scenario: the ordinary entries still ask for theirs
    for run in (bt.run_frames, bt.run_frames_streamed):
        with pytest.raises(capi.HipError, match=EINVAL + ".*scenario not committed"):
            run(0, 0)
    # and after all the refusals the handle runs (the cells of the refused calls were never staged: the replay is empty frames)
    bt.run_frames_replay(0, 4)
    bt.sync()
    assert [bt.num_cam_states(b) for b in range(RL.B)] == [4] * RL.B
    # a patched cell un-commits
    bt.replay_set_cell(5, 0, *ok)
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.run_frames_replay(0, 1)
    bt.close()
