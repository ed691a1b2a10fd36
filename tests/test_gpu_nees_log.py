"""The full-state NEES log of the frame loops (msckf_hip_truth_set, msckf_hip_nees_log_*; k_nees_log and k_nees_ensemble of
csrc/kernels_log.hip): every record against the numpy twin on the state read after its frame, the filter and the frame log
undisturbed, the replay's walk added on the device, skipped cells and an indefinite covariance flagged, the ensemble reduction
against numpy on the read-back, and the refusals.  Shapes, the twin's independent check and the bar: tests/nees_lab.py."""
import numpy as np
import pytest

import helpers as H
import nees_lab as NL
import ragged_imu as R
import replay_model_lab as ML
from msckf_mono_amd import scenario as sc
from test_gpu_configs import _resident_batch, _snapshot
from test_gpu_pruned_log import CAP, _small_drops, _staged

pytestmark = pytest.mark.gpu
SMALL = NL.SMALL
CUTS = [3, 4, 3, SMALL["nf"] - 10]


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as mod
    mod.lib()
    return mod


def _dtype(capi, name):
    return capi.F32 if name == "f32" else capi.F64


def _small_batch(capi, trajs, name, streams=1):
    g = SMALL
    return _resident_batch(capi, trajs, g["N"], g["F"], g["nf"], g["m_cap"], _dtype(capi, name), streams=streams)


def _twin_record(bt, b, truth16, f):
    """(the record the twin gives for trajectory b from the getters, kappa(C) of the read-back block)"""
    imu, P = bt.imu_state(b)[:16], bt.covariance(b)[:15, :15]
    cols, not_pd = sc.nees_record(imu, P, truth16)
    return np.concatenate([cols, [f, 1.0 if not_pd else 0.0]]), NL.corr_cond(P)


_REF = {}


def _reference(capi, trajs, name):
    """([nf][B][8], kappa [nf][B]) from one run_frames(k, k + 1) call per frame and the twin on the getters after each; computed
    once per (dtype, batch), shared, never written to"""
    key = (name, len(trajs))
    if key not in _REF:
        nf = SMALL["nf"]
        truth = sc.imu_state_gt(trajs, 0, nf)
        bt = _small_batch(capi, trajs, name)
        rec, kappa = np.zeros((nf, len(trajs), 8)), np.zeros((nf, len(trajs)))
        for k in range(nf):
            bt.run_frames(k, k + 1); bt.sync()
            for b in range(len(trajs)):
                rec[k, b], kappa[k, b] = _twin_record(bt, b, truth[k, b], k)
        bt.close()
        _REF[key] = (rec, kappa)
    return _REF[key]


def _logged_run(capi, trajs, name, cuts=None, streamed=False, streams=1):
    nf = SMALL["nf"]
    bt = _small_batch(capi, trajs, name, streams=streams)
    bt.truth_set(sc.imu_state_gt(trajs, 0, nf))
    bt.nees_log_enable(nf)
    k = 0
    for n in (cuts or [nf]):
        (bt.run_frames_streamed if streamed else bt.run_frames)(k, k + n)
        k += n
        assert bt.nees_log_count() == k
    return bt


def _hold(dev, ref, kappa, tag):
    """columns 0..5 within gpu_bar(kappa) of the twin, columns 6..7 exact; returns the worst difference over its bar"""
    assert dev.shape == ref.shape, tag
    assert np.array_equal(dev[..., 6:], ref[..., 6:]), (tag, np.argwhere(dev[..., 6:] != ref[..., 6:])[:4])
    bar = NL.gpu_bar(kappa)[..., None] * np.abs(ref[..., :6])
    diff = np.abs(dev[..., :6] - ref[..., :6])
    assert np.all(np.isfinite(dev)) and np.all(diff <= bar), (tag, np.argwhere(diff > bar)[:4], float(np.max(diff / np.maximum(bar, 1e-300))))
    return float(np.max(diff / np.maximum(bar, 1e-300)))


# ------------------------------------------------------------------------------------------------ 1. records against the twin
@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_every_record_against_the_twin_on_the_state_after_its_frame(capi, dtype_name):
    """Reference: one run_frames(k, k + 1) call per frame, scenario.nees_record on imu_state / covariance after each.  The
    logged runs -- one call, pieces of 3, 4, 3 and 7 frames, three slices (nb = 2: partial workgroups), streamed on two slices
    -- agree with each other bit for bit and with the reference within gpu_bar(kappa(C)) on columns 0..5, kappa by numpy on the
    read-back block; frame index and flags are exact (no record of this geometry is flagged)."""
    g, trajs = SMALL, NL.small_trajs()
    nf = g["nf"]
    ref, kappa = _reference(capi, trajs, dtype_name)
    # (until the first update, on frame 3, a double filter's biases are the truth's bit for bit: those columns are exactly zero)
    assert np.all(NL.gpu_bar(kappa) <= NL.COND_LIMIT) and np.all(ref[..., 0] > 0) and np.all(ref[4:, :, :6] > 0) and not ref[..., 7].any()
    first = None
    for cuts, kw in (([nf], {}), (CUTS, {}), ([nf], dict(streams=3)), ([4, nf - 4], dict(streamed=True, streams=2))):
        bt = _logged_run(capi, trajs, dtype_name, cuts, **kw)
        arr, views = bt.nees_log_read()
        bt.close()
        assert arr.shape == (nf, g["B"], 8) and np.array_equal(views["frame"][:, :, 0], np.tile(np.arange(nf)[:, None], (1, g["B"])))
        worst = _hold(arr, ref, kappa, (dtype_name, cuts, kw))
        if first is None:
            first = arr
            print("NEES log vs twin", dtype_name, "kappa(C) up to %.3g, worst difference over its bar %.3g" % (kappa.max(), worst))
        assert np.array_equal(arr, first), (dtype_name, cuts, kw, np.argwhere(arr != first)[:4])


@pytest.mark.parametrize("B", [1, 5])
def test_one_wavefront_and_a_second_workgroup_with_one_live_wavefront(capi, B):
    trajs = NL.small_trajs()[:B]
    ref, kappa = _reference(capi, trajs, "f32")
    bt = _logged_run(capi, trajs, "f32")
    arr, _ = bt.nees_log_read()
    part, views = bt.nees_log_read(5, 7, B - 1, 1)
    bt.close()
    _hold(arr, ref, kappa, B)
    assert np.array_equal(part, arr[5:12, B - 1:B]) and np.array_equal(views["nees_p"], arr[5:12, B - 1:B, 5:6])


# ------------------------------------------------------------------------------------------------ 2. the filter does not notice
def test_the_log_does_not_disturb_the_filter_or_the_frame_log(capi):
    """SMALL, float, two slices, the frame log on in both runs: state, covariance, camera states and every frame-log record are
    the same bits with the NEES log on and off"""
    g, trajs = SMALL, NL.small_trajs()
    res = []
    for on in (True, False):
        bt = _small_batch(capi, trajs, "f32", streams=2)
        bt.frame_log_enable(g["nf"])
        if on:
            bt.truth_set(sc.imu_state_gt(trajs, 0, g["nf"]))
            bt.nees_log_enable(g["nf"])
        bt.run_frames(0, 9); bt.run_frames_streamed(9, g["nf"]); bt.sync()
        assert bt.nees_log_count() == (g["nf"] if on else 0) and bt.frame_log_count() == g["nf"]
        res.append((_snapshot(bt, g["B"]), bt.frame_log_read()[0]))
        bt.close()
    assert np.array_equal(res[0][1], res[1][1])
    for b in range(g["B"]):
        for x, y in zip(res[0][0][b], res[1][0][b]):
            assert np.array_equal(x, y), b


# ------------------------------------------------------------------------------------------------ 3. replay with the walk
def _replay_batch(capi, name, nf):
    bt = capi.Batch(ML.B, ML.N_CAP, ML.F_CAP, ML.M_CAP, _dtype(capi, name))
    for b in range(ML.B):
        bt.initialize(b, *ML.init_of(nf, b))
    ML.stage_replay(bt, nf)
    return bt


@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_a_replay_adds_the_walk_to_the_truth(capi, dtype_name):
    """tests/replay_model_lab.py's geometry over 24 frames: truth rows by sequence (constant biases), add_walk = 1.  Reference:
    one run_frames_replay(k, k + 1) call per frame and the twin on the getters, its truth biases from scenario.replay_bias_gt on
    the device's walk table.  The logged run (one call, two slices) is held to gpu_bar(kappa(C)); the skipped cells (sequence
    1, frame 22) carry flag 2 and zeros.  run_frames and run_frames_streamed refuse a truth table that adds the walk."""
    nf = NL.NF_REPLAY
    paths = [ML._paths(nf)[s] for s in ML.SEQ_OF]
    table = NL.replay_truth(nf)
    step = _replay_batch(capi, dtype_name, nf)
    bias = sc.replay_bias_gt(paths, step.replay_walk())
    assert np.any(bias[-1, 0] != bias[0, 0]) and np.all(bias[:, 1] == bias[0, 1])       # dense Q walks, zero walk blocks do not
    ref, kappa = np.zeros((nf, ML.B, 8)), np.ones((nf, ML.B))
    for k in range(nf):
        step.run_frames_replay(k, k + 1); step.sync()
        for b in range(ML.B):
            if ML.k_of(ML.SEQ_OF[b], k) < 0:
                ref[k, b, 6:] = k, 2.0
                continue
            truth16 = np.array(table[k, ML.SEQ_OF[b]])
            truth16[4:7], truth16[10:13] = bias[k, b, 0:3], bias[k, b, 3:6]
            ref[k, b], kappa[k, b] = _twin_record(step, b, truth16, k)
    step.close()
    assert np.all(NL.gpu_bar(kappa) <= NL.COND_LIMIT) and np.count_nonzero(ref[..., 7]) == 2

    bt = _replay_batch(capi, dtype_name, nf)
    bt.set_streams(2)
    bt.truth_set(table, row_of=ML.SEQ_OF, add_walk=True)
    bt.nees_log_enable(nf)
    bt.run_frames_replay(0, 10); bt.run_frames_replay(10, nf)
    arr, _ = bt.nees_log_read()
    print("replay NEES log vs twin", dtype_name, "worst difference over its bar %.3g" % _hold(arr, ref, kappa, dtype_name))
    # the other two frame loops refuse the walk before anything is enqueued: an ordinary scenario of one empty frame is staged for them
    bt.scenario_alloc(1, ML.K)
    for b in range(ML.B):
        bt.scenario_set(0, b, np.zeros((0, 7)), [], [], np.zeros((0, 2)), 0)
    bt.scenario_commit()
    bt.nees_log_reset()
    before = [H.snapshot(bt, b) for b in range(ML.B)]
    for run in (bt.run_frames, bt.run_frames_streamed):
        with pytest.raises(capi.HipError, match=r"\(-22\).*only msckf_hip_run_frames_replay"):
            run(0, 1)
        bt.sync()
        assert bt.nees_log_count() == 0 and all(H.same_bits(H.snapshot(bt, b), before[b]) for b in range(ML.B))
    bt.truth_set(table, row_of=ML.SEQ_OF)                        # without the walk they run
    bt.run_frames(0, 1); bt.sync()
    assert bt.nees_log_count() == 1
    bt.close()


# ------------------------------------------------------------------------------------------------ 4. skipped and k = 0 cells
@pytest.fixture(scope="module")
def ragged_run(capi):
    """tests/ragged_imu.py's set (cells with their own sample count, k = 0 among them, two trajectories with skipped cells) run
    once with the NEES log on, three slices: (the set, records [nf][B][8])"""
    rs = R.RaggedImuSet()
    truth = np.zeros((rs.nf, rs.B, 16))
    for b, tr in enumerate(rs.trajs):
        own = sc.imu_state_gt([tr], 0, rs.nf)[:, 0]
        last = 0
        for f in range(rs.nf):
            last = rs.local[b][f] if rs.local[b][f] is not None else last
            truth[f, b] = own[last]
    bt = rs.batch(capi, capi.F64)
    rs.stage(bt)
    bt.set_streams(3)
    bt.truth_set(truth)
    bt.nees_log_enable(rs.nf)
    bt.run_frames(0, rs.nf)
    arr, _ = bt.nees_log_read()
    final = [_twin_record(bt, b, truth[rs.nf - 1, b], rs.nf - 1) for b in range(rs.B)]
    yield rs, bt, arr, final
    bt.close()


def test_flag_2_is_on_exactly_the_skipped_cells(ragged_run):
    """bit 2 on the cells without an image and nowhere else, their columns 0..5 zero; a cell with k = 0 is an ordinary record;
    the last frame's records of the trajectories that are not skipped there agree with the twin on the final state"""
    rs, _, arr, final = ragged_run
    skipped = np.array([[rs.skipped(b, f) for b in range(rs.B)] for f in range(rs.nf)])
    empty = np.array([[(not rs.skipped(b, f)) and rs.counts[b][rs.local[b][f]] == 0 for b in range(rs.B)] for f in range(rs.nf)])
    assert skipped.sum() == 7 and empty.sum() >= 3
    assert np.array_equal(arr[..., 7] == 2.0, skipped) and not arr[~skipped][:, 7].any()
    assert not arr[skipped][:, :6].any() and np.all(arr[~skipped][:, 0] > 0) and np.all(np.isfinite(arr))
    assert np.array_equal(arr[..., 6], np.tile(np.arange(rs.nf)[:, None], (1, rs.B)))
    for b in range(rs.B):
        if not skipped[-1, b]:
            _hold(arr[-1, b], final[b][0], np.array(final[b][1]), b)


# ------------------------------------------------------------------------------------------------ 5. flag 1
def test_an_indefinite_covariance_is_flagged_and_the_others_are_not_touched(capi):
    """Three filters, one frame with k = 0 and no tracks (only augmentState runs: P_II stays what it is).  With trajectory 1's
    P_II[5][5] negated through set_covariance its record carries flag 1 and zeros; the other two records are the bits of the
    run without it, unflagged, with the state one frame behind its truth."""
    trajs = NL.small_trajs()[:3]
    truth = sc.imu_state_gt(trajs, 0, 1)
    got = []
    for tamper in (False, True):
        bt = capi.Batch(3, SMALL["N"], SMALL["F"], SMALL["m_cap"], capi.F64)
        for b, tr in enumerate(trajs):
            bt.initialize(b, tr.cfg, tr.imu0)
        if tamper:
            P = bt.covariance(1)
            P[5, 5] = -P[5, 5]
            bt.set_covariance(1, P)
        bt.scenario_alloc(1, sc.IMU_PER_FRAME)
        for b in range(3):
            bt.scenario_set(0, b, np.zeros((0, 7)), [], [], np.zeros((0, 2)), 0)
        bt.scenario_commit()
        bt.truth_set(truth)
        bt.nees_log_enable(1)
        bt.run_frames(0, 1)
        got.append(bt.nees_log_read()[0][0])
        bt.close()
    clean, bad = got
    assert not clean[:, 7].any() and np.all(clean[:, [0, 1, 3, 5]] > 0)      # (the biases are still the truth's: columns 2 and 4 are zero)
    assert bad[1, 7] == 1.0 and not bad[1, :6].any()
    assert np.array_equal(bad[[0, 2]], clean[[0, 2]])


# ------------------------------------------------------------------------------------------------ 6. the ensemble reduction
def _numpy_ensemble(arr, group_of, n_groups):
    out = np.zeros((arr.shape[0], n_groups, 14))
    for g in range(n_groups):
        members = arr[:, np.asarray(group_of) == g]
        ok = members[..., 7] == 0
        out[:, g, 0], out[:, g, 1] = ok.sum(1), (~ok).sum(1)
        vals = np.where(ok[..., None], members[..., :6], 0.0)
        out[:, g, 2:8], out[:, g, 8:14] = vals.sum(1), (vals * vals).sum(1)
    return out


def _hold_ensemble(bt, arr, r0, r1, group_of, n_groups):
    dev, anees = bt.nees_log_ensemble(r0, r1, group_of, n_groups)
    again, _ = bt.nees_log_ensemble(r0, r1, group_of, n_groups)
    ref = _numpy_ensemble(arr[r0:r1], group_of, n_groups)
    assert dev.shape == ref.shape and np.array_equal(dev, again)
    assert np.array_equal(dev[..., :2], ref[..., :2])
    assert np.allclose(dev[..., 2:], ref[..., 2:], rtol=1e-12, atol=0), float(np.max(np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300)))
    some = ref[..., 0] > 0
    assert np.array_equal(anees[some], dev[some][:, 2:8] / dev[some][:, 0:1]) and np.all(np.isnan(anees[~some]))
    return dev


def test_the_ensemble_against_numpy_on_the_read_back(ragged_run):
    """The ragged run's records (flag 2 on the skipped cells) in four groups: a member left out with -1, group 2 empty, group 3
    a single member, flagged members in groups 0 and 1 on the frames their trajectory is skipped.  Counts exact, sums rtol
    1e-12 (a handful of terms), two calls the same bits, a sub-range the same as that slice, an empty range empty."""
    rs, bt, arr, _ = ragged_run
    group_of = [0, 0, -1, 1, 1, 0, 3]
    whole = _hold_ensemble(bt, arr, 0, rs.nf, group_of, 4)
    assert not whole[:, 2].any() and np.all(whole[:, 3, 0] == 1)
    assert whole[3, 0, 1] == 1 and whole[3, 0, 0] == 2 and whole[-1, 1, 1] == 1 and whole[0, 0, 0] == 3
    part = _hold_ensemble(bt, arr, 3, 9, group_of, 4)
    assert np.array_equal(part, whole[3:9])
    assert _hold_ensemble(bt, arr, 5, 5, group_of, 4).shape == (0, 4, 14)


def test_a_group_of_66_strides_over_the_64_lanes(capi):
    """B = 70 filters without tracks (N = 4, F = 8, 3 frames), 66 of them in group 0, two in group 1, two left out: lane 0 and
    lane 1 take two trajectories each"""
    B, N, F, nf = 70, 4, 8, 3
    trajs = [sc.Trajectory(2, 700 + b, N, F, nf) for b in range(B)]
    bt = _resident_batch(capi, trajs, N, F, nf, 4, capi.F64, streams=2)
    bt.truth_set(sc.imu_state_gt(trajs, 0, nf))
    bt.nees_log_enable(nf)
    bt.run_frames(0, nf)
    arr, _ = bt.nees_log_read()
    group_of = np.zeros(B, dtype=np.int32)
    group_of[[3, 68]] = 1
    group_of[[0, 65]] = -1
    dev = _hold_ensemble(bt, arr, 0, nf, group_of, 2)
    bt.close()
    assert np.all(dev[:, 0, 0] == 66) and np.all(dev[:, 1, 0] == 2) and not dev[..., 1].any() and np.all(dev[..., 2] > 0)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_the_refusals_refuse(capi):
    """the log on without a truth table, a table shorter than the range, a record range beyond the count, group_of out of
    range, and msckf_hip_truth_set's own: each -EINVAL with its message, nothing run"""
    g, trajs = SMALL, NL.small_trajs()
    nf, B = g["nf"], g["B"]
    truth = sc.imu_state_gt(trajs, 0, nf)
    bt = _small_batch(capi, trajs, "f32", streams=2)
    before = _snapshot(bt, B)

    def untouched():
        bt.sync()
        assert bt.nees_log_count() == 0
        for b, (got, want) in enumerate(zip(_snapshot(bt, B), before)):
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), b

    bt.run_frames(0, 0)                                            # the log off: no truth table is asked for
    bt.nees_log_enable(nf)
    for run in (bt.run_frames, bt.run_frames_streamed):
        with pytest.raises(capi.HipError, match=r"\(-22\).*without a truth table"):
            run(0, 2)
        untouched()
    bt.truth_set(truth[:5])
    for run in (bt.run_frames, bt.run_frames_streamed):
        with pytest.raises(capi.HipError, match=r"\(-22\).*does not cover"):
            run(3, 6)
        untouched()
    for kw, text in ((dict(row_of=[0, 1, 2, 3, 4, 6]), "row_of names no row"), (dict(row_of=[0, 1, 2, 3, 4, -1]), "row_of names no row"),
                     (dict(add_walk=True), "msckf_hip_replay_assign_q")):
        with pytest.raises(capi.HipError, match=r"\(-22\).*" + text):
            bt.truth_set(truth, **kw)
    for at, value, text in (((2, 3, 9), np.nan, "entry not finite"), ((2, 3, 9), np.inf, "entry not finite"),
                            ((4, 1, slice(0, 4)), truth[4, 1, 0:4] * (1.0 + 3e-6), "quaternion norm")):
        wrong = truth.copy()
        wrong[at] = value
        with pytest.raises(capi.HipError, match=r"\(-22\).*" + text):
            bt.truth_set(wrong)
    with pytest.raises(capi.HipError, match=r"\(-22\).*does not cover"):     # every refused table left the five-frame one in place
        bt.run_frames(0, 6)
    untouched()
    bt.run_frames(0, 5)
    assert bt.nees_log_count() == 5
    for r0, n in ((0, 6), (5, 1), (-1, 2)):
        with pytest.raises(capi.HipError, match=r"\(-22\).*record range"):
            bt.nees_log_read(r0, n)
    with pytest.raises(capi.HipError, match=r"\(-22\).*record range"):
        bt.nees_log_ensemble(0, 6, [0] * B, 1)
    for group_of, n_groups, text in (([0, 0, 0, 0, 0, 1], 1, "group_of outside"), ([0, -2, 0, 0, 0, 0], 1, "group_of outside"), ([0] * B, 0, "at least one group")):
        with pytest.raises(capi.HipError, match=r"\(-22\).*" + text):
            bt.nees_log_ensemble(0, 5, group_of, n_groups)
    bt.truth_set(None)                                             # the table freed: the log refuses again
    with pytest.raises(capi.HipError, match=r"\(-22\).*without a truth table"):
        bt.run_frames(5, 6)
    bt.nees_log_enable(0)
    bt.run_frames(5, 6); bt.sync()
    assert bt.nees_log_count() == 0
    bt.close()


CUT = 9


def _log_state(bt):
    return (bt.frame_log_count(), bt.map_log_frames(), bt.pruned_log_frames(), bt.nees_log_count(),
            [x.tolist() for x in bt.map_log_counts()], [x.tolist() for x in bt.pruned_log_counts()])


@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_a_full_nees_log_refuses_the_call_and_leaves_the_other_logs_alone(capi, dtype_name):
    """All four logs on, the NEES log one frame short of the two cuts [0, 9) and [9, 17): the second cut is refused with -ENOSPC
    by run_frames and by run_frames_streamed, and record counts, frame ordinals, cursors, states, covariances and window sizes
    are what they were after the first cut.  After nees_log_reset it runs, and the records of the two cuts are those of one
    uninterrupted run."""
    g, trajs = SMALL, NL.small_trajs()
    nf, B = g["nf"], g["B"]
    whole = _logged_run(capi, trajs, dtype_name)
    ref, _ = whole.nees_log_read()
    whole.close()
    bt = _staged(capi, trajs, dtype_name, g, _small_drops(trajs, last=1), streams=2)
    bt.frame_log_enable(nf); bt.map_log_enable(nf * g["F"]); bt.pruned_log_enable(CAP)
    bt.truth_set(sc.imu_state_gt(trajs, 0, nf))
    bt.nees_log_enable(nf - 1)
    bt.run_frames(0, CUT); bt.sync()
    logs, state, ncam = _log_state(bt), _snapshot(bt, B), [bt.num_cam_states(b) for b in range(B)]
    assert logs[:4] == (CUT, CUT, CUT, CUT)
    for run in (bt.run_frames, bt.run_frames_streamed):
        with pytest.raises(capi.HipError, match=r"\(-28\).*NEES log full"):
            run(CUT, nf)
        bt.sync()
        assert _log_state(bt) == logs, run.__name__
        assert [bt.num_cam_states(b) for b in range(B)] == ncam, run.__name__
        for b, (got, want) in enumerate(zip(_snapshot(bt, B), state)):
            assert all(np.array_equal(x, y) for x, y in zip(got, want)), (run.__name__, b)
    first, _ = bt.nees_log_read()
    bt.nees_log_reset()
    bt.run_frames(CUT, nf); bt.sync()
    assert _log_state(bt)[:4] == (nf, nf, nf, nf - CUT)
    second, _ = bt.nees_log_read()
    bt.close()
    # (a prune with its own launch, which the pruned-state log asks for, computes the bits of one that rides on the downdate)
    assert np.array_equal(np.concatenate([first, second]), ref)


def test_a_poisoned_handle_refuses_to_read_the_log(capi, monkeypatch):
    """after a streamed run whose upload failed (MSCKF_HIP_TEST_FAIL_UPLOAD) nees_log_read, nees_log_ensemble and
    nees_log_enable return -EIO; the count did not advance"""
    N, F, nf, B = 8, 24, 16, 2
    trajs = [sc.Trajectory(2, 30 + b, N, F, nf) for b in range(B)]
    monkeypatch.setenv("MSCKF_HIP_TEST_FAIL_UPLOAD", "11")
    bad = _resident_batch(capi, trajs, N, F, nf, N, capi.F32, streams=2)
    monkeypatch.delenv("MSCKF_HIP_TEST_FAIL_UPLOAD")
    bad.truth_set(sc.imu_state_gt(trajs, 0, nf))
    bad.nees_log_enable(nf)
    bad.run_frames(0, 8); bad.sync()
    assert bad.nees_log_read()[0].shape == (8, B, 8)
    with pytest.raises(capi.HipError, match=r"\(-5\).*undefined"):
        bad.run_frames_streamed(8, 14)
    assert bad.nees_log_count() == 8
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.nees_log_read(0, 8)
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.nees_log_ensemble(0, 8, [0, 0], 1)
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.nees_log_enable(4)
    bad.close()
