"""The pruned-state device log of run_frames / run_frames_streamed (msckf_hip_pruned_log_*, kernels_log.hip): a record is the
camera state as the getters read it after the frame's update and before its prune, with its 6 x 6 covariance block; drop
schedules, clamps and skipped cells log what the stage-wise run drops; the filter computes the same bits with the log on or
off; the records follow the double oracle; an overflowing log keeps the first records and goes on counting; the on-device
sums agree with numpy on the read-back; and the refusals refuse."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import pruned_log_ref as R
from msckf_mono_amd import scenario as sc
from test_gpu_configs import _snapshot

pytestmark = pytest.mark.gpu

SMALL = dict(N=8, F=40, B=6, nf=17, m_cap=12)   # the frame-log suite's geometry: two workgroups (4 + 2 wavefronts); three streams make slices of 2
CAP = 32                                        # a log that cannot overflow: 12 states are dropped per trajectory
# schedules without tracks: 12 frames in a window of 16, one schedule per trajectory (9 exceeds the window: it clamps)
SCHED = dict(N=16, F=8, nf=12, m_cap=12,
             drops=[[0, 0, 0, 3, 0, 2, 1, 0, 9, 0, 1, 1], [0] * 12, [1] * 12])


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as mod
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def small_trajs():
    g = SMALL
    return [sc.Trajectory(2, 300 + b, g["N"], g["F"], g["nf"]) for b in range(g["B"])]


@pytest.fixture(scope="module")
def bare_trajs():
    g = SCHED
    return [sc.Trajectory(2, 300 + b, g["N"], 0, g["nf"]) for b in range(3)]


def _dtype(capi, name):
    return capi.F32 if name == "f32" else capi.F64


def _small_drops(trajs, last=3):
    """[frame][trajectory]: 1 when the window is full; `last` on the last frame, where no later work-list depends on it"""
    g = SMALL
    return [[(last if k == g["nf"] - 1 else 1) if tr.frames[k]["Nw"] == g["N"] else 0 for tr in trajs] for k in range(g["nf"])]


def _sched_drops():
    return [[SCHED["drops"][b][k] for b in range(3)] for k in range(SCHED["nf"])]


def _staged(capi, trajs, name, geo, drops, streams=1, skipped=()):
    """a committed resident scenario with drops[frame][trajectory]; skipped: cells (frame, trajectory) without an image"""
    bt = capi.Batch(len(trajs), geo["N"], geo["F"], geo["m_cap"], _dtype(capi, name))
    for b, tr in enumerate(trajs):
        bt.initialize(b, tr.cfg, tr.imu0)
    bt.scenario_alloc(geo["nf"], sc.IMU_PER_FRAME)
    none = np.zeros(0, np.int32)
    for k in range(geo["nf"]):
        for b, tr in enumerate(trajs):
            fr = tr.frames[k]
            if (k, b) in skipped:
                bt.scenario_set(k, b, np.zeros((0, 7)), none, none, np.zeros((0, 2)), 0, skip=True)
            else:
                bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], drops[k][b])
    bt.scenario_commit()
    bt.set_streams(streams)
    return bt


def _logged_run(capi, trajs, name, geo, drops, cuts=None, streamed=False, streams=1, cap=CAP, skipped=()):
    bt = _staged(capi, trajs, name, geo, drops, streams=streams, skipped=skipped)
    bt.pruned_log_enable(cap)
    k = 0
    for n in (cuts or [geo["nf"]]):
        (bt.run_frames_streamed if streamed else bt.run_frames)(k, k + n)
        k += n
        assert bt.pruned_log_frames() == k
    assert k == geo["nf"]
    return bt


_REF = {}


def _reference(capi, trajs, name, geo, drops, tag):
    """Per trajectory the records [n][32] the log must hold, from the stage-wise run: propagate_range, augment_range,
    set_tracks, marginalize_range, then cam_states(b) and covariance(b) by the getters, then drop_oldest_range
    (test_resident_scenario_with_tracks_on_the_newest_camera holds this path bit-identical to run_frames).  Once per dtype."""
    if (tag, name) in _REF:
        return _REF[(tag, name)]
    bt = capi.Batch(len(trajs), geo["N"], geo["F"], geo["m_cap"], _dtype(capi, name))
    recs = [[np.zeros((0, 32))] for _ in trajs]
    for b, tr in enumerate(trajs):
        bt.initialize(b, tr.cfg, tr.imu0)
        for k in range(geo["nf"]):
            fr = tr.frames[k]
            bt.propagate_range(b, 1, tr.imu_for_frame(k)); bt.augment_range(b, 1)
            bt.set_tracks(b, fr["M"], fr["slots"], fr["obs"])
            if len(fr["M"]):
                bt.marginalize_range(b, 1)
            n = bt.num_cam_states(b)
            nd = min(max(drops[k][b], 0), n)
            if not nd:
                continue
            cams, P = bt.cam_states(b)[0], bt.covariance(b)
            assert len(cams) == n and P.shape == (15 + 6 * n, 15 + 6 * n)
            r = np.zeros((nd, 32))
            for j in range(nd):
                r[j, 0:7], r[j, 7], r[j, 8:29], r[j, 29], r[j, 30] = cams[j], k, R.triangle(P, j), n, j
            recs[b].append(r)
            bt.drop_oldest_range(b, 1, nd)
    bt.close()
    _REF[(tag, name)] = [np.concatenate(r) for r in recs]
    return _REF[(tag, name)]


def _assert_log(capi, bt, want, tag, cap=CAP):
    """every field of every record, the counts and the augment ordinals, bit for bit; every state entered the window inside
    the run, one per frame, and leaves it oldest-first: record j of a trajectory is the camera of frame ordinal j"""
    stored, found = bt.pruned_log_counts()
    for b, w in enumerate(want):
        arr, views, aug = bt.pruned_log_read(b)
        assert found[b] == len(w) and stored[b] == min(len(w), cap), (tag, b, stored[b], found[b], len(w))
        for name, sl in capi.PRUNED_LOG_FIELDS.items():
            assert np.array_equal(views[name], w[:cap, sl]), (tag, b, name, np.argwhere(views[name] != w[:cap, sl])[:4])
        assert np.array_equal(arr, w[:cap]), (tag, b)
        assert np.array_equal(aug, np.arange(min(len(w), cap))), (tag, b, aug)


# ------------------------------------------------------------------------------------------------ 1. the log is the state before the prune
@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_the_log_is_the_state_before_the_prune(capi, small_trajs, dtype_name):
    """One state is dropped per frame once the window is full (frames 7 .. 15) and three on the last frame, so that a frame
    with several records carries a real posterior: 12 records per trajectory.  One call, pieces of 3 / 4 / 3 / 7 frames,
    three slices and a streamed run on two slices must hold the bits of the stage-wise run's getters in every field."""
    g = SMALL
    drops = _small_drops(small_trajs)
    want = _reference(capi, small_trajs, dtype_name, g, drops, "small")
    assert all(len(w) == 12 for w in want)
    assert all(np.array_equal(w[:, 7], [7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 16, 16]) and np.array_equal(w[-3:, 30], [0, 1, 2]) for w in want)
    assert all(np.all(w[:, 29] == g["N"]) and np.all(w[:, 31] == 0) for w in want)
    assert all(np.all(w[:, 8:29] != 0) and np.all(w[:, [8, 14, 19, 23, 26, 28]] > 0) for w in want)   # full blocks, positive diagonals
    for cuts, kw in (([g["nf"]], {}), ([3, 4, 3, 7], {}), ([g["nf"]], dict(streams=3)), ([g["nf"]], dict(streamed=True, streams=2))):
        bt = _logged_run(capi, small_trajs, dtype_name, g, drops, cuts, **kw)
        _assert_log(capi, bt, want, (dtype_name, cuts, kw))
        part, _, aug = bt.pruned_log_read(4, 5, 6)                            # a range reads like the whole
        assert np.array_equal(part, want[4][5:11]) and np.array_equal(aug, np.arange(5, 11))
        bt.close()


# ------------------------------------------------------------------------------------------------ 2. drop schedules
@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_drop_schedules_without_tracks(capi, bare_trajs, dtype_name):
    """Three trajectories with empty work-lists: drops 0 0 0 3 0 2 1 0 9 0 1 1 (the 9 clamps to the window's 3), none at all,
    one on every frame from the first (the state augmented on that frame).  Records, order, k, window size, counts and
    ordinals against the stage-wise run with drop_oldest_range; and the same with the last four frames of trajectory 0
    skipped: it logs nothing there (its records are those of the frames before), the others are not touched."""
    g = SCHED
    drops = _sched_drops()
    want = _reference(capi, bare_trajs, dtype_name, g, drops, "sched")
    assert [len(w) for w in want] == [11, 0, 12]
    assert np.array_equal(want[0][:, 7], [3, 3, 3, 5, 5, 6, 8, 8, 8, 10, 11]) and np.array_equal(want[0][:, 30], [0, 1, 2, 0, 1, 0, 0, 1, 2, 0, 0])
    assert np.array_equal(want[0][:, 29], [4, 4, 4, 3, 3, 2, 3, 3, 3, 2, 2]) and np.all(want[2][:, 29] == 1)
    for kw in ({}, dict(streams=3), dict(streamed=True, streams=2)):
        bt = _logged_run(capi, bare_trajs, dtype_name, g, drops, **kw)
        _assert_log(capi, bt, want, (dtype_name, kw))
        bt.close()
    skipped = {(k, 0) for k in range(g["nf"] - 4, g["nf"])}
    cut = [want[0][want[0][:, 7] < g["nf"] - 4], want[1], want[2]]
    assert len(cut[0]) == 6
    for streamed in (False, True):
        bt = _logged_run(capi, bare_trajs, dtype_name, g, drops, streamed=streamed, streams=2, skipped=skipped)
        _assert_log(capi, bt, cut, (dtype_name, "skipped tail", streamed))
        assert bt.num_cam_states(0) == 2                                       # the window of frame 7: nothing came or went since
        bt.close()


# ------------------------------------------------------------------------------------------------ 3. the filter does not notice
def test_the_pruned_log_does_not_disturb_the_filter(capi, small_trajs):
    """Float, two slices: state, camera states, covariance, window size and statistics of all trajectories after
    run_frames(0, nf) are the same bits with the log off (every frame but the last prunes on the downdate), on (every frame
    prunes with its own launch), switched on and off again before the run, and on beside the frame log and the map log."""
    g = SMALL
    drops = _small_drops(small_trajs)

    def final(setup):
        bt = _staged(capi, small_trajs, "f32", g, drops, streams=2)
        setup(bt)
        bt.run_frames(0, g["nf"]); bt.sync()
        out = _snapshot(bt, g["B"]), [bt.num_cam_states(b) for b in range(g["B"])], [bt.last_stats(b) for b in range(g["B"])]
        return bt, out

    def on_then_off(bt):
        bt.pruned_log_enable(CAP); bt.pruned_log_enable(0)

    def all_three(bt):
        bt.frame_log_enable(g["nf"]); bt.map_log_enable(g["nf"] * g["F"]); bt.pruned_log_enable(CAP)

    bt, ref = final(lambda bt: None)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):                       # off: nothing to count
        bt.pruned_log_counts()
    bt.close()
    assert all(n == g["N"] - 3 for n in ref[1]) and all(s["n_passed"] > 0 for s in ref[2])
    for tag, setup in (("on", lambda bt: bt.pruned_log_enable(CAP)), ("on, then off", on_then_off), ("beside the other logs", all_three)):
        bt, got = final(setup)
        if tag == "on, then off":
            assert bt.pruned_log_frames() == 0
        else:
            assert bt.pruned_log_frames() == g["nf"] and np.all(bt.pruned_log_counts()[1] == 12)
        if tag == "beside the other logs":
            assert bt.frame_log_count() == g["nf"] and np.all(bt.map_log_counts()[1] > 0)
        bt.close()
        assert got[1] == ref[1] and got[2] == ref[2], tag
        for b in range(g["B"]):
            for x, y in zip(got[0][b], ref[0][b]):
                assert np.array_equal(x, y), (tag, b)


# ------------------------------------------------------------------------------------------------ 4. against the oracle
def test_records_against_the_double_oracle_free_running(capi, po, small_trajs):
    """One run_frames call with the log on (double); the double oracle walks the frames of trajectories 0 and 4 one by one from
    the same initial state, never re-seeded, and its camera states and covariance are read just before its dropOldest.  Pose
    within DESIGN 3.4's 1e-6 (H.state_errors' conventions: rotation angle, relative L2 of the position), the 6 x 6 block
    within 1e-6 relative in the Frobenius norm.  Measured: 1.1e-12 (angle), 2.4e-12 (position), 6.0e-11 (block)."""
    g = SMALL
    drops = _small_drops(small_trajs)
    bt = _logged_run(capi, small_trajs, "f64", g, drops)
    worst = dict(q=0.0, p=0.0, P=0.0)
    for b in (0, 4):
        arr, views, aug = bt.pruned_log_read(b)
        tr = small_trajs[b]
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        j = 0
        for k in range(g["nf"]):
            o.propagate(tr.imu_for_frame(k))
            o.augmentState(k, tr.frame_times[k])
            fr = tr.frames[k]
            if len(fr["M"]):
                o.setTracks(fr["M"], fr["slots"], fr["obs"])
                o.marginalize()
            if not drops[k][b]:
                continue
            cams, P = o.getCamStates()[0], o.getCovariance()
            for i in range(drops[k][b]):
                r = arr[j]
                assert (r[7], r[29], r[30], aug[j]) == (k, len(cams), i, j), (b, k, i, r[7], r[29], r[30], aug[j])
                errs = dict(q=H.quat_angle(r[0:4], cams[i][0:4]), p=H.rel(r[4:7], cams[i][4:7]), P=H.rel(R.block6(r[8:29]), R.block6(R.triangle(P, i)), 1e-30))
                for name, x in errs.items():
                    worst[name] = max(worst[name], x)
                assert max(errs.values()) < 1e-6, (b, k, i, errs)
                j += 1
            o.dropOldest(drops[k][b])
        assert j == len(arr) == 12
    bt.close()
    print("pruned log vs free-running f64 oracle, worst over 24 records:", {k: "%.2e" % x for k, x in worst.items()})


# ------------------------------------------------------------------------------------------------ 5. overflow
def test_an_overflowing_log_keeps_the_first_records_and_counts_on(capi, bare_trajs):
    """Capacity 4 on the schedules of test 2: trajectory 0 drops three states on frame 3 and two on frame 5, so the limit
    falls inside frame 5's records.  The first four records are kept in order, found counts on, a read beyond stored is
    refused, and reset starts over in the same storage."""
    g = SCHED
    drops = _sched_drops()
    want = _reference(capi, bare_trajs, "f32", g, drops, "sched")
    bt = _logged_run(capi, bare_trajs, "f32", g, drops, streams=2, cap=4)
    stored, found = bt.pruned_log_counts()
    print("pruned log overflow: capacity 4, stored", stored.tolist(), "found", found.tolist())
    assert stored.tolist() == [4, 0, 4] and found.tolist() == [11, 0, 12]
    _assert_log(capi, bt, want, "overflow", cap=4)
    assert bt.pruned_log_read(0)[0][3, 7] == 5 and bt.pruned_log_read(0)[0][3, 30] == 0
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.pruned_log_read(0, 3, 2)
    bt.pruned_log_reset()
    assert bt.pruned_log_frames() == 0 and np.all(bt.pruned_log_counts()[1] == 0)
    bt.close()


# ------------------------------------------------------------------------------------------------ 6. metrics on the device
EXACT, SUMS, NEES = [0, 1, 7, 8, 9], [2, 3, 4, 5], 6      # counts | f64 sums of a dozen terms, and maxima | the sum through the 6 x 6 solves


def _assert_metrics(dev, recs, augs, q0, q1, gt, tag):
    ref, kappa = zip(*[R.numpy_metrics(recs[b], augs[b], b, q0, q1, gt) for b in range(len(recs))])
    ref, kappa = np.stack(ref), max(kappa)
    rel = np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300)
    print("pruned metrics", tag, "max rel diff per column", np.max(rel, axis=0), "largest condition number %.2e" % kappa)
    assert np.array_equal(dev[:, EXACT], ref[:, EXACT]), (tag, dev[:, EXACT], ref[:, EXACT])
    assert np.allclose(dev[:, SUMS], ref[:, SUMS], rtol=1e-12, atol=0), (tag, dev[:, SUMS], ref[:, SUMS])
    assert np.allclose(dev[:, NEES], ref[:, NEES], rtol=100 * kappa * 2.0 ** -53, atol=0), (tag, dev[:, NEES], ref[:, NEES], kappa)
    return ref


@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_device_metrics_equal_numpy_on_the_read_back(capi, small_trajs, dtype_name):
    """k_pruned_metrics against numpy on pruned_log_read's arrays (which test 1 holds to the getters bit for bit), ground truth
    from the trajectories' C_CG[k], p_C[k] (scenario.camera_pose_gt): counts exact, sums and maxima to rtol 1e-12 (a dozen f64
    terms), the NEES sum to 100 kappa 2^-53 with kappa the largest condition number of the read-back blocks (the frame log's
    rule), two calls the same bits, a sub-range of prune ordinals agrees with numpy on that slice, ground truth cut one pose
    short moves exactly each trajectory's last record to "unmatched", and none at all moves every record there.  Measured:
    every sum within 4.4e-16 relative of numpy's, condition numbers up to 229."""
    g = SMALL
    nf, B = g["nf"], g["B"]
    bt = _logged_run(capi, small_trajs, dtype_name, g, _small_drops(small_trajs), streams=2)
    recs, augs = zip(*[bt.pruned_log_read(b)[0::2] for b in range(B)])
    gt = sc.camera_pose_gt(small_trajs, 0, nf)
    dev = bt.pruned_log_metrics(0, nf, gt)
    again = bt.pruned_log_metrics(0, nf, gt)
    assert np.array_equal(dev, again)
    ref = _assert_metrics(dev, recs, augs, 0, nf, gt, dtype_name + " all")
    assert np.all(ref[:, 0] == 12) and np.all(ref[:, 1] == 12) and np.all(ref[:, 7] == 12) and np.all(ref[:, [8, 9]] == 0) and np.all(ref[:, [2, 4, 6]] > 0)
    print("pruned metrics", dtype_name, "position RMSE per trajectory", np.sqrt(dev[:, 2] / dev[:, 1]), "angle RMSE", np.sqrt(dev[:, 4] / dev[:, 1]),
          "mean NEES (6 for a consistent filter)", dev[:, 6] / dev[:, 7])
    _assert_metrics(bt.pruned_log_metrics(9, 16, gt), recs, augs, 9, 16, gt, dtype_name + " [9, 16)")
    short = bt.pruned_log_metrics(0, nf, gt[:11])                             # the last record of every trajectory is the camera of frame 11
    _assert_metrics(short, recs, augs, 0, nf, gt[:11], dtype_name + " one pose short")
    assert np.all(short[:, 9] == 1) and np.all(short[:, 1] == 11) and np.all(short[:, 0] == 12)
    bare = bt.pruned_log_metrics(0, nf)
    bt.close()
    assert np.all(bare[:, 0] == 12) and np.all(bare[:, 9] == 12) and np.all(bare[:, 1:9] == 0)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_reads_beyond_the_log_negative_capacity_and_bad_ground_truth_are_refused(capi, small_trajs):
    g = SMALL
    nf, B = g["nf"], g["B"]
    bt = _staged(capi, small_trajs, "f32", g, _small_drops(small_trajs))
    with pytest.raises(capi.HipError, match=r"\(-22\)"):                       # never enabled
        bt.pruned_log_read(0, 0, 1)
    with pytest.raises(capi.HipError, match=r"\(-22\).*negative"):
        bt.pruned_log_enable(-1)
    bt.pruned_log_enable(CAP)
    bt.run_frames(0, nf - 1)
    stored, found = bt.pruned_log_counts()
    assert bt.pruned_log_frames() == nf - 1 and stored[0] == found[0] == 9
    assert bt.pruned_log_read(0, 8, 1)[0].shape == (1, 32) and bt.pruned_log_read(0, 9, 0)[0].shape == (0, 32)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.pruned_log_read(0, 9, 1)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.pruned_log_read(B, 0, 1)
    gt = sc.camera_pose_gt(small_trajs, 0, nf)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):                       # ordinals not handed out yet
        bt.pruned_log_metrics(0, nf, gt)
    L, out = capi.lib(), np.zeros((B, 10))
    dp = C.POINTER(C.c_double)
    assert L.msckf_hip_pruned_log_metrics(bt.h, 0, nf - 1, None, 3, out.ctypes.data_as(dp)) == -22            # null poses, n_ord > 0
    assert L.msckf_hip_pruned_log_metrics(bt.h, 0, nf - 1, gt.ctypes.data_as(dp), -1, out.ctypes.data_as(dp)) == -22
    with pytest.raises(ValueError):
        bt.pruned_log_metrics(0, nf - 1, gt[:, :B - 1])
    assert np.all(bt.pruned_log_metrics(0, nf - 1, gt)[:, 1] == 9)
    bt.pruned_log_enable(0)
    assert bt.pruned_log_frames() == 0
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.pruned_log_read(0, 0, 0)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.pruned_log_metrics(0, 0)
    bt.run_frames(nf - 1, nf); bt.sync()                                      # a plain run_frames still works
    assert bt.pruned_log_frames() == 0 and bt.num_cam_states(0) == g["N"] - 3
    bt.close()


def test_a_poisoned_handle_refuses_to_read_the_pruned_log(capi, monkeypatch):
    """After a streamed run whose upload failed (MSCKF_HIP_TEST_FAIL_UPLOAD) the slices stopped at different frames: the log of
    that call is as undefined as the states, the counts, reads and metrics return -EIO, the ordinal did not advance."""
    N, F, nf, B = 8, 24, 16, 2
    trajs = [sc.Trajectory(2, 30 + b, N, F, nf) for b in range(B)]
    geo = dict(N=N, F=F, nf=nf, m_cap=N)
    drops = [[1 if tr.frames[k]["Nw"] == N else 0 for tr in trajs] for k in range(nf)]
    monkeypatch.setenv("MSCKF_HIP_TEST_FAIL_UPLOAD", "11")
    bad = _staged(capi, trajs, "f32", geo, drops, streams=2)
    monkeypatch.delenv("MSCKF_HIP_TEST_FAIL_UPLOAD")
    bad.pruned_log_enable(CAP)
    bad.run_frames(0, 9); bad.sync()
    assert bad.pruned_log_read(0)[0].shape[0] == 2
    with pytest.raises(capi.HipError, match=r"\(-5\).*undefined"):
        bad.run_frames_streamed(9, 14)
    assert bad.pruned_log_frames() == 9
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.pruned_log_counts()
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.pruned_log_read(0, 0, 1)
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.pruned_log_metrics(0, 9)
    bad.close()
