"""The per-frame device log of run_frames / run_frames_streamed (msckf_hip_frame_log_*, kernels_log.hip): every record is the
state the getters return after that frame, the filter computes the same bits with the log on or off, the records follow
the oracle frame by frame, the on-device ATE / NEES sums agree with numpy on the read-back, and the refusals refuse."""
import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc
from msckf_mono_amd import shard
from test_gpu_configs import _resident_batch, _snapshot

pytestmark = pytest.mark.gpu

SMALL = dict(N=8, F=40, B=6, nf=8 + 9, m_cap=12)      # test_prune_on_the_downdate_equals_the_separate_prune's geometry
N_FULL_FROM = SMALL["N"] - 1     # from this frame on the window is full before the prune and one state is dropped per frame


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


def _dtype(capi, name):
    return capi.F32 if name == "f32" else capi.F64


def _small_batch(capi, trajs, name, streams=1):
    g = SMALL
    return _resident_batch(capi, trajs, g["N"], g["F"], g["nf"], g["m_cap"], _dtype(capi, name), streams=streams)


def _record_of_state(bt, b):
    """the record k_frame_log must have written for trajectory b, from the getters"""
    imu, P, cams, n = bt.imu_state(b), bt.covariance(b), bt.cam_states(b)[0], bt.num_cam_states(b)
    st = bt.last_stats(b, strict=False)
    rec = np.zeros(48)
    rec[0:16] = imu[0:16]
    rec[16:31] = np.diag(P)[:15]
    rec[31:37] = [P[12, 12], P[12, 13], P[12, 14], P[13, 13], P[13, 14], P[14, 14]]
    rec[37], rec[38], rec[39], rec[40] = n, st["n_tracks"], st["n_passed"], st["error_flags"]
    if n:
        rec[41:48] = cams[0]
    return rec


def _frame_by_frame_records(capi, trajs, name):
    """[nf][B][48] from one run_frames call per frame and the getters after each"""
    g = SMALL
    bt = _small_batch(capi, trajs, name)
    out = np.zeros((g["nf"], g["B"], 48))
    for k in range(g["nf"]):
        bt.run_frames(k, k + 1); bt.sync()
        for b in range(g["B"]):
            out[k, b] = _record_of_state(bt, b)
    bt.close()
    return out


def _logged_run(capi, trajs, name, cuts=None, streamed=False, streams=1):
    g = SMALL
    bt = _small_batch(capi, trajs, name, streams=streams)
    bt.frame_log_enable(g["nf"])
    k = 0
    for n in (cuts or [g["nf"]]):
        (bt.run_frames_streamed if streamed else bt.run_frames)(k, k + n)
        k += n
        assert bt.frame_log_count() == k
    assert k == g["nf"]
    return bt


# ------------------------------------------------------------------------------------------------ 1. the log is the state
@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_every_record_is_the_state_after_its_frame(capi, small_trajs, dtype_name):
    """Reference: one run_frames(k, k + 1) call per frame (no fused frame at all, window size final after every call) and
    imu_state / covariance / cam_states / num_cam_states / last_stats after each.  The logged runs -- one call, pieces of
    3, 4, 3 and nf - 10 frames (odd and even numbers of buffer swaps, a last-frame prune in the middle of the range), three
    slices, streamed on two slices -- must give the SAME BITS in every field of every record: the log kernel is handed the
    covariance buffer that is current after a fused frame and the window size that is still waiting for the next propagate."""
    g = SMALL
    nf = g["nf"]
    ref = _frame_by_frame_records(capi, small_trajs, dtype_name)
    assert np.all(ref[N_FULL_FROM:, :, 37] == g["N"] - 1) and np.all(ref[0, :, 37] == 1)      # empty -> full window
    assert np.any(ref[:, :, 39] > 0) and np.all(ref[:, :, 40] == 0)
    for cuts, kw in (([nf], {}), ([3, 4, 3, nf - 10], {}), ([nf], dict(streams=3)), ([4, nf - 4], dict(streamed=True, streams=2))):
        bt = _logged_run(capi, small_trajs, dtype_name, cuts, **kw)
        arr, views = bt.frame_log_read()
        bt.close()
        assert arr.shape == (nf, g["B"], 48)
        for name, sl in capi.FRAME_LOG_FIELDS.items():
            assert np.array_equal(views[name], ref[:, :, sl]), (dtype_name, cuts, kw, name, np.argwhere(views[name] != ref[:, :, sl])[:4])
        assert np.array_equal(arr, ref), (dtype_name, cuts, kw)


def test_a_range_of_the_log_reads_like_the_whole(capi, small_trajs):
    g = SMALL
    bt = _logged_run(capi, small_trajs, "f32")
    arr, _ = bt.frame_log_read()
    part, views = bt.frame_log_read(5, 7, 2, 3)
    bt.close()
    assert np.array_equal(part, arr[5:12, 2:5]) and np.array_equal(views["p"], arr[5:12, 2:5, 13:16])


# ------------------------------------------------------------------------------------------------ 2. the filter does not notice
def test_the_log_does_not_disturb_the_filter(capi):
    """cfg3 slice (30-camera window, 200 tracks, 16 trajectories, 33 frames, two slices, float): final state, covariance,
    camera states and statistics with the log on and off are the same bits."""
    N, F, B, nf = 30, 200, 16, 33
    trajs = [sc.Trajectory(3, b, N, F, nf) for b in range(B)]
    res = []
    for on in (True, False):
        bt = _resident_batch(capi, trajs, N, F, nf, 32, capi.F32, streams=2)
        if on:
            bt.frame_log_enable(nf)
        bt.run_frames(0, nf); bt.sync()
        assert bt.frame_log_count() == (nf if on else 0)
        res.append((_snapshot(bt, B), [bt.last_stats(b) for b in range(B)]))
        bt.close()
    for b in range(B):
        for x, y in zip(res[0][0][b], res[1][0][b]):
            assert np.array_equal(x, y), b
        assert res[0][1][b] == res[1][1][b], b
    assert all(s["n_passed"] > 150 for s in res[0][1])


# ------------------------------------------------------------------------------------------------ 3. against the oracle
def _record_errors(rec, o):
    """H.state_errors' conventions on what a record holds"""
    imu, P = o.getImuState(), o.getCovariance()
    ppp = np.array([P[12, 12], P[12, 13], P[12, 14], P[13, 13], P[13, 14], P[14, 14]])
    return dict(q=H.quat_angle(rec[0:4], imu[0:4]), bg=H.rel(rec[4:7], imu[4:7]), v=H.rel(rec[7:10], imu[7:10]),
                ba=H.rel(rec[10:13], imu[10:13]), p=H.rel(rec[13:16], imu[13:16]),
                Pii_diag=H.rel(rec[16:31], np.diag(P)[:15], 1e-30), Ppp=H.rel(rec[31:37], ppp, 1e-30))


def _check_record(views, arr, k, b, o, tol, worst, tag):
    errs = _record_errors(arr[k, b], o)
    for key, val in errs.items():
        worst[key] = max(worst.get(key, 0.0), val)
    so = o.lastStats()
    assert views["n_cam"][k, b, 0] == o.getNumCamStates(), (tag, b, k)
    assert (views["n_tracks"][k, b, 0], views["n_passed"][k, b, 0]) == (so["n_tracks"], so["n_passed"]), (tag, b, k, so)
    assert H.worst(errs) < tol, (tag, b, k, errs)


def test_records_against_the_double_oracle_free_running(capi, po, small_trajs):
    """One run_frames call over all 17 frames with the log on; the double oracle walks the frames one by one from the same
    initial state, FREE-RUNNING (never re-seeded), for trajectories 0 and 4.  Every record's q, b_g, v, b_a, p, P_II diagonal
    and P_pp entries stay within DESIGN 3.4's 1e-6 of the oracle's state after that frame (H.state_errors' conventions);
    window size, n_tracks and n_passed are equal.  Measured: worst 1.8e-9 (b_g), P_pp 8.6e-11."""
    g = SMALL
    bt = _logged_run(capi, small_trajs, "f64")
    arr, views = bt.frame_log_read()
    bt.close()
    worst = {}
    for b in (0, 4):
        tr = small_trajs[b]
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        for k in range(g["nf"]):
            H.oracle_frame(o, tr, k, g["N"])
            _check_record(views, arr, k, b, o, 1e-6, worst, "f64 free-running")
    print("frame log vs free-running f64 oracle, worst over 17 frames:", {k: "%.2e" % x for k, x in worst.items()})


def test_records_against_the_float_oracle_frame_by_frame(capi, po, small_trajs):
    """The same in float at DESIGN 3.4's 1e-3, re-seeded every frame (teacher forcing device -> oracle, as
    test_cfg3_batch_of_64_vs_oracle does).  Free-running, the float filter and the float oracle part by 1.68e-3 on b_g
    (trajectory 4, frame 5; every other field below 2e-5 there) -- two float roundings of the weakly observable gyro bias while
    the window fills, which the float oracle shows against the double oracle as well (1.25e-3 on b_g over the same frames,
    printed below), not something the log adds: the record is the filter's state bit for bit (test_every_record_is_the_state_after_its_frame).  So a frame-by-frame
    device run (whose state after every frame IS the logged run's record, asserted here again) seeds a float oracle before each
    frame, both take the frame, and the logged run's record of that frame is held to the oracle's state at 1e-3 (measured:
    1.1e-4 on b_g, 2.2e-5 on b_a, everything else below 6e-6)."""
    g = SMALL
    nf, N = g["nf"], g["N"]
    bt = _logged_run(capi, small_trajs, "f32")
    arr, views = bt.frame_log_read()
    bt.close()
    step = _small_batch(capi, small_trajs, "f32")
    worst = {}
    for k in range(nf):
        oracles = {}
        for b in (0, 4):
            o = po.Oracle(po.F32, po.LEAN)
            o.initialize(small_trajs[b].cfg, small_trajs[b].imu0)
            H.copy_device_to_oracle(step, b, o)
            oracles[b] = o
        step.run_frames(k, k + 1); step.sync()
        for b in (0, 4):
            assert np.array_equal(_record_of_state(step, b), arr[k, b]), (b, k)
            H.oracle_frame(oracles[b], small_trajs[b], k, N)
            _check_record(views, arr, k, b, oracles[b], 1e-3, worst, "f32 teacher-forced")
    step.close()
    print("frame log vs teacher-forced f32 oracle, worst over 17 frames:", {k: "%.2e" % x for k, x in worst.items()})
    # for the record: how far two float roundings of the same filter drift apart free-running -- float oracle against double oracle
    drift = {}
    for b in (0, 4):
        tr = small_trajs[b]
        of, od = po.Oracle(po.F32, po.LEAN), po.Oracle(po.F64, po.LEAN)
        of.initialize(tr.cfg, tr.imu0); od.initialize(tr.cfg, tr.imu0)
        for k in range(nf):
            H.oracle_frame(of, tr, k, N); H.oracle_frame(od, tr, k, N)
            fi, di = of.getImuState(), od.getImuState()
            for key, sl in (("q", None), ("bg", slice(4, 7)), ("v", slice(7, 10)), ("ba", slice(10, 13)), ("p", slice(13, 16))):
                val = H.quat_angle(fi[0:4], di[0:4]) if sl is None else H.rel(fi[sl], di[sl])
                drift[key] = max(drift.get(key, 0.0), val)
    print("free-running float oracle vs double oracle, worst over 17 frames:", {k: "%.2e" % x for k, x in drift.items()})


# ------------------------------------------------------------------------------------------------ 4. metrics on the device
def _numpy_metrics(arr, gt):
    """[B][6] and the largest cond(P_pp), from the read-back"""
    err = arr[:, :, 13:16] - gt
    d2 = np.sum(err * err, axis=2)
    dist = np.sqrt(d2)
    x = arr[:, :, 31:37]
    Ppp = np.stack([np.stack([x[..., 0], x[..., 1], x[..., 2]], -1), np.stack([x[..., 1], x[..., 3], x[..., 4]], -1),
                    np.stack([x[..., 2], x[..., 4], x[..., 5]], -1)], -2)
    nees = np.einsum("rbi,rbi->rb", err, np.linalg.solve(Ppp, err[..., None])[..., 0])
    out = np.stack([np.full(arr.shape[1], float(arr.shape[0])), d2.sum(0), np.max(dist, axis=0), dist[-1], nees.sum(0),
                    np.sum(arr[:, :, 40] != 0, axis=0).astype(np.float64)], 1)
    return out, float(np.max(np.linalg.cond(Ppp)))


@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_device_metrics_equal_numpy_on_the_read_back(capi, small_trajs, dtype_name):
    """k_log_metrics against numpy on frame_log_read's array (which test 1 holds to the state bit for bit), ground truth from
    the trajectories: the only differences are the order of the f64 sums and the 3 x 3 solve.  n, flagged records, max and
    final error, sum |e|^2: rtol 1e-12 (n eps for tens of terms); sum of NEES: rtol 100 kappa 2^-53 with kappa the largest
    cond(P_pp) over the records (required < 1e8).  Two calls give the same bits; a sub-range agrees with numpy on that slice;
    shard.ate_from_log_metrics gives ate_local's accumulator over all logged frames."""
    g = SMALL
    nf, B = g["nf"], g["B"]
    gt = np.stack([tr.gt_frames["p"][:nf] for tr in small_trajs], axis=1)          # [nf][B][3]
    bt = _logged_run(capi, small_trajs, dtype_name, streams=2)
    arr, _ = bt.frame_log_read()
    for r0, r1 in ((0, nf), (3, 11), (nf - 1, nf)):
        dev = bt.frame_log_metrics(r0, r1, gt[r0:r1])
        again = bt.frame_log_metrics(r0, r1, gt[r0:r1])
        ref, kappa = _numpy_metrics(arr[r0:r1], gt[r0:r1])
        print("metrics", dtype_name, (r0, r1), "kappa %.3g" % kappa, "max rel diff per column", np.max(np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300), axis=0))
        assert np.array_equal(dev, again), (r0, r1)
        assert kappa < 1e8, kappa
        assert np.array_equal(dev[:, 0], ref[:, 0]) and np.array_equal(dev[:, 5], ref[:, 5])
        assert np.allclose(dev[:, 1:4], ref[:, 1:4], rtol=1e-12, atol=0), (r0, r1, dev[:, 1:4], ref[:, 1:4])
        assert np.allclose(dev[:, 4], ref[:, 4], rtol=100 * kappa * 2.0 ** -53, atol=0), (r0, r1, dev[:, 4], ref[:, 4], kappa)
    dev = bt.frame_log_metrics(0, nf, gt)
    bt.close()
    assert np.all(dev[:, 1] > 0) and np.all(dev[:, 4] > 0)
    seq = [b % 2 for b in range(B)]
    acc = shard.ate_from_log_metrics(dev, seq, 2)
    want = shard.ate_local([arr[:, b, 13:16] for b in range(B)], [gt[:, b] for b in range(B)], seq, 2)
    assert np.array_equal(acc[:, 1], want[:, 1]) and np.allclose(acc[:, 0], want[:, 0], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_a_full_log_refuses_the_call_and_runs_nothing(capi, small_trajs):
    """-ENOSPC before anything is enqueued: state, covariance, camera states and the cursor are as before the refused call
    (resident and streamed).  A read beyond the cursor is -EINVAL.  After frame_log_reset the same storage takes a second
    run, whose records are those of an uninterrupted run; frame_log_enable(0) after use leaves a plain run_frames working."""
    g = SMALL
    nf, B = g["nf"], g["B"]
    whole = _logged_run(capi, small_trajs, "f32")
    ref, _ = whole.frame_log_read()
    whole.sync()
    ref_final = _snapshot(whole, B)
    whole.close()
    bt = _small_batch(capi, small_trajs, "f32", streams=2)
    bt.frame_log_enable(10)
    bt.run_frames(0, 8); bt.sync()
    before = _snapshot(bt, B)
    for go in (bt.run_frames, bt.run_frames_streamed):
        with pytest.raises(capi.HipError, match=r"\(-28\)"):
            go(8, 12)
        bt.sync()
        assert bt.frame_log_count() == 8
        for b in range(B):
            for x, y in zip(_snapshot(bt, B)[b], before[b]):
                assert np.array_equal(x, y), b
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.frame_log_read(5, 4)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.frame_log_metrics(0, 9, np.zeros((9, B, 3)))
    first, _ = bt.frame_log_read()
    assert np.array_equal(first, ref[:8])
    bt.frame_log_reset()
    assert bt.frame_log_count() == 0
    bt.run_frames(8, 12); bt.run_frames_streamed(12, nf - 1)
    assert bt.frame_log_count() == nf - 9
    second, _ = bt.frame_log_read()
    assert np.array_equal(second, ref[8:nf - 1])
    bt.frame_log_enable(0)
    assert bt.frame_log_count() == 0
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.frame_log_read(0, 1)
    bt.run_frames(nf - 1, nf); bt.sync()
    for b in range(B):
        for x, y in zip(_snapshot(bt, B)[b], ref_final[b]):
            assert np.array_equal(x, y), b
    bt.close()


def test_a_poisoned_handle_refuses_to_read_the_log(capi, monkeypatch):
    """After a streamed run whose upload failed (MSCKF_HIP_TEST_FAIL_UPLOAD) the slices stopped at different frames: the log of
    that call is as undefined as the states, frame_log_read and frame_log_metrics return -EIO, the cursor did not advance."""
    N, F, nf, B = 8, 24, 16, 2
    trajs = [sc.Trajectory(2, 30 + b, N, F, nf) for b in range(B)]
    monkeypatch.setenv("MSCKF_HIP_TEST_FAIL_UPLOAD", "11")
    bad = _resident_batch(capi, trajs, N, F, nf, N, capi.F32, streams=2)
    monkeypatch.delenv("MSCKF_HIP_TEST_FAIL_UPLOAD")
    bad.frame_log_enable(nf)
    bad.run_frames(0, 8); bad.sync()
    assert bad.frame_log_read()[0].shape == (8, B, 48)
    with pytest.raises(capi.HipError, match=r"\(-5\).*undefined"):
        bad.run_frames_streamed(8, 14)
    assert bad.frame_log_count() == 8
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.frame_log_read(0, 8)
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.frame_log_metrics(0, 8, np.zeros((8, B, 3)))
    bad.close()
