"""The per-track device log of run_frames / run_frames_streamed (msckf_hip_map_log_*, kernels_log.hip): the records are what
last_tracks returns after every frame, compacted in track order; the filter computes the same bits with the log on or off;
the landmarks and gate statistics follow the double oracle; an overflowing log keeps the first records and goes on counting;
the on-device sums agree with numpy on the read-back; a skipped cell logs nothing; and the refusals refuse."""
import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc
from test_gpu_configs import _resident_batch, _snapshot

pytestmark = pytest.mark.gpu

GEO = dict(N=8, F=150, nf=12, m_cap=12)      # F = 150: three chunks of 64 + 64 + 22 tracks per wavefront
CAP = GEO["nf"] * GEO["F"]                   # a log that cannot overflow
FAR_B = 5                                    # a second workgroup with one wavefront; three streams make slices of 1, 2, 2


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as mod
    mod.lib()
    return mod


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def far_trajs():
    """landmarks 20 to 200 m deep: low parallax, so that motion check, triangulation and gate reject tracks in every chunk"""
    g = GEO
    return [sc.Trajectory(2, 300 + b, g["N"], g["F"], g["nf"], depth_range=(20.0, 200.0)) for b in range(FAR_B)]


@pytest.fixture(scope="module")
def wide_trajs():
    g = GEO
    return [sc.Trajectory(2, s, g["N"], g["F"], g["nf"]) for s in (300, 302)]


def _dtype(capi, name):
    return capi.F32 if name == "f32" else capi.F64


def _batch(capi, trajs, name, streams=1):
    g = GEO
    return _resident_batch(capi, trajs, g["N"], g["F"], g["nf"], g["m_cap"], _dtype(capi, name), streams=streams)


def _logged_run(capi, trajs, name, cuts=None, streamed=False, streams=1, cap=CAP):
    nf = GEO["nf"]
    bt = _batch(capi, trajs, name, streams=streams)
    bt.map_log_enable(cap)
    k = 0
    for n in (cuts or [nf]):
        (bt.run_frames_streamed if streamed else bt.run_frames)(k, k + n)
        k += n
        assert bt.map_log_frames() == k
    assert k == nf
    return bt


def _read_all(bt, B):
    """([records of trajectory b], stored, found)"""
    stored, found = bt.map_log_counts()
    return [bt.map_log_read(b)[0] for b in range(B)], stored, found


_REF = {}


def _reference(capi, trajs, name):
    """per trajectory the records [n][8] the log must hold, from one run_frames(k, k + 1) call per frame with last_tracks(b)
    (rows: motion_ok tri_valid gate_pass included gamma p_f_G) and the frame's M after each; computed once per dtype"""
    if name in _REF:
        return _REF[name]
    nf, B = GEO["nf"], len(trajs)
    bt = _batch(capi, trajs, name)
    recs = [[] for _ in range(B)]
    for k in range(nf):
        bt.run_frames(k, k + 1); bt.sync()
        for b, tr in enumerate(trajs):
            M = tr.frames[k]["M"]
            if not len(M):
                recs[b].append(np.zeros((0, 8)))
                continue
            lt = bt.last_tracks(b)
            assert len(lt) == len(M), (k, b)
            t = np.nonzero((lt[:, 0] > 0) & (lt[:, 1] > 0))[0]
            r = np.zeros((len(t), 8))
            r[:, 0:3], r[:, 3], r[:, 4], r[:, 5] = lt[t, 5:8], lt[t, 4], k, t
            r[:, 6], r[:, 7] = (lt[t, 2] > 0) * 1 + (lt[t, 3] > 0) * 2, M[t]
            recs[b].append(r)
    bt.close()
    _REF[name] = recs
    return recs


_PLAIN = {}


def _plain_final(capi, trajs):
    """FAR, f32, two slices, no log: the final snapshot and statistics, computed once"""
    if "x" not in _PLAIN:
        nf, B = GEO["nf"], len(trajs)
        bt = _batch(capi, trajs, "f32", streams=2)
        bt.run_frames(0, nf); bt.sync()
        assert bt.map_log_frames() == 0
        _PLAIN["x"] = (_snapshot(bt, B), [bt.last_stats(b) for b in range(B)])
        bt.close()
    return _PLAIN["x"]


def _same_state(bt, B, ref_snap):
    snap = _snapshot(bt, B)
    for b in range(B):
        for x, y in zip(snap[b], ref_snap[b]):
            assert np.array_equal(x, y), b


# ------------------------------------------------------------------------------------------------ 1. the log is the getters
@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_the_log_is_what_last_tracks_returns_after_every_frame(capi, far_trajs, dtype_name):
    """Reference: one run_frames(k, k + 1) call per frame, last_tracks(b) and the frame's M after each.  The logged runs --
    one call, pieces of 3, 4 and nf - 7 frames, three slices (1, 2 and 2 trajectories), streamed on two slices (work-list
    counts read from the staging ring) -- must hold the SAME BITS in every field, the same stored and found counts, and
    have handed out nf frame ordinals.  The deep landmarks make the device reject tracks: every trajectory has a frame that
    keeps at most 145 of its 150 tracks, so ranks differ from track indices in the later chunks."""
    nf, F = GEO["nf"], GEO["F"]
    ref = _reference(capi, far_trajs, dtype_name)
    kept = np.array([[len(r) for r in ref[b]] for b in range(FAR_B)])
    print("map log", dtype_name, "kept per frame:", kept.tolist())
    assert np.all(kept[:, :3] == 0) and np.all(kept[:, 3:] > 0)              # the window holds four cameras from frame 3 on
    assert np.all(np.min(np.where(kept > 0, kept, F), axis=1) <= 145), kept
    want = [np.concatenate(ref[b]) for b in range(FAR_B)]
    assert all(np.any(w[:, 6] == 3) for w in want)                           # gate passed and included
    for cuts, kw in (([nf], {}), ([3, 4, nf - 7], {}), ([nf], dict(streams=3)), ([nf], dict(streamed=True, streams=2))):
        bt = _logged_run(capi, far_trajs, dtype_name, cuts, **kw)
        assert bt.map_log_frames() == nf
        stored, found = bt.map_log_counts()
        for b in range(FAR_B):
            arr, views = bt.map_log_read(b)
            assert stored[b] == found[b] == len(want[b]), (dtype_name, cuts, kw, b, stored[b], found[b], len(want[b]))
            for name, sl in capi.MAP_LOG_FIELDS.items():
                assert np.array_equal(views[name], want[b][:, sl]), (dtype_name, cuts, kw, b, name, np.argwhere(views[name] != want[b][:, sl])[:4])
            assert np.array_equal(arr, want[b]), (dtype_name, cuts, kw, b)
        part, _ = bt.map_log_read(2, 70, 130)                                # a range reads like the whole
        assert np.array_equal(part, want[2][70:200])
        bt.close()


# ------------------------------------------------------------------------------------------------ 2. the filter does not notice
def test_the_map_log_does_not_disturb_the_filter(capi, far_trajs):
    """FAR, float, two slices: final state, covariance, camera states and statistics with the log on and off are the same bits"""
    nf = GEO["nf"]
    off_snap, off_stats = _plain_final(capi, far_trajs)
    bt = _logged_run(capi, far_trajs, "f32", streams=2)
    bt.sync()
    _same_state(bt, FAR_B, off_snap)
    assert [bt.last_stats(b) for b in range(FAR_B)] == off_stats
    assert bt.map_log_frames() == nf and np.all(bt.map_log_counts()[1] > 0)
    bt.close()


# ------------------------------------------------------------------------------------------------ 3. against the oracle
def test_records_against_the_double_oracle_free_running(capi, po, wide_trajs):
    """One run_frames call over all frames with the log on (double); the double oracle walks the frames one by one from the same
    initial state, never re-seeded.  After each frame the trajectory's records with that ordinal carry the track indices of
    the oracle's lastTracks rows with motion and triangulation ok; p_f_G within 1e-6 absolute, gamma within rtol 1e-6 /
    atol 1e-9 (H.check_tracks' double bars); gate and inclusion flags and M equal; and the records' points are the oracle's
    getMap() rows of that frame, in order.  Measured: 3.4e-7 on p_f_G, 8.7e-10 on gamma; the oracle drops 8 of the 2 700 tracks."""
    nf, N, F = GEO["nf"], GEO["N"], GEO["F"]
    bt = _logged_run(capi, wide_trajs, "f64")
    recs, stored, found = _read_all(bt, len(wide_trajs))
    bt.close()
    assert np.array_equal(stored, found)
    worst_p, worst_g, dropped = 0.0, 0.0, 0
    for b, tr in enumerate(wide_trajs):
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        maps = []
        for k in range(nf):
            H.oracle_frame(o, tr, k, N)
            r = recs[b][recs[b][:, 4] == k]
            if not len(tr.frames[k]["M"]):
                assert len(r) == 0, (b, k)
                continue
            to = o.lastTracks()
            ok = np.nonzero((to[:, 0] > 0) & (to[:, 1] > 0))[0]
            dropped += F - len(ok)
            assert np.array_equal(r[:, 5], ok), (b, k, len(r), len(ok))
            worst_p = max(worst_p, float(np.abs(r[:, 0:3] - to[ok, 5:8]).max()))
            worst_g = max(worst_g, float((np.abs(r[:, 3] - to[ok, 4]) / (1e-9 / 1e-6 + np.abs(to[ok, 4]))).max()))
            assert np.allclose(r[:, 0:3], to[ok, 5:8], rtol=0, atol=1e-6), (b, k)
            assert np.allclose(r[:, 3], to[ok, 4], rtol=1e-6, atol=1e-9), (b, k)
            assert np.array_equal(r[:, 6], (to[ok, 2] > 0) * 1 + (to[ok, 3] > 0) * 2), (b, k)
            assert np.array_equal(r[:, 7], tr.frames[k]["M"][ok]), (b, k)
            maps.append(o.getMap())
        whole = np.concatenate(maps)
        assert whole.shape == recs[b][:, 0:3].shape, (b, whole.shape, recs[b].shape)
        assert np.allclose(recs[b][:, 0:3], whole, rtol=0, atol=1e-6), b
        assert np.all(np.diff(recs[b][:, 4]) >= 0)                           # frame order, track order inside a frame
    print("map log vs free-running f64 oracle: worst |p - p_oracle| %.2e, worst gamma error / (1e-3 + |gamma|) %.2e, tracks the oracle dropped %d"
          % (worst_p, worst_g, dropped))


# ------------------------------------------------------------------------------------------------ 4. overflow
def test_an_overflowing_log_keeps_the_first_records_and_counts_on(capi, far_trajs):
    """Capacity from the reference run of trajectory 0: its records of the first frame with tracks plus half of the next
    frame's, so the limit falls inside a frame.  stored == capacity where found > capacity, found is the full run's, the
    stored records are the full run's first `capacity`, and the final filter state is the same bits as without the log."""
    ref = _reference(capi, far_trajs, "f32")
    kept0 = [len(r) for r in ref[0]]
    k1 = next(k for k, n in enumerate(kept0) if n)
    cap = kept0[k1] + kept0[k1 + 1] // 2
    assert kept0[k1] < cap < kept0[k1] + kept0[k1 + 1]
    want = [np.concatenate(ref[b]) for b in range(FAR_B)]
    bt = _logged_run(capi, far_trajs, "f32", streams=2, cap=cap)
    recs, stored, found = _read_all(bt, FAR_B)
    print("map log overflow: capacity", cap, "stored", stored.tolist(), "found", found.tolist())
    for b in range(FAR_B):
        assert found[b] == len(want[b]) and found[b] > cap, (b, found[b], len(want[b]))
        assert stored[b] == cap
        assert np.array_equal(recs[b], want[b][:cap]), b
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.map_log_read(0, cap - 1, 2)
    bt.sync()
    _same_state(bt, FAR_B, _plain_final(capi, far_trajs)[0])
    bt.map_log_reset()                                                        # the cursors and the ordinal start over, the storage stays
    assert bt.map_log_frames() == 0 and np.all(bt.map_log_counts()[1] == 0)
    bt.close()


# ------------------------------------------------------------------------------------------------ 5. metrics on the device
def _numpy_metrics(arr, b, B, q0, q1, gt):
    """the eight columns of map_log_metrics for trajectory b, from the read-back"""
    r = arr[(arr[:, 4] >= q0) & (arr[:, 4] < q1)]
    out = np.zeros(8)
    out[0] = len(r)
    if gt is not None:
        xyz, off = gt
        cell = (r[:, 4].astype(np.int64) - q0) * B + b
        trk = r[:, 5].astype(np.int64)
        o0, ln = off[cell].astype(np.int64), off[cell + 1] - off[cell]
        m = trk < ln
        err = r[m, 0:3] - xyz[o0[m] + trk[m]]
        d2 = np.sum(err * err, axis=1)
        out[1], out[2], out[3], out[7] = m.sum(), d2.sum(), (np.sqrt(d2).max() if m.any() else 0.0), (~m).sum()
    fl = r[:, 6].astype(np.int64)
    g = ((fl & 1) != 0) & ((fl & 4) == 0)
    out[4], out[5], out[6] = g.sum(), r[g, 3].sum(), (2 * r[g, 7] - 3).sum()
    return out


EXACT, SUMS = [0, 1, 4, 6, 7], [2, 3, 5]      # counts and sums of integers | f64 sums of a few thousand terms, and a maximum


def _assert_metrics(dev, recs, B, q0, q1, gt, tag):
    ref = np.stack([_numpy_metrics(recs[b], b, B, q0, q1, gt) for b in range(B)])
    print("map metrics", tag, "max rel diff per column", np.max(np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-300), axis=0))
    assert np.array_equal(dev[:, EXACT], ref[:, EXACT]), (tag, dev[:, EXACT], ref[:, EXACT])
    assert np.allclose(dev[:, SUMS], ref[:, SUMS], rtol=1e-12, atol=0), (tag, dev[:, SUMS], ref[:, SUMS])
    return ref


@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_device_metrics_equal_numpy_on_the_read_back(capi, far_trajs, dtype_name):
    """k_map_metrics against numpy on map_log_read's arrays (which test 1 holds to the getters bit for bit), ground truth from
    scenario.landmark_csr: counts exact, sums to rtol 1e-12 (f64, a few thousand terms: n eps is 1e-13), two calls the same
    bits, a sub-range of ordinals agrees with numpy on that slice, null ground truth zeroes columns 1-3 and 7 and leaves the
    rest, and a CSR cell shortened by 3 moves exactly its last three tracks' records to column 7.  Measured: every sum within
    3.8e-16 relative of numpy's."""
    nf, F, B = GEO["nf"], GEO["F"], FAR_B
    bt = _logged_run(capi, far_trajs, dtype_name, streams=2)
    recs, _, _ = _read_all(bt, B)
    gt = sc.landmark_csr(far_trajs, 0, nf)
    dev = bt.map_log_metrics(0, nf, gt)
    again = bt.map_log_metrics(0, nf, gt)
    assert np.array_equal(dev, again)
    ref = _assert_metrics(dev, recs, B, 0, nf, gt, dtype_name + " all")
    assert np.all(ref[:, 0] == ref[:, 1]) and np.all(ref[:, 7] == 0) and np.all(ref[:, 2] > 0) and np.all(ref[:, 4] > 0)
    print("map metrics", dtype_name, "landmark RMSE per trajectory", np.sqrt(dev[:, 2] / dev[:, 1]), "mean normalised gate statistic", dev[:, 5] / dev[:, 6])
    _assert_metrics(bt.map_log_metrics(4, 9, sc.landmark_csr(far_trajs, 4, 9)), recs, B, 4, 9, sc.landmark_csr(far_trajs, 4, 9), dtype_name + " [4, 9)")
    bare = bt.map_log_metrics(0, nf)
    assert np.all(bare[:, [1, 2, 3, 7]] == 0) and np.array_equal(bare[:, [0, 4, 5, 6]], dev[:, [0, 4, 5, 6]])
    # a cell whose last three tracks are all logged, with three landmarks fewer
    xyz, off = gt
    pick = next((k, b) for k in range(3, nf) for b in range(B)
                if np.sum((recs[b][:, 4] == k) & (recs[b][:, 5] >= F - 3)) == 3)
    k, b = pick
    cell = k * B + b
    short = (np.delete(xyz, np.arange(off[cell + 1] - 3, off[cell + 1]), axis=0), np.concatenate([off[:cell + 1], off[cell + 1:] - 3]).astype(np.int32))
    cut = bt.map_log_metrics(0, nf, short)
    bt.close()
    _assert_metrics(cut, recs, B, 0, nf, short, dtype_name + " short cell")
    assert cut[b, 7] == 3 and cut[b, 1] == dev[b, 1] - 3 and cut[b, 0] == dev[b, 0]
    others = [i for i in range(B) if i != b]
    assert np.array_equal(cut[others], dev[others]) and np.array_equal(cut[b, 4:7], dev[b, 4:7])


# ------------------------------------------------------------------------------------------------ 6. a skipped tail
def _staged(capi, trajs, skip_from):
    """_resident_batch's staging in float, with the cells of trajectory 1 skipped from frame skip_from on"""
    g = GEO
    N, nf = g["N"], g["nf"]
    bt = capi.Batch(len(trajs), N, g["F"], g["m_cap"], capi.F32)
    for b, tr in enumerate(trajs):
        bt.initialize(b, tr.cfg, tr.imu0)
    bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    none = np.zeros(0, np.int32)
    for k in range(nf):
        for b, tr in enumerate(trajs):
            fr = tr.frames[k]
            if b == 1 and k >= skip_from:
                bt.scenario_set(k, b, np.zeros((0, 7)), none, none, np.zeros((0, 2)), 0, skip=True)
            else:
                bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    bt.set_streams(2)
    return bt


def test_a_skipped_tail_logs_nothing(capi, far_trajs):
    """Two trajectories, the second skipped from frame 9 on (its per-track arrays still hold frame 8's results): resident and
    streamed, its records are the unskipped run's up to frame 8 and hold no ordinal >= 9, the first trajectory's records are
    the bits of the unskipped run, and the ordinal advances over the skipped frames."""
    nf, skip_from = GEO["nf"], 9
    trajs = far_trajs[:2]
    bt = _staged(capi, trajs, nf)                                            # nothing skipped
    bt.map_log_enable(CAP)
    bt.run_frames(0, nf)
    full, _, _ = _read_all(bt, 2)
    bt.close()
    assert np.any(full[1][:, 4] >= skip_from)
    for streamed in (False, True):
        bt = _staged(capi, trajs, skip_from)
        bt.map_log_enable(CAP)
        (bt.run_frames_streamed if streamed else bt.run_frames)(0, nf)
        assert bt.map_log_frames() == nf
        recs, stored, found = _read_all(bt, 2)
        bt.close()
        assert np.array_equal(stored, found), streamed
        assert np.array_equal(recs[0], full[0]), streamed
        assert not np.any(recs[1][:, 4] >= skip_from), streamed
        assert np.array_equal(recs[1], full[1][full[1][:, 4] < skip_from]), streamed


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_reads_beyond_the_log_and_bad_ground_truth_are_refused(capi, wide_trajs):
    nf, B = GEO["nf"], len(wide_trajs)
    bt = _batch(capi, wide_trajs, "f32")
    with pytest.raises(capi.HipError, match=r"\(-22\)"):                      # never enabled
        bt.map_log_read(0, 0, 1)
    bt.map_log_enable(CAP)
    bt.run_frames(0, nf - 1)
    stored, found = bt.map_log_counts()
    assert bt.map_log_frames() == nf - 1 and stored[0] == found[0] > 0
    assert bt.map_log_read(0, int(stored[0]) - 1, 1)[0].shape == (1, 8) and bt.map_log_read(0, int(stored[0]), 0)[0].shape == (0, 8)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.map_log_read(0, int(stored[0]), 1)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.map_log_read(B, 0, 1)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):                      # ordinals not handed out yet
        bt.map_log_metrics(0, nf)
    xyz, off = sc.landmark_csr(wide_trajs, 0, nf - 1)
    bad = off.copy()
    bad[7] = bad[8] + 1                                                       # decreases between cells 7 and 8
    with pytest.raises(capi.HipError, match=r"\(-22\).*decreases"):
        bt.map_log_metrics(0, nf - 1, (xyz, bad))
    assert bt.map_log_metrics(0, nf - 1, (xyz, off))[0, 0] == stored[0]
    bt.map_log_enable(0)
    assert bt.map_log_frames() == 0
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.map_log_read(0, 0, 0)
    with pytest.raises(capi.HipError, match=r"\(-22\)"):
        bt.map_log_metrics(0, 0)
    bt.run_frames(nf - 1, nf); bt.sync()                                      # a plain run_frames still works
    assert bt.map_log_frames() == 0 and bt.last_stats(0)["n_tracks"] == GEO["F"]
    bt.close()


def test_a_poisoned_handle_refuses_to_read_the_map_log(capi, monkeypatch):
    """After a streamed run whose upload failed (MSCKF_HIP_TEST_FAIL_UPLOAD) the slices stopped at different frames: the map log
    of that call is as undefined as the states, map_log_read and map_log_metrics return -EIO, the ordinal did not advance."""
    N, F, nf, B = 8, 24, 16, 2
    trajs = [sc.Trajectory(2, 30 + b, N, F, nf) for b in range(B)]
    monkeypatch.setenv("MSCKF_HIP_TEST_FAIL_UPLOAD", "11")
    bad = _resident_batch(capi, trajs, N, F, nf, N, capi.F32, streams=2)
    monkeypatch.delenv("MSCKF_HIP_TEST_FAIL_UPLOAD")
    bad.map_log_enable(nf * F)
    bad.run_frames(0, 8); bad.sync()
    assert bad.map_log_read(0)[0].shape[0] > 0
    with pytest.raises(capi.HipError, match=r"\(-5\).*undefined"):
        bad.run_frames_streamed(8, 14)
    assert bad.map_log_frames() == 8
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.map_log_read(0, 0, 1)
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        bad.map_log_metrics(0, 8)
    bad.close()
