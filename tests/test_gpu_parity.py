"""GPU parity tests: the HIP path (through the C-ABI, msckf_mono_amd.capi) against the CPU oracle on the
same seeded inputs, against the committed golden fixtures, and -- at BASELINE.json's full sizes -- through
size-independent properties.  Tolerances are BASELINE.json's: 1e-6 relative in double, 1e-3 in float, on
state AND covariance (metric of SURVEY.md section 8c, implemented in tests/helpers.py)."""
import os

import numpy as np
import pytest

import helpers as H
import update_lab as UL
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = {"f64": 1e-6, "f32": 1e-3}


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def _dt(capi, po, name):
    return (capi.F64, po.F64) if name == "f64" else (capi.F32, po.F32)


def _errs(bt, b, o):
    return H.state_errors(bt.imu_state(b), o.getImuState(), bt.cam_states(b)[0], o.getCamStates()[0], bt.covariance(b), o.getCovariance())


def _stagewise(capi, po, prec, N, F, nf, teacher, traj=0, config=2, m_cap=None, check_tracks=True):
    cd, od = _dt(capi, po, prec)
    tr = sc.Trajectory(config, traj, N, F, nf)
    o = po.Oracle(od, po.LEAN)
    o.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N, max(F, 1), m_cap or max(N, 4), cd)
    bt.initialize(0, tr.cfg, tr.imu0)
    tol = TOL[prec]
    for k in range(nf):
        if teacher and k:
            H.copy_oracle_to_device(o, bt, 0)
        o.propagate(tr.imu_for_frame(k)); bt.propagate_range(0, 1, tr.imu_for_frame(k))
        assert H.worst(_errs(bt, 0, o)) < tol, ("propagate", k, _errs(bt, 0, o))
        o.augmentState(k, 0.0); bt.augment_range(0, 1)
        assert H.worst(_errs(bt, 0, o)) < tol, ("augment", k, _errs(bt, 0, o))
        fr = tr.frames[k]
        bt.set_tracks(0, fr["M"], fr["slots"], fr["obs"])
        if len(fr["M"]):
            o.setTracks(fr["M"], fr["slots"], fr["obs"]); o.marginalize()
            bt.marginalize_range(0, 1)
            so, sd = o.lastStats(), bt.last_stats(0)
            if check_tracks:
                for key in ("n_tracks", "n_motion_rejected", "n_tri_rejected", "n_gate_rejected", "n_passed", "m_rows"):
                    assert so[key] == sd[key], (k, key, so, sd)
                to, td = o.lastTracks(), bt.last_tracks(0)
                ok = (to[:, 0] > 0) & (to[:, 1] > 0)
                H.check_tracks(td, to, ok, prec, tr, fr, o, k)
            assert H.worst(_errs(bt, 0, o)) < tol, ("update", k, _errs(bt, 0, o))
        if o.getNumCamStates() == N:
            o.dropOldest(1); bt.drop_oldest_range(0, 1, 1)
            assert H.worst(_errs(bt, 0, o)) < tol, ("prune", k, _errs(bt, 0, o))
    return bt, o, tr


def test_cfg2_double_teacher_forced(capi, po):
    """BASELINE.json configs[1]: synthetic 10-cam window, 50 feats, double, single trajectory."""
    _stagewise(capi, po, "f64", 10, 50, 26, teacher=True)


def test_cfg2_double_free_running(capi, po):
    _stagewise(capi, po, "f64", 10, 50, 30, teacher=False)


def test_cfg2_float_teacher_forced(capi, po):
    _stagewise(capi, po, "f32", 10, 50, 26, teacher=True)


def test_cfg3_float_teacher_forced(capi, po):
    """BASELINE.json configs[2] problem size (30-cam window, 200 feats, float), one trajectory vs oracle."""
    _stagewise(capi, po, "f32", 30, 200, 36, teacher=True, config=3, m_cap=32)


def test_small_window_double(capi, po):
    _stagewise(capi, po, "f64", 5, 7, 12, teacher=False, traj=3)


@pytest.mark.parametrize("name", ["worklist_n6_f10", "worklist_n10_f50"])
def test_golden_fixtures(capi, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    N, F, nf = int(g["N"]), int(g["F"]), int(g["nf"])
    tr = sc.Trajectory(int(g["config_id"]), int(g["traj"]), N, F, nf)
    bt = capi.Batch(1, N, F, N, capi.F64)
    bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(nf):
        H.device_frame(bt, 0, tr, k, N)
        nc = int(g["ncam"][k])
        assert bt.num_cam_states(0) == nc
        D = 15 + 6 * nc
        e = H.state_errors(bt.imu_state(0), g["imu"][k], bt.cam_states(0)[0], g["cams"][k][:nc], bt.covariance(0), g["P"][k][:D, :D])
        assert H.worst(e) < 1e-6, (k, e)


def test_reference_api_path_vs_oracle_and_golden(capi, po):
    """initialize / propagate / augmentState / update / addFeatures / marginalize / pruneEmptyStates in the
    reference's call order (asl_msckf.cpp:269-294) through the MSCKF mirror class."""
    g = np.load(os.path.join(GOLD, "stream_n6_f8.npz"))
    N, F, nf = int(g["N"]), int(g["F"]), int(g["nf"])
    tr = sc.Trajectory(int(g["config_id"]), int(g["traj"]), N, F, nf)
    st = tr.stream()
    f = capi.MSCKF(capi.F64, n_cap=16, f_cap=32, m_cap=16)
    f.initialize(tr.cfg, tr.imu0)
    o = po.Oracle(po.F64, po.LEAN)
    o.initialize(tr.cfg, tr.imu0)
    for k in range(nf):
        for rd in tr.imu_for_frame(k):
            f.propagate(rd)                      # one launch per IMU sample, as the reference is called
        o.propagate(tr.imu_for_frame(k))
        f.augmentState(k, tr.frame_times[k]); o.augmentState(k, tr.frame_times[k])
        f.update(st[k]["cur"][0], st[k]["cur"][1]); o.update(st[k]["cur"][0], st[k]["cur"][1])
        f.addFeatures(st[k]["new"][0], st[k]["new"][1]); o.addFeatures(st[k]["new"][0], st[k]["new"][1])
        f.marginalize(); o.marginalize()
        assert len(f.getMap()) == len(o.getMap())
        f.pruneEmptyStates(); o.pruneEmptyStates()
        assert f.getNumCamStates() == o.getNumCamStates() == int(g["ncam"][k])
        assert H.rel(f.getImuState()[:16], g["imu"][k][:16]) < 1e-6
        assert H.worst(_errs(f.batch, 0, o)) < 1e-6
        assert np.array_equal(f.getCamStates()[1], o.getCamStates()[1])      # state ids
        for a, c in zip(f.getCamMeta(), o.getCamMeta()):                     # time, tracked_feature_ids.size(), last_correlated_id
            assert np.array_equal(a, c), k
    assert np.array_equal(f.getPrunedStates(), o.getPrunedIds())
    pf, pr = f.getPrunedStatesFull(), o.getPrunedStates()                    # poses and times of the pruned states (asl_msckf.cpp:409-424)
    assert len(pr) and pf.shape[0] == pr.shape[0]
    assert np.array_equal(pf[:, 7:9], pr[:, 7:9]) and np.allclose(pf[:, :7], pr[:, :7], atol=1e-8)
    assert H.rel(f.getCovariance(), g["P_final"], 1e-30) < 1e-6
    f.finish(); o.finish()
    assert H.worst(_errs(f.batch, 0, o)) < 1e-6


def test_prune_redundant_states_vs_oracle(capi, po):
    """MSCKF::pruneRedundantStates (msckf.h:453-682) in the ASL runner's call order (asl_msckf.cpp:269-294):
    keyframe selection, triangulation of not-yet-initialized features, second update, covariance gather."""
    N, F, nf = 26, 12, 40
    cfg = sc.filter_config(N)
    cfg["max_cam_states"] = 20
    cfg["redundancy_distance_thresh"] = 0.25
    cfg["redundancy_angle_thresh"] = 0.25
    tr = sc.Trajectory(2, 77, N, F, nf, cfg=cfg)
    st = tr.stream()
    f = capi.MSCKF(capi.F64, n_cap=40, f_cap=128, m_cap=40)
    f.initialize(tr.cfg, tr.imu0)
    o = po.Oracle(po.F64, po.LEAN)
    o.initialize(tr.cfg, tr.imu0)
    pruned_any = False
    for k in range(nf):
        f.propagate(tr.imu_for_frame(k)); o.propagate(tr.imu_for_frame(k))
        f.augmentState(k, tr.frame_times[k]); o.augmentState(k, tr.frame_times[k])
        f.update(st[k]["cur"][0], st[k]["cur"][1]); o.update(st[k]["cur"][0], st[k]["cur"][1])
        f.addFeatures(st[k]["new"][0], st[k]["new"][1]); o.addFeatures(st[k]["new"][0], st[k]["new"][1])
        f.marginalize(); o.marginalize()
        n_before = o.getNumCamStates()
        f.pruneRedundantStates(); o.pruneRedundantStates()
        pruned_any |= o.getNumCamStates() < n_before
        f.pruneEmptyStates(); o.pruneEmptyStates()
        assert f.getNumCamStates() == o.getNumCamStates(), k
        assert np.array_equal(f.getCamStates()[1], o.getCamStates()[1]), k
        assert H.worst(_errs(f.batch, 0, o)) < 1e-6, (k, _errs(f.batch, 0, o))
    assert pruned_any
    assert np.array_equal(f.getPrunedStates(), o.getPrunedIds())
    pf, pr = f.getPrunedStatesFull(), o.getPrunedStates()
    assert np.array_equal(pf[:, 7:9], pr[:, 7:9]) and np.allclose(pf[:, :7], pr[:, :7], atol=1e-7)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_batched_image_cycle_with_prune_redundant_equals_per_filter_calls_and_oracle(capi, po, prec):
    """msckf_hip_image_cycle_range: the ASL runner's per-image cycle (asl_msckf.cpp:269-294, pruneRedundantStates :289 included)
    for a BATCH of trajectories in lockstep -- host bookkeeping per trajectory, every device stage one launch sequence over
    the range, every read-back one copy for the range.  (1) bit for bit the per-filter API (augmentState / update /
    addFeatures / marginalize / pruneRedundantStates / pruneEmptyStates called filter by filter on a second handle): state,
    camera states and their ids, covariance, map, pruned states, after every image, camera-state metadata at the end;
    (2) against the oracle running the same cycle: 1e-6 in double after every image, free-running; in float the two
    free-running filters are compared at the end (2e-2) when they selected the same keyframes."""
    N, F, nf, B = 26, 12, 40, 5
    cd, pd, tol = (capi.F64, po.F64, 1e-6) if prec == "f64" else (capi.F32, po.F32, 1e-3)
    cfg = sc.filter_config(N)
    cfg["max_cam_states"] = 20
    cfg["redundancy_distance_thresh"] = 0.25
    cfg["redundancy_angle_thresh"] = 0.25
    trs = [sc.Trajectory(2, 70 + b, N, F, nf, cfg=cfg) for b in range(B)]
    sts = [tr.stream() for tr in trs]
    one, big = capi.Batch(B, 40, 128, 40, cd), capi.Batch(B, 40, 128, 40, cd)
    oracles = []
    for b, tr in enumerate(trs):
        one.initialize(b, tr.cfg, tr.imu0); big.initialize(b, tr.cfg, tr.imu0)
        o = po.Oracle(pd, po.LEAN); o.initialize(tr.cfg, tr.imu0); oracles.append(o)
    pruned_any = 0
    for k in range(nf):
        # per filter, as the shim calls them
        for b, tr in enumerate(trs):
            one.propagate_range(b, 1, tr.imu_for_frame(k))
            one.augment_state(b, k, tr.frame_times[k])
            one.update(b, sts[b][k]["cur"][0], sts[b][k]["cur"][1])
            one.add_features(b, sts[b][k]["new"][0], sts[b][k]["new"][1])
            one.marginalize(b)
            one.prune_redundant_states(b)
            one.prune_empty_states(b)
        # the batch in lockstep
        big.propagate_range(0, B, np.stack([tr.imu_for_frame(k) for tr in trs]))
        big.image_cycle_range(0, B, [k] * B, [tr.frame_times[k] for tr in trs], [sts[b][k]["cur"] for b in range(B)], [sts[b][k]["new"] for b in range(B)])
        for b, tr in enumerate(trs):
            o = oracles[b]
            o.propagate(tr.imu_for_frame(k)); o.augmentState(k, tr.frame_times[k])
            o.update(sts[b][k]["cur"][0], sts[b][k]["cur"][1]); o.addFeatures(sts[b][k]["new"][0], sts[b][k]["new"][1])
            o.marginalize(); n_before = o.getNumCamStates(); o.pruneRedundantStates(); pruned_any += o.getNumCamStates() < n_before; o.pruneEmptyStates()
            assert big.num_cam_states(b) == one.num_cam_states(b), (k, b)
            assert np.array_equal(big.cam_states(b)[1], one.cam_states(b)[1]), (k, b)
            if prec == "f64":
                assert big.num_cam_states(b) == o.getNumCamStates() and np.array_equal(big.cam_states(b)[1], o.getCamStates()[1]), (k, b)
            assert np.array_equal(big.imu_state(b), one.imu_state(b)), (k, b)
            assert np.array_equal(big.cam_states(b)[0], one.cam_states(b)[0]), (k, b)
            assert np.array_equal(big.covariance(b), one.covariance(b)), (k, b)
            assert np.array_equal(big.get_map(b), one.get_map(b)), (k, b)
            if prec == "f64":
                e = _errs(big, b, o)
                assert H.worst(e) < tol, (k, b, e)
    assert pruned_any >= B          # every trajectory pruned redundant states at least once
    for b in range(B):
        for mb, mo in zip(big.cam_meta(b), one.cam_meta(b)):    # times, tracked counts, last_correlated ids
            assert np.array_equal(mb, mo), b
        assert np.array_equal(big.pruned_state_ids(b), one.pruned_state_ids(b))
        assert np.array_equal(big.pruned_states(b), one.pruned_states(b))
        if prec == "f64":
            assert np.array_equal(big.pruned_state_ids(b), oracles[b].getPrunedIds())
        elif np.array_equal(big.cam_states(b)[1], oracles[b].getCamStates()[1]):
            # float, free-running against a free-running float oracle over 40 images: as long as both selected the same
            # keyframes (threshold decisions on float poses may flip) the filters stay together
            e = _errs(big, b, oracles[b])
            assert H.worst(e) < 2e-2, (b, e)
    one.close(); big.close()


def test_prune_redundant_over_f_cap_is_the_same_error_on_both_paths(capi):
    """pruneRedundantStates meeting more tracks than f_cap: msckf_hip_image_cycle_range and, on a second handle fed the same
    images filter by filter, msckf_hip_prune_redundant_states(0) refuse with the same -E2BIG at the same image, and the
    other trajectory of the range handle is what its per-filter twin is.
    The scenario (found with the oracle on the CPU): trajectory 0 has dense tracks (every track spans the window) and the
    redundancy thresholds of the test above, so the first selection -- image 21, states 1 and 2 of a 22-state window --
    finds 60 not-yet-initialized tracks that saw both states, against f_cap = 16; marginalize() never has more than the
    F = 12 tracks that end per image.  Trajectory 1 keeps the default thresholds, under which no state is ever selected
    (pruneRedundantStates is a no-op for it), so its twin is well defined whichever capacity check trips."""
    N, F, nf, f_cap = 26, 12, 24, 16
    cfg = sc.filter_config(N)
    cfg["max_cam_states"] = 20
    cfg["redundancy_distance_thresh"] = 0.25
    cfg["redundancy_angle_thresh"] = 0.25
    trs = [sc.Trajectory(2, 70, N, F, nf, cfg=cfg, dense_tracks=True), sc.Trajectory(2, 71, N, F, nf)]
    sts = [tr.stream() for tr in trs]
    one, big = capi.Batch(2, 40, f_cap, 40, capi.F64), capi.Batch(2, 40, f_cap, 40, capi.F64)
    for b, tr in enumerate(trs):
        one.initialize(b, tr.cfg, tr.imu0); big.initialize(b, tr.cfg, tr.imu0)

    def same(b, k):
        assert big.num_cam_states(b) == one.num_cam_states(b), (k, b)
        assert np.array_equal(big.cam_states(b)[1], one.cam_states(b)[1]), (k, b)
        assert np.array_equal(big.cam_states(b)[0], one.cam_states(b)[0]), (k, b)
        assert np.array_equal(big.imu_state(b), one.imu_state(b)), (k, b)
        assert np.array_equal(big.covariance(b), one.covariance(b)), (k, b)
        assert np.array_equal(big.get_map(b), one.get_map(b)), (k, b)
        for mb, mo in zip(big.cam_meta(b), one.cam_meta(b)):
            assert np.array_equal(mb, mo), (k, b)
        assert np.array_equal(big.pruned_states(b), one.pruned_states(b)), (k, b)

    for k in range(nf):
        err_big = err_one = None
        big.propagate_range(0, 2, np.stack([tr.imu_for_frame(k) for tr in trs]))
        try:
            big.image_cycle_range(0, 2, [k] * 2, [tr.frame_times[k] for tr in trs], [sts[b][k]["cur"] for b in range(2)], [sts[b][k]["new"] for b in range(2)])
        except capi.HipError as e:
            err_big = str(e)
        for b, tr in enumerate(trs):
            one.propagate_range(b, 1, tr.imu_for_frame(k))
            one.augment_state(b, k, tr.frame_times[k])
            one.update(b, sts[b][k]["cur"][0], sts[b][k]["cur"][1])
            one.add_features(b, sts[b][k]["new"][0], sts[b][k]["new"][1])
            one.marginalize(b)
            try:
                one.prune_redundant_states(b)
            except capi.HipError as e:
                assert b == 0, (k, str(e))
                err_one = str(e)
        print("image %d: range %r, per filter %r" % (k, err_big, err_one))
        assert err_big == err_one, k
        if err_one:
            break
        for b in range(2):
            one.prune_empty_states(b)
            same(b, k)
    assert err_one is not None and "(-7)" in err_one and "f_cap" in err_one, (k, err_one)     # -E2BIG
    assert k == 21
    same(1, k)
    one.close(); big.close()


def test_batched_image_cycle_error_text_reaches_the_calling_thread(capi, monkeypatch):
    """msckf_hip_image_cycle_range in which the second of eight trajectories is handed, as a new feature, an id it
    already tracks: -EEXIST with addFeatures' own text.  The update / addFeatures bookkeeping of a range runs on worker
    threads of the library when MSCKF_HIP_HOST_THREADS is unset and the range has two or more trajectories (the workers are
    started before the calling thread joins in, so an early trajectory of a range of eight is theirs), and
    msckf_hip_last_error() is per thread: the text written on a worker must be carried back to the thread that made the
    call, or the caller reads whatever its own last failure left (the code alone was always right)."""
    monkeypatch.delenv("MSCKF_HIP_HOST_THREADS", raising=False)
    N, F, nf, B = 8, 10, 8, 8
    trs = [sc.Trajectory(2, 80 + b, N, F, nf) for b in range(B)]
    sts = [tr.stream() for tr in trs]
    bt = capi.Batch(B, 16, 32, 16, capi.F64)
    for b, tr in enumerate(trs):
        bt.initialize(b, tr.cfg, tr.imu0)
    with pytest.raises(capi.HipError, match="out of bounds"):     # the calling thread's own last error: not the one below
        bt.propagate_range(0, B + 1, np.zeros((B + 1, 1, 7)))
    raised = False
    for k in range(nf):
        cur = [sts[b][k]["cur"] for b in range(B)]
        new = [sts[b][k]["new"] for b in range(B)]
        dup = k >= 2 and len(cur[1][1]) > 0
        if dup:     # an id that this image's update() keeps tracked comes again as new
            new[1] = (list(new[1][0]) + [cur[1][0][0]], list(new[1][1]) + [cur[1][1][0]])
        bt.propagate_range(0, B, np.stack([tr.imu_for_frame(k) for tr in trs]))
        if not dup:
            bt.image_cycle_range(0, B, [k] * B, [tr.frame_times[k] for tr in trs], cur, new)
            continue
        with pytest.raises(capi.HipError, match=r"\(-17\): .*already being tracked"):     # -EEXIST
            bt.image_cycle_range(0, B, [k] * B, [tr.frame_times[k] for tr in trs], cur, new)
        raised = True
        break
    assert raised
    bt.close()


def test_batched_range_equals_single(capi):
    """B trajectories in one launch give bit-identical results to B separate single-trajectory batches of
    the same geometry (same kernels, same chunking)."""
    N, F, nf, B = 8, 20, 14, 5
    trs = [sc.Trajectory(2, 40 + b, N, F, nf) for b in range(B)]
    big = capi.Batch(B, N, F, N, capi.F32)
    for b, tr in enumerate(trs):
        big.initialize(b, tr.cfg, tr.imu0)
    for k in range(nf):
        big.propagate_range(0, B, np.stack([tr.imu_for_frame(k) for tr in trs]))
        big.augment_range(0, B)
        for b, tr in enumerate(trs):
            fr = tr.frames[k]
            big.set_tracks(b, fr["M"], fr["slots"], fr["obs"])
        big.marginalize_range(0, B)
        if big.num_cam_states(0) == N:
            big.drop_oldest_range(0, B, 1)
    for b, tr in enumerate(trs):
        one = capi.Batch(B, N, F, N, capi.F32)      # same B => same TSQR chunking
        one.initialize(b, tr.cfg, tr.imu0)
        for k in range(nf):
            H.device_frame(one, b, tr, k, N)
        assert np.array_equal(one.covariance(b), big.covariance(b))
        assert np.array_equal(one.imu_state(b), big.imu_state(b))


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_information_form_equals_householder_route(capi, prec):
    """The library has two compression routes for the stacked Jacobian: the information form (default: H_o^T H_o
    accumulated in f64 + Cholesky, kernels_gram.hip) and the Householder TSQR (kernels_qr.hip, what the reference
    does, msckf.h:1338-1366).  Free-running filters on the two routes stay together to rounding; the information
    form reports the unobservable directions of the window as zero rows of T_H."""
    N, F, nf = 12, 40, 20
    tr = sc.Trajectory(2, 7, N, F, nf)
    cd = capi.F64 if prec == "f64" else capi.F32
    res = {}
    for route in (0, 3):                  # 3: information form, blocked matrix-core Cholesky (kernels_chol.hip)
        bt = capi.Batch(1, N, F, N, cd)
        bt.set_compression(route)
        bt.initialize(0, tr.cfg, tr.imu0)
        for k in range(nf):
            H.device_frame(bt, 0, tr, k, N)
        res[route] = (bt.imu_state(0), bt.cam_states(0)[0], bt.covariance(0), bt.last_stats(0))
        bt.close()
    e = H.state_errors(res[3][0], res[0][0], res[3][1], res[0][1], res[3][2], res[0][2])
    assert H.worst(e) < (1e-8 if prec == "f64" else 3e-4), e
    assert res[3][3]["m_rows"] == res[0][3]["m_rows"] > 0
    assert res[3][3]["r_rows"] < res[0][3]["r_rows"] == 6 * N            # gauge directions skipped


@pytest.mark.parametrize("prec,N,F", [("f64", 10, 50), ("f32", 10, 50), ("f64", 12, 40), ("f32", 13, 40), ("f64", 4, 16)])
def test_one_launch_update_of_short_windows_equals_the_chain(capi, prec, N, F, monkeypatch):
    """Windows of at most 14 cameras take everything after k_select_diag in ONE launch (k_update_small, kernels_kalman.hip:
    Gram matrix, both factorizations, gain, injection and downdate of msckf.h:404-431, 1338-1418 out of one workgroup's LDS)
    instead of the chain k_gram / k_chol_mfma / GEMMs / gain solve / downdate.  Same update, other arithmetic order: free-running
    over N + 10 frames the two must agree to rounding (double 1e-9 -- the 10-camera window is BASELINE configs[1]'s -- float
    1e-4), with the same gate decisions and row counts.  MSCKF_HIP_SMALL_UPDATE=0 at create time selects the chain."""
    nf = N + 10
    tr = sc.Trajectory(2, 21, N, F, nf)
    cd = capi.F64 if prec == "f64" else capi.F32
    res = {}
    for small in ("84", "0"):
        monkeypatch.setenv("MSCKF_HIP_SMALL_UPDATE", small)
        bt = capi.Batch(1, N, F, max(N, 4), cd)
        bt.initialize(0, tr.cfg, tr.imu0)
        stats = []
        for k in range(nf):
            H.device_frame(bt, 0, tr, k, N)
            stats.append(bt.last_stats(0, strict=False))
        res[small] = (bt.imu_state(0), bt.cam_states(0)[0], bt.covariance(0), stats)
        bt.close()
    a, c = res["84"], res["0"]
    e = H.state_errors(a[0], c[0], a[1], c[1], a[2], c[2])
    assert H.worst(e) < (1e-9 if prec == "f64" else 1e-4), e
    assert np.array_equal(a[2], a[2].T)
    strip = lambda st: [{k: v for k, v in s.items() if k != "r_rows"} for s in st]      # r_rows: pivots above a rounding-level tolerance
    assert strip(a[3]) == strip(c[3]) and sum(s["n_passed"] for s in a[3]) > 0


@pytest.mark.parametrize("prec,N,F", [("f64", 8, 24), ("f64", 26, 60), ("f32", 12, 40), ("f32", 30, 120), ("f64", 36, 80), ("f32", 44, 100), ("f64", 60, 120), ("f32", 32, 80), ("f32", 33, 80)])
def test_square_root_gain_form_equals_joseph_form(capi, prec, N, F):
    """Covariance update of measurementUpdate (msckf.h:1368-1418): the default square-root gain form (W = P T_H^T L^-T,
    P <- P - W W^T, dx = W L^-1 r_n; no gain matrix, no S^-1) against the reference's literal Joseph sequence, both on the
    device, free-running over the same frames: equal to rounding.  Window sizes cover the register-resident solve
    (n <= 128 double / 192 float), the LDS Cholesky + f64 matrix-core path (26 cameras in double) and, beyond 32 cameras,
    the two-level blocked factorization of S with the row solves for W (kernels_chol.hip: 36, 44 and 60 cameras)."""
    nf = N + 8
    tr = sc.Trajectory(2, 9, N, F, nf)
    cd = capi.F64 if prec == "f64" else capi.F32
    res = {}
    for form in (0, 1, 2):                 # 0 default (float: blocked matrix-core solve), 1 Joseph, 2 register-resident solve
        bt = capi.Batch(1, N, F, max(N, 4), cd)
        bt.set_covariance_update(form)
        bt.initialize(0, tr.cfg, tr.imu0)
        for k in range(nf):
            H.device_frame(bt, 0, tr, k, N)
        P = bt.covariance(0)
        assert np.array_equal(P, P.T)
        res[form] = (bt.imu_state(0), bt.cam_states(0)[0], P, bt.last_stats(0))
        bt.close()
    e = H.state_errors(res[0][0], res[1][0], res[0][1], res[1][1], res[0][2], res[1][2])
    # double: rounding level; the weakly observable accelerometer bias of a 36+ camera window amplifies it to a few 1e-9 over
    # 44+ free-running frames (tolerance of the double filter against the oracle: 1e-6).  float: two free-running float filters
    tol64 = 1e-9 if N <= 26 else 1e-8
    assert H.worst(e) < (tol64 if prec == "f64" else 1e-3), e
    strip = lambda st: {k: v for k, v in st.items() if k != "r_rows"}   # r_rows: count of pivots above a rounding-level tolerance
    assert strip(res[0][3]) == strip(res[1][3]) and res[0][3]["n_passed"] > 0
    e2 = H.state_errors(res[2][0], res[0][0], res[2][1], res[0][1], res[2][2], res[0][2])
    assert H.worst(e2) < (tol64 if prec == "f64" else 1e-3), e2


@pytest.mark.parametrize("N", [5, 11])
def test_register_resident_gain_kernels_with_a_partial_last_block(capi, po, N):
    """k_gain (set_covariance_update(1), the Joseph sequence) and k_gain_w (2, the register-resident square-root solve) keep S in
    registers as 16 x 16 blocks.  n = 6 N = 30 is two column blocks, the second partial (k_gain<., 4>, k_gain_w<., 4, 8>); n = 66
    is five, the last with two columns (the NBN = 8 instantiations); the window grows by six columns a frame, so on the way
    there every block boundary up to 64 is crossed with a partial block behind it.  Two trajectories in one launch, 12 tracks, 12 frames, against the oracle of the same scalar
    type after every step: double free-running at 1e-6, float teacher-forced at 1e-3 (the tolerances of the stage-wise tests
    above); the state carries dx, the covariance the downdate.  The sticky error flags stay clear."""
    F, nf, B = 12, 12, 2
    trs = [sc.Trajectory(2, 40 + b, N, F, nf) for b in range(B)]
    for prec in ("f64", "f32"):
        cd, od = _dt(capi, po, prec)
        for form in (1, 2):
            bt = capi.Batch(B, N, F, max(N, 4), cd)
            bt.set_covariance_update(form)
            orc = []
            for b, tr in enumerate(trs):
                orc.append(po.Oracle(od, po.LEAN)); orc[b].initialize(tr.cfg, tr.imu0)
                bt.initialize(b, tr.cfg, tr.imu0)
            rows = 0
            for k in range(nf):
                for b, tr in enumerate(trs):
                    if prec == "f32" and k:
                        H.copy_oracle_to_device(orc[b], bt, b)
                    bt.propagate_range(b, 1, tr.imu_for_frame(k))
                bt.augment_range(0, B)
                for b, tr in enumerate(trs):
                    fr = tr.frames[k]
                    bt.set_tracks(b, fr["M"], fr["slots"], fr["obs"])
                if any(len(tr.frames[k]["M"]) for tr in trs):
                    bt.marginalize_range(0, B)
                for b, (tr, o) in enumerate(zip(trs, orc)):
                    fr = tr.frames[k]
                    o.propagate(tr.imu_for_frame(k)); o.augmentState(k, 0.0)
                    if len(fr["M"]):
                        o.setTracks(fr["M"], fr["slots"], fr["obs"]); o.marginalize()
                        so, sd = o.lastStats(), bt.last_stats(b)        # (raises when a sticky flag is up)
                        assert so["m_rows"] == sd["m_rows"] and so["n_passed"] == sd["n_passed"], (prec, form, k, b, so, sd)
                        rows += sd["m_rows"]
                    e = _errs(bt, b, o)
                    assert H.worst(e) < TOL[prec], (prec, form, k, b, e)
                    # the Frobenius norm above passes a partial last block that keeps its prior (tests/test_update_inputs.py): every
                    # entry against the scale of its own row and column as well.  Float: the oracle here is the float one, so the bar
                    # is the device's against the double oracle plus the float oracle's own worst distance from it (update_lab)
                    ec = H.cov_scaled_err(bt.covariance(b), o.getCovariance())
                    assert ec < (UL.BAR_F64 if prec == "f64" else UL.bars("f32")[0] + UL.D32_COV), (prec, form, k, b, ec)
                    assert bt.error_flags(b) == 0, (prec, form, k, b)
                if orc[0].getNumCamStates() == N:
                    for o in orc:
                        o.dropOldest(1)
                    bt.drop_oldest_range(0, B, 1)
            assert rows > 0 and bt.num_cam_states(0) == N - 1, (prec, form, rows)
            bt.close()


def test_resident_scenario_equals_per_call(capi):
    N, F, nf, B = 8, 16, 13, 3
    trs = [sc.Trajectory(2, 60 + b, N, F, nf) for b in range(B)]
    a, c = capi.Batch(B, N, F, N, capi.F32), capi.Batch(B, N, F, N, capi.F32)
    c.scenario_alloc(nf, sc.IMU_PER_FRAME)
    for b, tr in enumerate(trs):
        a.initialize(b, tr.cfg, tr.imu0); c.initialize(b, tr.cfg, tr.imu0)
        for k in range(nf):
            fr = tr.frames[k]
            c.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    c.scenario_commit()
    c.run_frames(0, nf); c.sync()
    for b, tr in enumerate(trs):
        for k in range(nf):
            H.device_frame(a, b, tr, k, N)
        assert np.array_equal(a.covariance(b), c.covariance(b))
        assert np.array_equal(a.imu_state(b), c.imu_state(b))
        assert np.array_equal(a.cam_states(b)[0], c.cam_states(b)[0])


def test_resident_scenario_with_tracks_on_the_newest_camera(capi):
    """With msckf_hip_set_feature_overlap run_frames launches k_feature concurrently with the frame's propagate +
    augmentState when no track observes the camera that augmentState adds; a track terminated by max_track_length DOES observe it (msckf.h:246-262), and then
    the frame must take the ordered path.  Frames of both kinds, resident run vs per-call API: bit-identical."""
    N, F, nf, B = 8, 12, 14, 2
    trs = [sc.Trajectory(2, 80 + b, N, F, nf) for b in range(B)]
    frames = []
    for b, tr in enumerate(trs):
        fl = []
        for k in range(nf):
            fr = dict(tr.frames[k])
            if len(fr["M"]) and k % 3 == b:       # extend track 0 by an observation in the newest camera (slot Nw - 1)
                M = fr["M"].copy(); off = np.concatenate([[0], np.cumsum(M)])
                pt = tr.landmarks[k][0]
                pc = tr.C_CG[k] @ (pt - tr.p_C[k])
                if pc[2] > 0.5 and M[0] < N - 1:
                    z = pc[:2] / pc[2]
                    slots = np.insert(fr["slots"], off[1], fr["Nw"] - 1).astype(np.int32)
                    obs = np.insert(fr["obs"], off[1], z, axis=0)
                    M[0] += 1
                    fr = dict(Nw=fr["Nw"], M=M, slots=slots, obs=obs)
            fl.append(fr)
        frames.append(fl)
    assert any(len(fr["M"]) and fr["slots"].max() == fr["Nw"] - 1 for fl in frames for fr in fl)
    a, c = capi.Batch(B, N, F, N, capi.F64), capi.Batch(B, N, F, N, capi.F64)
    c.scenario_alloc(nf, sc.IMU_PER_FRAME)
    for b, tr in enumerate(trs):
        a.initialize(b, tr.cfg, tr.imu0); c.initialize(b, tr.cfg, tr.imu0)
        for k in range(nf):
            fr = frames[b][k]
            c.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    c.scenario_commit()
    c.set_streams(2)
    c.set_feature_overlap(True)
    c.run_frames(0, 5); c.run_frames(5, nf); c.sync()
    for b, tr in enumerate(trs):
        for k in range(nf):
            fr = frames[b][k]
            a.propagate_range(b, 1, tr.imu_for_frame(k)); a.augment_range(b, 1)
            a.set_tracks(b, fr["M"], fr["slots"], fr["obs"])
            if len(fr["M"]):
                a.marginalize_range(b, 1)
            if a.num_cam_states(b) == N:
                a.drop_oldest_range(b, 1, 1)
        assert np.array_equal(a.covariance(b), c.covariance(b)), b
        assert np.array_equal(a.imu_state(b), c.imu_state(b)), b
        assert a.last_stats(b) == c.last_stats(b) and a.last_stats(b)["n_passed"] > 0


# ----------------------------------------------------------------------------------- edge cases
def _pair(capi, po, prec, N, F, nf, cfg=None, traj=0, **kw):
    cd, od = _dt(capi, po, prec)
    tr = sc.Trajectory(2, traj, N, F, nf, cfg=cfg, **kw)
    o = po.Oracle(od, po.LEAN); o.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N + 2, max(F, 1), max(N, 4), cd); bt.initialize(0, tr.cfg, tr.imu0)
    return tr, o, bt


def test_empty_track_list_is_a_no_op(capi, po):
    tr, o, bt = _pair(capi, po, "f64", 6, 0, 8)
    for k in range(8):
        H.oracle_frame(o, tr, k, 6); H.device_frame(bt, 0, tr, k, 6)
    P0 = bt.covariance(0)
    bt.set_tracks(0, [], [], np.zeros((0, 2))); bt.marginalize_range(0, 1)
    assert np.array_equal(bt.covariance(0), P0)
    assert bt.last_stats(0)["n_tracks"] == 0
    assert H.worst(_errs(bt, 0, o)) < 1e-6


def test_all_tracks_gated_out_leaves_state_untouched(capi, po):
    """true pixel noise == assumed noise: the 5% quantile gate (Q3) rejects (nearly) everything."""
    tr, o, bt = _pair(capi, po, "f64", 7, 30, 10, obs_noise_px=20.0)
    for k in range(9):
        H.oracle_frame(o, tr, k, 7); H.device_frame(bt, 0, tr, k, 7)
    H.copy_oracle_to_device(o, bt, 0)
    k = 9
    o.propagate(tr.imu_for_frame(k)); bt.propagate_range(0, 1, tr.imu_for_frame(k))
    o.augmentState(k, 0); bt.augment_range(0, 1)
    fr = tr.frames[k]
    P0 = bt.covariance(0)
    o.setTracks(fr["M"], fr["slots"], fr["obs"]); o.marginalize()
    bt.set_tracks(0, fr["M"], fr["slots"], fr["obs"]); bt.marginalize_range(0, 1)
    so, sd = o.lastStats(), bt.last_stats(0)
    assert so["n_passed"] == sd["n_passed"] and so["n_gate_rejected"] + so["n_tri_rejected"] == sd["n_gate_rejected"] + sd["n_tri_rejected"]
    if sd["n_passed"] == 0:
        assert np.array_equal(bt.covariance(0), P0)
    assert H.worst(_errs(bt, 0, o)) < 1e-6


def test_motion_rejection_and_first_four_rule(capi, po):
    """Q4 (msckf.h:354) + D1: an absurd translation threshold rejects every track after the first four."""
    cfg = sc.filter_config(6)
    cfg["translation_threshold"] = 1e3
    tr, o, bt = _pair(capi, po, "f64", 6, 7, 7, cfg=cfg)
    for k in range(7):
        H.oracle_frame(o, tr, k, 6); H.device_frame(bt, 0, tr, k, 6)
        if len(tr.frames[k]["M"]):
            assert o.lastStats() == {**bt.last_stats(0), "r_rows": o.lastStats()["r_rows"]}
    assert bt.num_residualized(0) == o.numResidualized() == 4
    assert H.worst(_errs(bt, 0, o)) < 1e-6


def test_ragged_tracks_with_gaps_and_unseen_cameras(capi, po):
    """tracks with non-contiguous camera slots and cameras in the MIDDLE of the window that no track sees
    (zero columns inside the stacked Jacobian) -- isotropic noise, so any compression agrees."""
    N = 9
    tr, o, bt = _pair(capi, po, "f64", N, 12, 12)
    for k in range(11):
        H.oracle_frame(o, tr, k, N); H.device_frame(bt, 0, tr, k, N)
    H.copy_oracle_to_device(o, bt, 0)
    k = 11
    o.propagate(tr.imu_for_frame(k)); bt.propagate_range(0, 1, tr.imu_for_frame(k))
    o.augmentState(k, 0); bt.augment_range(0, 1)
    fr = tr.frames[k]
    # drop every observation made from slots 3 and 4, and the odd observations of long tracks
    M2, sl2, ob2, off = [], [], [], 0
    for M in fr["M"]:
        s, ob = fr["slots"][off:off + M], fr["obs"][off:off + M]
        keep = [i for i in range(M) if s[i] not in (3, 4) and not (M > 6 and i % 2 == 1)]
        off += M
        if len(keep) >= 3:
            M2.append(len(keep)); sl2 += [int(s[i]) for i in keep]; ob2 += [ob[i] for i in keep]
    o.setTracks(M2, sl2, np.array(ob2)); o.marginalize()
    bt.set_tracks(0, M2, sl2, np.array(ob2)); bt.marginalize_range(0, 1)
    assert o.lastStats()["n_passed"] == bt.last_stats(0)["n_passed"] > 0
    assert H.worst(_errs(bt, 0, o)) < 1e-6


def test_maximum_track_length_equals_m_cap(capi, po):
    """dense tracks: every track spans the whole window (M = N-1 = m_cap)."""
    N = 17
    cd, od = capi.F64, po.F64
    tr = sc.Trajectory(2, 8, N, 10, N + 2, dense_tracks=True)
    o = po.Oracle(od, po.LEAN); o.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N, 10, N - 1, cd); bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(N + 2):
        H.oracle_frame(o, tr, k, N); H.device_frame(bt, 0, tr, k, N)
    assert bt.last_stats(0)["m_rows"] == 10 * (2 * (N - 1) - 3)
    assert H.worst(_errs(bt, 0, o)) < 1e-6


def test_error_behaviour(capi):
    import ctypes as C
    tr = sc.Trajectory(2, 0, 6, 4, 3)
    bt = capi.Batch(1, 3, 4, 6, capi.F32)
    bad = dict(tr.cfg); bad["u_var_prime"] = 0.0
    with pytest.raises(capi.HipError, match="positive"):
        bt.initialize(0, bad, tr.imu0)
    bt.initialize(0, tr.cfg, tr.imu0)
    with pytest.raises(capi.HipError):
        bt.set_tracks(0, [3] * 5, [0, 1, 2] * 5, np.zeros((15, 2)))   # more tracks than f_cap
    with pytest.raises(capi.HipError):
        bt.set_tracks(0, [7], list(range(7)), np.zeros((7, 2)))       # longer than m_cap
    with pytest.raises(capi.HipError):
        bt.initialize(5, tr.cfg, tr.imu0)                   # trajectory index out of range
    for k in range(3):
        bt.augment_state(0, k, 0.0)
    with pytest.raises(capi.HipError, match="capacity"):
        bt.augment_state(0, 3, 0.0)                         # n_cap exceeded
    with pytest.raises(capi.HipError):
        capi.MSCKF(capi.F32, n_cap=4, f_cap=4, m_cap=4).update([[0, 0]], [1])   # update before initialize


def test_get_imu_state_after_propagate_is_answered_from_the_host_mirror(capi, po):
    """msckf_hip_propagate advances a host copy of the IMU state with the reference's RK sequence (msckf.h:1425-1467) beside the
    device, so that the by-value getImuState() the ASL runner makes per IMU sample (asl_msckf.cpp:231) needs no device round
    trip; the copy is dropped whenever the device changes the state otherwise.  Per sample: the getter vs the oracle; then the
    same state read from the device (a batched no-op propagate invalidates the copy) within rounding of it."""
    for dt_dev, dt_or, tol in ((capi.F64, po.F64, 1e-10), (capi.F32, po.F32, 2e-5)):
        N, F, nf = 6, 8, 8
        tr = sc.Trajectory(2, 31, N, F, nf)
        st = tr.stream()
        f = capi.MSCKF(dt_dev, n_cap=N + 3, f_cap=64, m_cap=N + 3)
        o = po.Oracle(dt_or, po.LEAN)
        f.initialize(tr.cfg, tr.imu0); o.initialize(tr.cfg, tr.imu0)
        sid = 0
        for k in range(nf):
            for r7 in tr.imu_for_frame(k):
                sid += 1
                f.propagate(r7); o.propagate(r7)
                a, b = f.getImuState(), o.getImuState()
                assert H.rel(a[:16], b[:16]) < tol and H.rel(a[19:29], b[19:29]) < tol, (k, sid)
            mirror = f.getImuState()
            assert f.batch.L.msckf_hip_propagate_range(f.batch.h, 0, 1, None, 0) == 0      # K = 0: launches nothing, drops the host copy
            dev = f.getImuState()
            assert H.rel(mirror[:16], dev[:16]) < (1e-13 if dt_dev == capi.F64 else 2e-6)
            f.augmentState(sid, float(k)); o.augmentState(sid, float(k))
            f.update(*st[k]["cur"]); o.update(*st[k]["cur"])
            f.addFeatures(*st[k]["new"]); o.addFeatures(*st[k]["new"])
            f.marginalize(); o.marginalize(); f.pruneEmptyStates(); o.pruneEmptyStates()
            assert H.rel(f.getImuState()[:16], o.getImuState()[:16]) < (1e-6 if dt_dev == capi.F64 else 1e-3)
        f.batch.close()


def test_anisotropic_pixel_noise_euroc_intrinsics(capi, po):
    """f_u != f_v (the reference's shipped EuRoC configuration, asl_msckf.cpp:77-78), the device's pre-whitened route
    (msckf_hip_set_anisotropic_noise(h, 1); the default literal route is held in tests/test_gpu_literal.py).  The device
    pre-whitens the observation rows; the oracle's `whiten` mode is the same construction (1e-6 in double), and its literal
    restatement of the reference's A_j^T R_j A_j / Q_1^T R_o Q_1 path agrees at the level two valid
    implementations can (~1e-3 per update in dx)."""
    N, F, nf = 8, 30, 16
    cfg = sc.filter_config(N, isotropic=False)
    assert cfg["u_var_prime"] != cfg["v_var_prime"]
    tr = sc.Trajectory(2, 12, N, F, nf, cfg=cfg)
    ow = po.Oracle(po.F64, po.LEAN); ow.initialize(tr.cfg, tr.imu0); ow.setWhiten(True)
    ol = po.Oracle(po.F64, po.LEAN); ol.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N, F, N, capi.F64); bt.set_anisotropic_noise(1); bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(nf):
        H.oracle_frame(ow, tr, k, N); H.oracle_frame(ol, tr, k, N); H.device_frame(bt, 0, tr, k, N)
        assert H.worst(_errs(bt, 0, ow)) < 1e-6, (k, _errs(bt, 0, ow))
        if len(tr.frames[k]["M"]):
            assert ow.lastStats()["n_passed"] == bt.last_stats(0)["n_passed"]
    e = _errs(bt, 0, ol)
    assert H.worst(e) < 2e-2, e            # literal reference construction: same filter up to the documented basis effect
    assert e["p"] < 1e-3 and e["q"] < 1e-3


# ----------------------------------------------------------------------------------- full-size properties
def test_cfg3_batch_properties(capi):
    """64 trajectories x (30-cam window, 200 feats), float: the bench configuration.  Size-independent
    properties: exact symmetry of P after every stage, positive diagonal, PSD up to float rounding, gate
    pass-rate > 95 %, finite states, small position error against ground truth."""
    N, F, B, nf = 30, 200, 64, 34
    trs = [sc.Trajectory(3, b, N, F, nf) for b in range(B)]
    bt = capi.Batch(B, N, F, N, capi.F32)
    bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    for b, tr in enumerate(trs):
        bt.initialize(b, tr.cfg, tr.imu0)
        for k in range(nf):
            fr = tr.frames[k]
            bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    bt.run_frames(0, nf); bt.sync()
    rates = []
    for b in range(0, B, 7):
        P = bt.covariance(b)
        assert P.shape == (15 + 6 * (N - 1),) * 2 and np.all(np.isfinite(P))
        assert np.array_equal(P, P.T)
        assert np.all(np.diag(P) > 0)
        w = np.linalg.eigvalsh(P)
        assert w.min() > -1e-6 * w.max()
        s = bt.last_stats(b)
        rates.append(s["n_passed"] / s["n_tracks"])
        assert s["m_rows"] > 4000
        e = np.linalg.norm(bt.imu_state(b)[13:16] - trs[b].gt_frames["p"][nf - 1])
        assert e < 0.05, e
    assert np.mean(rates) > 0.95


def test_gate_early_accept_changes_no_decision(capi):
    """msckf_hip_set_gate_early_accept: tracks whose |r_o|^2 / sigma^2 is already below the chi-square threshold pass
    without forming S.  Same gate decisions, hence bit-identical states and covariance; the bound is flagged."""
    N, F, nf = 10, 40, 18
    tr = sc.Trajectory(2, 23, N, F, nf)
    res = {}
    for on in (0, 1):
        bt = capi.Batch(1, N, F, N, capi.F32)
        bt.set_gate_early_accept(on)
        bt.initialize(0, tr.cfg, tr.imu0)
        for k in range(nf):
            H.device_frame(bt, 0, tr, k, N)
        res[on] = (bt.imu_state(0), bt.cam_states(0)[0], bt.covariance(0), bt.last_stats(0), bt.last_tracks(0))
        bt.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert res[0][3] == res[1][3] and res[1][3]["n_passed"] > 0
    t0, t1 = res[0][4], res[1][4]                      # columns: motion_ok, tri_valid, gate_pass, included, gamma, p_f
    assert np.array_equal(t0[:, :4], t1[:, :4]) and np.array_equal(t0[:, 5:], t1[:, 5:])
    g0, g1 = t0[:, 4], t1[:, 4]
    assert np.all(g1 >= g0 * (1 - 1e-5)) and np.any(g1 > g0 * 1.001)   # early-accepted tracks report the upper bound


def test_float_long_run_stays_with_the_double_oracle(capi, po):
    """300 free-running frames in float (information-form compression, Joseph update) against the double oracle
    on the same inputs: the float filter must neither drift away nor lose the structure of P (symmetry, PSD up to
    rounding) -- the failure modes a Gram-matrix compression would show first."""
    N, F, nf = 10, 40, 300
    tr = sc.Trajectory(2, 91, N, F, nf)
    o = po.Oracle(po.F64, po.LEAN)
    o.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N, F, N, capi.F32)
    bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(nf):
        fr = tr.frames[k]
        bt.scenario_set(k, 0, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
        H.oracle_frame(o, tr, k, N)
    bt.scenario_commit()
    bt.run_frames(0, nf); bt.sync()
    xd, xo = bt.imu_state(0), o.getImuState()
    P, Po = bt.covariance(0), o.getCovariance()
    assert np.all(np.isfinite(xd)) and np.array_equal(P, P.T)
    w = np.linalg.eigvalsh(P)
    assert w.min() > -1e-6 * w.max()
    assert np.linalg.norm(xd[13:16] - xo[13:16]) < 2e-3 * max(1.0, np.linalg.norm(xo[13:16]))   # position, metres
    assert H.quat_angle(xd[0:4], xo[0:4]) < 1e-3
    assert np.linalg.norm(P - Po) / np.linalg.norm(Po) < 2e-2
    assert np.linalg.norm(xd[13:16] - tr.gt_frames["p"][nf - 1]) < 0.1


def _long_run(capi, tr, N, F, nf, form, step, stop_on_trip=False):
    """free-running float filter over nf frames in chunks of `step`; per chunk: P finite / bit-symmetric / positive up to
    float rounding of lambda_max, the sticky pivot flag read and cleared.  Returns snapshots and the frames at which the
    flag was found raised."""
    bt = capi.Batch(1, N, F, N, capi.F32)
    bt.set_covariance_update(form)
    bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(nf):
        fr = tr.frames[k]
        bt.scenario_set(k, 0, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    snaps, trips = {}, []
    for k0 in range(0, nf, step):
        bt.run_frames(k0, k0 + step); bt.sync()
        tripped = False
        try:
            st = bt.last_stats(0)
        except capi.HipError as e:
            assert "pivot" in str(e)
            tripped = True
            trips.append(k0 + step)
            bt.clear_error_flags(0)
        P = bt.covariance(0)
        healthy = bool(np.all(np.isfinite(P)))
        # the flag must be up no later than the first checkpoint at which P is no longer finite
        assert healthy or trips, ("covariance not finite and no pivot flag was ever raised", form, k0)
        if not healthy or (tripped and stop_on_trip):
            break
        assert np.array_equal(P, P.T), (form, k0)
        w = np.linalg.eigvalsh(P)
        assert w.min() > -4e-6 * w.max(), (form, k0, w.min(), w.max())
        snaps[k0 + step] = (bt.imu_state(0), P)
    bt.close()
    return snaps, trips


def test_float_long_horizon_square_root_gain_form_keeps_p_positive(capi):
    """4 000 free-running frames in float (200 s of flight; the variance of the unobservable global position grows to
    ~2e2 m^2, six orders of magnitude above sigma^2).  The default covariance update P <- P - W W^T has, unlike the
    reference's Joseph form (msckf.h:1394-1403), no PSD guarantee under rounding; measured on MI355X it is nevertheless the
    robust one: over the whole run no factorization of S meets a non-positive pivot (sticky STAT_ERR_PIVOT flag, read through
    last_stats at every checkpoint), P stays finite, bit-symmetric and positive to float rounding, the estimate stays with
    ground truth.  The Joseph form in float on the SAME inputs agrees with it for the first 1 500 frames and later loses
    positive definiteness (its S goes indefinite around frame 2 000 and P turns NaN): the flag is what reports that -- it
    must be raised no later than the first checkpoint with a non-finite P (_long_run asserts it)."""
    N, F, nf, step = 10, 40, 4000, 100
    tr = sc.Trajectory(2, 91, N, F, nf)
    snaps0, trips0 = _long_run(capi, tr, N, F, nf, 0, step)
    assert not trips0 and nf in snaps0, trips0
    for k in (1000, 2000, 3000, 4000):
        assert np.linalg.norm(snaps0[k][0][13:16] - tr.gt_frames["p"][k - 1]) < 1.0, k
    snaps1, trips1 = _long_run(capi, tr, N, F, nf, 1, step, stop_on_trip=True)
    last_common = max(k for k in snaps1 if k in snaps0 and k <= 1500)
    assert last_common >= 1000, (sorted(snaps1)[-3:], trips1)
    (x0, P0), (x1, P1) = snaps0[last_common], snaps1[last_common]
    # two free-running float filters, 75 s in: the global position is unobservable (its std is metres by now) and the two
    # covariance updates round differently at every frame
    assert np.linalg.norm(x0[13:16] - x1[13:16]) < 0.15
    assert np.linalg.norm(P0 - P1) / np.linalg.norm(P1) < 0.05
    print("Joseph form in float: pivot flag first found raised at frame", trips1[:1], "(sqrt-gain form: never in", nf, "frames)")


def test_scenario_cells_can_be_restaged_and_committed_again(capi):
    """Work-lists are stored compactly, so re-staging a cell with a different number of observations moves every later
    offset: run_frames refuses a scenario with uncommitted changes; after the second commit the run equals a batch that
    was staged that way from the start (resident and streamed)."""
    N, F, nf, B = 8, 16, 13, 3
    trs = [sc.Trajectory(2, 60 + b, N, F, nf) for b in range(B)]

    def stage(bt, patched):
        for b, tr in enumerate(trs):
            bt.initialize(b, tr.cfg, tr.imu0)
            for k in range(nf):
                fr = tr.frames[k]
                M, slots, obs = fr["M"], fr["slots"], fr["obs"]
                if patched and k == 10 and b == 1:           # drop the first three tracks of one cell
                    n0 = int(np.sum(M[:3]))
                    M, slots, obs = M[3:], slots[n0:], obs[n0:]
                bt.scenario_set(k, b, tr.imu_for_frame(k), M, slots, obs, 1 if fr["Nw"] == N else 0)
    a, c, e = capi.Batch(B, N, F, N, capi.F32), capi.Batch(B, N, F, N, capi.F32), capi.Batch(B, N, F, N, capi.F32)
    for bt in (a, c, e):
        bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    stage(a, True); a.scenario_commit()
    stage(c, False); c.scenario_commit()
    fr = trs[1].frames[10]
    n0 = int(np.sum(fr["M"][:3]))
    c.scenario_set(10, 1, trs[1].imu_for_frame(10), fr["M"][3:], fr["slots"][n0:], fr["obs"][n0:], 1 if fr["Nw"] == N else 0)
    with pytest.raises(Exception):
        c.run_frames(0, nf)
    c.scenario_commit()
    stage(e, True); e.scenario_commit()
    a.run_frames(0, nf); a.sync()
    c.run_frames(0, nf); c.sync()
    e.run_frames_streamed(0, nf); e.sync()
    for b in range(B):
        for other in (c, e):
            assert np.array_equal(a.covariance(b), other.covariance(b))
            assert np.array_equal(a.imu_state(b), other.imu_state(b))
            assert np.array_equal(a.cam_states(b)[0], other.cam_states(b)[0])


def test_cfg5_geometry_runs_and_stays_consistent(capi):
    """60-camera window (BASELINE.json configs[4] geometry, fewer tracks): exercises NC = 6 QR tiles and the
    global-memory Cholesky path; float."""
    N, F, B, nf = 60, 60, 2, 64
    trs = [sc.Trajectory(5, b, N, F, nf) for b in range(B)]
    bt = capi.Batch(B, N, F, 64, capi.F32)
    bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    for b, tr in enumerate(trs):
        bt.initialize(b, tr.cfg, tr.imu0)
        for k in range(nf):
            fr = tr.frames[k]
            bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    bt.run_frames(0, nf); bt.sync()
    for b in range(B):
        P = bt.covariance(b)
        assert np.all(np.isfinite(P)) and np.array_equal(P, P.T) and np.all(np.diag(P) > 0)
        assert np.linalg.norm(bt.imu_state(b)[13:16] - trs[b].gt_frames["p"][nf - 1]) < 0.1
        assert bt.last_stats(b)["n_passed"] > 0.9 * F


def test_work_list_rules_are_the_same_on_set_tracks_and_scenario_set(capi):
    """The rules for a work-list -- at most f_cap tracks, a track at most m_cap long, every camera slot in [0, n_cap), no slot
    twice within a track -- are stated once in the library.  Each single violation raises with the SAME code and message on
    msckf_hip_set_tracks and on msckf_hip_scenario_set, before anything is staged or written: the valid list given afterwards
    produces the same bits as on a handle that never saw a bad list."""
    N, F, nf = 8, 24, 12
    tr = sc.Trajectory(2, 7, N, F, nf)
    k = nf - 1
    fr = tr.frames[k]
    assert len(fr["M"]) > 0 and max(fr["M"]) <= N - 1
    bad_lists = [   # (M, slots, code, message)
        ([2] * (F + 1), [0, 1] * (F + 1), -7, "more tracks than f_cap"),
        ([N], list(range(N)), -7, "track longer than m_cap"),
        ([3], [0, -1, 2], -22, "camera slot out of range"),
        ([3], [0, N, 2], -22, "camera slot out of range"),
        ([3], [0, 1, 1], -22, "camera slot repeated within a track"),
    ]

    def give_bad_lists(call):
        said = []
        for M, slots, code, msg in bad_lists:
            with pytest.raises(capi.HipError, match=r"\(%d\): %s$" % (code, msg)) as ei:
                call(M, slots, np.zeros((len(slots), 2)))
            said.append(str(ei.value))
        return said

    def per_call(with_bad):
        bt = capi.Batch(1, N, F, N - 1, capi.F64)          # n_cap > m_cap: a track can be too long with every slot valid
        bt.initialize(0, tr.cfg, tr.imu0)
        for j in range(k):
            H.device_frame(bt, 0, tr, j, N)
        bt.propagate_range(0, 1, tr.imu_for_frame(k)); bt.augment_range(0, 1)
        said = give_bad_lists(lambda M, s, o: bt.set_tracks(0, M, s, o)) if with_bad else None
        bt.set_tracks(0, fr["M"], fr["slots"], fr["obs"]); bt.marginalize_range(0, 1)
        out = bt.imu_state(0), bt.cam_states(0)[0], bt.covariance(0), bt.last_stats(0)
        bt.close()
        return out, said

    def resident(with_bad):
        bt = capi.Batch(1, N, F, N - 1, capi.F64)
        bt.initialize(0, tr.cfg, tr.imu0)
        bt.scenario_alloc(nf, sc.IMU_PER_FRAME)

        def cell(j):
            f = tr.frames[j]
            bt.scenario_set(j, 0, tr.imu_for_frame(j), f["M"], f["slots"], f["obs"], 1 if f["Nw"] == N else 0)
        for j in range(nf):
            cell(j)
        said = give_bad_lists(lambda M, s, o: bt.scenario_set(k, 0, tr.imu_for_frame(k), M, s, o, 0)) if with_bad else None
        if with_bad:
            cell(k)
        bt.scenario_commit()
        bt.run_frames(0, nf); bt.sync()
        out = bt.imu_state(0), bt.cam_states(0)[0], bt.covariance(0), bt.last_stats(0)
        bt.close()
        return out, said

    said_by = []
    for run in (per_call, resident):
        fresh, _ = run(False)
        after, said = run(True)
        assert fresh[3]["n_passed"] > 0 and fresh[3] == after[3]
        for x, y in zip(fresh[:3], after[:3]):
            assert np.array_equal(x, y), run.__name__
        said_by.append(said)
    assert said_by[0] == said_by[1]
