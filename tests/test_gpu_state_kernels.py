"""k_propagate, k_augment and k_prune_inplace (msckf_mono_amd/csrc/kernels_state.hip) and the host code in front of them (the
queue of pending IMU samples, the host copy of the IMU state, the keep-list upload) away from "ten equal IMU samples per image".

Inputs, metric and bars are those of tests/test_state_inputs.py, where they are derived on the CPU (its docstring has the table):
covariances are compared entry by entry, scaled by the reference's diagonal (helpers.cov_scaled_err), the state by attitude angle
and relative error of v and p; the reference is the double oracle (the numpy twin where the oracle has no full Q_imu).  P == P^T is
asserted to the bit after every propagate and augment, and everything the code promises to be a copy -- the prune, the sample
chain across calls -- is held with ==.
"""
import numpy as np
import pytest

import helpers as H
from test_state_inputs import (BAR, PRUNE_EMPTY_EXACT, keep_after_prune_empty, prune_patterns, redundant_patterns, redundant_poses,
                               run_prune_empty)

pytestmark = pytest.mark.gpu
PRECS = ["f64", "f32"]
_REF = {}


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def _dt(capi, prec):
    return capi.F64 if prec == "f64" else capi.F32


def _case(po, fam, K, nc, seed=None):
    """inputs of one propagate and the double oracle's answer, computed once per (family, K, window)"""
    key = (fam, K, nc, seed)
    if key not in _REF:
        s = K if seed is None else seed
        imu, cfg, rd = H.state_inputs(fam, s, K)
        P, poses = H.state_spd(nc, s), H.state_cam_poses(nc, s)
        o = H.oracle_window(po.Oracle(po.F64), cfg, imu, P, poses)
        o.propagate(rd)
        _REF[key] = dict(imu=imu, cfg=cfg, rd=rd, P=P, poses=poses, x=o.getImuState(), Pout=o.getCovariance())
    return _REF[key]


def _dist(bt, b, x_ref, P_ref):
    P = bt.covariance(b)
    assert np.array_equal(P, P.T), "P is not symmetric to the bit"
    return H.cov_scaled_err(P, P_ref), H.imu_state_err(bt.imu_state(b), x_ref)


def _hold(d, prec, what):
    assert d[0] <= BAR[prec]["cov"] and d[1] <= BAR[prec]["state"], (what, prec, "cov %.3e (bar %.3e) state %.3e (bar %.3e)" % (d[0], BAR[prec]["cov"], d[1], BAR[prec]["state"]))


# ------------------------------------------------------------------------------------------------- propagate and augment
@pytest.mark.parametrize("fam", H.STATE_FAMILIES)
@pytest.mark.parametrize("prec", PRECS)
def test_one_propagate_against_the_double_oracle(capi, po, prec, fam):
    """one propagate_range of K samples on an 11-camera window with a random SPD covariance, K on both sides of the group size
    16 and of twice it; float starts from the oracle's inputs (teacher forcing)"""
    bt = capi.Batch(1, 11, 1, 11, _dt(capi, prec))
    worst = np.zeros(2)
    fails = []
    for K in (1, 15, 16, 17, 31, 32, 33, 40):
        c = _case(po, fam, K, 11)
        H.device_window(bt, 0, c["cfg"], c["imu"], c["P"], c["poses"])
        bt.propagate_range(0, 1, c["rd"])
        d = _dist(bt, 0, c["x"], c["Pout"])
        worst = np.maximum(worst, d)
        if d[0] > BAR[prec]["cov"] or d[1] > BAR[prec]["state"]:
            fails.append((K, "%.3e" % d[0], "%.3e" % d[1]))
    print("FIGURE propagate %s %-8s worst cov %.3e (bar %.3e) state %.3e (bar %.3e)" % (prec, fam, worst[0], BAR[prec]["cov"], worst[1], BAR[prec]["state"]))
    bt.close()
    assert not fails, (prec, fam, fails)


@pytest.mark.parametrize("prec", PRECS)
def test_pic_write_back_on_the_tile_edges(capi, po, prec):
    """P_IC <- Phi_total P_IC goes in tiles of 16 camera columns: window sizes on both sides of every tile edge of 6 ncam, the
    empty window and the full one, on one n_cap = 63 handle; all of P, and the last camera's rows and columns on their own"""
    bt = capi.Batch(1, 63, 1, 63, _dt(capi, prec))
    worst = np.zeros(3)
    fails = []
    for nc in (0, 1, 2, 3, 5, 6, 10, 11, 21, 22, 42, 43, 63):
        c = _case(po, "mixed", 17, nc, seed=200 + nc)
        H.device_window(bt, 0, c["cfg"], c["imu"], c["P"], c["poses"])
        bt.propagate_range(0, 1, c["rd"])
        assert bt.num_cam_states(0) == nc
        d = _dist(bt, 0, c["x"], c["Pout"])
        last = 0.0
        if nc:
            s = np.sqrt(np.diag(c["Pout"]))
            E = np.abs(bt.covariance(0) - c["Pout"]) / np.outer(s, s)
            last = max(E[-6:, :].max(), E[:, -6:].max())
        worst = np.maximum(worst, [d[0], d[1], last])
        if d[0] > BAR[prec]["cov"] or d[1] > BAR[prec]["state"] or last > BAR[prec]["cov"]:
            fails.append((nc, "%.3e" % d[0], "%.3e" % d[1], "%.3e" % last))
    print("FIGURE tile_edges %s worst cov %.3e last camera %.3e (bar %.3e) state %.3e" % (prec, worst[0], worst[2], BAR[prec]["cov"], worst[1]))
    bt.close()
    assert not fails, (prec, fails)


def test_grown_window_free_running_and_the_64th_augment(capi, po):
    """63 x (propagate of K = 1, 16, 17, 33 in turn, augment) from initialize, double, free-running beside the oracle, checked
    after every step; then a 64th augment: the n_cap flag, and nothing else, changes"""
    imu, cfg, _ = H.state_inputs("mixed", 63, 1)
    o = po.Oracle(po.F64)
    o.initialize(cfg, imu)
    bt = capi.Batch(1, 63, 1, 63, capi.F64)
    bt.initialize(0, cfg, imu)
    worst = np.zeros(3)
    fails = []
    for k in range(63):
        rd = H.state_inputs("mixed", 1000 + k, (1, 16, 17, 33)[k % 4])[2]
        o.propagate(rd); bt.propagate_range(0, 1, rd)
        d = _dist(bt, 0, o.getImuState(), o.getCovariance())
        o.augmentState(k, 0.0); bt.augment_range(0, 1)
        assert bt.num_cam_states(0) == k + 1 == o.getNumCamStates()
        d = np.maximum(d, _dist(bt, 0, o.getImuState(), o.getCovariance()))
        cd, co = bt.cam_states(0)[0], o.getCamStates()[0]
        dc = max(max(H.quat_angle(a[:4], b[:4]), H.rel(a[4:], b[4:])) for a, b in zip(cd, co))
        worst = np.maximum(worst, [d[0], d[1], dc])
        if d[0] > BAR["f64"]["cov"] or max(d[1], dc) > BAR["f64"]["state"]:
            fails.append((k, "%.3e" % d[0], "%.3e" % d[1], "%.3e" % dc))
    print("FIGURE grown_window f64 worst cov %.3e (bar %.3e) state %.3e camera %.3e (bar %.3e)" % (worst[0], BAR["f64"]["cov"], worst[1], worst[2], BAR["f64"]["state"]))
    before = (bt.covariance(0), bt.cam_states(0)[0], bt.imu_state(0))
    assert bt.error_flags(0) == 0
    bt.augment_range(0, 1)
    assert bt.error_flags(0) & 1                                        # STAT_ERR_NCAP
    assert bt.num_cam_states(0) == 63
    after = (bt.covariance(0), bt.cam_states(0)[0], bt.imu_state(0))
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    bt.clear_error_flags(0)
    assert bt.error_flags(0) == 0
    bt.close()
    assert not fails, fails[:8]


@pytest.mark.parametrize("prec", PRECS)
def test_splitting_a_block_of_samples(capi, po, prec):
    """K = 33 in one call, as 16 + 17, and as 33 calls of one sample: each within the bar of the oracle, and of each other.  The
    state chain is sequential and one call hands the next its last state as a copy (imu, and the anchors written from it), so
    the IMU state comes out the same to the bit however the block is cut.  The kernel promises no such thing for P: P_IC is
    multiplied by the product of the call's Phi, and P_II, equal to the bit in double and for 16 + 17 in float, differs in
    the last bits between one call and 33 single-sample calls in float (6.0e-6 against 6.2e-6 off the oracle).  Held to the bar."""
    c = _case(po, "mixed", 33, 11)
    bt = capi.Batch(3, 11, 1, 11, _dt(capi, prec))
    for b in range(3):
        H.device_window(bt, b, c["cfg"], c["imu"], c["P"], c["poses"])
    bt.propagate_range(0, 1, c["rd"])
    bt.propagate_range(1, 1, c["rd"][:16]); bt.propagate_range(1, 1, c["rd"][16:])
    for k in range(33):
        bt.propagate_range(2, 1, c["rd"][k:k + 1])
    P = [bt.covariance(b) for b in range(3)]
    for b in range(3):
        d = _dist(bt, b, c["x"], c["Pout"])
        print("FIGURE split %s way %d cov %.3e state %.3e" % (prec, b, d[0], d[1]))
        _hold(d, prec, ("split", b))
    for b in (1, 2):
        assert np.array_equal(bt.imu_state(b), bt.imu_state(0)), b
        assert H.cov_scaled_err(P[b], P[0]) <= BAR[prec]["cov"], (b, H.cov_scaled_err(P[b], P[0]))
    bt.close()


def _fused_inputs(K, B, nf):
    return [H.state_inputs("mixed", b, 1)[:2] for b in range(B)], [[H.state_inputs("mixed", 100 + 10 * b + k, K)[2] for k in range(nf)] for b in range(B)]


@pytest.mark.parametrize("K", [17, 33])
@pytest.mark.parametrize("prec", PRECS)
def test_fused_route_with_more_than_one_group(capi, po, prec, K):
    """run_frames with K = 17 and 33 samples per frame: k_propagate with the fused augment, and the window size committed by the
    next frame's propagate once a prune rides on the downdate.  Equal to the per-call path to the bit; double also against the
    oracle."""
    N, B, nf = 4, 2, 6
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))
    init, rds = _fused_inputs(K, B, nf)
    a, c = capi.Batch(B, N, 1, N, _dt(capi, prec)), capi.Batch(B, N, 1, N, _dt(capi, prec))
    c.scenario_alloc(nf, K)
    for b in range(B):
        a.initialize(b, init[b][1], init[b][0]); c.initialize(b, init[b][1], init[b][0])
        for k in range(nf):
            c.scenario_set(k, b, rds[b][k], *E, 1 if k >= N - 1 else 0)
    c.scenario_commit()
    c.run_frames(0, nf); c.sync()
    for b in range(B):
        o = po.Oracle(po.F64)
        o.initialize(init[b][1], init[b][0])
        for k in range(nf):
            a.propagate_range(b, 1, rds[b][k]); a.augment_range(b, 1); a.set_tracks(b, *E)
            o.propagate(rds[b][k]); o.augmentState(k, 0.0)
            if a.num_cam_states(b) == N:
                a.drop_oldest_range(b, 1, 1); o.dropOldest(1)
        assert a.num_cam_states(b) == c.num_cam_states(b) == N - 1
        assert np.array_equal(a.covariance(b), c.covariance(b)), b
        assert np.array_equal(a.imu_state(b), c.imu_state(b)), b
        assert np.array_equal(a.cam_states(b)[0], c.cam_states(b)[0]), b
        if prec == "f64":
            d = _dist(c, b, o.getImuState(), o.getCovariance())
            print("FIGURE fused f64 K %d b %d cov %.3e state %.3e" % (K, b, d[0], d[1]))
            _hold(d, prec, ("fused", K, b))
    a.close(); c.close()


@pytest.mark.parametrize("prec", PRECS)
def test_full_q_trajectory_in_a_mixed_batch(capi, prec):
    """B = 3, the middle trajectory with a whole 12 x 12 Q_imu: the diagonal-Q and the full-Q instantiation both launch over the
    range.  K = 33, `mixed`.  Every trajectory equals its solo run to the bit, and the numpy twin holding the same Q_imu to the bar."""
    from test_full_noise import correlated
    B, K, nc = 3, 33, 11
    cases = []
    for b in range(B):
        imu, cfg, rd = H.state_inputs("mixed", 300 + b, K)
        if b == 1:
            cfg = dict(cfg, Q_imu=correlated(H.STATE_Q_DIAG, 77))
        cases.append((imu, cfg, rd, H.state_spd(nc, 300 + b), H.state_cam_poses(nc, 300 + b)))
    bt = capi.Batch(B, nc, 1, nc, _dt(capi, prec))
    for b, (imu, cfg, rd, P, poses) in enumerate(cases):
        H.device_window(bt, b, cfg, imu, P, poses)
    bt.propagate_range(0, B, np.stack([c[2] for c in cases]))
    for b, (imu, cfg, rd, P, poses) in enumerate(cases):
        solo = capi.Batch(1, nc, 1, nc, _dt(capi, prec))
        H.device_window(solo, 0, cfg, imu, P, poses)
        solo.propagate_range(0, 1, rd)
        assert np.array_equal(solo.covariance(0), bt.covariance(b)) and np.array_equal(solo.imu_state(0), bt.imu_state(b)), b
        solo.close()
        tw = H.TwinMutant(cfg, imu, None, P, nc)
        tw.propagate_block(rd)
        d = _dist(bt, b, tw.imu29(), tw.P)
        print("FIGURE full_q %s b %d (%s Q) cov %.3e state %.3e" % (prec, b, "full" if b == 1 else "diagonal", d[0], d[1]))
        _hold(d, prec, ("full_q", b))
        if b == 1:      # the off-diagonal part of Q_imu is far above the bar: the twin with only the diagonal is not matched
            td = H.TwinMutant(dict(cfg, Q_imu=np.diag(H.STATE_Q_DIAG)), imu, None, P, nc)
            td.propagate_block(rd)
            assert H.cov_scaled_err(bt.covariance(b), td.P) > 10 * BAR[prec]["cov"]
    bt.close()


@pytest.mark.parametrize("prec", PRECS)
def test_host_mirror_over_forty_queued_samples(capi, po, prec):
    """40 msckf_hip_propagate calls of one `jitter` sample each (dT = 0 among them): they wait in the pending queue while the host
    copy of the IMU state advances.  getImuState from the host copy, then -- after a K = 0 propagate_range, which flushes the
    queue as one K = 40 launch and drops the copy -- from the device, and the oracle: all within the state bar; the covariance
    the flush leaves within the covariance bar."""
    imu, cfg, rd = H.state_inputs("jitter", 40, 40)
    f = capi.MSCKF(_dt(capi, prec), n_cap=4, f_cap=4, m_cap=4)
    o = po.Oracle(po.F64)
    f.initialize(cfg, imu); o.initialize(cfg, imu)
    for r7 in rd:
        f.propagate(r7)
    o.propagate(rd)
    mirror = f.getImuState()
    assert f.batch.L.msckf_hip_propagate_range(f.batch.h, 0, 1, None, 0) == 0
    dev = f.getImuState()
    ref = o.getImuState()
    d = (H.imu_state_err(mirror, ref), H.imu_state_err(dev, ref), H.imu_state_err(mirror, dev))
    dc = _dist(f.batch, 0, ref, o.getCovariance())[0]
    print("FIGURE mirror %s host-oracle %.3e device-oracle %.3e host-device %.3e (bar %.3e) cov %.3e" % ((prec,) + d + (BAR[prec]["state"], dc)))
    assert max(d) <= BAR[prec]["state"], d
    assert dc <= BAR[prec]["cov"], dc
    f.batch.close()


# ------------------------------------------------------------------------------------------------------------------ prune
def _int_cov(D, seed):
    """symmetric D x D matrix of distinct integers below 2^24 (exact in float), in a seeded random order"""
    from msckf_mono_amd import scenario as sc
    cnt = D * (D + 1) // 2
    vals = 1 + 211 * np.arange(cnt, dtype=np.int64) + (seed % 200)
    assert vals.max() < 2 ** 24
    vals = vals[np.argsort(sc.SplitMix64(0x1A7C0000 + seed).uniform(cnt), kind="stable")]
    P = np.zeros((D, D))
    iu = np.triu_indices(D)
    P[iu] = vals
    return P + np.triu(P, 1).T


def _f32_poses(n, seed):
    return H.state_cam_poses(n, seed).astype(np.float32).astype(np.float64)


def _gather_idx(keep):
    return np.r_[0:15, np.array([15 + 6 * k + j for k in keep for j in range(6)], dtype=np.int64)]


def _check_pruned(bt, b, P0, poses0, keep, what):
    idx = _gather_idx(keep)
    assert bt.num_cam_states(b) == len(keep), what
    assert np.array_equal(bt.covariance(b), P0[np.ix_(idx, idx)]), what
    assert np.array_equal(bt.cam_states(b)[0], poses0[list(keep)].reshape(-1, 7)), what


def _stage_window(f, o, n, seed, poses=None):
    """integer covariance and distinct float-exact poses on a filter that holds n camera states, and on its oracle; the poses as
    the device returns them are the reference"""
    P0 = _int_cov(15 + 6 * n, seed)
    poses = _f32_poses(n, seed) if poses is None else poses
    f.batch.set_covariance(0, P0)
    for i in range(n):
        f.batch.set_cam_pose(0, i, poses[i])
    back = f.getCamStates()[0]
    assert np.array_equal(back, poses)
    assert np.array_equal(f.getCovariance(), P0)
    o.setCovariance(P0)
    for i in range(n):
        o.setCamPose(i, back[i])
    return P0, back


@pytest.mark.parametrize("n_cap", [40, 41, 63])
@pytest.mark.parametrize("prec", PRECS)
def test_keep_lists_through_the_reference_api(capi, po, prec, n_cap):
    """Full windows of 40, 41 and 63 camera states (ld 256 | 272 | 400: both instantiations of k_prune_inplace; D = 255, 261, 393,
    no multiple of the chunk of 64 or 48 columns), no update() call.  pruneEmptyStates after addFeatures on the surviving
    frames only: it drops the leading run of states without features (test_state_inputs.py), which gives "all but the oldest",
    "only the newest", "none" (D = 15) and "all" (a no-op) exactly, and the leading run of the other patterns.  The interior keep
    lists -- every other, every third, two random subsets of the slots 1 .. n - 4 -- go through pruneRedundantStates without
    tracks, the other user of the host keep list.  After either: covariance == P[idx, idx], poses and ids == the kept ones,
    pruned ids and poses == the oracle's, all with ==."""
    n = n_cap
    imu, cfg, rd = H.state_inputs("nominal", 3, 64)
    f = capi.MSCKF(_dt(capi, prec), n_cap=n_cap, f_cap=4, m_cap=n_cap)
    for name, survive in prune_patterns(n).items():
        c = dict(cfg, max_cam_states=0)
        o = po.Oracle(po.F64)
        f.initialize(c, imu); o.initialize(c, imu)
        run_prune_empty(f, survive, rd, f.propagate, f.augmentState, f.addFeatures, lambda: None)
        run_prune_empty(o, survive, rd, o.propagate, o.augmentState, o.addFeatures, lambda: None)
        assert f.getNumCamStates() == n
        P0, poses0 = _stage_window(f, o, n, n + len(name))
        f.pruneEmptyStates(); o.pruneEmptyStates()
        keep = keep_after_prune_empty(survive)
        if name in PRUNE_EMPTY_EXACT:
            assert keep == list(np.nonzero(survive)[0]), name
        _check_pruned(f.batch, 0, P0, poses0, keep, name)
        assert list(f.getCamStates()[1]) == [100 + k for k in keep] == list(o.getCamStates()[1]), name
        assert np.array_equal(f.getCovariance(), o.getCovariance()), name
        assert np.array_equal(f.getCamStates()[0], o.getCamStates()[0].reshape(-1, 7)), name
        gone = [k for k in range(n) if k not in keep]
        pd, pr = f.getPrunedStatesFull(), o.getPrunedStates()
        assert list(pd[:, 8]) == [100 + k for k in gone] == list(pr[:, 8]), name
        assert np.array_equal(pd[:, :7], poses0[gone].reshape(-1, 7)) and np.array_equal(pd[:, :7], pr[:, :7].reshape(-1, 7)), name
    for name, removed in redundant_patterns(n).items():
        c = dict(cfg, max_cam_states=n - len(removed))
        o = po.Oracle(po.F64)
        f.initialize(c, imu); o.initialize(c, imu)
        for k in range(n):
            f.propagate(rd[k:k + 1]); f.augmentState(100 + k, 0.01 * k)
            o.propagate(rd[k:k + 1]); o.augmentState(100 + k, 0.01 * k)
        poses = redundant_poses(n, removed, n).astype(np.float32).astype(np.float64)
        P0, poses0 = _stage_window(f, o, n, n + 50 + len(name), poses)
        x0 = f.getImuState()
        f.pruneRedundantStates(); o.pruneRedundantStates()
        keep = [k for k in range(n) if k not in removed]
        _check_pruned(f.batch, 0, P0, poses0, keep, name)
        assert list(f.getCamStates()[1]) == [100 + k for k in keep] == list(o.getCamStates()[1]), name
        assert np.array_equal(f.getCovariance(), o.getCovariance()) and np.array_equal(f.getImuState(), x0), name
        assert list(f.getPrunedStates()) == [100 + k for k in removed] == [int(i) for i in o.getPrunedStates()[:, 8]], name
    f.batch.close()


@pytest.mark.parametrize("n_cap,windows", [(63, (63, 41, 7, 0)), (40, (40, 17, 7, 0))])
@pytest.mark.parametrize("prec", PRECS)
def test_drop_oldest_range_clamps_per_trajectory(capi, prec, n_cap, windows):
    """one drop_oldest_range launch over four trajectories with different windows (the full one, an empty one), n from 0 to
    beyond every window: each trajectory drops min(n, its own window), as a gather to the bit"""
    bt = capi.Batch(4, n_cap, 1, n_cap, _dt(capi, prec))
    imu, cfg, _ = H.state_inputs("nominal", 5, 1)
    for b in range(4):
        bt.initialize(b, cfg, imu)
    for n in (0, 1, 2, 6, 62, 63, 70):
        staged = []
        for b, w in enumerate(windows):
            P0, poses = _int_cov(15 + 6 * w, 10 * n + b), _f32_poses(w, 10 * n + b)
            bt.set_covariance(b, P0)
            for i in range(w):
                bt.set_cam_pose(b, i, poses[i])
            back = bt.cam_states(b)[0]
            assert np.array_equal(back, poses.reshape(-1, 7))
            staged.append((P0, back))
        bt.drop_oldest_range(0, 4, n)
        for b, w in enumerate(windows):
            _check_pruned(bt, b, staged[b][0], staged[b][1], list(range(min(n, w), w)), (n, b))
            assert bt.error_flags(b) == 0
    bt.close()


@pytest.mark.parametrize("prec", PRECS)
def test_n_drop_above_one_inside_run_frames(capi, prec):
    """scenario_set(..., n_drop): three states dropped on one frame, none on the next, two and one later -- on the downdate's back
    (every frame but the call's last) and with the prune's own launch (the last).  Equal to the per-call sequence to the bit."""
    N, B, nf, K = 6, 2, 8, 10
    drops = [0, 0, 0, 0, 3, 0, 2, 1]
    E = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))
    init = [H.state_inputs("nominal", 40 + b, 1)[:2] for b in range(B)]
    rds = [[H.state_inputs("nominal", 400 + 10 * b + k, K)[2] for k in range(nf)] for b in range(B)]
    a, c = capi.Batch(B, N, 1, N, _dt(capi, prec)), capi.Batch(B, N, 1, N, _dt(capi, prec))
    c.scenario_alloc(nf, K)
    for b in range(B):
        a.initialize(b, init[b][1], init[b][0]); c.initialize(b, init[b][1], init[b][0])
        for k in range(nf):
            c.scenario_set(k, b, rds[b][k], *E, drops[k] if b == 0 else (1 if k >= 4 else 0))
    c.scenario_commit()
    c.run_frames(0, nf); c.sync()
    for b in range(B):
        for k in range(nf):
            a.propagate_range(b, 1, rds[b][k]); a.augment_range(b, 1); a.set_tracks(b, *E)
            nd = drops[k] if b == 0 else (1 if k >= 4 else 0)
            if nd:
                a.drop_oldest_range(b, 1, nd)
        assert a.num_cam_states(b) == c.num_cam_states(b) == (2 if b == 0 else 4), b
        assert np.array_equal(a.covariance(b), c.covariance(b)), b
        assert np.array_equal(a.imu_state(b), c.imu_state(b)), b
        assert np.array_equal(a.cam_states(b)[0], c.cam_states(b)[0]), b
    a.close(); c.close()
