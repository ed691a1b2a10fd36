"""The inputs, the metric and the bars of tests/test_gpu_state_kernels.py, checked on the CPU: no kernel runs here.

The state kernels (k_propagate, k_augment, k_prune_inplace) are held to max_ij |P_ij - Pref_ij| / sqrt(Pref_ii Pref_jj)
(helpers.cov_scaled_err) and to the attitude angle / relative error of v and p (helpers.imu_state_err) on inputs whose
process noise is large against P_II (helpers.STATE_Q_DIAG: every noisy diagonal entry of P_II starts at 0.1 s x its Q_imu entry,
so one sample adds dT / 0.1 s = 2.5e-2 .. 2e-1 of it).  The bars come from two distances measured HERE, over the five reading
families x K in {1, 10, 16, 17, 33, 40} x windows of 0, 3, 11 and 22 camera states with a random SPD covariance:

  d64  double oracle (Pade expm, dense products) against the numpy/scipy twin: two correct double implementations
  d32  float oracle against the double oracle

    family     d64 cov    d64 state   d32 cov    d32 state
    nominal    6.14e-15   1.96e-16    1.38e-05   2.58e-07
    still      2.57e-15   1.50e-16    3.32e-05   1.52e-07
    fast       3.32e-15   9.62e-16    9.38e-06   4.61e-07
    jitter     2.18e-15   1.38e-16    1.39e-05   3.92e-07
    mixed      2.13e-15   4.34e-16    1.49e-05   3.07e-07
    max        6.2e-15    9.7e-16     3.4e-05    4.7e-07      (D64_COV, D64_STATE, D32_COV, D32_STATE, rounded up)

  double bar = 8 x max d64 (a different, equally valid summation order: MFMA chain against dense product):
               4.96e-14 covariance, 7.76e-15 state
  float bar  = 4 x max d32:  1.36e-04 covariance, 1.88e-06 state

`fast` (|omega - b_g| dT = 0.5 rad) does not raise d32: it stays at 0.5 rad in float too.  dT = 0 is finite in both references and is
part of `jitter` (samples 5 and 20).  `still` (omega - b_g = 0 exactly) is finite in both.

One deliberate mistake in the twin (helpers.TwinMutant), `mixed`, K = 33, 11 camera states, distance to the unmutated twin:
    a  no G Q G^T dT for sample 16            covariance 3.65e-02  = 268 x the float bar
    b  sample 16 anchored before sample 0     covariance 1.30e-01  = 955 x
    c  last camera's P_IC columns untouched   covariance 1.05e-01  = 772 x
    d  p advanced with the new velocity       state      4.17e-03  = 2200 x the float state bar

Prune patterns: pruneEmptyStates (msckf.h:685-717) only ever removes a LEADING run of camera states without features (up to
the first one that has some, at most size - max_cam_states of them).  Of the keep patterns of the GPU module it therefore
produces exactly: all but the oldest, only the newest, none, all; "every other" / "every third" / a random subset lose only their
leading run, and "all but the newest" / "only the oldest" lose nothing.  The interior patterns reach the same kernel (host keep
list, k_prune_inplace) through pruneRedundantStates without feature tracks (msckf.h:453-682, findRedundantCamStates
:1049-1098): a camera state within the redundancy thresholds of the keyframe before it goes; state 0 and the last three always
stay.  Both are checked here on the oracle, without update(): the reference's update() only moves observations between lists and is
not needed for either prune to be well defined.
"""
import numpy as np
import pytest

import helpers as H

KS = (1, 10, 16, 17, 33, 40)
WINDOWS = (0, 3, 11, 22)
D64_COV, D64_STATE, D32_COV, D32_STATE = 6.2e-15, 9.7e-16, 3.4e-5, 4.7e-7          # the table's maxima
BAR = {"f64": dict(cov=8 * D64_COV, state=8 * D64_STATE), "f32": dict(cov=4 * D32_COV, state=4 * D32_STATE)}
TABLE = {   # d64 cov, d64 state, d32 cov, d32 state per family, as measured (the docstring's table)
    "nominal": (6.14e-15, 1.96e-16, 1.38e-05, 2.58e-07), "still": (2.57e-15, 1.50e-16, 3.32e-05, 1.52e-07),
    "fast": (3.32e-15, 9.62e-16, 9.38e-06, 4.61e-07), "jitter": (2.18e-15, 1.38e-16, 1.39e-05, 3.92e-07),
    "mixed": (2.13e-15, 4.34e-16, 1.49e-05, 3.07e-07)}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def measure(po, fam):
    """largest d64 / d32 (covariance, state) of one family over KS x WINDOWS; every result finite"""
    w = np.zeros(4)
    for K in KS:
        for nc in WINDOWS:
            imu, cfg, rd = H.state_inputs(fam, K, K)
            P, poses = H.state_spd(nc, K), H.state_cam_poses(nc, K)
            o64 = H.oracle_window(po.Oracle(po.F64), cfg, imu, P, poses)
            o32 = H.oracle_window(po.Oracle(po.F32), cfg, imu, P, poses)
            tw = H.TwinMutant(cfg, imu, None, P, nc)
            o64.propagate(rd); o32.propagate(rd); tw.propagate_block(rd)
            P64, P32, x64, x32 = o64.getCovariance(), o32.getCovariance(), o64.getImuState(), o32.getImuState()
            for a in (P64, P32, tw.P, x64, x32, tw.imu29()):
                assert np.all(np.isfinite(a)), (fam, K, nc)
            w = np.maximum(w, [H.cov_scaled_err(tw.P, P64), H.imu_state_err(tw.imu29(), x64), H.cov_scaled_err(P32, P64), H.imu_state_err(x32, x64)])
    return w


@pytest.mark.parametrize("fam", H.STATE_FAMILIES)
def test_measured_distances_are_the_recorded_ones(po, fam):
    """the table above is what this machine measures (to 2 %: libm / BLAS may round differently), and no family exceeds the maxima the bars are built on"""
    w = measure(po, fam)
    print(fam, " ".join("%.2e" % x for x in w))
    assert np.all(w <= [D64_COV, D64_STATE, D32_COV, D32_STATE]), w
    # the float distances are reproducible; the double ones are a handful of ulps and only held from above
    assert np.allclose(w[2:], TABLE[fam][2:], rtol=0.02), (w, TABLE[fam])


def test_inputs_follow_their_family_and_the_noise_scale():
    P = H.state_spd(11, 1)
    assert np.array_equal(P, P.T) and np.all(np.linalg.eigvalsh(P) > 0)
    assert np.all(np.linalg.eigvalsh(P.astype(np.float32).astype(np.float64)) > 0)
    for fam in H.STATE_FAMILIES:
        imu, cfg, rd = H.state_inputs(fam, 2, 40)
        imu2, _, rd2 = H.state_inputs(fam, 2, 40)
        assert np.array_equal(rd, rd2) and np.array_equal(imu, imu2)            # a function of (family, seed) alone
        assert abs(np.linalg.norm(imu[:4]) - 1) < 1e-15
        wdt = np.linalg.norm(rd[:, :3] - imu[4:7], axis=1) * rd[:, 6]
        if fam == "still":
            assert np.all(rd[:, :3] == imu[4:7]) and np.all(rd[:, :3].astype(np.float32) == imu[4:7].astype(np.float32))
        if fam == "fast":
            assert np.allclose(wdt, H.STATE_FAST_ANGLE, rtol=1e-12)
        if fam == "jitter":
            assert set(rd[:, 6]) == set(H.STATE_JITTER_DT) | {0.0} and all(rd[k, 6] == 0 for k in H.STATE_JITTER_ZERO_AT)
        if fam == "mixed":
            assert wdt[14] == 0 and wdt[18] == 0 and abs(wdt[15] - 0.5) < 1e-12 and abs(wdt[17] - 0.5) < 1e-12 and rd[16, 6] == 0.01
            assert len(set(rd[:, 6])) > 2
        # one sample's process noise against the P_II diagonal it feeds (theta b_g v b_a), at the start and -- P grows -- at the end
        tw = H.TwinMutant(cfg, imu, None, H.state_spd(3, 2), 3)
        q = np.array(cfg["Q_imu_diag"])
        for when in range(2):
            for dT in rd[rd[:, 6] > 0, 6]:
                assert np.all(q * dT >= 1e-3 * np.diag(tw.P)[:12]), (fam, when)
            tw.propagate_block(rd)


@pytest.mark.parametrize("mut", ["a", "b", "c", "d"])
def test_each_mutant_lies_ten_bars_from_the_twin(mut):
    imu, cfg, rd = H.state_inputs("mixed", 33, 33)
    P = H.state_spd(11, 33)
    ref, t = H.TwinMutant(cfg, imu, None, P, 11), H.TwinMutant(cfg, imu, mut, P, 11)
    ref.propagate_block(rd); t.propagate_block(rd)
    dc, ds = H.cov_scaled_err(t.P, ref.P), H.imu_state_err(t.imu29(), ref.imu29())
    print(mut, "cov %.2e state %.2e" % (dc, ds))
    for prec in ("f64", "f32"):
        assert max(dc / BAR[prec]["cov"], ds / BAR[prec]["state"]) >= 10, (mut, prec, dc, ds)
    # and each is seen by the metric it belongs to
    assert (ds if mut == "d" else dc) >= 10 * BAR["f32"]["state" if mut == "d" else "cov"]


# ------------------------------------------------------------------------------------------------------------ prune patterns
def prune_patterns(n):
    """name -> survive[n] (frames whose camera state is given a feature) of the GPU module's keep patterns"""
    from msckf_mono_amd import scenario as sc
    rng = sc.SplitMix64(0x9A77E000 + n)
    r1, r2 = rng.uniform(n) < 0.5, rng.uniform(n) < 0.8
    i = np.arange(n)
    return {"all_but_oldest": i > 0, "all_but_newest": i < n - 1, "every_other": i % 2 == 1, "every_third": i % 3 == 2,
            "only_newest": i == n - 1, "only_oldest": i == 0, "none": i < 0, "all": i >= 0, "random_half": r1, "random_most": r2}


def keep_after_prune_empty(survive):
    """pruneEmptyStates with max_cam_states = 0 (msckf.h:685-717): the leading states without features go"""
    n = len(survive)
    lead = 0
    while lead < n and not survive[lead]:
        lead += 1
    return list(range(lead, n))


PRUNE_EMPTY_EXACT = ("all_but_oldest", "only_newest", "none", "all")      # patterns pruneEmptyStates produces as intended


def redundant_patterns(n):
    """name -> removed slots for pruneRedundantStates without tracks: interior slots only (1 .. n - 4), at least two"""
    from msckf_mono_amd import scenario as sc
    rng = sc.SplitMix64(0x4ED00000 + n)
    inner = np.arange(1, n - 3)
    return {"every_other": [int(i) for i in inner if i % 2 == 1], "every_third": [int(i) for i in inner if i % 3 != 2],
            "random_half": [int(i) for i in inner[rng.uniform(len(inner)) < 0.5]], "random_few": [int(i) for i in inner[rng.uniform(len(inner)) < 0.2]]}


def redundant_poses(n, removed, seed):
    """distinct poses of which exactly the `removed` slots lie within the redundancy thresholds (0.005 rad, 0.05 m) of the
    keyframe before them: 2e-4 rad and 1e-3 m off the pose of the slot in front"""
    poses = H.state_cam_poses(n, seed)
    for k in sorted(removed):
        q = poses[k - 1, :4] + 1e-4 * np.array([0.3, 1.0, -0.5, 0.7])
        poses[k] = np.concatenate([q / np.linalg.norm(q), poses[k - 1, 4:] + 1e-3 * np.array([0.5, -0.6, 0.4])])
    return poses


def run_prune_empty(f, survive, rd, propagate, augment, add, prune):
    for k, s in enumerate(survive):
        propagate(rd[k:k + 1]); augment(100 + k, 0.01 * k)
        if s:
            add([[0.01 * k, -0.02]], [5000 + k])
    prune()


@pytest.mark.parametrize("n", [7, 40])
def test_prune_patterns_on_the_oracle(po, n):
    imu, cfg, rd = H.state_inputs("nominal", 3, 64)
    cfg = dict(cfg, max_cam_states=0)
    for name, survive in prune_patterns(n).items():
        o = po.Oracle(po.F64)
        o.initialize(cfg, imu)
        run_prune_empty(o, survive, rd, o.propagate, o.augmentState, o.addFeatures, o.pruneEmptyStates)
        keep = keep_after_prune_empty(survive)
        assert o.getNumCamStates() == len(keep), name
        assert list(o.getCamStates()[1]) == [100 + k for k in keep], name
        assert list(o.getPrunedStates()[:, 8]) == [100 + k for k in range(n) if k not in keep], name
        assert (keep == list(np.nonzero(survive)[0])) == (name in PRUNE_EMPTY_EXACT), name
    # interior keep lists: pruneRedundantStates without tracks is a pure gather on the oracle
    if n < 20:
        return
    for name, removed in redundant_patterns(n).items():
        assert len(removed) >= 2, name
        o = po.Oracle(po.F64)
        o.initialize(dict(cfg, max_cam_states=n - len(removed)), imu)
        for k in range(n):
            o.propagate(rd[k:k + 1]); o.augmentState(100 + k, 0.01 * k)
        poses = redundant_poses(n, removed, n)
        for k in range(n):
            o.setCamPose(k, poses[k])
        P0, x0 = o.getCovariance(), o.getImuState()
        o.pruneRedundantStates()
        keep = [k for k in range(n) if k not in removed]
        assert list(o.getCamStates()[1]) == [100 + k for k in keep], name
        assert list(o.getPrunedStates()[:, 8]) == [100 + k for k in removed], name
        idx = np.r_[0:15, np.concatenate([15 + 6 * k + np.arange(6) for k in keep])]
        assert np.array_equal(o.getCovariance(), P0[np.ix_(idx, idx)]) and np.array_equal(o.getImuState(), x0), name
        assert np.array_equal(o.getCamStates()[0], poses[keep]), name
