"""Ragged batches and batches beyond 64 against the CPU oracle.

Every other GPU module runs its batches in lockstep: one window size, every trajectory updating on every frame, all of them
dropping their oldest camera on the same frame, at most 64 trajectories.  The kernels take their launch shapes from the
handle's capacity and the range, and each workgroup then reads its own window size, row count and drop flag.  Here one range
holds windows of 5 to 40 cameras at once (helpers.RAGGED: the sizes straddle the one-launch update's limit of 14 cameras and
the single-level factorizations' of 31), a trajectory that never updates, one that is handed empty track lists while its
neighbours update, one whose tracks are all gated out on a frame, one with a track of m_cap observations; and lockstep
batches of 65 to 160 trajectories reach the launch forms that are chosen by the batch size.

The reference is po.Oracle(..., po.LEAN), one instance per trajectory on the same seeded scenario.Trajectory; the bars are
the suite's: 1e-6 (double) / 1e-3 (float) on helpers.state_errors, equal statistics, and np.array_equal wherever the library
promises the same bits."""
import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu
TOL = {"f64": 1e-6, "f32": 1e-3}


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def ragged_sets():
    return {h: H.RaggedSet(h) for h in (1, 2)}


def _dt(capi, po, prec):
    return (capi.F64, po.F64) if prec == "f64" else (capi.F32, po.F32)


def _errs(bt, b, o):
    return H.state_errors(bt.imu_state(b), o.getImuState(), bt.cam_states(b)[0], o.getCamStates()[0], bt.covariance(b), o.getCovariance())


def _same_stats(so, sd, where):
    for key in H.STAT_KEYS:
        assert so[key] == sd[key], (where, key, so, sd)


def _forced_frame(po, od, rs, bt, k, sample, tol, run, passed):
    """teacher forcing device -> oracle: fresh oracles take the sampled trajectories' state and covariance, the device runs
    frame k through `run`, the oracles run it on the same inputs; statistics equal, state and covariance within tol"""
    oracles = {}
    for b in sample:
        oracles[b] = rs.oracle(po, od, b)
        H.copy_device_to_oracle(bt, b, oracles[b])
    run()
    for b in sample:
        o = oracles[b]
        rs.oracle_frame(o, b, k)
        if len(rs.frames[b][k]["M"]):
            so, sd = o.lastStats(), bt.last_stats(b)
            _same_stats(so, sd, (k, b))
            passed[b] = passed.get(b, 0) + sd["n_passed"]
        e = _errs(bt, b, o)
        assert H.worst(e) < tol, (k, b, rs.specs[b], e)


# ------------------------------------------------------------------------------------------------ A: ragged ranges, per call
# (tests/test_ragged_scenarios.py checks without a GPU that the oracle alone updates on every scenario used here)
@pytest.mark.parametrize("handle", [1, 2])
def test_ragged_range_double_free_running_vs_oracle(capi, po, ragged_sets, handle):
    """Double, free-running from the first frame, every device stage ONE launch sequence over the whole ragged range: 1e-6
    against each trajectory's own oracle after every stage of every frame, statistics equal on every update.  The trajectory
    that never updates equals an oracle that only propagates and augments; the gated frame leaves its trajectory's covariance
    untouched bit for bit while the neighbours update."""
    rs = ragged_sets[handle]
    B = rs.B
    bt = rs.batch(capi, capi.F64)
    oracles = [rs.oracle(po, po.F64, b) for b in range(B)]
    passed = [0] * B

    def check(stage, k):
        for b in range(B):
            e = _errs(bt, b, oracles[b])
            assert H.worst(e) < 1e-6, (stage, k, b, rs.specs[b], e)

    for k in range(rs.nf):
        bt.propagate_range(0, B, rs.imu(k))
        for b, o in enumerate(oracles):
            o.propagate(rs.trajs[b].imu_for_frame(k))
        check("propagate", k)
        bt.augment_range(0, B)
        for b, o in enumerate(oracles):
            o.augmentState(k, rs.trajs[b].frame_times[k])
        check("augment", k)
        P_before = {b: bt.covariance(b) for b in range(B) if rs.specs[b][2] == "gated" and k == H.GATED_FRAME}
        for b in range(B):
            fr = rs.frames[b][k]
            bt.set_tracks(b, fr["M"], fr["slots"], fr["obs"])
        bt.marginalize_range(0, B)
        for b, o in enumerate(oracles):
            fr = rs.frames[b][k]
            sd = bt.last_stats(b)
            if not len(fr["M"]):
                assert sd["n_tracks"] == 0 and sd["m_rows"] == 0, (k, b, sd)
                continue
            o.setTracks(fr["M"], fr["slots"], fr["obs"]); o.marginalize()
            _same_stats(o.lastStats(), sd, (k, b))
            passed[b] += sd["n_passed"]
            if rs.full(b, k) and b not in P_before:
                assert sd["n_passed"] > 0 and sd["m_rows"] > 0, (k, b, sd)
        for b, P0 in P_before.items():
            assert bt.last_stats(b)["n_passed"] == 0 and np.array_equal(bt.covariance(b), P0), (k, b)
        check("update", k)
        for b, o in enumerate(oracles):
            assert bt.num_cam_states(b) == o.getNumCamStates() == rs.frames[b][k]["Nw"], (k, b)
            if rs.full(b, k):
                o.dropOldest(1); bt.drop_oldest_range(b, 1, 1)
        check("prune", k)
    for b in range(B):
        assert (passed[b] > 0) == rs.updating(b), (b, rs.specs[b], passed[b])
    bt.close()


@pytest.mark.parametrize("handle", [1, 2])
def test_ragged_range_float_teacher_forced_vs_oracle(capi, po, ragged_sets, handle):
    """Float: before every frame each trajectory's state and covariance go device -> float oracle (as
    test_cfg3_batch_of_64_vs_oracle does), both run the frame -- the device as one launch sequence over the ragged range --
    and agree to 1e-3 with equal statistics."""
    rs = ragged_sets[handle]
    bt = rs.batch(capi, capi.F32)
    passed = {}
    for k in range(rs.nf):
        _forced_frame(po, po.F32, rs, bt, k, range(rs.B), 1e-3, lambda: rs.device_frame(bt, k), passed)
    for b in range(rs.B):
        assert (passed.get(b, 0) > 0) == rs.updating(b), (b, rs.specs[b])
    bt.close()


# ------------------------------------------------------------------------------------------------ B: neighbours change no bit
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("handle", [1, 2])
def test_a_trajectory_does_not_depend_on_its_neighbours(capi, ragged_sets, handle, prec):
    """Each trajectory once inside the ragged range and once as the only active trajectory of a handle of the same shape (its
    neighbours initialised, propagated, without camera states or tracks): state, camera states, covariance, window size and
    statistics are the same bits after every frame -- which launch sequence updates a trajectory depends on its own window
    size only (msckf_hip.hip, launch_update), never on the largest window of the range it is launched in.  Then once more with
    the idle neighbours' covariance and IMU state NaN: same bits, all finite."""
    rs = ragged_sets[handle]
    cd = capi.F64 if prec == "f64" else capi.F32
    B = rs.B
    bt = rs.batch(capi, cd)
    ref = []
    for k in range(rs.nf):
        rs.device_frame(bt, k)
        ref.append([H.snapshot(bt, b) for b in range(B)])
    bt.close()
    for b in range(B):
        assert (sum(ref[k][b][4]["n_passed"] for k in range(rs.nf)) > 0) == rs.updating(b), (b, rs.specs[b])
    bad = []
    for poison in (False, True):
        for b in range(B):
            solo = rs.batch(capi, cd)
            if poison:
                for other in range(B):
                    if other != b:
                        solo.set_covariance(other, np.full((15, 15), np.nan)); solo.set_imu_state(other, np.full(29, np.nan))
            for k in range(rs.nf):
                rs.device_frame(solo, k, only=b)
                snap = H.snapshot(solo, b, strict=not poison)
                if not all(np.all(np.isfinite(x)) for x in snap[:3]):
                    bad.append(("not finite", poison, b, rs.specs[b], k)); break
                if not H.same_bits(snap, ref[k][b]):
                    bad.append(("bits differ", poison, b, rs.specs[b], k, float(np.abs(snap[2] - ref[k][b][2]).max()), snap[4], ref[k][b][4])); break
            if poison:
                for other in range(B):
                    solo.clear_error_flags(other)
            solo.close()
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ C: ragged windows in run_frames
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("handle", [1, 2])
def test_ragged_windows_inside_run_frames(capi, ragged_sets, handle, prec):
    """The ragged trajectories as a resident scenario, the drop flag per trajectory from its own window: on most frames some
    trajectories of a launch drop their oldest camera and others do not (the prune rides on the downdate).  However the frames
    are cut into calls, on one or three streams, resident or streamed, and through the per-call API: the same bits, and every
    record of the frame log holds the window size and state the per-call path has after that frame."""
    rs = ragged_sets[handle]
    cd = capi.F64 if prec == "f64" else capi.F32
    B, nf = rs.B, rs.nf
    assert any(len({rs.full(b, k) for b in range(B)}) == 2 for k in range(nf))      # mixed drop flags within one launch
    a = rs.batch(capi, cd)
    per_call = []
    for k in range(nf):
        rs.device_frame(a, k)
        per_call.append([H.snapshot(a, b) for b in range(B)])
    a.close()
    twos_and_threes = []
    while sum(twos_and_threes) < nf:
        twos_and_threes.append(min((2, 3)[len(twos_and_threes) % 2], nf - sum(twos_and_threes)))
    bad = []
    for cuts, kw in (([nf], {}), ([1] * nf, {}), (twos_and_threes, {}), ([nf], dict(streams=3)), ([4, nf - 4], dict(streamed=True, streams=2))):
        bt = rs.batch(capi, cd)
        rs.stage_scenario(bt)
        bt.set_streams(kw.get("streams", 1))
        bt.frame_log_enable(nf)
        f = 0
        for c in cuts:
            (bt.run_frames_streamed if kw.get("streamed") else bt.run_frames)(f, f + c)
            f += c
        assert f == nf
        bt.sync()
        for b in range(B):
            if not H.same_bits(H.snapshot(bt, b), per_call[-1][b]):
                bad.append(("final state", cuts[:4], kw, b, rs.specs[b]))
        arr, views = bt.frame_log_read()
        assert arr.shape[0] == nf
        for k in range(nf):
            for b in range(B):
                imu, _, P, ncam, _ = per_call[k][b]
                if not (views["n_cam"][k, b, 0] == ncam and np.array_equal(arr[k, b, :16], imu[:16]) and np.array_equal(views["P_II_diag"][k, b], np.diag(P)[:15])):
                    bad.append(("frame log", cuts[:4], kw, b, rs.specs[b], k)); break
        bt.close()
    assert not bad, bad[:12]


# ------------------------------------------------------------------------------------------------ D: batches beyond 64
def _resident(capi, trajs, N, F, nf, m_cap, dtype, streams=1, form=0):
    bt = capi.Batch(len(trajs), N, F, m_cap, dtype)
    if form:
        bt.set_covariance_update(form)
    for b, tr in enumerate(trajs):
        bt.initialize(b, tr.cfg, tr.imu0)
    bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    for k in range(nf):
        for b, tr in enumerate(trajs):
            fr = tr.frames[k]
            bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    bt.set_streams(streams)
    return bt


def _snap_all(bt, B):
    return [H.snapshot(bt, b) for b in range(B)]


def _differing(x, y, n):
    return [b for b in range(n) if not H.same_bits(x[b], y[b])]


class _Lockstep:
    """RaggedSet's interface for a lockstep batch (the teacher-forced comparison takes either)"""

    def __init__(self, trajs, N):
        self.trajs, self.N = trajs, N
        self.frames = [tr.frames for tr in trajs]
        self.specs = [(N, tr.F, "") for tr in trajs]

    def oracle(self, po, dtype, b):
        o = po.Oracle(dtype, po.LEAN)
        o.initialize(self.trajs[b].cfg, self.trajs[b].imu0)
        return o

    def oracle_frame(self, o, b, k):
        H.oracle_frame(o, self.trajs[b], k, self.N)


def _sample(B):
    return sorted({0, 7, 13, 21, 30, 42, 63, B - 1})


_TRAJ_CACHE = {}


def _trajs(config, seed0, N, F, nf, B):
    key = (config, seed0, N, F, nf)
    have = _TRAJ_CACHE.setdefault(key, [])
    while len(have) < B:
        have.append(sc.Trajectory(config, seed0 + len(have), N, F, nf))
    return have[:B]


BIG = dict(N=30, F=40, nf=33, m_cap=32)


def _big_run(capi, B, upto=None):
    g = BIG
    bt = _resident(capi, _trajs(3, 0, g["N"], g["F"], g["nf"], B), g["N"], g["F"], g["nf"], g["m_cap"], capi.F32)
    bt.run_frames(0, g["nf"] if upto is None else upto)
    bt.sync()
    return bt


@pytest.fixture(scope="module")
def big64(capi):
    bt = _big_run(capi, 64)
    snap = _snap_all(bt, 64)
    bt.close()
    assert all(s[4]["n_passed"] > 0 for s in snap)
    return snap


@pytest.mark.parametrize("B", [65, 96, 127, 128, 129, 160])
def test_float_batches_beyond_64(capi, po, big64, monkeypatch, B):
    """Float, 30-camera window, lockstep, B trajectories: from 96 on the blocked gain solve runs two workgroups per trajectory
    instead of four (kernels_chol.hip, launch_chol_gain: "same bits either way"), and the XCD placement pads B to a multiple of
    8.  (1) eight sampled trajectories, the last one included, against the float oracle for one update, teacher-forced, 1e-3;
    (2) trajectories 0 .. 63 are bit for bit what they are in a batch of 64 (four workgroups per trajectory there, whatever B
    launches); (3) for B >= 96, MSCKF_HIP_GAIN_PARTS=4 and =2 (read and checked when the handle is created) give the bits of the
    default, on every trajectory."""
    g = BIG
    monkeypatch.delenv("MSCKF_HIP_GAIN_PARTS", raising=False)
    rs = _Lockstep(_trajs(3, 0, g["N"], g["F"], g["nf"], B), g["N"])
    bt = _big_run(capi, B, upto=g["nf"] - 1)
    passed = {}
    k = g["nf"] - 1
    _forced_frame(po, po.F32, rs, bt, k, _sample(B), 1e-3, lambda: (bt.run_frames(k, k + 1), bt.sync()), passed)
    assert all(passed[b] > 0 for b in _sample(B)), passed
    default = _snap_all(bt, B)
    bt.close()
    assert _differing(default, big64, 64) == []
    if B >= 96:
        # the knob belongs to the handle: a value that names no form is refused when a handle is created (a process-wide
        # read-once setting would neither refuse it nor see the values set below), and the next handle takes the next value
        monkeypatch.setenv("MSCKF_HIP_GAIN_PARTS", "3")
        with pytest.raises(capi.HipError, match=r"\(-22\): MSCKF_HIP_GAIN_PARTS must be 0, 2 or 4"):
            capi.Batch(B, g["N"], g["F"], g["m_cap"], capi.F32)
        for parts in ("4", "2"):
            monkeypatch.setenv("MSCKF_HIP_GAIN_PARTS", parts)
            bt = _big_run(capi, B)
            forced = _snap_all(bt, B)
            bt.close()
            assert _differing(forced, default, B) == [], parts


@pytest.mark.parametrize("B", [65, 129, 130])
@pytest.mark.parametrize("prec,N,small,form", [("f64", 12, "84", 0), ("f64", 12, "0", 0), ("f64", 20, "84", 0), ("f32", 12, "84", 2), ("f32", 20, "84", 2)])
def test_register_resident_gain_solve_beyond_64(capi, po, monkeypatch, prec, N, small, form, B):
    """The register-resident gain solve k_gain_w (every double update of a 15 .. 20 camera window, float with
    set_covariance_update(2)) runs 8 workgroups per trajectory up to 64 trajectories, 4 up to 128, 2 beyond; B is no multiple
    of 8.  A 12-camera window in double takes the one-launch update (B workgroups of k_update_small) unless
    MSCKF_HIP_SMALL_UPDATE=0 sends it down the chain, to k_gain_w<double, 8, .>: both are run.  Sampled trajectories against the
    oracle: double free-running at 1e-6 after the last frame, float teacher-forced for the last update at 1e-3.  Every
    workgroup of a trajectory factors S itself and rows are eliminated independently, so trajectories 0 .. 63 are also bit for
    bit what they are in a batch of 64."""
    monkeypatch.setenv("MSCKF_HIP_SMALL_UPDATE", small)
    cd, od = _dt(capi, po, prec)
    F, nf = 24, N + 6
    trajs = _trajs(2, 700, N, F, nf, B)
    rs = _Lockstep(trajs, N)
    bt = _resident(capi, trajs, N, F, nf, N, cd, form=form)
    sample = _sample(B)
    if prec == "f64":
        bt.run_frames(0, nf); bt.sync()
        for b in sample:
            o = rs.oracle(po, od, b)
            for k in range(nf):
                rs.oracle_frame(o, b, k)
            _same_stats(o.lastStats(), bt.last_stats(b), b)
            assert bt.last_stats(b)["n_passed"] > 0
            e = _errs(bt, b, o)
            assert H.worst(e) < 1e-6, (b, e)
    else:
        bt.run_frames(0, nf - 1); bt.sync()
        passed = {}
        _forced_frame(po, od, rs, bt, nf - 1, sample, 1e-3, lambda: (bt.run_frames(nf - 1, nf), bt.sync()), passed)
        assert all(passed[b] > 0 for b in sample), passed
    snap = _snap_all(bt, B)
    bt.close()
    bt = _resident(capi, trajs[:64], N, F, nf, N, cd, form=form)
    bt.run_frames(0, nf); bt.sync()
    ref = _snap_all(bt, 64)
    bt.close()
    assert _differing(snap, ref, 64) == []


def test_streams_change_no_bit_of_a_double_batch_of_130(capi):
    """130 trajectories in double, 20-camera window: on one stream k_gain_w runs 2 workgroups per trajectory, on three streams
    (slices of 43 / 43 / 44) 8.  Streams never change bits (test_cfg3_streams_give_bit_identical_results promises it at 64)."""
    N, F, B = 20, 24, 130
    nf = N + 6
    trajs = _trajs(2, 700, N, F, nf, B)
    ref = None
    for ns in (1, 2, 3):
        bt = _resident(capi, trajs, N, F, nf, N, capi.F64, streams=ns)
        bt.run_frames(0, nf); bt.sync()
        snap = _snap_all(bt, B)
        bt.close()
        assert all(s[4]["n_passed"] > 0 for s in snap)
        if ref is None:
            ref = snap
        else:
            assert _differing(snap, ref, B) == [], ns


def test_ragged_batch_of_96_vs_oracle(capi, po):
    """96 trajectories in float, the first handle's window sizes (5 .. 32 cameras) cycled over the batch, per-call API over the
    whole range: the two-part blocked gain solve with its shared-S rendezvous meets windows of every size (parts of short
    windows have no rows and return early; trajectories of at most 14 cameras take the one-launch update in the same range).
    One trajectory of every window size and the last one against the float oracle, teacher-forced before every frame, 1e-3."""
    Ns = [s[0] for s in H.RAGGED[1]["specs"][:7]]
    B = 96
    rs = H.RaggedSet(0, seed0=900, n_cap=32, specs=[(Ns[b % 7], 10 + (7 * b) % 31, "") for b in range(B)])
    bt = rs.batch(capi, capi.F32)
    sample = list(range(7)) + [B - 1]
    passed = {}
    for k in range(rs.nf):
        _forced_frame(po, po.F32, rs, bt, k, sample, 1e-3, lambda: rs.device_frame(bt, k), passed)
    assert all(passed[b] > 0 for b in sample), passed
    for b in range(B):
        P = bt.covariance(b)
        assert np.all(np.isfinite(P)) and np.array_equal(P, P.T), b
    bt.close()


# ------------------------------------------------------------------------------------------------ E: a copy keeps its source's routes
@pytest.mark.parametrize("env", [{"MSCKF_HIP_SMALL_UPDATE": "0", "MSCKF_HIP_FEATURE_PAIR": "0"}, {}], ids=["source created under other routes", "ordinary twin"])
def test_a_copy_continues_on_its_source_s_routes_bit_for_bit(capi, ragged_sets, monkeypatch, env):
    """msckf_hip_copy_state hands over every setting that decides which kernels run, whoever chose it: handle A is created with
    MSCKF_HIP_SMALL_UPDATE=0 and MSCKF_HIP_FEATURE_PAIR=0 in the environment (the chain of kernels instead of k_update_small,
    k_feature instead of k_feature_pair), handle B without them; A runs two frames, B takes A's state over, both run three more
    (two updates at 4 and 5 cameras, the 5-camera window's first drop): IMU state, camera states, the whole covariance, window
    size and statistics of both trajectories are the same bits.  (The two routes agree to 1e-4 in float, not to the bit:
    tests/test_gpu_parity.py.)  Without the variables: the ordinary twin.  Float, the first handle's capacities, its 5- and
    14-camera trajectories."""
    rs = H.RaggedSet(0, seed0=500, n_cap=ragged_sets[1].n_cap, specs=[(5, 7, ""), (14, 40, "")], nf=5)
    rs.f_cap = ragged_sets[1].f_cap
    for name in ("MSCKF_HIP_SMALL_UPDATE", "MSCKF_HIP_FEATURE_PAIR"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    a = rs.batch(capi, capi.F32)
    for name in env:
        monkeypatch.delenv(name)
    b = capi.Batch(rs.B, rs.n_cap, rs.f_cap, rs.m_cap, capi.F32)
    for k in range(2):
        rs.device_frame(a, k)
    b.copy_state_from(a)
    passed = [0] * rs.B
    for k in range(2, 5):
        rs.device_frame(a, k); rs.device_frame(b, k)
        for t in range(rs.B):
            passed[t] += a.last_stats(t)["n_passed"] if len(rs.frames[t][k]["M"]) else 0
    sa, sb = _snap_all(a, rs.B), _snap_all(b, rs.B)
    a.close(); b.close()
    assert min(passed) > 0, passed                       # both trajectories updated after the copy
    assert sa[0][3] == 4 and sa[1][3] == 5, (sa[0][3], sa[1][3])      # the 5-camera window has dropped its oldest camera
    assert _differing(sa, sb, rs.B) == [], [float(np.abs(x[2] - y[2]).max()) for x, y in zip(sa, sb)]
