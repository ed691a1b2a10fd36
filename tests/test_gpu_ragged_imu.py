"""Ragged IMU counts and sequences of unequal length inside run_frames / run_frames_streamed / propagate_range_counts.

Every other GPU module hands every (frame, trajectory) cell of a scenario the same number of IMU samples and every trajectory
an image on every frame.  Here a cell has its own count -- tests/ragged_imu.py: 1 to 33 samples, every boundary of
k_propagate's groups of 16, cells without any sample -- one trajectory pauses for two frames and one ends five frames early,
in a batch of 7 (windows of 6 and 15 cameras: the one-launch update and the kernel chain in one launch; 7 is no multiple of
the three slices).  tests/test_ragged_imu_scenarios.py checks without a GPU that the oracle alone updates on every full-window
frame of every non-skipped cell.

The reference is po.Oracle(..., po.LEAN), one instance per trajectory on the same resampled readings; the bars are the
suite's: 1e-6 (double, free-running) / 1e-3 (float, teacher-forced) on helpers.state_errors with equal statistics, and
np.array_equal wherever the library promises the same bits."""
import numpy as np
import pytest

import helpers as H
import ragged_imu as R

pytestmark = pytest.mark.gpu
EINVAL = r"\(-22\)"


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def sets():
    """parity: compared with the oracle (empty cells on last frames); bits: a full Q_imu on trajectory 2 and empty cells mid-run
    (both Q instantiations of k_propagate in one launch; bit comparisons only); equal: ten samples everywhere, nobody skipped"""
    return dict(parity=R.RaggedImuSet(), bits=R.RaggedImuSet(full_q=True, zeros="rotating"), equal=R.RaggedImuSet(equal=True))


def _cd(capi, prec):
    return capi.F64 if prec == "f64" else capi.F32


def _errs(bt, b, o):
    return H.state_errors(bt.imu_state(b), o.getImuState(), bt.cam_states(b)[0], o.getCamStates()[0], bt.covariance(b), o.getCovariance())


def _state(bt, b):
    """what a skipped cell must leave alone: IMU state, camera states, covariance, window size"""
    return bt.imu_state(b), bt.cam_states(b)[0], bt.covariance(b), bt.num_cam_states(b)


def _same_state(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x[:3], y[:3])) and x[3] == y[3]


def _run(capi, rs, cd, cuts=None, streams=1, streamed=False, K=None, only=None):
    """the set's cells staged on a fresh handle (only = b: trajectory b alone in a handle of one) and run in calls of `cuts`
    frames: (snapshot per trajectory, frame log [nf][B][48])"""
    bt = rs.batch(capi, cd) if only is None else rs.solo_batch(capi, cd, only)
    rs.stage(bt, K=K, only=only)
    bt.set_streams(streams)
    if streamed:
        bt.set_upload_ring(2, 0)
    bt.frame_log_enable(rs.nf)
    f = 0
    for c_ in cuts or [rs.nf]:
        (bt.run_frames_streamed if streamed else bt.run_frames)(f, f + c_)
        f += c_
    assert f == rs.nf
    bt.sync()
    snap = [H.snapshot(bt, b) for b in range(bt.B)]
    log = bt.frame_log_read()[0]
    bt.close()
    return snap, log


_REF = {}


def _reference(capi, sets, name, prec):
    """one call over all frames, one stream, resident: computed once per set and dtype"""
    if (name, prec) not in _REF:
        _REF[(name, prec)] = _run(capi, sets[name], _cd(capi, prec))
    return _REF[(name, prec)]


# ------------------------------------------------------------------------------------------------ parity with the oracle
def test_ragged_imu_batch_double_free_running_vs_oracle(capi, po, sets):
    """Double, free-running from the first frame through run_frames, frame by frame: 1e-6 against each trajectory's own oracle
    on the same k samples after every frame, equal statistics on every update, a real update on every full-window frame.  A
    cell without samples is an oracle that only augments; a skipped cell is an oracle that does nothing."""
    rs = sets["parity"]
    bt = rs.batch(capi, capi.F64)
    rs.stage(bt)
    oracles = [rs.oracle(po, po.F64, b) for b in range(rs.B)]
    passed = [0] * rs.B
    for f in range(rs.nf):
        bt.run_frames(f, f + 1)
        bt.sync()
        for b, o in enumerate(oracles):
            rs.oracle_cell(o, b, f)
            j = rs.local[b][f]
            if j is not None and len(rs.frames[b][j]["M"]):
                so, sd = o.lastStats(), bt.last_stats(b)
                for key in H.STAT_KEYS:
                    assert so[key] == sd[key], (f, b, key, so, sd)
                passed[b] += sd["n_passed"]
                if rs.full(b, j):
                    assert sd["n_passed"] > 0 and sd["m_rows"] > 0, (f, b, sd)
            assert bt.num_cam_states(b) == o.getNumCamStates(), (f, b)
            err = _errs(bt, b, o)
            assert H.worst(err) < 1e-6, (f, b, j, None if j is None else rs.counts[b][j], err)
    assert min(passed) > 0, passed
    bt.close()


def test_ragged_imu_batch_float_teacher_forced_vs_oracle(capi, po, sets):
    """Float: before every frame each trajectory's state and covariance go device -> float oracle, both run the frame's cells,
    and agree to 1e-3 with equal statistics (as test_gpu_ragged._forced_frame does)."""
    rs = sets["parity"]
    bt = rs.batch(capi, capi.F32)
    rs.stage(bt)
    passed = [0] * rs.B
    for f in range(rs.nf):
        oracles = []
        for b in range(rs.B):
            o = rs.oracle(po, po.F32, b)
            H.copy_device_to_oracle(bt, b, o)
            oracles.append(o)
        bt.run_frames(f, f + 1)
        bt.sync()
        for b, o in enumerate(oracles):
            rs.oracle_cell(o, b, f)
            j = rs.local[b][f]
            if j is not None and len(rs.frames[b][j]["M"]):
                so, sd = o.lastStats(), bt.last_stats(b)
                for key in H.STAT_KEYS:
                    assert so[key] == sd[key], (f, b, key, so, sd)
                passed[b] += sd["n_passed"]
            err = _errs(bt, b, o)
            assert H.worst(err) < 1e-3, (f, b, j, err)
    assert min(passed) > 0, passed
    bt.close()


# ------------------------------------------------------------------------------------------------ bits
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_a_full_cell_through_the_new_entry_is_scenario_set(capi, sets, prec):
    """(1) k = K and no skip through msckf_hip_scenario_set_cell (capi.Batch.scenario_set) = the same scenario through
    msckf_hip_scenario_set, called directly"""
    rs = sets["equal"]
    new, _ = _reference(capi, sets, "equal", prec)
    bt = rs.batch(capi, _cd(capi, prec))
    bt.scenario_alloc(rs.nf, rs.K)
    for f in range(rs.nf):
        for b in range(rs.B):
            rd, M, slots, obs, drop, skip = rs.cell(b, f)
            assert not skip and len(rd) == rs.K
            r_, pr = capi._d(rd); m_, pm = capi._i(M); s_, ps = capi._i(slots); o_, pob = capi._d(obs)
            assert bt.L.msckf_hip_scenario_set(bt.h, f, b, pr, len(m_), pm, ps, pob, drop) == 0
    bt.scenario_commit()
    bt.run_frames(0, rs.nf)
    bt.sync()
    old = [H.snapshot(bt, b) for b in range(rs.B)]
    bt.close()
    assert all(s[4]["n_passed"] > 0 for s in old)
    assert [b for b in range(rs.B) if not H.same_bits(old[b], new[b])] == []


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["parity", "bits"])
def test_a_trajectory_of_the_ragged_imu_batch_is_what_it_is_alone(capi, sets, name, prec):
    """(2) each trajectory's cells in a handle of ONE trajectory: the same bits after the run, and in every record of the
    frame log on the way (its neighbours' counts, their skipped cells and the full Q_imu next to it change nothing)"""
    rs = sets[name]
    snap, log = _reference(capi, sets, name, prec)
    bad = []
    for b in range(rs.B):
        solo, slog = _run(capi, rs, _cd(capi, prec), only=b)
        if not H.same_bits(solo[0], snap[b]):
            bad.append(("final state", b, rs.specs[b]))
        if not np.array_equal(slog[:, 0], log[:, b]):
            bad.append(("frame log", b, int(np.nonzero((slog[:, 0] != log[:, b]).any(1))[0][0])))
    assert not bad, bad


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["parity", "bits"])
def test_calls_streams_upload_and_padding_change_no_bit(capi, sets, name, prec):
    """(3) run_frames = run_frames_streamed at ring depth 2, one stream = three (slices start at trajectories 0, 2, 4: the count
    array is offset); (4) any cut of the frames into calls -- also calls that end on a skipped frame (the separate prune meets
    the skipped cell) and start on one, while one call over everything meets them with the prune riding on the downdate;
    (5) a scenario allocated with K = 40 instead of 33: the padding behind a cell's samples is not read"""
    rs = sets[name]
    nf = rs.nf
    ref, rlog = _reference(capi, sets, name, prec)
    mid, tail = R.MID_SKIP[1], nf - 5
    variants = [dict(cuts=[1] * nf), dict(cuts=[mid[0] + 1, nf - mid[0] - 1]), dict(cuts=[mid[1] + 1, nf - mid[1] - 1]),
                dict(cuts=[tail + 1, nf - tail - 1]), dict(streams=3), dict(streamed=True), dict(cuts=[4, nf - 4], streamed=True, streams=3),
                dict(K=40), dict(K=40, streamed=True, streams=3)]
    bad = []
    for kw in variants:
        snap, log = _run(capi, rs, _cd(capi, prec), **kw)
        diff = [b for b in range(rs.B) if not H.same_bits(snap[b], ref[b])]
        if diff or not np.array_equal(log, rlog):
            bad.append((kw, diff))
    assert not bad, bad


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("env", [{}, {"MSCKF_HIP_FUSE_PRUNE": "0"}, {"MSCKF_HIP_SMALL_UPDATE": "0"}], ids=["default", "separate prune", "kernel chain"])
def test_a_skipped_cell_leaves_its_trajectory_alone(capi, sets, monkeypatch, env, prec):
    """(6) IMU state, camera states, covariance and num_cam_states of a skipped trajectory are the same bits before and after --
    with the prune riding on the downdate (the covariance moves to the other buffer), as the last frame of a call, with
    MSCKF_HIP_FUSE_PRUNE=0, and with the update's kernel chain instead of the one-launch update -- while its neighbours update.
    Its frame-log records repeat the state."""
    rs = sets["parity"]
    nf = rs.nf
    for name in ("MSCKF_HIP_FUSE_PRUNE", "MSCKF_HIP_SMALL_UPDATE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    bm, (m0, m1), bt_tail, t0 = R.MID_SKIP[0], R.MID_SKIP[1], R.TAIL_SKIP, nf - 5
    bt = rs.batch(capi, _cd(capi, prec))
    rs.stage(bt)
    bt.frame_log_enable(nf)
    bt.run_frames(0, m0); bt.sync()
    before = _state(bt, bm)
    others = [_state(bt, b) for b in range(rs.B)]
    bt.run_frames(m0, m1 + 1); bt.sync()              # frame m0 mid-call (prune on the downdate), frame m1 the call's last
    assert _same_state(_state(bt, bm), before)
    assert all(not _same_state(_state(bt, b), others[b]) for b in range(rs.B) if b != bm)
    bt.run_frames(m1 + 1, t0); bt.sync()
    assert not _same_state(_state(bt, bm), before)     # it resumed
    before = _state(bt, bt_tail)
    assert before[3] == rs.N[bt_tail] - 1              # a full window that has just dropped its oldest camera
    bt.run_frames(t0, t0 + 2); bt.run_frames(t0 + 2, nf); bt.sync()
    assert _same_state(_state(bt, bt_tail), before)
    log = bt.frame_log_read()[0]
    for b, frames in ((bm, range(m0, m1 + 1)), (bt_tail, range(t0, nf))):
        for f in frames:
            assert np.array_equal(log[f, b, :38], log[f - 1, b, :38]) and np.array_equal(log[f, b, 41:], log[f - 1, b, 41:]), (b, f)
    assert np.array_equal(log[nf - 1, bt_tail, :16], before[0][:16]) and log[nf - 1, bt_tail, 37] == before[3]
    bt.close()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_an_empty_cell_is_augment_alone(capi, prec):
    """k = 0, not skipped: nothing is propagated -- IMU state, P_II and P_IC keep their bits -- and the fused augment is
    msckf_hip_augment_range alone, bit for bit; for a diagonal and for a full Q_imu (both instantiations of k_propagate)"""
    ncam = 3
    a = capi.Batch(2, 8, 8, 8, _cd(capi, prec))
    c = capi.Batch(2, 8, 8, 8, _cd(capi, prec))
    for b in range(2):
        imu, cfg, _ = H.state_inputs("mixed", 40 + b, K=4)
        if b == 1:
            cfg = dict(cfg, Q_imu=R.correlated(H.STATE_Q_DIAG, 77))
        for bt in (a, c):
            H.device_window(bt, b, cfg, imu, H.state_spd(ncam, 40 + b), H.state_cam_poses(ncam, 40 + b))
    before = [_state(c, b) for b in range(2)]
    a.scenario_alloc(1, 10)
    none = np.zeros(0, np.int32)
    for b in range(2):
        a.scenario_set(0, b, np.zeros((0, 7)), none, none, np.zeros((0, 2)), 0)
    a.scenario_commit()
    a.run_frames(0, 1); a.sync()
    c.augment_range(0, 2); c.sync()
    for b in range(2):
        sa, sc_ = _state(a, b), _state(c, b)
        assert sa[3] == ncam + 1 and _same_state(sa, sc_), b
        D = 15 + 6 * ncam
        assert np.array_equal(sa[0], before[b][0]) and np.array_equal(sa[2][:D, :D], before[b][2]), b
    a.close(); c.close()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_propagate_range_counts_is_propagate_range_per_trajectory(capi, prec):
    """(7) counts 0, 1, 63, 64, 65 and 130 in one range (the 64-sample staging chunks are cut per trajectory; the 65-sample
    trajectory carries a full Q_imu): the bits of msckf_hip_propagate_range(b, 1, ., K_b) trajectory by trajectory, the
    trajectory without samples untouched; then a sub-range that does not start at trajectory 0.  A negative count is refused
    and propagates nothing."""
    counts = [64, 0, 130, 65, 1, 63]
    B, ncam = len(counts), 3
    a = capi.Batch(B, 8, 8, 8, _cd(capi, prec))
    c = capi.Batch(B, 8, 8, 8, _cd(capi, prec))
    rds = []
    for b in range(B):
        imu, cfg, rd = H.state_inputs("mixed", 60 + b, K=130)
        if counts[b] == 65:
            cfg = dict(cfg, Q_imu=R.correlated(H.STATE_Q_DIAG, 77))
        rds.append(rd)
        for bt in (a, c):
            H.device_window(bt, b, cfg, imu, H.state_spd(ncam, 60 + b), H.state_cam_poses(ncam, 60 + b))
    start = [_state(a, b) for b in range(B)]
    with pytest.raises(capi.HipError, match=EINVAL + r": .*negative"):
        K_, pK = capi._i([3, -1, 3, 3, 3, 3]); r_, pr = capi._d(np.concatenate([rd[:3] for rd in rds]))
        capi._chk(a.L.msckf_hip_propagate_range_counts(a.h, 0, B, pr, pK))
    assert all(_same_state(_state(a, b), start[b]) for b in range(B))

    def both(b0, nb, ks, first):
        a.propagate_range_counts(b0, nb, [rds[b0 + i][first:first + ks[i]] for i in range(nb)])
        for i in range(nb):
            if ks[i]:
                c.propagate_range(b0 + i, 1, rds[b0 + i][first:first + ks[i]])
        a.sync(); c.sync()
        return [b0 + i for i in range(nb) if not _same_state(_state(a, b0 + i), _state(c, b0 + i))]

    assert both(0, B, counts, 0) == []
    for b in range(B):
        assert _same_state(_state(a, b), start[b]) == (counts[b] == 0), b
    mid = [_state(a, b) for b in range(B)]
    assert both(1, 4, [17, 0, 66, 5], 0) == []
    assert _same_state(_state(a, 2), mid[2]) and _same_state(_state(a, 0), mid[0]) and _same_state(_state(a, 5), mid[5])
    a.close(); c.close()


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_frame_log_metrics_ranges(capi, sets, prec):
    """(8) equal ranges: the bits of frame_log_metrics; a range per trajectory (r1[b] = the sequence's own frame count, the
    skipped tail left out; also with its own r0[b]): row b of frame_log_metrics(r0[b], r1[b]), for every b.  r1[b] beyond the
    records written is refused."""
    rs = sets["parity"]
    nf, B = rs.nf, rs.B
    bt = rs.batch(capi, _cd(capi, prec))
    rs.stage(bt)
    bt.frame_log_enable(nf)
    bt.run_frames(0, nf); bt.sync()
    gt = np.stack([np.stack([rs.trajs[b].gt_frames["p"][min(rs.local[b][f] if rs.local[b][f] is not None else 0, nf - 1)] for b in range(B)]) for f in range(nf)])
    gt = gt + 0.01 * np.random.default_rng(3).normal(size=gt.shape)
    whole = bt.frame_log_metrics(0, nf, gt)
    assert np.all(whole[:, 0] == nf) and np.all(np.isfinite(whole)) and np.all(whole[:, 1] > 0)
    assert np.array_equal(bt.frame_log_metrics_ranges([0] * B, [nf] * B, gt), whole)
    assert np.array_equal(bt.frame_log_metrics_ranges([2] * B, [nf - 3] * B, gt[2:nf - 3]), bt.frame_log_metrics(2, nf - 3, gt[2:nf - 3]))
    r1 = [nf - 5 if b == R.TAIL_SKIP else (nf, nf - 2, 12, 5)[b % 4] for b in range(B)]
    for r0 in ([0] * B, [0, 2, 1, 0, 3, 0, 4]):
        got = bt.frame_log_metrics_ranges(r0, r1, gt[min(r0):max(r1)])
        for b in range(B):
            want = bt.frame_log_metrics(r0[b], r1[b], gt[r0[b]:r1[b]])[b]
            assert np.array_equal(got[b], want) and got[b, 0] == r1[b] - r0[b], (b, r0[b], r1[b], got[b], want)
    for r0, r1 in (([0] * B, [nf] * (B - 1) + [nf + 1]), ([0] * (B - 1) + [-1], [nf] * B), ([0, 0, 6] + [0] * (B - 3), [nf, nf, 5] + [nf] * (B - 3))):
        with pytest.raises(capi.HipError, match=EINVAL + r": record range of trajectory"):
            bt.frame_log_metrics_ranges(r0, r1, np.zeros((max(r1) - min(r0), B, 3)))
    bt.close()


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("prec", ["f64"])
def test_refused_cells_leave_the_scenario_as_it_was(capi, sets, prec):
    """k > K, k < 0, a skipped cell with samples, tracks or a drop, an unknown flag bit: -EINVAL with a message, and the
    committed scenario still runs to the bits it had (the refusals neither un-commit it nor touch a cell)."""
    rs = sets["parity"]
    ref, _ = _reference(capi, sets, "parity", prec)
    bt = rs.batch(capi, _cd(capi, prec))
    rs.stage(bt)
    f, b = 7, 3
    rd, M, slots, obs, drop, skip = rs.cell(b, f)
    assert len(M) and not skip
    none = np.zeros(0, np.int32)
    for kw, why in ((dict(readings=np.ones((rs.K + 1, 7))), "exceeds"), (dict(readings=rd[:1], skip=True, M=none, slots=none, obs=np.zeros((0, 2)), n_drop=0), "skipped"),
                    (dict(readings=rd[:0], skip=True, n_drop=0), "skipped"), (dict(readings=rd[:0], skip=True, M=none, slots=none, obs=np.zeros((0, 2)), n_drop=1), "skipped")):
        args = dict(readings=rd, M=M, slots=slots, obs=obs, n_drop=drop, skip=False)
        args.update(kw)
        with pytest.raises(capi.HipError, match=EINVAL + r": .*" + why):
            bt.scenario_set(f, b, args["readings"], args["M"], args["slots"], args["obs"], args["n_drop"], skip=args["skip"])
    r_, pr = capi._d(rd); m_, pm = capi._i(M); s_, ps = capi._i(slots); o_, pob = capi._d(obs)
    for k, flags, why in ((-1, 0, b"negative"), (len(rd), 2, b"flag"), (len(rd), 4 | 1, b"flag")):
        assert bt.L.msckf_hip_scenario_set_cell(bt.h, f, b, pr, k, len(m_), pm, ps, pob, drop, flags) == -22
        assert why in bt.L.msckf_hip_last_error()
    bt.run_frames(0, rs.nf); bt.sync()            # still committed
    snap = [H.snapshot(bt, t) for t in range(rs.B)]
    bt.close()
    assert [t for t in range(rs.B) if not H.same_bits(snap[t], ref[t])] == []
