"""run_frames' feature-first order (msckf_hip_set_frame_order 1, the default: k_feature, then ONE launch with the track selection
beside propagate + augmentState -- k_propagate's HEAD instance -- then the rest of the update) against the propagate-first order of the same
build, bit for bit: states, covariances, statistics, per-track results, and every frame's log record on the way.  The counter
(msckf_hip_get_frame_order_count) says that the frames that may take the new order did, and the others did not.

3 float trajectories, 6-camera windows, 10 tracks of 2 .. 5 observations, 12 frames in two calls (7 + 5); the one-launch update of
short windows is off (MSCKF_HIP_SMALL_UPDATE=0), so every update takes the kernel chain whose head the order changes."""
import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu

B, N, F, M_CAP, NF, CUT = 3, 6, 10, 6, 12, 7
KINDS = ("resident", "streamed", "replay")
SIGMA = (2e-4, 2e-3, 1e-4, 1e-4)
SEEDS = (11, 12, 13)


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(autouse=True)
def chain_only(monkeypatch):
    monkeypatch.setenv("MSCKF_HIP_SMALL_UPDATE", "0")


@pytest.fixture(scope="module")
def trajectories():
    return [sc.Trajectory(2, 300 + b, N, F, NF) for b in range(B)]


def _cells(trs, variant):
    """[frame][trajectory] -> (readings, M, slots, obs, drop, skip) of a case"""
    cells = []
    for k in range(NF):
        row = []
        for b, tr in enumerate(trs):
            fr = tr.frames[k]
            M, slots, obs = fr["M"].copy(), fr["slots"].copy(), fr["obs"].copy()
            if len(M):
                # tracks 1 and 2 keep their last two observations only: lengths 2 .. 5 in every work-list
                off = np.concatenate([[0], np.cumsum(M)])
                keep = np.ones(len(slots), bool)
                for t in (1, 2):
                    keep[off[t]:off[t + 1] - 2] = False
                    M[t] = 2
                slots, obs = slots[keep], obs[keep]
            if variant == "newest" and b == 1 and k in (4, 9):
                # track 0 of trajectory 1 gets an observation in the camera state this frame's augmentState adds (slot Nw - 1)
                pc = tr.C_CG[k] @ (tr.landmarks[k][0] - tr.p_C[k])
                assert pc[2] > 0.5 and M[0] < M_CAP
                slots = np.insert(slots, M[0], fr["Nw"] - 1).astype(np.int32)
                obs = np.insert(obs, M[0], pc[:2] / pc[2], axis=0)
                M[0] += 1
            if variant == "few" and k <= 5 and len(M):
                # one track per frame up to frame 5: fewer than four tracks have been residualized through frame 6 (Q4, serial path)
                slots, obs, M = slots[:M[0]], obs[:M[0]], M[:1]
            skip = variant == "skip" and b == 2 and k == 5
            if skip:
                row.append((np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), 0, True))
            else:
                row.append((tr.imu_for_frame(k), M.astype(np.int32), slots.astype(np.int32), obs, 1 if fr["Nw"] == N else 0, False))
        cells.append(row)
    return cells


def _run(capi, trs, cells, kind, order, dtype=None, pruned_log=False, cut=CUT):
    bt = capi.Batch(B, N, F, M_CAP, capi.F32 if dtype is None else dtype)
    for b, tr in enumerate(trs):
        bt.initialize(b, tr.cfg, tr.imu0)
    bt.set_frame_order(order)
    bt.frame_log_enable(NF)
    if pruned_log:
        bt.pruned_log_enable(NF)
    if kind == "replay":
        bt.replay_alloc(B, NF, sc.IMU_PER_FRAME)
        for k in range(NF):
            for b in range(B):
                rd, M, slots, obs, drop, skip = cells[k][b]
                bt.replay_set_cell(k, b, rd, M, slots, obs, drop, skip=skip)
        bt.replay_assign(list(range(B)), SEEDS, SIGMA)
        bt.replay_commit()
        run = bt.run_frames_replay
    else:
        bt.scenario_alloc(NF, sc.IMU_PER_FRAME)
        for k in range(NF):
            for b in range(B):
                rd, M, slots, obs, drop, skip = cells[k][b]
                bt.scenario_set(k, b, rd, M, slots, obs, drop, skip=skip)
        bt.scenario_commit()
        run = bt.run_frames if kind == "resident" else bt.run_frames_streamed
    run(0, cut); run(cut, NF); bt.sync()
    out = dict(snap=[H.snapshot(bt, b, strict=False) for b in range(B)], tracks=[bt.last_tracks(b) for b in range(B)], log=bt.frame_log_read()[0],
               nres=[bt.num_residualized(b) for b in range(B)], count=bt.frame_order_count())
    bt.close()
    return out


def _same(new, old):
    bad = [b for b in range(B) if not H.same_bits(new["snap"][b], old["snap"][b])]
    assert not bad, ("state, covariance or last_stats", bad)
    assert all(np.array_equal(p, q) for p, q in zip(new["tracks"], old["tracks"])), "per-track results"
    assert new["nres"] == old["nres"]
    assert np.array_equal(new["log"], old["log"]), ("frame log", int(np.nonzero((new["log"] != old["log"]).any((1, 2)))[0][0]))


@pytest.fixture(scope="module")
def old_order(capi, trajectories):
    """the propagate-first run of a (variant, kind), computed once"""
    memo = {}

    def get(variant, kind, **kw):
        key = (variant, kind, tuple(sorted(kw.items())))
        if key not in memo:
            memo[key] = _run(capi, trajectories, _cells(trajectories, variant), kind, 0, **kw)
            assert memo[key]["count"] == 0
        return memo[key]
    return get


# frames of the two calls that are not a call's first: 12 - 2
EVERY = NF - 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("variant,count", [("plain", EVERY), ("newest", EVERY - 2), ("skip", EVERY - 1), ("few", EVERY)],
                         ids=["a no track on the newest camera", "b newest camera seen in frames 4 and 9", "c skipped cell in frame 5", "d serial selection"])
def test_feature_first_is_propagate_first_bit_for_bit(capi, trajectories, old_order, kind, variant, count):
    """(a) every frame but the first of each call takes the new order; (b) a track of trajectory 1 on the newest camera state sends
    frames 4 and 9 back to the old order, for the whole slice; (c) so does trajectory 2's skipped cell in frame 5; (d) with one
    track per frame at first, the selection of k_propagate's HEAD instance takes its serial path (fewer than four tracks residualized)"""
    old = old_order(variant, kind)
    new = _run(capi, trajectories, _cells(trajectories, variant), kind, 1)
    assert new["count"] == count
    assert all(s[4]["n_passed"] > 0 for s in new["snap"][:2])
    _same(new, old)


def test_the_few_tracks_case_reaches_the_serial_selection(capi, trajectories):
    """(d) after frames 0 .. 5 no trajectory has residualized more than three tracks: every selection so far, and frame 6's
    after them, starts with n_resid <= 3 and takes the serial path"""
    cells = _cells(trajectories, "few")
    assert [len(cells[k][0][1]) for k in range(CUT)] == [0, 0, 0, 1, 1, 1, F]
    bt = capi.Batch(B, N, F, M_CAP, capi.F32)
    for b, tr in enumerate(trajectories):
        bt.initialize(b, tr.cfg, tr.imu0)
    bt.scenario_alloc(NF, sc.IMU_PER_FRAME)
    for k in range(NF):
        for b in range(B):
            rd, M, slots, obs, drop, skip = cells[k][b]
            bt.scenario_set(k, b, rd, M, slots, obs, drop, skip=skip)
    bt.scenario_commit()
    bt.run_frames(0, CUT - 1); bt.sync()
    assert bt.frame_order_count() == CUT - 2
    assert all(bt.num_residualized(b) <= 3 for b in range(B))
    bt.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_pruned_state_log_keeps_the_order(capi, trajectories, old_order, kind):
    """(e) with the pruned-state log on no prune rides on the downdate: the new order is taken all the same"""
    old = old_order("plain", kind, pruned_log=True)
    new = _run(capi, trajectories, _cells(trajectories, "plain"), kind, 1, pruned_log=True)
    assert new["count"] == EVERY
    _same(new, old)


def test_a_double_handle_keeps_the_old_order(capi, trajectories, old_order):
    """(f) order 1 on a double handle: the counter stays 0, the results are order 0's"""
    old = old_order("plain", "resident", dtype=capi.F64)
    new = _run(capi, trajectories, _cells(trajectories, "plain"), "resident", 1, dtype=capi.F64)
    assert new["count"] == 0
    _same(new, old)


def test_the_setter_takes_zero_and_one_only(capi):
    bt = capi.Batch(1, N, F, M_CAP, capi.F32)
    with pytest.raises(capi.HipError):
        bt.set_frame_order(2)
    bt.set_frame_order(0); bt.set_frame_order(1)
    assert bt.frame_order_count() == 0
    bt.close()


def test_a_copy_of_the_handle_takes_the_order_over(capi, trajectories, old_order):
    """msckf_hip_copy_state hands the order to the destination like every setting that decides which kernels run: a fresh handle
    (order 1) copied from an initialized one with order 0 runs the frames in the old order, and the other way round"""
    cells = _cells(trajectories, "plain")
    for order, count in ((0, 0), (1, EVERY)):
        src = capi.Batch(B, N, F, M_CAP, capi.F32)
        for b, tr in enumerate(trajectories):
            src.initialize(b, tr.cfg, tr.imu0)
        src.set_frame_order(order)
        dst = capi.Batch(B, N, F, M_CAP, capi.F32)
        dst.set_frame_order(1 - order)
        dst.copy_state_from(src)
        dst.scenario_alloc(NF, sc.IMU_PER_FRAME)
        for k in range(NF):
            for b in range(B):
                rd, M, slots, obs, drop, skip = cells[k][b]
                dst.scenario_set(k, b, rd, M, slots, obs, drop, skip=skip)
        dst.scenario_commit()
        dst.run_frames(0, CUT); dst.run_frames(CUT, NF); dst.sync()
        assert dst.frame_order_count() == count
        snap = [H.snapshot(dst, b, strict=False) for b in range(B)]
        src.close(); dst.close()
        assert [b for b in range(B) if not H.same_bits(snap[b], old_order("plain", "resident")["snap"][b])] == []


def test_the_benchmark_shape(capi):
    """(a) once at 64 trajectories x 30 cameras x 200 tracks, 6 frames in one call, two slices"""
    Bb, Nb, Fb, nf = 64, 30, 200, 6
    trs = [sc.Trajectory(3, b, Nb, Fb, nf) for b in range(Bb)]
    out = []
    for order in (0, 1):
        bt = capi.Batch(Bb, Nb, Fb, Nb, capi.F32)
        for b, tr in enumerate(trs):
            bt.initialize(b, tr.cfg, tr.imu0)
        bt.set_frame_order(order)
        bt.set_streams(2)
        bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
        for k in range(nf):
            for b, tr in enumerate(trs):
                fr = tr.frames[k]
                bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == Nb else 0)
        bt.scenario_commit()
        bt.run_frames(0, nf); bt.sync()
        out.append(([H.snapshot(bt, b) for b in range(Bb)], bt.frame_order_count()))
        bt.close()
    (old, n0), (new, n1) = out
    assert n0 == 0 and n1 > 0 and n1 % (nf - 1) == 0        # every slice's frames but the first
    assert min(s[4]["n_passed"] for s in new) > 0
    assert [b for b in range(Bb) if not H.same_bits(new[b], old[b])] == []
