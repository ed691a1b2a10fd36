"""run_frames' order 2 (msckf_hip_set_frame_order 1 with msckf_hip_set_frame_order_chol on, the default: k_feature, k_select_diag, k_gram, then ONE launch with the
Gram Cholesky's workgroups and one propagate + augmentState workgroup per trajectory -- k_propagate's CHOL instances -- then the
rest of the update) against orders 1 and 0 of the same build, bit for bit: states, covariances, statistics, per-track results,
n_resid and every frame's log record.  Two counters say which frames ran k_feature first (msckf_hip_get_frame_order_count) and
which of them took order 2 (msckf_hip_get_frame_order_chol_count).

3 float trajectories, 16 tracks, the window fill and 12 frames past it in two calls (cut 6 frames past the fill):
  * 30-camera windows: 12 column blocks of the Gram matrix, the one-launch update of short windows as it comes (84 columns asked,
    72 fit k_update_small -- routes::small_limit: (15 + n) n <= 7 168 --, so the frames with up to 12 cameras are
    k_update_small's and count 0 for order 2);
  * 14-camera windows: 8 blocks, MSCKF_HIP_SMALL_UPDATE=60 (the frames with up to 10 cameras are k_update_small's);
  * 10-camera windows: 4 blocks, MSCKF_HIP_SMALL_UPDATE=0 (every frame takes the chain).
A frame k of the fill has k + 1 cameras when its update runs, so with L the small update's limit in cameras the frames
k >= max(L, 1) that are not a call's first can take order 2: NF - max(L, 1) - 1 of them; NF - 2 run k_feature first."""
import contextlib
import os

import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu

B, F, PAST = 3, 16, 12
SIGMA = (2e-4, 2e-3, 1e-4, 1e-4)
SEEDS = (21, 22, 23)
LAG = 3   # "mixed": trajectory 2 starts this many frames late
# window size -> (MSCKF_HIP_SMALL_UPDATE or None for the default, limit L in cameras, column blocks of the Gram Cholesky)
SHAPES = {30: (None, 12, 12), 14: ("60", 10, 8), 10: ("0", 0, 4)}


def _nf(N):
    return N + PAST


def _cut(N):
    return N + 6


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@contextlib.contextmanager
def _small_update(value):
    old = os.environ.get("MSCKF_HIP_SMALL_UPDATE")
    if value is not None:
        os.environ["MSCKF_HIP_SMALL_UPDATE"] = value
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ["MSCKF_HIP_SMALL_UPDATE"]
            else:
                os.environ["MSCKF_HIP_SMALL_UPDATE"] = old


def _correlated(diag, seed, lo=0.3, hi=0.6):
    rng = np.random.default_rng(seed)
    c = rng.uniform(np.sqrt(lo), np.sqrt(hi), len(diag)) * rng.choice([-1.0, 1.0], len(diag))
    R = np.outer(c, c)
    np.fill_diagonal(R, 1.0)
    s = np.sqrt(np.asarray(diag, dtype=np.float64))
    return R * np.outer(s, s)


_TRS = {}


def _trajectories(N, fullq=False):
    key = (N, fullq)
    if key not in _TRS:
        cfg = sc.filter_config(N, Q_imu=_correlated(sc.filter_config(N)["Q_imu_diag"], 77)) if fullq else None
        _TRS[key] = [sc.Trajectory(2, 500 + b, N, F, _nf(N), cfg=cfg) for b in range(B)]
    return _TRS[key]


def _set_order(bt, order):
    """0: propagate first; 1: feature first with the in-Cholesky form switched off; 2: the default, set explicitly"""
    bt.set_frame_order(1 if order else 0)
    bt.set_frame_order_chol(order == 2)


SKIPPED = (np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), 0, True)


def _cells(trs, N, variant):
    """[frame][trajectory] -> (readings, M, slots, obs, drop, skip) of a case"""
    cells = []
    for k in range(_nf(N)):
        row = []
        for b, tr in enumerate(trs):
            kk = k - LAG if (variant == "mixed" and b == 2) else k     # trajectory 2 runs its own frames LAG frames late
            if kk < 0 or (variant == "skip" and b == 2 and k == N + 3):
                row.append(SKIPPED)
                continue
            fr = tr.frames[kk]
            M, slots, obs = fr["M"].copy(), fr["slots"].copy(), fr["obs"].copy()
            drop = 1 if fr["Nw"] == N else 0
            if variant == "newest" and b == 1 and k == N + 2:
                # the first track that allows it gets an observation in the camera state this frame's augmentState adds (slot Nw - 1)
                off = np.concatenate([[0], np.cumsum(M)])
                pcs = [tr.C_CG[k] @ (p - tr.p_C[k]) for p in tr.landmarks[k]]
                t = next(t for t in range(len(M)) if pcs[t][2] > 0.5 and M[t] < N)
                slots = np.insert(slots, off[t + 1], fr["Nw"] - 1).astype(np.int32)
                obs = np.insert(obs, off[t + 1], pcs[t][:2] / pcs[t][2], axis=0)
                M[t] += 1
            if variant == "full" and b == 0 and k == N + 1:
                drop = 0                                                 # nothing dropped: frame N + 2 finds trajectory 0's window full
            row.append((tr.imu_for_frame(kk), M.astype(np.int32), slots.astype(np.int32), obs, drop, False))
        cells.append(row)
    return cells


def _run(capi, N, variant, kind, order, dtype=None, pruned_log=False, fullq=False):
    trs = _trajectories(N, fullq)
    cells = _cells(trs, N, variant)
    NF, CUT = _nf(N), _cut(N)
    with _small_update(SHAPES[N][0]):
        bt = capi.Batch(B, N, F, N, capi.F32 if dtype is None else dtype)
    for b, tr in enumerate(trs):
        bt.initialize(b, tr.cfg, tr.imu0)
    _set_order(bt, order)
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
    run(0, CUT); run(CUT, NF); bt.sync()
    out = dict(snap=[H.snapshot(bt, b, strict=False) for b in range(B)], tracks=[bt.last_tracks(b) for b in range(B)], log=bt.frame_log_read()[0],
               nres=[bt.num_residualized(b) for b in range(B)], first=bt.frame_order_count(), chol=bt.frame_order_chol_count())
    bt.close()
    return out


def _same(new, old, what):
    bad = [b for b in range(B) if not H.same_bits(new["snap"][b], old["snap"][b])]
    assert not bad, (what, "state, covariance or last_stats", bad)
    assert all(np.array_equal(p, q) for p, q in zip(new["tracks"], old["tracks"])), (what, "per-track results")
    assert new["nres"] == old["nres"], what
    assert np.array_equal(new["log"], old["log"]), (what, "frame log", int(np.nonzero((new["log"] != old["log"]).any((1, 2)))[0][0]))


def _check(capi, N, variant, kind, first, chol, **kw):
    """orders 0, 1 and 2 of one case: the counters, and order 2's results against both others"""
    o0, o1, o2 = (_run(capi, N, variant, kind, order, **kw) for order in (0, 1, 2))
    assert (o0["first"], o0["chol"]) == (0, 0)
    assert (o1["first"], o1["chol"]) == (first, 0)
    assert (o2["first"], o2["chol"]) == (first, chol)
    assert o2["snap"][1][4]["n_passed"] > 0      # (trajectory 1: no case takes a camera state or a frame away from it)
    _same(o2, o1, "order 2 against order 1")
    _same(o2, o0, "order 2 against order 0")


def _plain(N):
    """(frames that run k_feature first, frames that take order 2) of a case where nothing but the window fill refuses"""
    return _nf(N) - 2, _nf(N) - max(SHAPES[N][1], 1) - 1


def test_the_expected_counts_are_these():
    assert _plain(30) == (40, 29) and _plain(14) == (24, 15) and _plain(10) == (20, 20)


@pytest.mark.parametrize("kind", ("resident", "streamed", "replay"))
def test_twelve_blocks_every_input_kind(capi, kind):
    """30-camera windows: frames 0 .. 11 are k_update_small's (order 1 from frame 1 on, order 2 never), frames 12 .. 41 but the
    second call's first (36) take order 2: 40 and 29"""
    _check(capi, 30, "plain", kind, 40, 29)


@pytest.mark.parametrize("N,variant,first,chol", [
    (30, "newest", 39, 28),   # a track of trajectory 1 on the newest camera in frame 32: the slice's frame keeps order 0
    (30, "skip", 39, 28),     # trajectory 2's cell of frame 33 skipped: order 0
    (30, "full", 39, 28),     # trajectory 0 drops nothing in frame 31: frame 32 finds its window full, order 0
    (30, "mixed", 38, 26),    # trajectory 2 three frames late: frames 1, 2 skipped (order 0); frames 12 .. 14 mix k_update_small and the chain (order 1); 15 .. 41 but 36 take order 2
    (14, "mixed", 22, 12),    # the same at 8 blocks: frames 10 .. 12 are mixed, 13 .. 25 but 20 take order 2
], ids=["newest camera seen", "skipped cell", "full window", "mixed small and chain", "mixed small and chain, 8 blocks"])
def test_the_frames_that_refuse(capi, N, variant, first, chol):
    _check(capi, N, variant, "resident", first, chol)


def test_eight_blocks(capi):
    """14-camera windows, small update up to 10 cameras: frames 10 .. 25 but 20 take order 2"""
    _check(capi, 14, "plain", "resident", 24, 15)


def test_four_blocks_without_the_small_update(capi):
    """10-camera windows, k_update_small off: every frame but the two calls' first takes order 2 (the first three have no tracks:
    the Cholesky's workgroups leave at once, propagate + augmentState run)"""
    _check(capi, 10, "plain", "resident", 20, 20)


@pytest.mark.parametrize("N,kind", [(30, "resident"), (14, "replay")])
def test_full_q_imu(capi, N, kind):
    """every trajectory with a full Q_imu: the QM = 2 instances"""
    first, chol = _plain(N)
    _check(capi, N, "plain", kind, first, chol, fullq=True)


def test_the_pruned_state_log_keeps_the_order(capi):
    """no prune rides on the downdate: order 2 is taken all the same, the window size comes from the prune's own launch"""
    _check(capi, 30, "plain", "resident", 40, 29, pruned_log=True)


def test_a_double_handle_counts_zero(capi):
    _check(capi, 14, "plain", "resident", 0, 0, dtype=capi.F64)


def test_the_switch_is_on_by_default_acts_under_order_one_only_and_a_copy_takes_it_over(capi):
    """10-camera windows without the small update, 22 frames in two calls: an untouched handle counts 20 / 20; with order 0 the
    switch changes nothing (0 / 0); a fresh handle copied from one with the switch off runs order 1 (20 / 0), and the other way
    round (20 / 20); msckf_hip_set_frame_order still takes 0 and 1 only"""
    N = 10
    trs, NF, CUT = _trajectories(N), _nf(N), _cut(N)
    cells = _cells(trs, N, "plain")

    def run(prepare):
        with _small_update("0"):
            bt = capi.Batch(B, N, F, N, capi.F32)
        for b, tr in enumerate(trs):
            bt.initialize(b, tr.cfg, tr.imu0)
        prepare(bt)
        bt.scenario_alloc(NF, sc.IMU_PER_FRAME)
        for k in range(NF):
            for b in range(B):
                rd, M, slots, obs, drop, skip = cells[k][b]
                bt.scenario_set(k, b, rd, M, slots, obs, drop, skip=skip)
        bt.scenario_commit()
        bt.run_frames(0, CUT); bt.run_frames(CUT, NF); bt.sync()
        out = (bt.frame_order_count(), bt.frame_order_chol_count())
        bt.close()
        return out

    def copied_from(on):
        def prepare(bt):
            with _small_update("0"):
                src = capi.Batch(B, N, F, N, capi.F32)
            for b, tr in enumerate(trs):
                src.initialize(b, tr.cfg, tr.imu0)
            src.set_frame_order_chol(on)
            bt.set_frame_order_chol(not on)
            bt.copy_state_from(src)
            src.close()
        return prepare

    def refuses_two(bt):
        with pytest.raises(capi.HipError):
            bt.set_frame_order(2)

    assert run(refuses_two) == (20, 20)
    assert run(lambda bt: (bt.set_frame_order(0), bt.set_frame_order_chol(True))) == (0, 0)
    assert run(copied_from(False)) == (20, 0)
    assert run(copied_from(True)) == (20, 20)


def test_the_benchmark_shape_in_two_slices(capi):
    """once at 64 trajectories x 30 cameras x 200 tracks, 8 frames in one call with k_update_small off, two slices where the
    process has the hardware queues for them: every slice's frames but the first take order 2, slices x 7"""
    Bb, Nb, Fb, nf = 64, 30, 200, 8
    trs = [sc.Trajectory(3, b, Nb, Fb, nf) for b in range(Bb)]
    out = []
    for order in (0, 1, 2):
        with _small_update("0"):
            bt = capi.Batch(Bb, Nb, Fb, Nb, capi.F32)
        for b, tr in enumerate(trs):
            bt.initialize(b, tr.cfg, tr.imu0)
        _set_order(bt, order)
        bt.set_streams(2)
        slices = bt.effective_streams()
        bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
        for k in range(nf):
            for b, tr in enumerate(trs):
                fr = tr.frames[k]
                bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == Nb else 0)
        bt.scenario_commit()
        bt.run_frames(0, nf); bt.sync()
        out.append(([H.snapshot(bt, b) for b in range(Bb)], bt.frame_order_count(), bt.frame_order_chol_count(), slices))
        bt.close()
    (s0, f0, c0, _), (s1, f1, c1, _), (s2, f2, c2, slices) = out
    assert (f0, c0) == (0, 0) and c1 == 0 and f1 == f2 == c2 == slices * (nf - 1)
    assert min(s[4]["n_passed"] for s in s2) > 0
    assert [b for b in range(Bb) if not H.same_bits(s2[b], s1[b])] == []
    assert [b for b in range(Bb) if not H.same_bits(s2[b], s0[b])] == []
