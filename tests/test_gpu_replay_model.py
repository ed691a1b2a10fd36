"""The Monte-Carlo replay's Q_imu model on the device (msckf_hip_replay_assign_q, msckf_hip_replay_walk; csrc/replay_plan.h MODEL,
k_replay_walk_scan and the model instantiation of k_replay_expand in kernels_replay.hip): correlated IMU noise drawn from the
filter's own Q_imu and the two bias random walks, tabulated once per assignment.  Shapes and bounds: tests/replay_model_lab.py.

  1. the walk table against the numpy twin, at frame counts around the scan's chunk (REPLAY_SCAN_CHUNK of csrc/dev_common.h)
  2. the expansion's read-backs against the twin: integers, dT, slots and off exact, readings and coordinates to the lab's bounds
     (double) / one float ulp of float32(twin) (float); also with more samples than one pass of the kernel's IMU phase takes
     (MODEL_TILE of kernels_replay.hip) and an entry count that puts the workgroup edge (REPLAY_CHUNK) among the dT items
  3. the frame loop reads what the kernel wrote: an ordinary scenario staged from the read-backs gives the same bits through
     run_frames, however the replay's call is cut and sliced
  4. switching between the two assignments and back, equal and different seeds
  5. scale = 0 is the sequence replicated, with an all-zero walk table
  6. every refusal reaches HipError with its code
  7. two slices on different frames read the same table

Measured on an MI355X, worst |device - twin| over its bound in double: walk table 1.05e-3 at 63, 64 and
65 frames, stored values 0.158 on the common cells and 0.505 at the tile and workgroup edges (one ulp of a coordinate); the tests
print the figures (-s)."""
import os
import re

import numpy as np
import pytest

import helpers as H
import replay_model_lab as ML
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu
PRECS = ("f32", "f64")
_DEV_COMMON = open(os.path.join(H.ROOT, "msckf_mono_amd", "csrc", "dev_common.h")).read()
CHUNK = int(re.search(r"constexpr int REPLAY_CHUNK = (\d+);", _DEV_COMMON).group(1))
SCAN = int(re.search(r"constexpr int REPLAY_SCAN_CHUNK = (\d+);", _DEV_COMMON).group(1))
TILE = int(re.search(r"constexpr int MODEL_TILE = (\d+);", open(os.path.join(H.ROOT, "msckf_mono_amd", "csrc", "kernels_replay.hip")).read()).group(1))
NFS = (SCAN - 1, SCAN, SCAN + 1)
NF = SCAN + 1                       # the frame count of everything but check 1
CUT = SCAN // 2 + 5                 # a cut inside the first scan chunk
SIGMA4 = (7.07e-3, 7.07e-2) + ML.SIGMA_UV


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c_
    c_.lib()
    return c_


def _cd(capi, prec):
    return capi.F64 if prec == "f64" else capi.F32


def _init(bt, nf):
    for b in range(ML.B):
        bt.initialize(b, *ML.init_of(nf, b))


def _batch(capi, prec, nf=NF):
    bt = capi.Batch(ML.B, ML.N_CAP, ML.F_CAP, ML.M_CAP, _cd(capi, prec))
    _init(bt, nf)
    return bt


def _replay_batch(capi, prec, nf=NF, **kw):
    bt = _batch(capi, prec, nf)
    ML.stage_replay(bt, nf, **kw)
    return bt


def _results(bt):
    bt.sync()
    return dict(snap=[H.snapshot(bt, b) for b in range(bt.B)], log=bt.frame_log_read()[0])


def _same(x, y):
    assert len(x["snap"]) == len(y["snap"])
    for b, (p, q) in enumerate(zip(x["snap"], y["snap"])):
        assert H.same_bits(p, q), b
    assert np.array_equal(x["log"], y["log"])


def _run(bt, cuts=((0, NF),)):
    bt.frame_log_enable(NF)
    for f0, f1 in cuts:
        bt.run_frames_replay(f0, f1)
    return _results(bt)


_READ, _ORD = {}, {}


def _readbacks(capi, prec):
    """replay_expand of every (frame, trajectory) and the walk table of the common assignment: read once per dtype, shared,
    never written to"""
    if prec not in _READ:
        bt = _replay_batch(capi, prec)
        _READ[prec] = ([[bt.replay_expand(f, b) for b in range(ML.B)] for f in range(NF)], bt.replay_walk())
        bt.close()
    return _READ[prec]


def _stage_ordinary(bt, cells):
    """cells[f][b] (replay_expand read-backs) as an ordinary resident scenario"""
    bt.scenario_alloc(len(cells), ML.K)
    for f, row in enumerate(cells):
        for b, ex in enumerate(row):
            k = max(ex["k"], 0)
            bt.scenario_set(f, b, ex["rd"][:k], ex["M"][:ex["n"]], ex["slots"], ex["obs"], ex["drop"], skip=ex["k"] < 0)
    bt.scenario_commit()


def _ordinary(capi, prec):
    """run_frames(0, NF) on the scenario staged from the read-backs, one stream: once per dtype"""
    if prec not in _ORD:
        bt = _batch(capi, prec)
        _stage_ordinary(bt, _readbacks(capi, prec)[0])
        bt.set_streams(1)
        bt.frame_log_enable(NF)
        bt.run_frames(0, NF)
        _ORD[prec] = _results(bt)
        bt.close()
    return _ORD[prec]


# -------------------------------------------------------------------------------------------- 1. the walk table against the twin
def _check_walk(dev, nf, cells_of, seeds, scale, factors):
    """dev [nf + 1][B][6] against the twin under the lab's bound; returns the worst |device - twin| / bound"""
    worst = 0.0
    for b in range(dev.shape[1]):
        cells = cells_of(b)
        twin = sc.replay_walk(cells, seeds[b], factors[b], scale[b])
        tol = ML.walk_tol(factors[b], scale[b], ML.dt_max(cells), ML.samples_before(cells), twin)
        ratio = np.abs(dev[:, b] - twin) / tol
        worst = max(worst, float(ratio.max()))
        assert np.all(np.abs(dev[:, b] - twin) <= tol), (b, float(ratio.max()))
    return worst


@pytest.mark.parametrize("nf", NFS)
@pytest.mark.parametrize("prec", PRECS)
def test_walk_table_against_the_twin_around_the_scan_chunk(capi, prec, nf):
    """frames + 1 rows per trajectory, the table in double whatever the handle's scalar: SCAN - 1 frames (one chunk, not full),
    SCAN (one full chunk: the last row is the chunk's last lane's) and SCAN + 1 (the carry into a second chunk); row 0 zero, the
    rows over the cell with k = 0 and over the skipped cell equal, the trajectory with zero walk blocks all zero; ranges of the
    table read back as what they are"""
    bt = _replay_batch(capi, prec, nf)
    dev = bt.replay_walk()
    assert dev.shape == (nf + 1, ML.B, 6) and not dev[0].any() and not dev[:, 1].any()
    worst = _check_walk(dev, nf, lambda b: ML.readings_of(nf, b), ML.SEEDS, ML.SCALE, ML.factors())
    print("worst |device - twin| / bound of the walk table (%s, %d frames): %.3g" % (prec, nf, worst))
    for b in (0, 2):
        assert np.all(dev[-1, b] != 0.0)
        for f in (ML.ZERO_FRAME, ML.SKIP_FRAME):
            assert np.array_equal(dev[f, b], dev[f + 1, b]) and not np.array_equal(dev[f - 1, b], dev[f, b])
    assert not np.array_equal(dev[:, 0], dev[:, 2])                       # the same sequence, Q and scale under another seed
    assert np.array_equal(bt.replay_walk(nf - 2, nf + 1, 1, 2), dev[nf - 2:, 1:]) and np.array_equal(bt.replay_walk(3, 4, 2, 1), dev[3:4, 2:])
    assert bt.replay_walk(5, 5).shape == (0, ML.B, 6) and bt.replay_walk(0, 2, 1, 0).shape == (2, 0, 6)
    bt.close()


# ------------------------------------------------------------------------------------------ 2. the expansion against the twin
def _check_cell(prec, ex, rd, obs, twin_rd, twin_obs, tol_imu, where, worst):
    """a read-back against the twin's doubles: dT and the rows from k on exact, the rest under the bounds (double) or within one
    float ulp of float32(twin) (float)"""
    k = len(rd)
    assert ex["rd"].shape == twin_rd.shape and ex["obs"].shape == twin_obs.shape, where
    assert not ex["rd"][k:].any(), where
    if prec == "f64":
        assert np.array_equal(ex["rd"][:, 6], twin_rd[:, 6]), where
        for d, t, tol in ((ex["rd"][:k, :6], twin_rd[:k, :6], tol_imu), (ex["obs"], twin_obs, ML.obs_tol(twin_obs))):
            if d.size:
                ratio = np.abs(d - t) / tol
                worst[0] = max(worst[0], float(ratio.max()))
                assert np.all(np.abs(d - t) <= tol), (where, float(ratio.max()))
        return
    for d, t in ((ex["rd"], twin_rd), (ex["obs"], twin_obs)):
        t32 = t.astype(np.float32)
        assert np.array_equal(d, d.astype(np.float32).astype(np.float64)), where          # a float widened
        assert np.all(np.abs(d - t32.astype(np.float64)) <= np.spacing(np.abs(t32)).astype(np.float64)), where
    assert np.array_equal(ex["rd"][:, 6], twin_rd[:, 6].astype(np.float32).astype(np.float64)), where


@pytest.mark.parametrize("prec", PRECS)
def test_expansion_against_the_twin(capi, prec):
    """every (frame, trajectory) of SCAN + 1 frames: cells of k = 4, 3, 1 and 0 samples with unequal dT and a skipped cell; n,
    drop, k, M and slots are the sequence's, off the sequence's rebased, readings = (value + walk) + noise and coordinates the
    twin's.  The twin's cell starts from the twin's own walk: the bound carries the walk's"""
    reads, _ = _readbacks(capi, prec)
    worst, ks = [0.0], set()
    walks = [ML.twin_walk(NF, b) for b in range(ML.B)]
    for b in range(ML.B):
        cells = ML.readings_of(NF, b)
        n, dtm, L, scale = ML.samples_before(cells), ML.dt_max(cells), ML.factors()[b], ML.SCALE[b]
        for f in range(NF):
            ex = reads[f][b]
            rd, M, slots, obs, drop, skip = ML.sequences(NF)[ML.SEQ_OF[b]][f]
            assert (ex["n"], ex["drop"], ex["k"]) == (len(M), drop, -1 if skip else len(rd)), (f, b)
            ks.add(ex["k"])
            Mp = np.zeros(ML.F_CAP, np.int32)
            Mp[:len(M)] = M
            base = sum(len(ML.sequences(NF)[ML.SEQ_OF[q]][f][2]) for q in range(b))
            assert np.array_equal(ex["M"], Mp) and np.array_equal(ex["slots"], slots), (f, b)
            assert np.array_equal(ex["off"], base + np.concatenate([[0], np.cumsum(Mp)[:-1]])), (f, b)
            twin_rd, twin_obs = ML.twin_cell(NF, f, b, walks[b])
            tol = None
            if len(rd):
                noise, delta = sc.replay_model_increments(rd[:, 6], sc.replay_model_draws(ML.SEEDS[b], f, len(rd), L), scale)
                prefix = np.concatenate([np.zeros((1, 6)), np.cumsum(delta, 0)[:-1]])
                tol = ML.imu_tol(L, scale, dtm, n[f], rd[:, 6], twin_rd[:len(rd), :6], walks[b][f] + prefix)
                assert len(set(rd[:, 6].tolist())) > 1 or len(rd) == 1
            _check_cell(prec, ex, rd, obs, twin_rd, twin_obs, tol, (f, b), worst)
    assert ks == {4, 3, 1, 0, -1}
    assert sum(len(ML.sequences(NF)[s][f][2]) for s in range(ML.S) for f in ML.TRACK_FRAMES) > 20
    print("worst |device - twin| / bound of the expansion (%s): %.3g" % (prec, worst[0]))


def _edge_cells():
    """S = 2 sequences x 3 frames for a handle of n_cap = m_cap = 32, f_cap = 9 (no filter runs on it), K = TILE + 1: cells of
    TILE + 1 samples (a second pass of the IMU phase for one sample, the walk's prefix carried over), TILE (one full pass) and a
    few.  Sequence 1's cell of frame 1 has CHUNK - 2 entries: the workgroup that forms the IMU readings also has a full load of
    entries, and the edge to the second workgroup falls among the dT items.  Sequence 0's cells have five to nine entries, so
    that the trajectories' bases differ."""
    rng = sc.SplitMix64(0xED6F)

    def cell(k, counts):
        M = np.array(counts, dtype=np.int32)
        slots = np.concatenate([np.arange(m, dtype=np.int32) for m in counts]) if len(counts) else np.zeros(0, np.int32)
        rd = np.concatenate([rng.normal(6 * k).reshape(k, 6), 0.004 + 0.002 * rng.uniform(k).reshape(k, 1)], 1)
        return rd, M, slots, 2.0 * rng.uniform(2 * int(M.sum())).reshape(-1, 2) - 1.0, 0, False

    n = CHUNK - 2
    assert n + 1 <= 9 * 32 and n < CHUNK < n + TILE + 1
    return [[cell(TILE + 1, [5]), cell(3, [7]), cell(TILE, [9])], [cell(4, [3, 4]), cell(TILE + 1, [32] * (n // 32) + [n % 32]), cell(2, [6])]]


@pytest.mark.parametrize("prec", PRECS)
def test_expansion_at_the_tile_and_workgroup_edges(capi, prec):
    """cells of TILE + 1, TILE and a few samples, one of them beside CHUNK - 2 entries, with a walk that frame 0 has started and
    frame 2 continues: walk table and expansion against the twin"""
    seqs = _edge_cells()
    factors = ML.factors()
    bt = capi.Batch(ML.B, 32, 9, 32, _cd(capi, prec))
    K = TILE + 1
    bt.replay_alloc(2, 3, K)
    for f in range(3):
        for s in range(2):
            rd, M, slots, obs, drop, skip = seqs[s][f]
            bt.replay_set_cell(f, s, rd, M, slots, obs, drop, skip=skip)
    bt.replay_commit()
    bt.replay_assign_q(ML.SEQ_OF, ML.SEEDS, ML.q_of(), ML.SCALE, ML.SIGMA_UV)

    def cells_of(b):
        return [seqs[ML.SEQ_OF[b]][f][0] for f in range(3)]

    dev = bt.replay_walk()
    worst = [_check_walk(dev, 3, cells_of, ML.SEEDS, ML.SCALE, factors)]
    assert len(seqs[1][1][2]) == CHUNK - 2
    for b in range(ML.B):
        cells = cells_of(b)
        walk = sc.replay_walk(cells, ML.SEEDS[b], factors[b], ML.SCALE[b])
        n, dtm = ML.samples_before(cells), ML.dt_max(cells)
        for f in range(3):
            rd, M, slots, obs, drop, skip = seqs[ML.SEQ_OF[b]][f]
            ex = bt.replay_expand(f, b)
            assert (ex["n"], ex["drop"], ex["k"]) == (len(M), 0, len(rd)) and np.array_equal(ex["slots"], slots), (f, b)
            base = sum(len(seqs[ML.SEQ_OF[q]][f][2]) for q in range(b))
            assert ex["off"][0] == base, (f, b)
            twin_rd, twin_obs, _ = sc.replay_model_cell(rd, obs, f, ML.SEEDS[b], factors[b], ML.SCALE[b], ML.SIGMA_UV, walk[f], K=K)
            noise, delta = sc.replay_model_increments(rd[:, 6], sc.replay_model_draws(ML.SEEDS[b], f, len(rd), factors[b]), ML.SCALE[b])
            prefix = np.concatenate([np.zeros((1, 6)), np.cumsum(delta, 0)[:-1]])
            tol = ML.imu_tol(factors[b], ML.SCALE[b], dtm, n[f], rd[:, 6], twin_rd[:len(rd), :6], walk[f] + prefix)
            _check_cell(prec, ex, rd, obs, twin_rd, twin_obs, tol, (f, b), worst)
    print("worst |device - twin| / bound at the tile and workgroup edges (%s): %.3g" % (prec, worst[0]))
    bt.close()


# --------------------------------------------------------------------------- 3. the loop reads what the kernel wrote, bit for bit
@pytest.mark.parametrize("slices", (1, 2))
@pytest.mark.parametrize("cuts", ([(0, NF)], [(0, CUT), (CUT, NF)]), ids=["one_call", "two_calls"])
@pytest.mark.parametrize("prec", PRECS)
def test_model_replay_runs_the_bits_of_the_ordinary_run_on_its_read_backs(capi, prec, cuts, slices):
    """run_frames_replay under the model against run_frames(0, NF) on a second handle whose ordinary scenario holds the
    expansion's read-backs: snapshot of every trajectory and every frame-log record, in one call and in two cut inside a scan
    chunk, with one slice and with exactly two (trajectory 0 | 1, 2)"""
    want = _ordinary(capi, prec)
    bt = _replay_batch(capi, prec)
    bt.set_streams(slices)
    bt.set_slices_exact(slices > 1)
    assert bt.effective_streams() == slices
    got = _run(bt, cuts)
    bt.close()
    assert got["log"].shape == (NF, ML.B, 48) and got["log"][:, :, 38].max() > 0          # (n_tracks: some frames do update)
    _same(got, want)


# ------------------------------------------------------------------------------------------------- 4. switching, and the seeds
@pytest.mark.parametrize("prec", PRECS)
def test_switching_between_the_two_assignments_and_back(capi, prec):
    """under the model, then under sigma4 (the bits of a handle that only ever knew sigma4), then under the model again (the
    bits of the first run, the walk table those of the first); the filters start afresh each time"""
    bt = _replay_batch(capi, prec)
    first, walk = _run(bt), bt.replay_walk()
    _same(first, _ordinary(capi, prec))
    _init(bt, NF)
    bt.replay_assign(ML.SEQ_OF, ML.SEEDS, SIGMA4)
    with pytest.raises(capi.HipError, match=r"\(-22\).*not assigned through msckf_hip_replay_assign_q"):
        bt.replay_walk()
    second = _run(bt)
    _init(bt, NF)
    bt.replay_assign_q(ML.SEQ_OF, ML.SEEDS, ML.q_of(), ML.SCALE, ML.SIGMA_UV)
    third = _run(bt)
    assert np.array_equal(bt.replay_walk(), walk)
    bt.close()
    only = _batch(capi, prec)
    ML.stage_sequences(only, NF)
    only.replay_assign(ML.SEQ_OF, ML.SEEDS, SIGMA4)
    only.replay_commit()
    _same(second, _run(only))
    only.close()
    _same(third, first)
    assert not np.array_equal(second["log"], first["log"])


@pytest.mark.parametrize("prec", PRECS)
def test_equal_seeds_equal_bits_and_another_seed_another_walk(capi, prec):
    """trajectories 0 and 2 replay sequence 1 under the same Q and scale: with one seed their walks, expansions and final
    states agree bit for bit; the common shape's seeds differ, and so do the walks"""
    seeds = [77, 78, 77]
    bt = _replay_batch(capi, prec, seeds=seeds)
    walk = bt.replay_walk()
    ex0, ex2 = bt.replay_expand(CUT, 0), bt.replay_expand(CUT, 2)
    got = _run(bt)
    bt.close()
    assert np.array_equal(walk[:, 0], walk[:, 2]) and walk[-1, 0].all()
    assert np.array_equal(ex0["rd"], ex2["rd"]) and np.array_equal(ex0["obs"], ex2["obs"])
    assert H.same_bits(got["snap"][0], got["snap"][2])
    common = _readbacks(capi, prec)[1]
    assert not np.array_equal(common[:, 0], common[:, 2]) and not np.array_equal(common[:, 0], walk[:, 0])
    assert not H.same_bits(_ordinary(capi, prec)["snap"][0], _ordinary(capi, prec)["snap"][2])


# ------------------------------------------------------------------------------------------------------------------ 5. scale = 0
@pytest.mark.parametrize("prec", PRECS)
def test_no_scale_is_the_sequence_replicated(capi, prec):
    """scale = 0: an all-zero walk table and the sequence's own readings whatever Q is; with sigma_u = sigma_v = 0 as well the
    bits of run_frames on an ordinary scenario that holds each trajectory's noise-free sequence"""
    bt = _replay_batch(capi, prec, scale=0.0, sigma_uv=(0.0, 0.0))
    assert not bt.replay_walk().any()
    for f in (0, 6, ML.ZERO_FRAME, ML.SKIP_FRAME, NF - 1):
        for b in range(ML.B):
            rd, _, _, obs, _, _ = ML.sequences(NF)[ML.SEQ_OF[b]][f]
            ex = bt.replay_expand(f, b)
            want_rd, want_obs = (rd, obs) if prec == "f64" else (rd.astype(np.float32).astype(np.float64), obs.astype(np.float32).astype(np.float64))
            assert np.array_equal(ex["rd"][:len(rd)], want_rd) and not ex["rd"][len(rd):].any() and np.array_equal(ex["obs"], want_obs), (f, b)
    got = _run(bt)
    bt.close()
    bo = _batch(capi, prec)
    bo.scenario_alloc(NF, ML.K)
    for f in range(NF):
        for b, s in enumerate(ML.SEQ_OF):
            rd, M, slots, obs, drop, skip = ML.sequences(NF)[s][f]
            bo.scenario_set(f, b, rd, M, slots, obs, drop, skip=skip)
    bo.scenario_commit()
    bo.frame_log_enable(NF)
    bo.run_frames(0, NF)
    want = _results(bo)
    bo.close()
    _same(got, want)
    assert H.same_bits(got["snap"][0], got["snap"][2])


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_every_refusal_of_the_model_reaches_the_caller_with_its_code(capi):
    EINVAL = r"\(-22\)"
    Q, ok = ML.q_of(), (ML.SEQ_OF, ML.SEEDS)
    bt = _batch(capi, "f32")
    with pytest.raises(capi.HipError, match=EINVAL + ".*no replay allocated"):
        bt.replay_assign_q(*ok, Q, ML.SCALE, ML.SIGMA_UV)
    with pytest.raises(capi.HipError, match=EINVAL + ".*no replay allocated"):
        bt.replay_walk(0, 0)
    ML.stage_sequences(bt, NF)
    # the assignment, in the header's order: each call is wrong in everything after its own rule as well
    bad_q = [Q[0], Q[1], -np.eye(12)]
    for seq_of in ([1, 2, 1], [1, 0, -1]):
        with pytest.raises(capi.HipError, match=EINVAL + ".*seq_of names no sequence"):
            bt.replay_assign_q(seq_of, ML.SEEDS, bad_q, [0.05, -1.0, 0.05], ML.SIGMA_UV)
    for bad in (float("inf"), float("nan")):
        nq = [Q[0], Q[1].copy(), -np.eye(12)]
        nq[1][3, 7] = bad
        with pytest.raises(capi.HipError, match=EINVAL + ".*Q, scale and sigma must be finite"):
            bt.replay_assign_q(*ok, nq, [0.05, -1.0, 0.05], ML.SIGMA_UV)
        with pytest.raises(capi.HipError, match=EINVAL + ".*Q, scale and sigma must be finite"):
            bt.replay_assign_q(*ok, bad_q, [0.05, bad, 0.05], (-1.0, 1e-3))
        with pytest.raises(capi.HipError, match=EINVAL + ".*Q, scale and sigma must be finite"):
            bt.replay_assign_q(*ok, bad_q, -1.0, (1e-3, bad))
    with pytest.raises(capi.HipError, match=EINVAL + ".*scale and sigma must not be negative"):
        bt.replay_assign_q(*ok, bad_q, [0.05, -1e-9, 0.05], ML.SIGMA_UV)
    with pytest.raises(capi.HipError, match=EINVAL + ".*scale and sigma must not be negative"):
        bt.replay_assign_q(*ok, bad_q, ML.SCALE, (1e-3, -1e-3))
    with pytest.raises(capi.HipError, match=EINVAL + ".*Q is not positive semi-definite"):
        bt.replay_assign_q(*ok, bad_q, ML.SCALE, ML.SIGMA_UV)
    with pytest.raises(ValueError):
        bt.replay_assign_q([1, 0], ML.SEEDS, Q, ML.SCALE, ML.SIGMA_UV)
    # nothing is assigned after all that; the walk asks for the commit, then for the model's assignment
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.replay_walk()
    bt.replay_commit()
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not assigned"):
        bt.run_frames_replay(0, NF)
    with pytest.raises(capi.HipError, match=EINVAL + ".*not assigned through msckf_hip_replay_assign_q"):
        bt.replay_walk()
    bt.replay_assign(ML.SEQ_OF, ML.SEEDS, SIGMA4)
    with pytest.raises(capi.HipError, match=EINVAL + ".*not assigned through msckf_hip_replay_assign_q"):
        bt.replay_walk()
    bt.replay_assign_q(*ok, Q, ML.SCALE, ML.SIGMA_UV)
    for bad in ((-1, 2, 0, 3), (0, NF + 2, 0, 3), (3, 2, 0, 3), (0, 2, 1, 3), (0, 2, -1, 1), (0, 2, 0, -1)):
        with pytest.raises(capi.HipError, match=EINVAL + ".*walk range out of bounds"):
            bt.replay_walk(*bad)
    # a refused assignment leaves the one made before: the walk is still the common one, and the handle runs
    with pytest.raises(capi.HipError, match=EINVAL + ".*Q is not positive semi-definite"):
        bt.replay_assign_q(*ok, bad_q, ML.SCALE, ML.SIGMA_UV)
    assert np.array_equal(bt.replay_walk(), _readbacks(capi, "f32")[1])
    bt.run_frames_replay(0, 4)
    bt.sync()
    assert [bt.num_cam_states(b) for b in range(ML.B)] == [4] * ML.B
    # a patched cell un-commits, and the table is rebuilt from the new cells
    rd = ML.sequences(NF)[1][5][0].copy()
    rd[:, 6] *= 2.0
    bt.replay_set_cell(5, 1, rd, [], [], np.zeros((0, 2)), 0)
    with pytest.raises(capi.HipError, match=EINVAL + ".*replay not committed"):
        bt.replay_walk()
    bt.replay_commit()
    walk, common = bt.replay_walk(), _readbacks(capi, "f32")[1]
    assert np.array_equal(walk[:6], common[:6]) and np.array_equal(walk[:, 1], common[:, 1]) and not np.array_equal(walk[6:, 0], common[6:, 0])
    bt.close()


# ------------------------------------------------------------------------------- 7. two slices on different frames, one table
@pytest.mark.parametrize("prec", PRECS)
def test_two_slices_on_different_frames_read_one_table(capi, prec):
    """two slices enqueue their frames independently, so they are on different frames at any time, each reading its frame's row
    of the one table: the states of the one-slice run, and the table unchanged by the runs"""
    runs = []
    for slices in (1, 2):
        bt = _replay_batch(capi, prec)
        bt.set_streams(slices)
        bt.set_slices_exact(slices > 1)
        before = bt.replay_walk()
        runs.append(_run(bt, [(0, 3), (3, NF)]))
        assert bt.effective_streams() == slices and np.array_equal(bt.replay_walk(), before)
        bt.close()
    _same(runs[0], runs[1])
    _same(runs[1], _ordinary(capi, prec))
