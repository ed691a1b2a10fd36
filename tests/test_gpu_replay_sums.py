"""msckf_hip_replay_imu_sums (k_replay_imu_sums) and the per-seed stand-still initialisation built on it.

Inputs of the sums: two IMU-only sequences (no track at all) of 130 frames, K = 11, cells of 9, 10 and 11 samples in turn, one
cell with k = 0 and one skipped cell (both inside the first 64 frames and on sequence 1, which two of the B = 3 trajectories
replay with their own seeds); ranges of 1, 63, 64, 65 and 130 frames -- a lane with one frame, a wavefront one short of full,
full, one frame into the second pass, and three passes.  Both noise models (assign_q with replay_model_lab's dense Q_imu: both
walk densities non-zero), float and double.

Reference: the sum, in long double on the host, of the rows msckf_hip_replay_expand returns for every frame of the range -- the
expansion kernel itself, which is older than the sums.  The count is exact; every column is held to n 2^-52 sum |x| (n samples
in the range), twice the bound (n - 1) 2^-53 sum |x| of a double sum in ANY order, the tree's included.  Against the numpy twin
the per-sample bars of tests/test_gpu_replay.py and tests/test_gpu_replay_model.py (replay_model_lab's bounds) are summed over
the range's samples, plus the summation bound.

Measured on an MI355X (the tests print the figures, -s): against the host sum 0.067 (sigma4) and 0.086
(Q_imu model) of the bar in double, 0 in float (sums of floats in double are exact at these sizes); against the twin 0.0064 of its
bar in double, 0 in float."""
import numpy as np
import pytest

import helpers as H
import replay_model_lab as ML
from msckf_mono_amd import asl, scenario as sc

pytestmark = pytest.mark.gpu
PRECS = ("f32", "f64")
MODELS = ("sigma4", "q")
NF, K, B = 130, 11, 3
SEQ_OF = [1, 0, 1]
SEEDS = [0x5EA50000, 0x5EA50001, 0x5EA50002]
SIGMA = (7.07e-3, 7.07e-2, 0.0, 0.0)
SCALE = [0.05, 0.08, 0.05]
ZERO_FRAME, SKIP_FRAME = 20, 41
RANGES = ((7, 8), (0, 63), (1, 65), (0, 65), (0, NF))
_CELLS, _READ = {}, {}


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c_
    c_.lib()
    return c_


def _cd(capi, prec):
    return capi.F64 if prec == "f64" else capi.F32


def _cells():
    """cells[s][f]: the noise-free readings [k][7] of sequence s on frame f (None: skipped), cut from a trajectory's IMU stream"""
    if not _CELLS:
        for s in (0, 1):
            tr = sc.Trajectory(7, s, 6, 0, NF, imu_noise_scale=0.0, obs_noise_px=0.0, path_id=s)
            at, out = 0, []
            for f in range(NF):
                k = (10, 9, 11)[(f + s) % 3]
                if s == 1 and f in (ZERO_FRAME, SKIP_FRAME):
                    k = 0
                out.append(None if (s == 1 and f == SKIP_FRAME) else tr.readings[at:at + k])
                at += k
            assert at <= len(tr.readings)
            _CELLS[s] = out
    return _CELLS


def _factor():
    return sc.replay_noise_factor(ML.q_dense())


def _staged(capi, prec, model):
    bt = capi.Batch(B, 6, 4, 6, _cd(capi, prec))
    bt.replay_alloc(2, NF, K)
    none = np.zeros((0, 2))
    for s, cells in _cells().items():
        for f, rd in enumerate(cells):
            bt.replay_set_cell(f, s, np.zeros((0, 7)) if rd is None else rd, [], [], none, 0, skip=rd is None)
    if model == "q":
        bt.replay_assign_q(SEQ_OF, SEEDS, ML.q_dense(), SCALE, (0.0, 0.0))
    else:
        bt.replay_assign(SEQ_OF, SEEDS, SIGMA)
    bt.replay_commit()
    return bt


def _rows(capi, prec, model):
    """(per trajectory and frame the rows [k][7] the expansion writes, read back once; sums of all RANGES and of two halves)"""
    if (prec, model) not in _READ:
        bt = _staged(capi, prec, model)
        rows = []
        for b in range(B):
            per = []
            for f in range(NF):
                ex = bt.replay_expand(f, b)
                assert ex["k"] == (-1 if _cells()[SEQ_OF[b]][f] is None else len(_cells()[SEQ_OF[b]][f]))
                per.append(ex["rd"][:max(ex["k"], 0)])
            rows.append(per)
        sums = {r: bt.replay_imu_sums(*r) for r in RANGES + ((0, 40), (40, NF), (9, 9))}
        again = bt.replay_imu_sums(0, NF)
        whole = bt.replay_imu_sums()
        bt.close()
        _READ[(prec, model)] = rows, sums, again, whole
    return _READ[(prec, model)]


def _host_sum(per, f0, f1):
    """(the long double sum [8] of the read-back rows of frames [f0, f1), sum |x| [8])"""
    tot, mag = np.zeros(8, dtype=np.longdouble), np.zeros(8, dtype=np.longdouble)
    for f in range(f0, f1):
        for r in per[f]:
            tot[0] += 1
            tot[1:] += r.astype(np.longdouble)
            mag[1:] += np.abs(r).astype(np.longdouble)
    return tot, mag


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("prec", PRECS)
def test_sums_against_the_host_sum_of_the_expansions_rows(capi, prec, model):
    rows, sums, again, whole = _rows(capi, prec, model)
    assert {len(r) for r in rows[0]} == {0, 9, 10, 11} and {len(r) for r in rows[1]} == {9, 10, 11}
    worst = 0.0
    for (f0, f1) in RANGES:
        got = sums[(f0, f1)]
        assert got.shape == (B, 8)
        for b in range(B):
            tot, mag = _host_sum(rows[b], f0, f1)
            n = int(tot[0])
            assert got[b, 0] == n > 0, (f0, f1, b)
            bar = n * 2.0 ** -52 * mag[1:]
            diff = np.abs(got[b, 1:].astype(np.longdouble) - tot[1:])
            worst = max(worst, float(np.max(diff / bar)))
            assert np.all(diff <= bar), (f0, f1, b, diff / bar)
    print("worst |device sum - long double host sum| / (n 2^-52 sum|x|) (%s, %s): %.3g" % (prec, model, worst))
    # the same inputs, the same bits; the default range is all frames; an empty range is zeros
    assert np.array_equal(again, sums[(0, NF)]) and np.array_equal(whole, again) and not sums[(9, 9)].any()
    # sums and counts: two intervals add to the whole, within the whole's bar
    two = sums[(0, 40)] + sums[(40, NF)]
    for b in range(B):
        tot, mag = _host_sum(rows[b], 0, NF)
        assert two[b, 0] == sums[(0, NF)][b, 0]
        assert np.all(np.abs(two[b, 1:] - sums[(0, NF)][b, 1:]) <= int(tot[0]) * 2.0 ** -52 * mag[1:].astype(np.float64)), b
    # two seeds of one sequence draw different noise, and the same dT
    assert not np.array_equal(sums[(0, NF)][0, 1:7], sums[(0, NF)][2, 1:7]) and sums[(0, NF)][0, 7] == sums[(0, NF)][2, 7]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("prec", PRECS)
def test_sums_against_the_numpy_twin(capi, prec, model):
    """per sample the bar the expansion's own tests hold a stored reading to -- sigma4: 1e-13 sigma in double (dT exact); the
    model: replay_model_lab.imu_tol; float, either model: one ulp of float32(twin) -- summed over the samples of the range, plus
    the summation bound n 2^-52 sum |x| for the two different orders"""
    _, sums, _, _ = _rows(capi, prec, model)
    dtype = np.float64 if prec == "f64" else np.float32
    L = _factor()
    worst = 0.0
    for b in range(B):
        cells = _cells()[SEQ_OF[b]]
        as_list = [np.zeros((0, 7)) if c is None else c for c in cells]
        walk = sc.replay_walk(cells, SEEDS[b], L, SCALE[b]) if model == "q" else None
        before = ML.samples_before(as_list)
        dtm = ML.dt_max(as_list)
        bars, mags = np.zeros((NF, 7)), np.zeros((NF, 7))
        for f, rd in enumerate(as_list):
            if not len(rd):
                continue
            if model == "q":
                twin = sc.replay_model_cell(rd, np.zeros((0, 2)), f, SEEDS[b], L, SCALE[b], (0.0, 0.0), walk[f])[0]
                noise, delta = sc.replay_model_increments(rd[:, 6], sc.replay_model_draws(SEEDS[b], f, len(rd), L), SCALE[b])
                prefix = np.concatenate([np.zeros((1, 6)), np.cumsum(delta, 0)[:-1]])
                tol = ML.imu_tol(L, SCALE[b], dtm, before[f], rd[:, 6], twin[:, :6], walk[f] + prefix)
            else:
                twin = sc.replay_cell(rd, np.zeros((0, 2)), f, SEEDS[b], SIGMA)[0]
                tol = 1e-13 * np.array([SIGMA[0]] * 3 + [SIGMA[1]] * 3)[None, :] * np.ones((len(rd), 1))
            if prec == "f32":
                t32 = twin.astype(np.float32)
                bars[f] = np.spacing(np.abs(t32)).astype(np.float64).sum(0)
                bars[f, 6] = 0.0
            else:
                bars[f, :6] = tol.sum(0)
            mags[f] = np.abs(twin).sum(0)
        for (f0, f1) in RANGES:
            want = sc.replay_imu_sums(cells, SEEDS[b], f0, f1, sigma4=SIGMA if model == "sigma4" else None,
                                      model=(L, SCALE[b]) if model == "q" else None, dtype=dtype)
            got = sums[(f0, f1)][b]
            assert got[0] == want[0]
            bar = bars[f0:f1].sum(0) + want[0] * 2.0 ** -52 * mags[f0:f1].sum(0)
            diff = np.abs(got[1:] - want[1:])
            worst = max(worst, float(np.max(diff / bar)))
            assert np.all(diff <= bar), (b, f0, f1, diff / bar)
    print("worst |device sum - twin sum| / bar (%s, %s): %.3g" % (prec, model, worst))


def test_sums_are_refused_as_a_run_is(capi):
    bt = capi.Batch(B, 6, 4, 6, capi.F64)
    bt.replay_alloc(2, 4, K)
    with pytest.raises(capi.HipError, match=r"\(-22\).*frame range out of bounds"):
        bt.replay_imu_sums(0, 5)
    with pytest.raises(capi.HipError, match=r"\(-22\).*frame range out of bounds"):
        bt.replay_imu_sums(3, 2)
    with pytest.raises(capi.HipError, match=r"\(-22\).*replay not committed"):
        bt.replay_imu_sums(0, 4)
    bt.replay_commit()
    with pytest.raises(capi.HipError, match=r"\(-22\).*replay not assigned"):
        bt.replay_imu_sums(0, 4)
    assert bt.L.msckf_hip_replay_imu_sums(bt.h, 0, 4, None) == -22
    bt.close()


# ------------------------------------------------------------------------------------------------ the stand-still initialisation
@pytest.mark.parametrize("prec", PRECS)
def test_replay_standstill_sets_every_seed_from_its_own_samples(capi, prec):
    """a hand-made stand-still sequence -- constant omega (the gyro bias), a specific force that is a rotated -g plus a bias -- of
    12 frames of 10 samples, then 4 frames to run; white noise per seed.  Every trajectory's state equals asl.standstill_state of
    the means of its own replay_expand rows to 1e-12 relative; two seeds differ; the run that follows succeeds and logs"""
    still, nf, k = 12, 16, 10
    ang = 0.2
    C_IG = np.array([[np.cos(ang), 0, -np.sin(ang)], [0, 1, 0], [np.sin(ang), 0, np.cos(ang)]])
    bg, ba = np.array([0.002, -0.001, 0.003]), np.array([0.02, 0.01, -0.03])
    row = np.concatenate([bg, C_IG @ (-sc.GRAVITY) + ba, [0.005]])
    cfg = sc.filter_config(6)
    bt = capi.Batch(B, 6, 8, 6, _cd(capi, prec))
    for b in range(B):
        bt.initialize(b, cfg, sc.imu29_from_gt(sc.ground_truth(np.array(0.0)), np.zeros(3), np.zeros(3)))
    bt.replay_alloc(1, nf, k)
    for f in range(nf):
        bt.replay_set_cell(f, 0, np.tile(row, (k, 1)), [], [], np.zeros((0, 2)), 0)
    bt.replay_assign([0] * B, SEEDS, (1e-4, 1e-3, 0.0, 0.0))
    bt.replay_commit()
    states = bt.replay_standstill(0, still)
    assert states.shape == (B, 29)
    for b in range(B):
        rd = np.concatenate([bt.replay_expand(f, b)["rd"][:k] for f in range(still)])
        assert rd.shape == (still * k, 7)
        ref = asl.standstill_state(rd[:, 0:3].mean(0), rd[:, 3:6].mean(0))
        for sl in (slice(0, 4), slice(4, 7), slice(10, 13)):
            assert np.linalg.norm(states[b, sl] - ref[sl]) <= 1e-12 * np.linalg.norm(ref[sl]), (b, sl)
        assert not states[b, 7:10].any() and np.array_equal(states[b, 13:19], ref[13:19])
        assert np.array_equal(states[b, 19:23], states[b, 0:4]) and not states[b, 23:29].any()
        got = bt.imu_state(b)
        assert np.array_equal(got, states[b]) if prec == "f64" else np.allclose(got, states[b], rtol=1e-6, atol=1e-9)
        # the filter starts where the samples say: the tilt and the biases of the hand-made sequence, to the noise of 120 samples
        assert H.quat_angle(states[b, 0:4], sc.rot_to_quat(C_IG)) < 0.05 and np.allclose(states[b, 4:7], bg, atol=1e-4)
    assert not np.array_equal(states[0], states[1]) and not np.array_equal(states[0], states[2])
    bt.frame_log_enable(nf)
    assert bt.frame_log_count() == 0
    bt.run_frames_replay(still, nf)
    bt.sync()
    assert bt.frame_log_count() == nf - still
    log = bt.frame_log_read()[0]
    assert np.all(np.isfinite(log)) and np.all(log[:, :, 37] == np.arange(1, nf - still + 1)[:, None]) and np.all(log[:, :, 40] == 0)
    with pytest.raises(ValueError):
        bt.replay_standstill(3, 3)
    bt.close()
