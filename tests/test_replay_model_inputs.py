"""The numpy twin of the Monte-Carlo replay's Q_imu model (scenario.replay_noise_factor / replay_model_* / replay_walk /
replay_bias_gt) on its own, without a device: the walk is the naive loop's, a cell's end is the next frame's start, white-only
noise walks nowhere, the draws have the covariance they are drawn from, and the bounds of tests/test_gpu_replay_model.py
(tests/replay_model_lab.py) are tight enough to tell five wrong models from the right one by a factor of 100."""
import numpy as np
import pytest

import replay_model_lab as ML
from msckf_mono_amd import scenario as sc

NF = 63


def _naive_walk(cells, seed, L, scale):
    """Wstart by the header's text, one scalar operation after the other"""
    W = np.zeros((len(cells) + 1, 6))
    for f, rd in enumerate(cells):
        s_imu = sc.replay_subseeds(seed, f)[0]
        pairs = sc.replay_pairs(s_imu, 6 * len(rd))
        P = [0.0] * 6
        for i in range(len(rd)):
            z = pairs[6 * i:6 * i + 6].ravel()
            w = []
            for r in range(12):
                acc = 0.0
                for c in range(r + 1):
                    acc = acc + L[r, c] * z[c]
                w.append(acc)
            dT = rd[i, 6]
            if dT > 0.0:
                sq = np.sqrt(dT)
                for c, r in enumerate(ML.WALK_ROWS):
                    P[c] = P[c] + (scale * w[r]) * sq
        for c in range(6):
            W[f + 1, c] = W[f, c] + P[c]
    return W


@pytest.mark.parametrize("b", range(ML.B))
def test_the_walk_is_the_naive_loops_bit_for_bit(b):
    cells = ML.readings_of(NF, b)
    W = ML.twin_walk(NF, b)
    assert W.shape == (NF + 1, 6) and not W[0].any()
    assert np.array_equal(W, _naive_walk(cells, ML.SEEDS[b], ML.factors()[b], ML.SCALE[b]))
    assert np.array_equal(W, sc.replay_walk([c if len(c) else None for c in cells], ML.SEEDS[b], ML.factors()[b], ML.SCALE[b]))
    if b != 1:
        assert np.all(W[-1] != 0.0) and len(set(W[:, 0].tolist())) > NF - 3
    # a Trajectory's own cells: ten samples per frame
    tr = sc.Trajectory(7, 0, 6, 3, 5, imu_noise_scale=0.0, obs_noise_px=0.0)
    assert np.array_equal(sc.replay_walk(tr, 5, ML.factors()[0], 0.05), sc.replay_walk([tr.imu_for_frame(f) for f in range(5)], 5, ML.factors()[0], 0.05))


def test_a_cells_end_is_the_next_frames_start():
    """w_end of replay_model_cell = Wstart(f + 1), also over the cell with k = 0 and the skipped one; the first sample of a frame
    reads Wstart(f), the others the prefix on top of it"""
    for b in range(ML.B):
        W = ML.twin_walk(NF, b)
        L, scale = ML.factors()[b], ML.SCALE[b]
        for f, rd in enumerate(ML.readings_of(NF, b)):
            out, _, w_end = sc.replay_model_cell(rd, np.zeros((0, 2)), f, ML.SEEDS[b], L, scale, ML.SIGMA_UV, W[f], K=ML.K)
            assert np.array_equal(w_end, W[f + 1]), (b, f)
            assert out.shape == (ML.K, 7) and not out[len(rd):].any() and np.array_equal(out[:len(rd), 6], rd[:, 6])
            if len(rd):
                noise, delta = sc.replay_model_increments(rd[:, 6], sc.replay_model_draws(ML.SEEDS[b], f, len(rd), L), scale)
                assert np.array_equal(out[0, :6], (rd[0, :6] + (W[f] + 0.0)) + noise[0])
                if len(rd) > 1:
                    assert np.array_equal(out[1, :6], (rd[1, :6] + (W[f] + (0.0 + delta[0]))) + noise[1])
    for f in (ML.ZERO_FRAME, ML.SKIP_FRAME):
        W = ML.twin_walk(NF, 0)
        assert np.array_equal(W[f], W[f + 1]) and not np.array_equal(W[f - 1], W[f])


def test_white_only_noise_walks_nowhere_and_no_scale_is_the_sequence():
    L = sc.replay_noise_factor(ML.q_white_diag())
    assert np.array_equal(L, np.diag(np.sqrt(np.diag(ML.q_white_diag()))))
    for b in range(ML.B):
        W = sc.replay_walk(ML.readings_of(NF, b), ML.SEEDS[b], L, ML.SCALE[b])
        assert W.shape == (NF + 1, 6) and not W.any()
    assert not ML.twin_walk(NF, 1).any()                                  # zero walk blocks under correlated white noise
    W = sc.replay_walk(ML.readings_of(NF, 0), ML.SEEDS[0], ML.factors()[0], 0.0)
    assert not W.any()
    rd, _, _, obs, _, _ = ML.sequences(NF)[1][6]
    out, ob, _ = sc.replay_model_cell(rd, obs, 6, 9, ML.factors()[0], 0.0, (0.0, 0.0), W[6], K=ML.K)
    assert np.array_equal(out[:len(rd)], rd) and np.array_equal(ob, obs) and len(obs)


def test_a_sample_without_a_step_gets_neither_noise_nor_increment():
    rd = ML.sequences(NF)[0][4][0].copy()
    assert len(rd) == 4
    rd[1, 6], rd[2, 6] = 0.0, -0.005
    L = ML.factors()[0]
    start = np.arange(6) * 1e-3
    out, _, w_end = sc.replay_model_cell(rd, np.zeros((0, 2)), 4, 7, L, 0.05, ML.SIGMA_UV, start)
    noise, delta = sc.replay_model_increments(rd[:, 6], sc.replay_model_draws(7, 4, 4, L), 0.05)
    assert not noise[1:3].any() and not delta[1:3].any() and noise[0].all() and delta[3].all()
    assert np.array_equal(out[1, :6], rd[1, :6] + (start + delta[0])) and np.array_equal(out[2, :6], rd[2, :6] + (start + delta[0]))
    assert np.array_equal(w_end, start + ((0.0 + delta[0]) + delta[3]))


def test_the_draws_have_the_covariance_they_are_drawn_from():
    """20 000 samples of one cell at a fixed seed: the sample covariance of w = L z within five standard errors of Q, entry by
    entry (standard error of entry (i, j) of a Gaussian sample covariance: sqrt((Q_ii Q_jj + Q_ij^2) / n)); a deterministic
    regression of the twin, not a statistical gate"""
    n = 20000
    for Q in (ML.q_dense(), ML.q_no_walk()):
        w = sc.replay_model_draws(0x5EED, 0, n, sc.replay_noise_factor(Q))
        assert w.shape == (n, 12) and np.all(np.isfinite(w))
        cov = w.T @ w / n
        se = np.sqrt((np.outer(np.diag(Q), np.diag(Q)) + Q * Q) / n)
        ratio = np.abs(cov - Q) / np.where(se > 0, se, 1.0)
        print("worst |cov - Q| / standard error: %.2f" % ratio.max())
        assert np.all(np.abs(cov - Q) <= 5.0 * se)
        assert abs(w.mean(0) / np.sqrt(np.where(np.diag(Q) > 0, np.diag(Q), 1.0) / n)).max() < 5.0


def test_bias_ground_truth_is_the_constant_bias_plus_the_walk():
    trs = [sc.Trajectory(7, p, 6, 3, 4, imu_noise_scale=0.0, obs_noise_px=0.0, path_id=p) for p in (1, 0, 1)]
    walks = np.stack([sc.replay_walk(tr, ML.SEEDS[b], ML.factors()[b], ML.SCALE[b]) for b, tr in enumerate(trs)], 1)
    gt = sc.replay_bias_gt(trs, walks)
    assert walks.shape == (5, 3, 6) and gt.shape == (4, 3, 6)
    for f in range(4):
        for b, tr in enumerate(trs):
            assert np.array_equal(gt[f, b], np.concatenate([tr.b_g, tr.b_a]) + walks[f + 1, b])
    assert np.array_equal(gt[:, 1], np.tile(np.concatenate([trs[1].b_g, trs[1].b_a]), (4, 1)))      # zero walk blocks


# ------------------------------------------------------------------------------------------------------------------ sensitivity
def _expand_all(b, L=None, shift=0, swap=False, pairs=6, unskip=False):
    """every cell of trajectory b over NF frames from the twin's parts, with a wrong model on request: (Wstart [NF + 1][6],
    stored readings per frame [k][6], W(f, i) per frame [k][6]).
      shift = 1   a sample reads the walk after its own increment        swap     sqrt(dT) and 1 / sqrt(dT) exchanged
      pairs = 3   sample i starts at pair 3 i                            unskip   the walk runs on over a skipped cell (on the
      L           another factor (the transposed one)                             samples of the cell before it)"""
    L = ML.factors()[b] if L is None else L
    seed, scale = ML.SEEDS[b], ML.SCALE[b]
    W, stored, walks, prev = np.zeros((NF + 1, 6)), [], [], None
    for f, cell in enumerate(ML.sequences(NF)[ML.SEQ_OF[b]]):
        rd, skipped = cell[0], cell[5]
        src = prev if (unskip and skipped) else rd
        k = len(src)
        w = sc.replay_model_draws(seed, f, k, L, pairs_per_sample=pairs)
        noise, delta = sc.replay_model_increments(src[:, 6], w, scale)
        if swap:
            sq = np.sqrt(src[:, 6])[:, None]
            noise, delta = (scale * w)[:, ML.WHITE] * sq, (scale * w)[:, ML.WALK_ROWS] / sq
        P = np.zeros((k + 2, 6))
        for i in range(k):
            P[i + 1] = P[i] + delta[i]
        P[k + 1] = P[k]
        Wfi = W[f] + P[shift:shift + len(rd)]
        stored.append((rd[:, :6] + Wfi) + noise[:len(rd)])
        walks.append(Wfi)
        W[f + 1] = W[f] + P[k]
        if len(rd):
            prev = rd
    return W, stored, walks


def _ratios(b, mutant):
    """(worst walk-table error, worst stored-reading error) of a mutant against the twin, each over the GPU test's bound"""
    L, scale = ML.factors()[b], ML.SCALE[b]
    cells = ML.readings_of(NF, b)
    W, stored, walks = _expand_all(b)
    n, dtm = ML.samples_before(cells), ML.dt_max(cells)
    Wm, sm, _ = mutant
    r_walk = float(np.max(np.abs(Wm - W) / ML.walk_tol(L, scale, dtm, n, W)))
    r_imu = 0.0
    for f, rd in enumerate(cells):
        if len(rd):
            r_imu = max(r_imu, float(np.max(np.abs(sm[f] - stored[f]) / ML.imu_tol(L, scale, dtm, n[f], rd[:, 6], stored[f], walks[f]))))
    return r_walk, r_imu


def test_the_parts_put_together_are_the_twin():
    for b in range(ML.B):
        W, stored, _ = _expand_all(b)
        assert np.array_equal(W, ML.twin_walk(NF, b))
        for f in (0, 5, ML.ZERO_FRAME, ML.SKIP_FRAME, NF - 1):
            k = len(stored[f])
            assert np.array_equal(stored[f], ML.twin_cell(NF, f, b, W)[0][:k, :6]), (b, f)
        assert _ratios(b, _expand_all(b)) == (0.0, 0.0)


@pytest.mark.parametrize("name, kwargs, walk_sees, imu_sees", [
    ("walk shifted by one sample", dict(shift=1), (), (0, 2)),
    ("L transposed", dict(L="T"), (0, 2), (0, 1, 2)),
    ("sqrt(dT) and 1 / sqrt(dT) exchanged", dict(swap=True), (0, 2), (0, 1, 2)),
    ("pair index 6 i -> 3 i", dict(pairs=3), (0, 2), (0, 1, 2)),
    ("skipped cell not skipped", dict(unskip=True), (0, 2), (0, 2)),
])
def test_a_wrong_model_misses_the_device_tests_bounds_by_a_factor_of_100(name, kwargs, walk_sees, imu_sees):
    """the walk table's bound sees a wrong model on the trajectories whose Q has a walk (0, 2; both replay the sequence with the
    skipped cell), the stored readings' bound on those named: each by 100 times the bound at least"""
    for b in range(ML.B):
        kw = dict(kwargs)
        if kw.get("L") == "T":
            kw["L"] = np.ascontiguousarray(ML.factors()[b].T)
        r_walk, r_imu = _ratios(b, _expand_all(b, **kw))
        print("%s, trajectory %d: walk %.3g x bound, readings %.3g x bound" % (name, b, r_walk, r_imu))
        if b in walk_sees:
            assert r_walk >= 100.0, (name, b, r_walk)
        if b in imu_sees:
            assert r_imu >= 100.0, (name, b, r_imu)
