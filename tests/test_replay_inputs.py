"""The Monte-Carlo replay's numpy twin (scenario.replay_*) and the common shape of its tests, without a device: the random
stream is a usable normal one, the frame sub-seeds do not collide, no noise level returns the sequence, and the double oracle
really updates on what the twin hands it -- so the device's parity with the oracle on the same inputs is about something."""
import numpy as np
import pytest

import helpers as H
import replay_lab as RL
from msckf_mono_amd import scenario as sc


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def test_the_twins_draws_are_standard_normal_and_uncorrelated():
    """4 x 10^5 draws (2 x 10^5 pairs of one sub-seed): mean within 0.01 of 0, variance within 0.02 of 1 (standard errors 0.0016
    and 0.0022), and the cosine and sine halves of the pairs correlated below 0.01 (standard error 0.0022)"""
    p = sc.replay_pairs(sc.replay_subseeds(RL.SEEDS[0], 3)[1], 200000)
    x = p.ravel()
    assert x.shape == (400000,) and np.all(np.isfinite(x))
    print("mean %.4f variance %.4f correlation %.4f" % (x.mean(), x.var(), np.corrcoef(p[:, 0], p[:, 1])[0, 1]))
    assert abs(x.mean()) < 0.01 and abs(x.var() - 1.0) < 0.02
    assert abs(np.corrcoef(p[:, 0], p[:, 1])[0, 1]) < 0.01


def test_frame_subseeds_are_distinct():
    """mix(seed, i) over 64 neighbouring seeds x 400 indices (200 frames' s_imu and s_obs): 25 600 different values, none of
    them one of the seeds"""
    seeds = [0xC0FFEE00 + b for b in range(64)]
    sub = np.concatenate([sc.replay_mix(s, np.arange(400)) for s in seeds])
    assert len(set(sub.tolist())) == 64 * 400
    assert not set(sub.tolist()) & set(seeds)
    assert sc.replay_subseeds(seeds[5], 7) == (int(sub[5 * 400 + 14]), int(sub[5 * 400 + 15]))


def test_noise_layout_of_a_cell():
    """sample i takes the pairs 3 i .. 3 i + 2 of s_imu as (g_x, g_y), (g_z, a_x), (a_y, a_z), entry e pair e of s_obs; rows from
    k on carry none; neighbouring frames and seeds share nothing"""
    imu, obs = sc.replay_noise(RL.SEEDS[2], 9, 10, 7, 33)
    s_imu, s_obs = sc.replay_subseeds(RL.SEEDS[2], 9)
    assert np.array_equal(imu[:7].reshape(21, 2), sc.replay_pairs(s_imu, 21)) and not imu[7:].any()
    assert np.array_equal(obs, sc.replay_pairs(s_obs, 33))
    for other in (sc.replay_noise(RL.SEEDS[2], 10, 10, 7, 33), sc.replay_noise(RL.SEEDS[3], 9, 10, 7, 33)):
        assert not np.isin(other[0][:7], imu[:7]).any() and not np.isin(other[1], obs).any()
    assert not sc.replay_noise(RL.SEEDS[2], 9, 10, -1, 0)[0].any()      # a skipped cell's count


def test_no_noise_level_returns_the_sequence():
    for tr in RL.sequences():
        for f in (0, 3, RL.NF - 1):
            rd, obs = sc.replay_expand(tr, f, 12345, (0.0, 0.0, 0.0, 0.0))
            assert np.array_equal(rd, tr.imu_for_frame(f)) and np.array_equal(obs, tr.frames[f]["obs"])
    rd, obs = sc.replay_cell(RL.sequences()[0].imu_for_frame(4)[:7], RL.sequences()[0].frames[4]["obs"], 4, 1, RL.SIGMA, K=10)
    assert rd.shape == (10, 7) and not rd[7:].any() and np.array_equal(rd[:7, 6], RL.sequences()[0].imu_for_frame(4)[:7, 6])
    one = sc.replay_expand(RL.sequences()[0], 4, 1, RL.SIGMA)
    assert np.array_equal(rd[:7], one[0][:7]) and np.array_equal(obs, one[1])      # the noise of a sample does not depend on k


def test_the_oracle_updates_on_the_common_shape(po):
    """double oracle, free-running on the twin's cells of every trajectory: at least one track passes the gate on every
    full-window frame, and the position stays within 2 cm of the ground truth over the 16 frames"""
    for b in range(RL.B):
        tr = RL.twin_trajectory(b)
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        n_full = 0
        for f in range(RL.NF):
            H.oracle_frame(o, tr, f, RL.N)
            if tr.frames[f]["Nw"] == RL.N:
                st = o.lastStats()
                assert st["n_passed"] >= 1 and st["m_rows"] > 0, (b, f, st)
                n_full += 1
        assert n_full == RL.NF - RL.N + 1
        err = np.linalg.norm(o.getImuState()[13:16] - tr.gt_frames["p"][RL.NF - 1])
        print("trajectory %d: position error after %d frames %.4f m" % (b, RL.NF, err))
        assert err < 0.02, (b, err)
