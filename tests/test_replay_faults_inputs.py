"""The replay's fault model on the CPU (scenario.replay_fault_*, the twin of csrc/replay_plan.h's FAULTS): the draws, the rule,
the layout of a faulted cell -- and the conditions the device parity tests rest on, measured on the double oracle over the lab
assignment (tests/replay_faults_lab.py) with zero tracks excluded."""
import numpy as np
import pytest

import replay_faults_lab as FLB
import replay_lab as RL
from msckf_mono_amd import scenario as sc


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


# ------------------------------------------------------------------------------------------------------------------ the draws
def test_missed_share_is_within_four_standard_errors():
    """p_miss = 0.15 over 2 * 10^5 entries in tracks long enough that the rule never bites (one track: M - #raw >= 2)"""
    n, p = 200000, 0.15
    code = sc.replay_fault_code([n], sc.replay_fault_draws(0xC0FFEE00, 3, n), p, 0.10)
    share = float((code == sc.FAULT_MISSED).mean())
    assert abs(share - p) <= 4.0 * np.sqrt(p * (1 - p) / n), share
    out = float((code == sc.FAULT_OUTLIER).sum()) / float((code != sc.FAULT_MISSED).sum())
    assert abs(out - 0.10) <= 4.0 * np.sqrt(0.10 * 0.90 / (n * (1 - p))), out


def test_the_three_uniforms_of_an_entry_and_of_its_neighbours_are_distinct():
    u = np.stack(sc.replay_fault_draws(0xC0FFEE01, 5, 4096), 1)                # [n][3]: entry e has draws 3 e, 3 e + 1, 3 e + 2
    assert np.all((u >= 0.0) & (u < 1.0))
    flat = u.reshape(-1)
    assert len(np.unique(flat)) == len(flat)                                   # pairwise distinct, within and across entries
    s = sc.replay_fault_seed(0xC0FFEE01, 5)
    assert np.array_equal(flat, sc.replay_uniform(s, np.arange(len(flat), dtype=np.uint64)))


def test_fault_sub_seeds_collide_with_no_frame_sub_seed_and_no_seed():
    """64 seeds x 200 frames: the fault sub-seeds are distinct from each other, from every frame's s_imu and s_obs, from the
    initial-error sub-seed mix(s, 2^63) and from the seeds themselves"""
    seeds = [0xC0FFEE00 + i for i in range(64)]
    flt, other = set(), set(seeds)
    for s in seeds:
        fr = np.arange(200, dtype=np.uint64)
        other |= set(int(x) for x in sc.replay_mix(s, np.uint64(2) * fr)) | set(int(x) for x in sc.replay_mix(s, np.uint64(2) * fr + np.uint64(1)))
        other.add(int(sc.replay_mix(s, 1 << 63)))
        mine = [sc.replay_fault_seed(s, f) for f in range(200)]
        assert sc.replay_subseeds(s, 7) == (int(sc.replay_mix(s, 14)), int(sc.replay_mix(s, 15)))
        flt |= set(mine)
    assert len(flt) == 64 * 200 and not flt & other
    assert sc.REPLAY_FAULT_STREAM == 2 ** 63 + 1 and sc.REPLAY_FAULT_STREAM > 2 * 2 ** 31 + 1      # beyond 2 f + 1 of any int frame


# ------------------------------------------------------------------------------------------------------- the rule and the layout
def _common_cells():
    for f in range(RL.NF):
        for b in range(RL.B):
            yield f, b, RL.twin_cell(f, b, seeds=FLB.SEEDS)


def test_p_zero_is_todays_expansion_bit_for_bit():
    zero = np.array([[0.0, 0.0, 0.01, 0.02]] * RL.B)
    for f, b, (rd, M, slots, obs, drop) in _common_cells():
        c = FLB.twin_cell(f, b, zero)
        assert np.array_equal(c["rd"], rd) and np.array_equal(c["Mp"], M) and np.array_equal(c["slots"], slots), (f, b)
        assert np.array_equal(c["obs"], obs) and not c["code"].any(), (f, b)


def test_p_miss_one_leaves_every_track_untouched():
    """every entry raw-missed: every track would keep none, so by the rule none loses any"""
    one = np.array([[1.0, 0.0, 0.0, 0.0]] * RL.B)
    n = 0
    for f, b, (rd, M, slots, obs, drop) in _common_cells():
        c = FLB.twin_cell(f, b, one)
        assert np.array_equal(c["Mp"], M) and np.array_equal(c["slots"], slots) and np.array_equal(c["obs"], obs), (f, b)
        n += len(M)
    assert n > 400


def test_p_out_one_displaces_every_entry_by_exactly_the_ring():
    rho_u, rho_v = 3 * FLB.PX, 30 * FLB.PX
    ring = np.array([[0.0, 1.0, rho_u, rho_v]] * RL.B)
    worst = 0.0
    for f, b, (rd, M, slots, obs, drop) in _common_cells():
        c = FLB.twin_cell(f, b, ring)
        assert np.array_equal(c["Mp"], M) and np.array_equal(c["slots"], slots) and np.all(c["code"] == sc.FAULT_OUTLIER), (f, b)
        if len(obs):
            d = c["obs"] - obs
            worst = max(worst, float(np.abs(np.hypot(d[:, 0] / rho_u, d[:, 1] / rho_v) - 1.0).max()))
    # the displaced coordinate is rounded at the coordinate's size (<= 1), the ring is rho: 1.1e-16 / rho_u = 1.7e-14 per axis
    assert worst <= 1e-12, worst


def test_partition_is_stable_and_every_track_keeps_two():
    """both probabilities high: the layout of every cell -- the survivors in sequence order, then the missed entries in sequence
    order, each with its own slot and noisy coordinates; M' >= 2 wherever M >= 2; the compact survivors are the kept entries"""
    f4 = np.array([[0.5, 0.3, 0.01, 0.02]] * RL.B)
    shielded = shortened = 0
    for f, b, (rd, M, slots, obs, drop) in _common_cells():
        c = FLB.twin_cell(f, b, f4)
        code, o = c["code"], 0
        assert np.array_equal(code, sc.replay_fault_code(M, sc.replay_fault_draws(FLB.SEEDS[b], f, len(slots)), 0.5, 0.3))
        for t, m in enumerate(int(x) for x in M):
            miss = code[o:o + m] == sc.FAULT_MISSED
            raw = sc.replay_fault_draws(FLB.SEEDS[b], f, len(slots))[0][o:o + m] < 0.5
            assert c["Mp"][t] == m - miss.sum() and c["Mp"][t] >= min(m, 2), (f, b, t)
            assert np.array_equal(miss, raw) or (m - raw.sum() < 2 and not miss.any()), (f, b, t)
            shielded += m - raw.sum() < 2 and raw.any(); shortened += miss.any()
            order = np.concatenate([np.nonzero(~miss)[0], np.nonzero(miss)[0]])
            assert np.array_equal(c["slots"][o:o + m], slots[o:o + m][order]), (f, b, t)
            clean = code[o:o + m][order] != sc.FAULT_OUTLIER
            assert np.array_equal(c["obs"][o:o + m][clean], obs[o:o + m][order][clean]), (f, b, t)
            o += m
        Mp, ss, so = FLB.survivors(c)
        assert np.array_equal(Mp, c["Mp"]) and len(ss) == Mp.sum() == (code != sc.FAULT_MISSED).sum()
    assert shielded > 10 and shortened > 100


def test_counts_are_the_codes_counted():
    got = FLB.counts(FLB.FAULT4)
    for b in range(RL.B):
        codes = [FLB.twin_cell(f, b)["code"] for f in range(RL.NF)]
        assert got[b, 0] == sum(len(c) for c in codes) and got[b, 1] == sum((c == 2).sum() for c in codes) and got[b, 2] == sum((c == 1).sum() for c in codes)
        assert got[b, 3] == sum(len(m) for m in FLB.cells_M(b))
    assert not got[0, 1:3].any() and not got[0, 4:].any() and got[1, 1] > 0 and got[1, 2] == 0 and got[2, 1] == 0 and got[2, 2] > 0
    cut = FLB.counts(FLB.FAULT4, f0=3, f1=11)
    assert np.array_equal(cut + FLB.counts(FLB.FAULT4, f0=0, f1=3) + FLB.counts(FLB.FAULT4, f0=11, f1=RL.NF), got)


# --------------------------------------------------------------------------------------------------------- on the double oracle
def test_lab_conditions_hold_with_zero_tracks_excluded(po):
    """the lab's per-trajectory assignment at the lab's seeds, every track of every frame: no double-oracle gamma within 1 % of
    its threshold, no triangulation cost within 5 % of its limit, a passing track on every full-window frame, a contaminated
    track passed at 3 px and one rejected at 30 px; and no track of fewer than two observations reaches the oracle"""
    run = FLB.lab_run(po)
    print("min |gamma / threshold - 1| per trajectory:", ["%.3g" % g for g in run["gate"]])
    print("min |cost / limit - 1| per trajectory:", ["%.3g" % g for g in run["tri"]])
    assert min(run["gate"]) >= FLB.GATE_MARGIN, run["gate"]
    assert min(run["tri"]) >= FLB.TRI_MARGIN, run["tri"]
    assert run["empty"] == 0
    conf = FLB.confusion(run, FLB.FAULT4)
    print("confusion per trajectory:\n", conf[:, :5])
    assert conf[2, 3] >= 1 and conf[3, 4] >= 1, conf
    assert not conf[:, 7].any() and not conf[:2, 3:5].any()
    assert np.array_equal(conf[:, 0], conf[:, 1:5].sum(1))
    for b in range(RL.B):
        tr = FLB.survivor_trajectory(b)
        assert all(fr["M"].min() >= 2 for fr in tr.frames if len(fr["M"])), b
    assert run["pos_err"] < 0.05, run["pos_err"]


@pytest.mark.parametrize("px", [None, 3, 10, 30])
def test_the_uniform_table_is_reproduced(po, px):
    """every trajectory at (0.15, 0.10, rho, rho), replay_lab's seeds: the fault counts of the twin, and replay_gate_confusion
    on the oracle's lastTracks -- the figures the model was designed at.  10 px is the radius NOT to compare flags at: a gamma
    within 4e-4 of its threshold"""
    f4 = FLB.uniform_fault4(px)
    run = FLB.oracle_run(po, f4, RL.SEEDS)
    cnt, conf = FLB.counts(f4, RL.SEEDS).sum(0), FLB.confusion(run, f4, RL.SEEDS).sum(0)
    missed, outliers, clean_pass, cont_pass, cont_rej, untriangulated = FLB.UNIFORM_TABLE[px]
    assert (cnt[0], cnt[1], cnt[2]) == (2072, missed, outliers)
    assert (conf[1], conf[3], conf[4]) == (clean_pass, cont_pass, cont_rej), conf
    assert cnt[5] - conf[3] - conf[4] == untriangulated
    assert run["empty"] == 0 and run["pos_err"] < 0.02
    if px == 10:
        assert min(run["gate"]) < 1e-3
    elif px is not None:
        assert min(run["gate"]) > 0.01
