"""The numpy twin of the replay's timing model (scenario.replay_image_table / replay_timing_delta / replay_timing_shift /
replay_expand_timed) on replay_lab's sequences, without a device: the table and the preconditions on the lab's sequences, delta = 0
returns the input bits, every rule of the model is visible above the device comparison's bar, and the shifted observation against
the analytic one at the shifted time.

Measured fidelity on the lab's two paths (20 Hz images, noise-free, delta = +-2, +-5, +-10 ms; error |interpolated - exact| in
pixels at f_u = 458.654, over the entries whose exact shift exceeds 0.05 px): printed by test_fidelity_against_the_analytic_
observation (-s) and recorded in DESIGN.md section 4.13."""
import numpy as np
import pytest

import replay_faults_lab as FLB
import replay_lab as RL
import replay_timing_lab as TL
from msckf_mono_amd import scenario as sc

FRAMES = [f for f in range(RL.NF) if len(RL.sequences()[0].frames[f]["M"])]


def test_the_lab_sequences_meet_the_preconditions_and_their_table_is_the_frame_times():
    assert len(FRAMES) >= 12
    for s, tr in enumerate(RL.sequences()):
        time, frame_of, base = TL.table(s)
        assert np.array_equal(frame_of, np.arange(RL.NF)) and np.allclose(time, tr.frame_times, rtol=1e-14, atol=0)
        for f in range(RL.NF):
            fr = tr.frames[f]
            assert base[f] == f + 1 - fr["Nw"]
            o = 0
            for m in (int(x) for x in fr["M"]):
                sl = fr["slots"][o:o + m]
                assert np.all(sl < fr["Nw"]) and np.all(np.diff(sl) > 0) and np.all(np.diff(time[base[f] + sl]) > 0)
                o += m


@pytest.mark.parametrize("record", ([0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.7, 0.0]), ids=["zeros", "y0_only"])
def test_delta_zero_returns_the_input_bits(record):
    """a zero record, and one with y_0 alone: every delta is exactly 0 and the timed twin is the un-timed twin, bit for bit"""
    for f in FRAMES:
        for b in range(RL.B):
            tr = RL.sequences()[RL.SEQ_OF[b]]
            fr = tr.frames[f]
            rd, obs = sc.replay_expand_timed(tr, f, FLB.SEEDS[b], RL.SIGMA, record, table=TL.table(RL.SEQ_OF[b]))
            rd0, obs0 = sc.replay_expand(tr, f, FLB.SEEDS[b], RL.SIGMA)
            assert np.array_equal(rd, rd0) and np.array_equal(obs, obs0), (f, b)
            assert np.array_equal(sc.replay_timing_shift(fr["M"], fr["slots"], fr["obs"], TL.table(RL.SEQ_OF[b])[0], 0, np.zeros(len(fr["obs"]))), fr["obs"])


def test_the_shift_reproduces_a_quadratic_and_leaves_tracks_of_one_alone():
    """three nodes: exact on a quadratic of time, at interior entries and at both ends, for uneven node times; two nodes: exact
    on a line; one: the value itself"""
    time = np.array([0.0, 0.05, 0.11, 0.18, 0.22, 0.31])
    quad = lambda t: np.stack([0.3 - 2.0 * t + 5.0 * t * t, -0.1 + 0.7 * t - 3.0 * t * t], -1)
    line = lambda t: np.stack([0.3 - 2.0 * t, -0.1 + 0.7 * t], -1)
    M, slots = [5, 2, 1], np.array([0, 1, 2, 4, 5, 1, 3, 2])
    delta = np.array([0.004, -0.003, 0.002, 0.006, -0.005, 0.01, -0.02, 0.03])
    t = time[slots]
    obs = np.concatenate([quad(t[:5]), line(t[5:7]), quad(t[7:])])
    got = sc.replay_timing_shift(M, slots, obs, time, 0, delta)
    assert np.allclose(got[:5], quad(t[:5] + delta[:5]), rtol=0, atol=1e-14)
    assert np.allclose(got[5:7], line(t[5:7] + delta[5:7]), rtol=0, atol=1e-14)
    assert np.array_equal(got[7], obs[7])
    # the same cell one image later in the table: base enters only through the times
    assert np.array_equal(sc.replay_timing_shift(M, slots, obs, np.concatenate([[-1.0], time]), 1, delta), got)


def _moved(f, b, **kw):
    """|a variant of the model - the model| over trajectory b's cell of frame f, no noise: the largest coordinate change"""
    s = RL.SEQ_OF[b]
    tr = RL.sequences()[s]
    fr = tr.frames[f]
    time, frame_of, base = TL.table(s)
    rec = np.array(kw.get("record", TL.ALL))
    img = base[f] + fr["slots"]
    want = sc.replay_timing_shift(fr["M"], fr["slots"], fr["obs"], time, base[f], sc.replay_timing_delta(fr["obs"][:, 1], frame_of[img], FLB.SEEDS[b], TL.ALL))
    if "delta" in kw:
        delta = kw["delta"](fr, frame_of[img])
    else:
        delta = sc.replay_timing_delta(fr["obs"][:, 1], frame_of[img + kw.get("base", 0)], FLB.SEEDS[b], rec)
    got = sc.replay_timing_shift(fr["M"], fr["slots"], fr["obs"], time, base[f] + kw.get("base", 0), delta, kw.get("stencil", sc.replay_timing_stencil))
    return float(np.abs(got - want).max())


def _off_by_one(l, M):
    l0, n = sc.replay_timing_stencil(l, M)
    return (l0 + 1 if l0 + 1 <= M - 3 else l0 - 1 if l0 >= 1 else l0, n) if n == 3 else (l0, n)


def test_every_rule_of_the_model_is_visible_above_the_comparison_bar():
    """on every frame of the lab that has a track of three or more (all that have tracks), for a trajectory of either sequence:
    the other sign of t_d, jitter drawn per entry instead of per image, and base(f) off by one image each move some coordinate
    by more than the bar of the device comparison; node l0 off by one does so on every frame that has a track of four or more (a
    track of three has one stencil: there is no other l0 to take)"""
    for b in (0, 1):
        tr = RL.sequences()[RL.SEQ_OF[b]]
        for f in FRAMES:
            assert max(tr.frames[f]["M"]) >= 3
            flipped = TL.ALL * np.array([-1.0, 1.0, 1.0, 1.0])
            assert _moved(f, b, record=flipped) > TL.BAR, ("sign of t_d", f, b)
            per_entry = lambda fr, frames: sc.replay_timing_delta(fr["obs"][:, 1], np.arange(len(fr["obs"])) + 1000, FLB.SEEDS[b], TL.ALL)
            assert _moved(f, b, delta=per_entry) > TL.BAR, ("jitter per entry", f, b)
            assert _moved(f, b, base=1) > TL.BAR, ("base off by one", f, b)
            if max(tr.frames[f]["M"]) >= 4:
                assert _moved(f, b, stencil=_off_by_one) > TL.BAR, ("l0 off by one", f, b)
    assert sum(max(RL.sequences()[0].frames[f]["M"]) >= 4 for f in FRAMES) >= 10


def test_fidelity_against_the_analytic_observation():
    """obs_noise_px = 0, delta in {+-2, +-5, +-10 ms}: at three-node interior entries whose exact shift exceeds 0.05 px,
    |interpolated - exact| < 0.1 |exact - unshifted| (the expected ratio |z'''| dt^2 / (6 |z'|) is about 1e-3 at 20 Hz on these
    paths; a wrong node or sign gives >= 1).  Worst and median error per stencil kind are printed, not asserted; the two-node
    figures come from the same tracks cut to their first two entries."""
    f_u = 458.654
    stats = {0: [], 1: [], 2: []}
    worst_ratio, n_checked = 0.0, 0
    for s, tr in enumerate(RL.sequences()):
        time, _, base = TL.table(s)
        # delta = 0 reproduces the sequence's own observations: the analytic camera is the sequence's
        for f in FRAMES:
            assert np.allclose(TL.exact_obs(tr, f, np.zeros(len(tr.frames[f]["obs"]))), tr.frames[f]["obs"], rtol=0, atol=1e-12)
        for d in (2e-3, -2e-3, 5e-3, -5e-3, 10e-3, -10e-3):
            for f in FRAMES:
                fr = tr.frames[f]
                delta = np.full(len(fr["obs"]), d)
                got = sc.replay_timing_shift(fr["M"], fr["slots"], fr["obs"], time, base[f], delta)
                ex = TL.exact_obs(tr, f, delta)
                err, shift = np.linalg.norm(got - ex, axis=1), np.linalg.norm(ex - fr["obs"], axis=1)
                kind = TL.stencil_kind(fr["M"])
                big = shift * f_u > 0.05
                inner = big & (kind == 0)
                n_checked += int(inner.sum())
                if inner.any():
                    worst_ratio = max(worst_ratio, float((err[inner] / shift[inner]).max()))
                for k in (0, 1):
                    stats[k] += list(err[big & (kind == k)] * f_u)
                # two nodes: every track cut to its first two entries
                off = np.concatenate([[0], np.cumsum(fr["M"])])[:-1]
                two = np.stack([off, off + 1], 1).ravel()
                got2 = sc.replay_timing_shift([2] * len(fr["M"]), fr["slots"][two], fr["obs"][two], time, base[f], delta[two])
                stats[2] += list(np.linalg.norm(got2 - ex[two], axis=1)[big[two]] * f_u)
    for k, name in ((0, "interior"), (1, "track end"), (2, "two-node")):
        print("fidelity, %s: worst %.3g px, median %.3g px over %d entries" % (name, max(stats[k]), float(np.median(stats[k])), len(stats[k])))
    print("worst |interpolated - exact| / |exact - unshifted| at interior entries: %.3g over %d entries" % (worst_ratio, n_checked))
    assert n_checked > 1000
    assert worst_ratio < 0.1, worst_ratio
