"""CPU only: the inputs and the metric of tests/test_gpu_feature_kernels.py can see a fault.  Everything here runs on the two
CPU oracles (double = the reference of the GPU suite, float = what a correct float implementation looks like); the mutants are
applied to the oracle's INPUT, never to the code under test."""
import numpy as np
import pytest

import feature_lab as FL
import helpers as H


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def win(po):
    return FL.window(po)


def _jac(rows):
    return (rows[:, 0] > 0) & (rows[:, 1] > 0)


def test_every_edge_has_a_reason_and_both_neighbours():
    for a, b in ((6, 7), (14, 15), (22, 23), (30, 31), (38, 39), (46, 47), (54, 55), (62, 63), (47, 48), (32, 33), (29, 30), (16, 17), (10, 11), (18, 19), (26, 27)):
        assert a in FL.EDGES and b in FL.EDGES
    assert {2, 3, 4, 60, 61, 62, 63} <= set(FL.EDGES) and all(len(r) > 10 for r in FL.EDGES.values())
    assert FL.chi2_threshold(2) == pytest.approx(0.35184631774927144) and FL.chi2_threshold(63) == pytest.approx(46.594905, rel=1e-6)


def test_slot_patterns(win):
    for p in FL.PATTERNS:
        for L in range(2, FL.pattern_max_len(p) + 1):
            s = FL.pattern_slots(p, L)
            assert len(s) == L and len(set(s.tolist())) == L and s.min() >= 0 and s.max() < FL.N_WIN and np.all(np.diff(s) > 0)
            if p == "gapped":
                assert not set(FL.GAP_SLOTS) & set(s.tolist())
    assert FL.pattern_slots("tail", 5).tolist() == [58, 59, 60, 61, 62] and FL.pattern_slots("head", 3).tolist() == [0, 1, 2]
    assert FL.pattern_slots("spread", 63).tolist() == list(range(63)) and FL.pattern_slots("spread", 2).tolist() == [0, 62]
    for p in FL.PATTERNS:       # shuffled lengths, distinct landmarks: two tracks with swapped outputs cannot pass
        tr = FL.lab(win.po)[p]
        Ls = [t.L for t in tr]
        assert Ls != sorted(Ls) and set(range(2, FL.pattern_max_len(p) + 1)) <= set(Ls)
        lm = np.array([t.landmark for t in tr])
        d = np.linalg.norm(lm[:, None] - lm[None], axis=2) + 10 * np.eye(len(lm))
        assert d.min() > 0.02, d.min()      # 10 x the float bar on the point (2e-3 of a depth of at most ~ 9 m is 1.8e-2)


@pytest.mark.parametrize("pattern", FL.PATTERNS)
def test_lab_conditions_hold_with_zero_exclusions(po, win, pattern):
    """no gamma within 1 % of its threshold, no triangulation cost within 5 % of its limit, every `huber` track has exactly its
    moved observation above the Huber threshold at the oracle's point, every `gross` track is rejected at triangulation and no
    `base` / `huber` track is: on every track of the list, none excluded"""
    tr = FL.lab(po)[pattern]
    rows, st = FL.reference(po, pattern)
    assert FL.lab_violations(win, pattern, tr, rows) == []
    assert st == dict(FL.stats_of(rows), r_rows=st["r_rows"])
    # the triangulation-rejected case on every route's range of lengths: at least three lengths each
    rej = sorted(t.L for i, t in enumerate(tr) if rows[i, 0] > 0 and rows[i, 1] <= 0)
    for lo, hi in ((4, 30), (31, 40), (31, 47), (48, 63), (31, 62)):
        hi = min(hi, FL.pattern_max_len(pattern))
        assert len(set(L for L in rej if lo <= L <= hi)) >= 3, (lo, hi, rej)
    hub = [t.L for i, t in enumerate(tr) if t.kind == "huber" and _jac(rows)[i]]
    moving = set(t.L for i, t in enumerate(tr) if t.kind == "huber" and rows[i, 0] > 0)      # (head: 4 is motion-rejected)
    assert set(hub) == moving >= set(L for L in FL.EDGE_LENGTHS if 6 <= L <= FL.pattern_max_len(pattern))


def test_both_gate_decisions_on_each_side_of_every_edge_and_the_motion_rejects(po):
    dec = {L: set() for L in FL.EDGE_LENGTHS}
    mot = {p: set() for p in FL.PATTERNS}
    for p in FL.PATTERNS:
        rows, _ = FL.reference(po, p)
        for i, t in enumerate(FL.lab(po)[p]):
            if rows[i, 0] <= 0:
                mot[p].add(t.L)
            elif rows[i, 1] > 0 and t.L in dec:
                dec[t.L].add(int(rows[i, 2] > 0))
    assert all(d == {0, 1} for d in dec.values()), dec
    assert 2 in mot["tail"] and {2, 3} <= mot["head"], mot       # the ST_MOTION_OK = 0 cases
    assert not mot["spread"] and not mot["gapped"], mot


@pytest.mark.parametrize("pattern", FL.PATTERNS)
def test_float_oracle_holds_the_bars_of_the_gpu_suite(po, win, pattern):
    """the reference alone must hold them: float oracle against double oracle through helpers.check_tracks itself, and with
    room (measured over the lab: gamma within 3.8e-4 relative, reprojection within 3.7e-5, point within 1.1e-4 of depth)"""
    tr = FL.lab(po)[pattern]
    ref, st = FL.reference(po, pattern)
    r32, st32 = FL.run_oracle(win, po.F32, tr)
    assert st32 == st
    M, slots, _ = FL.worklist(tr)
    dev = r32.copy()
    dev[:, 3] = _jac(r32) & (r32[:, 2] > 0)          # the device's column 3 is `included`
    H.check_tracks(dev, ref, _jac(ref), "f32", win.tr, dict(M=M, slots=slots), win.o, pattern)
    e = FL.track_errors(win, r32, ref, tr)
    a = np.array(list(e.values()))
    g = max(v[3] / FL.gamma_bar(ref[t, 4]) for t, v in e.items())
    assert a[:, 0].max() < 0.5 * FL.BAR_REPROJ and a[:, 1].max() < 0.5 * FL.BAR_DEPTH and g < 0.5, (a.max(0), g)


def test_metric_rejects_two_tracks_with_swapped_outputs(po, win):
    tr = FL.lab(po)["spread"]
    ref, _ = FL.reference(po, "spread")
    M, slots, _ = FL.worklist(tr)
    inc = np.nonzero(_jac(ref) & (ref[:, 2] > 0))[0]
    dev = ref.copy()
    dev[:, 3] = _jac(ref) & (ref[:, 2] > 0)
    for prec in ("f32", "f64"):
        H.check_tracks(dev, ref, _jac(ref), prec, win.tr, dict(M=M, slots=slots), win.o, 0)
        for a, b in ((inc[0], inc[1]), (inc[2], inc[-1])):       # equal flags, outputs swapped
            sw = dev.copy()
            sw[[a, b], 4:8] = dev[[b, a], 4:8]
            with pytest.raises(AssertionError):
                H.check_tracks(sw, ref, _jac(ref), prec, win.tr, dict(M=M, slots=slots), win.o, 0)
    big = np.nonzero(_jac(ref) & (ref[:, 4] > 0.05))[0][0]       # 2e-3 relative on a gamma above 0.05 but below 0.5: the absolute
    sm = dev.copy()                                              # term alone would have let it through
    sm[big, 4] = ref[big, 4] * (1 + 2e-3)
    assert ref[big, 4] < 0.5 or abs(sm[big, 4] - ref[big, 4]) > 1e-3
    with pytest.raises(AssertionError):
        H.check_tracks(sm, ref, _jac(ref), "f32", win.tr, dict(M=M, slots=slots), win.o, 0)
    fl = dev.copy()
    fl[inc[0], 3] = 0
    with pytest.raises(AssertionError):
        H.check_tracks(fl, ref, _jac(ref), "f64", win.tr, dict(M=M, slots=slots), win.o, 0)


@pytest.mark.parametrize("L", FL.EDGE_LENGTHS)
def test_mutants_and_one_track_update_at_every_edge_length(po, win, L):
    """The one-track case of length L passes the gate; the float oracle's update is within ONE_TRACK_ILL of the double oracle's
    (no ill-conditioned input remains); each reference-side mutant moves gamma or the point by at least 10 x the float bars of
    helpers.check_tracks (a changed flag counts); and `drop_last` moves deltaX and the covariance change by at least 10 x the bar
    the device's one-track update is held to (ONE_TRACK_FLOAT_FACTOR x the float oracle's own distance).  `neighbour_slot` does
    not exist at L = 63: every camera of the window is in the track, and a repeated slot is refused by the work-list rules."""
    i = FL.EDGE_LENGTHS.index(L)
    t = FL.one_track_cases(po)[i]
    rows, st, dx, dP = FL.one_track_reference(po, po.F64)[i]
    r32, st32, dx32, dP32 = FL.one_track_reference(po, po.F32)[i]
    assert st["n_passed"] == 1 and st32 == st and len(dx) == 15 + 6 * FL.N_WIN
    e32 = FL.update_errors(dx32, dP32, dx, dP)
    assert max(e32) < FL.ONE_TRACK_ILL, e32
    for m in FL.MUTANTS:
        score, out = FL.mutant_score(win, t, rows, m)
        if score is None:
            assert m == "neighbour_slot" and L == FL.N_WIN
            continue
        assert score >= 10.0, (L, m, score)
        if m == "drop_last" and L > 2:                  # (L = 2: the mutant is motion-rejected, no update at all)
            em = FL.update_errors(out[2], out[3], dx, dP)
            assert em[0] >= 10 * FL.ONE_TRACK_FLOAT_FACTOR * e32[0] and em[1] >= 10 * FL.ONE_TRACK_FLOAT_FACTOR * e32[1], (L, em, e32)


def test_early_accept_line_cases_land_on_both_sides_of_the_line(po, win):
    """feature_lab.line_cases: per length class and landmark one track whose |r_o|^2 / sigma^2 is 0.98 of half its chi-square
    threshold and one at 1.02 (the double twin of tests/h16_lab.py, which the double oracle agrees with on gamma and the
    decision); both have a Jacobian and pass the gate, the second one by the real statistic: gamma <= ub = 0.51 x threshold."""
    import h16_lab as HL
    cases = FL.line_cases(po)
    assert len(cases) == len(FL.LINE_LENGTHS) * FL.LINE_SUBS * len(FL.LINE_TARGETS)
    infos = HL.line_reference(po)
    rows, _ = FL.run_oracle(win, po.F64, cases)
    k = 0
    for L in FL.LINE_LENGTHS:
        for sub in range(FL.LINE_SUBS):
            for tg in FL.LINE_TARGETS:
                t, i = cases[k], infos[k]
                assert t.L == L and t.kind == "line" and i["own"] is not None and i["thresh"] == FL.chi2_threshold(L)
                ratio = i["ub"] / (0.5 * i["thresh"])
                assert abs(ratio - tg) <= FL.LINE_TOL, (L, sub, tg, ratio)
                assert list(rows[k, :3]) == [1, 1, 1] and abs(rows[k, 4] - i["gamma"]) <= 1e-9 * i["gamma"], (L, sub, tg, rows[k], i["gamma"])
                assert i["gamma"] < 0.52 * i["thresh"]
                k += 1
