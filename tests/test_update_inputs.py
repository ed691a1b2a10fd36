"""CPU only: the inputs and the metric of tests/test_gpu_update_kernels.py can see a fault.  Everything here runs on the CPU
oracles (double in LEAN mode = the reference of the GPU suite; float in LEAN and GRAM mode = what a correct float implementation
of either compression looks like; double in GRAM mode = a second valid double algorithm); the mutants are applied to the double
oracle's own RESULT, never to the code under test.

Measured over update_lab.SIZES x FAMILIES (distance from the double LEAN oracle on the entry-scaled metric: covariance,
correction; the float bars are 4 x the float maxima, rounded up: 1.36e-4 and 5.68e-5):
    float LEAN  <= 3.390e-05 (26 cameras, tall)   1.395e-05 (53 cameras, tall)
    float GRAM  <= 3.207e-05 (4 cameras, thin)    1.415e-05 (26 cameras, tall)
    double GRAM <= 8.3e-12 (14 cameras, tall)     1.4e-11 (62 cameras, tall)"""
import numpy as np
import pytest

import helpers as H
import update_lab as UL

ALL_SIZES = tuple(sorted(set(UL.SIZES) | set(UL.GAP_BLOCK_SIZES) | set(UL.GAP_DOWN_SIZES)))


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def test_every_edge_has_a_reason_and_both_neighbours():
    # 64-column panels of ldR at 6 n + 1; 16-column blocks of S at 6 n; k_update_small's limit; CH_SPLIT; N_CAP_MAX
    for a, b in ((10, 11), (21, 22), (31, 32), (42, 43), (53, 54), (13, 14), (26, 27), (32, 33), (12, 13), (14, 15), (62, 63), (3, 4)):
        assert a in UL.E and b in UL.E
    for a, b in ((10, 11), (21, 22), (31, 32), (42, 43), (53, 54)):
        assert (6 * a + 1 + 63) // 64 + 1 == (6 * b + 1 + 63) // 64
    for a, b in ((10, 11), (13, 14), (21, 22), (26, 27), (32, 33)):
        assert (6 * a + 15) // 16 + 1 == (6 * b + 15) // 16
    assert set(n for n in range(UL.N_MIN, UL.N_WIN + 1) if (6 * n) % 16 == 0) == {8, 16, 24, 32, 40, 48, 56} <= set(UL.E)
    assert min(UL.E) == UL.N_MIN and max(UL.E) == UL.N_WIN == 63 and all(len(r) > 10 for r in UL.E.values())
    assert len(UL.SIZES) == 28       # the 27 sizes the suite was specified with, and 12


def test_slots_and_lengths():
    for n in range(UL.N_MIN, UL.N_WIN + 1):
        Ls = UL.tall_lengths(n)
        assert len(Ls) == UL.N_TALL and max(Ls) == min(n, UL.L_MAX) and min(Ls) == 3
        for M in set(Ls) | set(UL.THIN_LENGTHS):
            s = UL.slots_of(n, M)
            assert len(s) == M and s[0] == 0 and s[-1] == n - 1 and np.all(np.diff(s) > 0), (n, M, s)
        if n >= 10:
            assert sum(2 * M - 3 for M in Ls) > 6 * n       # `tall`: more rows than camera columns


def test_the_window_of_n_cameras_is_the_tail_of_the_big_one(po):
    big = UL.window(po, 63)
    P63, c63 = big.getCovariance(), big.getCamStates()[0]
    for n in (3, 33):
        o = UL.window(po, n)
        keep = np.r_[0:15, 15 + 6 * (63 - n):15 + 6 * 63]
        assert np.array_equal(o.getCovariance(), P63[np.ix_(keep, keep)]) and np.array_equal(o.getCamStates()[0], c63[63 - n:])
        f = UL.window(po, n, po.F32, po.GRAM)
        assert f.getNumCamStates() == n and H.cov_scaled_err(f.getCovariance(), o.getCovariance()) < 1e-6


@pytest.mark.parametrize("n", ALL_SIZES)
def test_conditions_and_mutants_hold_with_zero_exclusions(po, n):
    """In both lists of the window: the double, float-LEAN and float-GRAM oracles (and the double GRAM one) agree on every
    track's flags, on n_passed > 0, on every count and on m_rows; r_rows as update_lab.case_violations states it (GRAM counts
    pivots, not rows); no double-oracle gamma within 1 % of its threshold; no float oracle beyond FLOAT_ILL; every mutant at
    10 float bars or more (but MUTANT_EXEMPT, which is asserted to be what it says).  From 5 cameras on every track passes (at 4:
    23 of 24 and both `thin` ones, at 3: 5 and 1; the rest is motion-rejected)."""
    for fam in UL.FAMILIES:
        ref, oth = UL.reference(po, n, fam), UL.others(po, n, fam)
        M = UL.tracks_of(po, n, fam)[0]
        assert UL.case_violations(ref, oth, M) == [], (n, fam)
        assert UL.mutant_violations(ref, n) == [], (n, fam)
        d = {k: UL.distances(r, ref) for k, r in oth.items()}
        print("update-lab n=%d %s passed %d m_rows %d r_rows %d/%d/%d | d32 LEAN %.2e %.2e GRAM %.2e %.2e | d64 %.2e %.2e | mutants %s" % (
            n, fam, ref.stats["n_passed"], ref.stats["m_rows"], ref.stats["r_rows"], oth["f64_gram"].stats["r_rows"], oth["f32_gram"].stats["r_rows"],
            *d["f32_lean"], *d["f32_gram"], *d["f64_gram"], " ".join("%.1e" % UL.mutant_score(ref, m) for m in UL.MUTANTS)))
        assert ref.stats["n_passed"] + ref.stats["n_motion_rejected"] == len(M), (n, fam, ref.stats)     # nothing lost at triangulation or gate
        if n >= 5:
            assert ref.stats["n_passed"] == len(M) and ref.stats["m_rows"] == int(np.sum(2 * M - 3)), (n, fam, ref.stats)
        if fam == "thin" and n >= 4:
            assert ref.stats["m_rows"] == 4 and ref.stats["r_rows"] == 4
        assert max(d["f64_gram"]) <= UL.D64_ROOM, (n, fam, d["f64_gram"])
        for nn, m in UL.MUTANT_EXEMPT:
            if nn == n:
                assert 1e-4 < UL.mutant_score(ref, m) < UL.MUTANT_FACTOR * UL.bars("f32")[0]


def test_float_bars_are_the_measured_ones(po):
    """ONE bar per metric: 4 x the largest distance of the float oracle from the double oracle over SIZES x FAMILIES x {LEAN,
    GRAM}.  The recorded maxima reproduce (to 2 %: another libm may round differently) and no case exceeds the constants the
    bars are built on; the double oracle in GRAM mode, a second valid double algorithm, stays five orders below the double bar."""
    w = np.zeros(2)
    w64 = np.zeros(2)
    for n in UL.SIZES:
        for fam in UL.FAMILIES:
            ref, oth = UL.reference(po, n, fam), UL.others(po, n, fam)
            w = np.maximum(w, np.maximum(UL.distances(oth["f32_lean"], ref), UL.distances(oth["f32_gram"], ref)))
            w64 = np.maximum(w64, UL.distances(oth["f64_gram"], ref))
    print("update-lab float maxima %.3e %.3e double %.2e %.2e" % (w[0], w[1], w64[0], w64[1]))
    assert np.all(w <= [UL.D32_COV, UL.D32_DX]), w
    assert np.allclose(w, UL.D32_MEASURED, rtol=0.02), (w, UL.D32_MEASURED)
    assert np.all(w64 <= UL.D64_ROOM) and UL.D64_ROOM <= 1e-4 * UL.BAR_F64
    assert UL.bars("f32") == (4 * 3.40e-5, 4 * 1.42e-5) and UL.bars("f64") == (1e-6, 1e-6)
    assert UL.FLOAT_ILL < 3 * UL.D32_COV       # what counts as ill-conditioned is within a factor of three of the worst accepted case


def test_the_frobenius_metric_passes_what_the_scaled_metric_rejects(po):
    """The documented gap.  A block of P_after that keeps its prior -- the newest camera's attitude block, the trailing partial
    16-block, theta_I x newest camera -- passes helpers.state_errors at its 1e-3 at 11, 30 and 33 cameras on the `tall` list and
    scores at least 10 float bars (found: >= 2 000) on the scaled metric.  2 % of the downdate missing everywhere passes
    state_errors on the `thin` lists at 4, 5, 30 and 33 cameras and scores at least 10 bars there; on the `tall` lists of this
    lab (24 tracks on a window whose position is well observed) the Frobenius norm does see it, at 1.2e-3 .. 3.9e-3: between
    one and four times its bar, where the scaled metric has it at 26 .. 150 bars."""
    bc = UL.bars("f32")[0]
    for n in UL.GAP_BLOCK_SIZES:
        ref = UL.reference(po, n, "tall")
        for m in ("att_block", "tail_block", "cross_block"):
            f, s = UL.mutant_frobenius(ref, m), UL.mutant_score(ref, m)
            print("update-lab gap n=%d tall %s frobenius %.1e scaled %.1e" % (n, m, f, s))
            assert f < 1e-3 and s >= UL.MUTANT_FACTOR * bc, (n, m, f, s)
    for n in UL.GAP_DOWN_SIZES:
        ref = UL.reference(po, n, "thin")
        f, s = UL.mutant_frobenius(ref, "downdate_2pc"), UL.mutant_score(ref, "downdate_2pc")
        ft, st = UL.mutant_frobenius(UL.reference(po, n, "tall"), "downdate_2pc"), UL.mutant_score(UL.reference(po, n, "tall"), "downdate_2pc")
        print("update-lab gap n=%d downdate_2pc thin frobenius %.1e scaled %.1e | tall frobenius %.1e scaled %.1e" % (n, f, s, ft, st))
        assert f < 1e-3 and s >= UL.MUTANT_FACTOR * bc, (n, f, s)
        assert st >= 2 * UL.MUTANT_FACTOR * bc and ft < 5e-3, (n, ft, st)


def test_metric_sees_one_entry_and_ignores_none():
    P = np.diag([1.0, 1e-6, 1e-2])
    Q = P.copy()
    Q[1, 1] *= 1 + 1e-3
    assert H.cov_scaled_err(Q, P) == pytest.approx(1e-3) and H.rel(Q, P) < 1e-8
    assert UL.dx_scaled(np.array([0.0, 1e-6, 0.0]), np.zeros(3), P) == pytest.approx(1e-3)


def test_empty_and_rejected_lists(po):
    """the row-less trajectories of the GPU suite: the 40 px list passes no track on the oracle at any window size (at most
    lengths the triangulation's cost check rejects it before the gate does) and leaves the covariance untouched"""
    for n in UL.SIZES:
        for dtype in (po.F64, po.F32):
            r = UL.run_oracle(po, n, UL.rejected_tracks(po, n), dtype)
            st = r.stats
            assert st["n_tracks"] == UL.N_TALL and st["n_passed"] == 0 and st["m_rows"] == 0, (n, st)
            assert st["n_motion_rejected"] + st["n_tri_rejected"] + st["n_gate_rejected"] == UL.N_TALL
            assert np.array_equal(r.P0, r.P1)
        if n >= 5:
            assert st["n_motion_rejected"] == 0
    r = UL.run_oracle(po, 63, UL.EMPTY)
    assert np.array_equal(r.P0, r.P1)


@pytest.mark.parametrize("n,sub", UL.HARD_THIN)
def test_hard_thin_lists_are_hard_for_the_float_gram_oracle_only(po, n, sub):
    """the `thin` lists the float GRAM oracle cannot do (why they are not in SUB_SEEDS: it is beyond FLOAT_ILL or finds a fifth
    pivot) are ordinary inputs for the two references the GPU suite rests on: double and float LEAN oracle agree on every flag and
    count, both tracks pass, no gamma within 1 % of its threshold, the float LEAN oracle is within FLOAT_ILL (found: <= 7.6e-6)"""
    fam = "thin:%d" % sub
    M = UL.tracks_of(po, n, fam)[0]
    ref = UL.reference(po, n, fam)
    fl, fg = UL.run_oracle(po, n, UL.tracks_of(po, n, fam), po.F32, po.LEAN), UL.run_oracle(po, n, UL.tracks_of(po, n, fam), po.F32, po.GRAM)
    assert np.array_equal(fl.rows[:, :3] > 0, ref.rows[:, :3] > 0) and fl.stats == ref.stats and ref.stats["n_passed"] == 2 and ref.stats["m_rows"] == 4
    for i in range(2):
        thr = UL.FL.chi2_threshold(int(M[i]))
        assert abs(ref.rows[i, 4] - thr) >= UL.GATE_MARGIN * thr
    assert max(UL.distances(fl, ref)) <= UL.FLOAT_ILL
    assert max(UL.distances(fg, ref)) > UL.FLOAT_ILL or fg.stats["r_rows"] > 4 or UL.run_oracle(po, n, UL.tracks_of(po, n, fam), po.F64, po.GRAM).stats["r_rows"] > 4
