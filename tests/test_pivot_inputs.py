"""CPU only: the damaged covariances of tests/pivot_lab.py are what tests/test_gpu_pivot_report.py takes them for.  For every
(window, support) the GPU file uses, none left out: u solves T u = w to 1e-12; the unpivoted Cholesky of S' in double meets its
first non-positive pivot at row a exactly, at least 2^10 float epsilons of the largest diagonal entry below zero; every passing
track's own gate matrix keeps a quarter of its margin (c g_j <= 0.75), and so does the unprojected 2 M x 2 M matrix the device's
gate factors in its place; the double oracle run from P' takes the same per-track
decisions and returns the same counts as from P, with no gamma within update_lab.GATE_MARGIN of its threshold.

Also here: the `thin` cases (c = 1.2 / g, row 0) and why c = 2 / g cannot serve them; which `tail` cases fail inside the last
pivot-bearing 16-block, per site; the draw that separates the device's gate from the reference's; the frame-loop damage.

Measured over pivot_lab.CASES (printed per case by the first test):
    worst c g_j                  0.734 (5 cameras, thin); of the unprojected N_j 0.748 (5 cameras, thin); `tall`: 0.714 / 0.731
    weakest bad pivot            -5.7e-3 of max diag S' (23 cameras, tail): 46 x the margin of 1.2e-4
    lambda_min / lambda_max S'   -0.036 (33 cameras, mid) .. -0.276 (5 cameras, first)"""
import numpy as np
import pytest

import pivot_lab as PL

CASES = PL.CASES


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.mark.parametrize("n,fam,which", CASES, ids=["n%d-%s-%s" % c for c in CASES])
def test_damage_holds_with_zero_exclusions(po, n, fam, which):
    st, dm, f = PL.stack(po, n, fam), PL.damage(po, n, fam, which), PL.figures(po, n, fam, which)
    print("pivot-lab n=%d %s %s r=%d [%d,%d) device rows %d..%d sub %d | resid %.1e | first bad pivot %d: %.2e of max diag | c g_j %.3f, unprojected %.3f | lambda %.3f | min diag P' %.1e" % (
        n, fam, which, st.r, dm.a, dm.b, st.lead[dm.a], st.lead[dm.b - 1], PL.SUB_SEEDS.get((n, fam, which), 0), f["resid"], f["row"], f["pivot_rel"], f["cg"], f["cn"], f["lam"], f["diag_min"]))
    assert PL.gram_error(st) <= PL.GRAM_TOL
    assert f["resid"] < PL.LSTSQ_TOL
    assert f["clean"] == -1                                         # the healthy S has no bad pivot
    assert f["row"] == dm.a
    assert f["pivot_rel"] <= -PL.PIVOT_MARGIN == -(2.0 ** -13)
    assert f["cg"] <= PL.TRACK_MARGIN == 0.75
    assert f["cg"] <= f["cn"] * (1 + 1e-9) and f["cn"] <= PL.TRACK_MARGIN      # the unprojected N_j the device's gate factors
    assert f["lam"] < -0.03                                         # firmly indefinite, not at the rounding level
    assert dm.c * dm.g == pytest.approx(1.2 if fam == "thin" else 2.0)   # c = 2 / g but on the `thin` lists
    assert np.allclose(dm.Sd, st.T @ dm.Pd @ st.T.T + st.sig2 * np.eye(st.r), rtol=0, atol=1e-9 * np.abs(dm.Sd).max())
    assert np.array_equal(dm.Sd[:dm.a, :dm.a], st.S[:dm.a, :dm.a])  # the leading minor is the healthy one
    assert PL.violations(po, n, fam, which) == []                   # all of the above, and the double oracle run on P' against the reference
    ref, got = PL.reference(po, n, fam), PL.run_damaged(po, n, fam, which)
    assert got.stats["n_passed"] == ref.stats["n_passed"] > 0 and got.stats["m_rows"] == ref.stats["m_rows"]


def test_supports_sit_where_the_device_cases_need_them(po):
    for n, fam in PL.WINDOWS:
        st = PL.stack(po, n, fam)
        assert st.r >= 23 and np.all(np.diff(st.lead) > 0)
        # the seven unobservable directions of the window close the staircase: the device's trailing rows are skipped pivots
        assert 6 * n - st.r >= 7 and np.array_equal(np.arange(6 * n - 7, 6 * n), np.setdiff1d(np.arange(6 * n), st.lead)[-7:])
        a0, b0 = PL.support_of(st.r, "first", n > 32)
        am, bm = PL.support_of(st.r, "mid", n > 32)
        at, bt = PL.support_of(st.r, "tail", n > 32)
        assert (a0, b0) == (0, 1) and bt == st.r and bt - at == 8 and bm - am == 8 and 0 < am and bm <= at + 4
        dev = st.lead[am]
        assert dev % 16 != 0                                        # not at the head of a 16-block, in the device's rows too
        if st.r >= 41:
            assert am % 16 != 0 and 16 <= am <= st.r - 24 and dev >= 16
        else:
            assert n == 5
        # `tail` ends in the last 16-block of the device's S that holds a pivot at all; its first bad pivot (row a) sits in that
        # block at the sizes of TAIL_IN_LAST_BLOCK and in the block before it at the others
        assert st.lead[bt - 1] // 16 == st.lead[-1] // 16
        assert st.lead[-1] // 16 - st.lead[at] // 16 == (0 if n in PL.TAIL_IN_LAST_BLOCK else 1), (n, st.lead[at], st.lead[-1])
        if n > 32:
            assert st.lead[bm - 1] < PL.CH_SPLIT                    # level A, the whole support
        if n in PL.LEVEL_B_SIZES:
            assert st.r > PL.CH_SPLIT and st.lead[at] >= PL.CH_SPLIT
        elif n > 32:
            assert n == 33 and st.r == 191                          # every row is level A there
    assert set(PL.LEVEL_B_SIZES) <= set(PL.TALL_SIZES)
    # every site that factors S in 16-blocks has a case whose `tail` fails inside the last pivot-bearing block, and the two-level
    # route one at each level count it can (33: level A alone; 63: level B)
    for site, (_, cases) in PL.SITES.items():
        sizes = set(n for _, _, n in cases)
        assert sizes <= set(PL.TALL_SIZES)
        if site != "k_update_small":
            assert sizes & set(PL.TAIL_IN_LAST_BLOCK), site
    assert {33, 63} <= set(n for _, _, n in PL.SITES["two-level"][1]) & set(PL.TAIL_IN_LAST_BLOCK)


def test_sub_seeds_are_the_first_that_hold(po):
    """a recorded sub-seed is the smallest whose case holds what needs no oracle run (row, margins); `first` is never re-seeded"""
    for (n, fam, which), sub in PL.SUB_SEEDS.items():
        assert (n, fam, which) in PL.CASES and (which != "first" or fam == "thin") and sub > 0
        for s in range(sub):
            assert PL.violations(po, n, fam, which, s) != [], (n, fam, which, s)


def test_thin_lists_carry_the_damage_in_row_0_with_a_smaller_c(po):
    """With the recipe's c = 2 / g the two tracks' quantities sum to at least 2 / lambda_max whatever w (5 cameras: 1.617, 10:
    1.598, 12: 1.697), so the larger exceeds 0.80: the `thin` cases use c = 1.2 / g (S' is indefinite for every c > 1 / g) on the
    support [0, 4), and hold everything the other cases hold (test_damage_holds_with_zero_exclusions).  A first bad pivot in row 1,
    2 or 3 was not found within the margin: 3000 draws each at c g = 1.2, 1.1 and 1.05 leave the quantity of the unprojected
    N_j at 0.96 or more."""
    for n in PL.THIN_SIZES:
        st = PL.stack(po, n, "thin")
        assert len(st.rows) == 2 and st.r == 4 and list(st.lead[:3]) == [0, 1, 2] and st.lead[3] >= 12
        floor = PL.thin_floor(st)
        print("pivot-lab thin n=%d: with c = 2 / g, c (g_1 + g_2) >= %.3f" % (n, floor))
        assert floor / 2 > PL.TRACK_MARGIN + 0.04
        for sub in range(4):
            dm = PL.damage_of(st, 0, 4, PL.seed_of(n, "thin", "first", sub))
            assert PL.track_quantity(st, dm) >= floor / 2 * (1 - 1e-9)
        assert (n, "thin", "first") in PL.CASES and PL.C_FACTOR["thin"] == 1.2
        for a in (1, 2, 3):                     # (a sample of the search the docstring records)
            for sub in range(40):
                dm = PL.damage_of(st, a, 4, PL.seed_of(n, "thin", "first", sub) + 7 * a, 1.2)
                assert PL.first_bad_pivot(dm.Sd)[0] != a or PL.track_quantity_unprojected(st, dm) > PL.TRACK_MARGIN


def test_the_gate_draw_has_two_indefinite_unprojected_gate_matrices(po):
    """pivot_lab.GATE_DRAW (10 cameras, `mid`, sub-seed 12) holds everything but the unprojected margin: every projected S_j' is
    positive definite with c g_j = 0.34 and the double oracle passes all 24 tracks, while two tracks' unprojected N_j' are
    indefinite (the quantity reaches 1.45) -- the two tracks the device's gate rejects (tests/test_gpu_pivot_report.py)."""
    n, fam, which, sub = PL.GATE_DRAW
    st, dm = PL.stack(po, n, fam), PL.damage(po, n, fam, which, sub)
    assert PL.violations(po, n, fam, which, sub) == [("track margin, unprojected", pytest.approx(1.446, abs=1e-3))]
    assert PL.indefinite_tracks(st, dm) == (0, 2) and PL.track_quantity(st, dm) <= 0.35
    got = PL.run_damaged(po, n, fam, which, sub)
    assert got.stats["n_passed"] == 24 and got.stats["n_gate_rejected"] == 0
    assert sub < PL.SUB_SEEDS[(n, fam, which)]


@pytest.mark.parametrize("N", sorted(PL.FRAME_SHAPES))
def test_frame_loop_damage_holds(po, N):
    """the damage of the frame-loop test, built on the double oracle driven to frame K's augment: row, margins, and u zero on the
    IMU's columns and on the newest camera's (no track sees it), so that the pre-augment window takes u without its last six"""
    st, dm = PL.frame_damage(po, N)
    assert PL.frame_violations(po, N) == [] and PL.gram_error(st) <= PL.GRAM_TOL and st.r >= 16
    assert all(PL.frame_violations(po, N, s) != [] for s in range(PL.FRAME_SUB_SEEDS[N]))
    assert max(np.abs(dm.u[:15]).max(), np.abs(dm.u[-6:]).max()) <= 1e-12 * np.abs(dm.u).max()
    assert not np.any(st.T[:, :15]) and not np.any(st.T[:, -6:]) and len(dm.u) == 15 + 6 * N
    ev = np.linalg.eigvalsh(dm.Sd)
    print("pivot-lab frame loop N=%d r=%d [%d,%d) sub %d c g_j %.3f unprojected %.3f lambda %.3f" % (
        N, st.r, dm.a, dm.b, PL.FRAME_SUB_SEEDS[N], PL.track_quantity(st, dm), PL.track_quantity_unprojected(st, dm), ev[0] / ev[-1]))
    assert ev[0] / ev[-1] < -0.03


def test_first_bad_pivot_and_staircase_on_known_matrices():
    A = np.diag([4.0, 1.0, 9.0])
    assert PL.first_bad_pivot(A) == (-1, 1.0)
    A[1, 1] = -1.0
    assert PL.first_bad_pivot(A) == (1, -1.0)
    A = np.array([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0], [0.0, 0.0, 1.0]])        # second pivot exactly zero
    assert PL.first_bad_pivot(A) == (1, 0.0)
    H = np.array([[1.0, 2.0, 0.0, 1.0], [0.0, 0.0, 3.0, 1.0], [1.0, 2.0, 3.0, 2.5]])      # column 1 = 2 x column 0
    T, lead = PL.staircase(H)
    assert list(lead) == [0, 2, 3] and np.allclose(T.T @ T, H.T @ H, atol=1e-14) and T[1, 0] == T[1, 1] == 0.0
