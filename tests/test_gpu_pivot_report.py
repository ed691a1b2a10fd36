"""The non-positive pivot report (STAT_ERR_PIVOT: "reported, run continues") at every factorization of S = T_H P T_H^T + sigma^2 I
on the device: k_update_small (us_chol_tall), the blocked gain at 4, 8 and 12 column blocks and CH_S_A / CH_S_B of the two-level
route (chol_mfma_body's non-Gram modes), k_gain, k_gain_w, and k_chol_inv with S in LDS and in global memory.

The inputs are tests/pivot_lab.py's: a rank-one change of P that makes the joint S firmly indefinite with the first non-positive
pivot in the first row (`first`), in the middle of a 16-block (`mid`: level A on the two-level route) or in the last eight rows
(`tail`: level B), while every per-track gate matrix stays positive definite and the double oracle takes the same decisions
(tests/test_pivot_inputs.py proves all of it on the CPU).  A handle holds six trajectories on the same window and `tall` list --
healthy, `first`, healthy, `mid`, `tail`, healthy --, a control handle of the same shape six healthy ones.  Held per case:
  1. reported: error_flags == 2 exactly on the damaged trajectories, last_stats raises naming the pivot, the counts it still
     returns and last_tracks equal the double oracle's run on P';
  2. not over-reported, isolated: the healthy trajectories have no flag, are within the ordinary bars of update_lab.reference and
     carry the control handle's bits (state, camera states, covariance, correction);
  3. sticky and clearable: a second, healthy update leaves the flag at 2; clear_error_flags reads 0 afterwards;
  4. recovery on the same handle: flags cleared, all six teacher-forced with the healthy window again and updated: all within the
     bars, no flag, and bit-equal to the control handle put through the same rounds -- nothing non-finite is left in Sm, Linv,
     PHt, W, Lam, Dg or the split-K copies for a mask-free step to pick up.
Nothing is asserted about the numbers a damaged trajectory holds after its failed update: the contract leaves them undefined.

The `thin` lists (S of rank 4 behind 6 n - 4 skipped pivots in front of k_update_small) do not carry the damage with c = 2 / g
(two tracks: one gate matrix would lose more than 0.80 of its margin); with c = 1.2 / g they carry it in row 0, and run as
handles of three trajectories -- healthy, damaged, healthy -- held in the same four ways.  One more test holds what the header
says of the gate: a track whose unprojected N_j is indefinite is gate-rejected.  The literal anisotropic route leaves its information matrix where k_gram leaves H_o^T H_o and
runs the same factorizations of S from there on (csrc/kernels_literal.hip): it has no factorization of S of its own; one case
holds that the report survives the route (22 cameras, float, every trajectory anisotropic).

The frame loop (its damage is proven on the CPU like the others, its routes through the same tool): the flag reaches the frame log, the NEES log and k_log_metrics' count from the frame of the failure on, and the
other trajectories of the run keep their bits."""
import contextlib
import os

import numpy as np
import pytest

import helpers as H
import literal_lab as LL
import pivot_lab as PL
import test_gpu_literal_kernels as TL
import update_lab as UL
from msckf_mono_amd import scenario as sc
from test_gpu_update_kernels import VARIANTS, assert_routes, make_handle, meant, routes_exe, state_bits  # noqa: F401  (routes_exe: a fixture)

pytestmark = pytest.mark.gpu

SITES = PL.SITES
CASES = [(site, v, p, n) for site, (_, cases) in SITES.items() for v, p, n in cases]
THIN_CASES = [(v, p, n) for v, p, n in SITES["k_update_small"][1]]       # the `thin` list on the three k_update_small sizes, both dtypes
LAYOUT = (None, "first", None, "mid", "tail", None)
LAYOUT_THIN = (None, "first", None)                                      # the one support a `thin` list can carry (pivot_lab)
FAM = "tall"


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def test_every_case_has_its_inputs_proven_on_the_cpu():
    assert set(n for _, _, _, n in CASES) == set(PL.TALL_SIZES) and all((n, FAM) in PL.WINDOWS for n in PL.TALL_SIZES)
    assert len(CASES) == 34 and PL.STAT_ERR_PIVOT == 2 and set(n for _, _, n in THIN_CASES) == set(PL.THIN_SIZES)
    used = set((n, FAM, w) for _, _, _, n in CASES for w in LAYOUT if w) | set((n, "thin", w) for _, _, n in THIN_CASES for w in LAYOUT_THIN if w)
    assert used | set((PL.LITERAL_SIZE, PL.LITERAL, w) for w in PL.SUPPORTS) == set(PL.CASES)


def _force_healthy(po, bt, n, lst):
    for b in range(bt.B):
        H.copy_oracle_to_device(UL.window(po, n), bt, b)
        bt.set_tracks(b, *UL.tracks_of(po, n, lst))


def _bits(bt):
    return [state_bits(bt, b) + (bt.last_deltax(b),) for b in range(bt.B)]


def _same(x, y):
    return all(np.array_equal(p, q) for p, q in zip(x, y))


def _assert_healthy(po, bt, b, n, prec, what, fam=FAM):
    """no flag, the oracle's counts and per-track results, covariance and correction within the dtype's bars"""
    ref = PL.reference(po, n, fam)
    assert bt.error_flags(b) == 0, (what, b)
    st = bt.last_stats(b)
    for key in H.STAT_KEYS:
        assert st[key] == ref.stats[key], (what, b, key, st, ref.stats)
    M, slots, _ = UL.tracks_of(po, n, PL.list_of(fam))
    ok = (ref.rows[:, 0] > 0) & (ref.rows[:, 1] > 0)
    H.check_tracks(bt.last_tracks(b), ref.rows, ok, prec, None, dict(M=M, slots=slots), UL.window(po, n), (what, b))
    P = bt.covariance(b)
    dc, dd = H.cov_scaled_err(P, ref.P1), UL.dx_scaled(bt.last_deltax(b), ref.dx, ref.P0)
    bar_c, bar_d = LL.bars(prec) if fam == PL.LITERAL else UL.bars(prec)
    assert np.array_equal(P, P.T) and dc <= bar_c and dd <= bar_d, (what, b, dc, dd)
    return dc, dd


def run_case(capi, po, routes_exe, monkeypatch, site, variant, prec, n, fam=FAM):
    layout = LAYOUT_THIN if fam == "thin" else LAYOUT
    B, lst = len(layout), PL.list_of(fam)
    DAMAGED, HEALTHY = [b for b, w in enumerate(layout) if w], [b for b, w in enumerate(layout) if not w]
    if fam == PL.LITERAL:
        # every trajectory anisotropic (v' = 4 u'): the literal route in front of the chain (test_gpu_literal_kernels' `default` handle)
        specs = [(n, FAM, PL.LITERAL_K)] * B
        bt, f_cap, m_cap = TL.make_handle(capi, po, monkeypatch, variant, prec, n, specs)
        ct = TL.make_handle(capi, po, monkeypatch, variant, prec, n, specs)[0]
        got = TL.assert_routes(routes_exe, variant, prec, n, f_cap, m_cap, [n] * B)
    else:
        specs = [(n, lst)] * B
        bt, m_cap = make_handle(capi, po, monkeypatch, variant, prec, n, specs)
        ct, _ = make_handle(capi, po, monkeypatch, variant, prec, n, specs)
        # (`mixed` is meant for a handle whose windows straddle the one-launch update's limit; these all have the handle's size)
        got = assert_routes(routes_exe, variant, prec, B, n, m_cap, [n] * B, skip=("V",) if meant(variant, prec, n, B)["V"].startswith("mixed") else ())
    line, text = SITES[site][0]
    assert text in " " + got[line] + " ", (site, got)
    assert (" small " in " " + got["V"] + " ") == (site == "k_update_small") and (site == "k_update_small" or " chain " in " " + got["V"] + " "), got
    for b in DAMAGED:
        bt.set_covariance(b, PL.damage(po, n, fam, layout[b]).Pd)

    # ---- round 1: the failed update
    bt.marginalize_range(0, B)
    ct.marginalize_range(0, B)
    M, slots, _ = UL.tracks_of(po, n, lst)
    for b in DAMAGED:
        what = (site, variant, prec, n, fam, layout[b])
        assert bt.error_flags(b) == PL.STAT_ERR_PIVOT, (what, bt.error_flags(b))
        with pytest.raises(capi.HipError, match="pivot"):
            bt.last_stats(b)
        got_o = PL.run_damaged(po, n, fam, layout[b])
        if fam == PL.LITERAL:
            info = bt.literal_info(b)
            assert info["route"] == 3 and info["m_rows"] == got_o.stats["m_rows"], (what, info)
        st = bt.last_stats(b, strict=False)
        assert st["error_flags"] == PL.STAT_ERR_PIVOT
        for key in H.STAT_KEYS:
            assert st[key] == got_o.stats[key], (what, key, st, got_o.stats)
        ok = (got_o.rows[:, 0] > 0) & (got_o.rows[:, 1] > 0)
        H.check_tracks(bt.last_tracks(b), got_o.rows, ok, prec, None, dict(M=M, slots=slots), UL.window(po, n), what)
    first, first_c = _bits(bt), _bits(ct)
    # (what a failed trajectory holds is undefined; printed for DESIGN.md section 3.4f, never asserted)
    print("pivot-dev %s %s %s n=%d %s: failed trajectories hold a finite P / dx: %s" % (
        site, variant, prec, n, fam, [(layout[b], bool(np.all(np.isfinite(first[b][2]))), bool(np.all(np.isfinite(first[b][3])))) for b in DAMAGED]))
    for b in HEALTHY:
        dc, dd = _assert_healthy(po, bt, b, n, prec, (site, variant, prec, n, "beside a failure"), fam)
        print("pivot-dev %s %s %s n=%d healthy %d beside a failure: cov %.3e dx %.3e" % (site, variant, prec, n, b, dc, dd))
        assert bt.error_flags(b) == 0 and ct.error_flags(b) == 0
        assert _same(first[b], first_c[b]), (site, variant, prec, n, b, "a healthy trajectory differs from the control handle's")
    assert all(ct.error_flags(b) == 0 for b in range(B))

    # ---- round 2: a healthy update of every trajectory, flags untouched: sticky
    for h in (bt, ct):
        _force_healthy(po, h, n, lst)
        h.marginalize_range(0, B)
    assert [bt.error_flags(b) for b in range(B)] == [PL.STAT_ERR_PIVOT if w else 0 for w in layout], (site, variant, prec, n)
    for b in DAMAGED:
        bt.clear_error_flags(b)
        assert bt.error_flags(b) == 0
        bt.last_stats(b)                                # raises no more

    # ---- round 3: recovery on the same handle, against the oracle and, bit for bit, against the control handle
    for h in (bt, ct):
        _force_healthy(po, h, n, lst)
        h.marginalize_range(0, B)
    third, third_c = _bits(bt), _bits(ct)
    for b in range(B):
        what = (site, variant, prec, n, fam, "recovery", layout[b])
        _assert_healthy(po, bt, b, n, prec, what, fam)
        assert bt.error_flags(b) == 0 and all(np.all(np.isfinite(x)) for x in third[b]), what
        assert _same(third[b], third_c[b]), what
    bt.close()
    ct.close()


@pytest.mark.parametrize("site,variant,prec,n", CASES, ids=["%s-%s-%s-n%d" % c for c in CASES])
def test_pivot_is_reported_isolated_sticky_and_the_handle_recovers(capi, po, routes_exe, monkeypatch, site, variant, prec, n):
    """Measured on an MI355X: DESIGN.md section 3.4f lists the sites at which the flag was seen for `first`, `mid` and `tail`."""
    run_case(capi, po, routes_exe, monkeypatch, site, variant, prec, n)


@pytest.mark.parametrize("variant,prec,n", THIN_CASES, ids=["%s-%s-n%d" % c for c in THIN_CASES])
def test_rank_4_stack_in_front_of_k_update_small(capi, po, routes_exe, monkeypatch, variant, prec, n):
    """The `thin` list: S of rank 4 behind 6 n - 4 skipped pivots.  Three trajectories -- healthy, damaged, healthy; the damage
    has c = 1.2 / g and its first bad pivot in row 0, the one place such a list can carry it within the per-track margin
    (tests/pivot_lab.py)."""
    run_case(capi, po, routes_exe, monkeypatch, "k_update_small", variant, prec, n, fam="thin")


def test_an_indefinite_unprojected_gate_matrix_rejects_the_track_without_a_flag_of_its_own(capi, po, routes_exe, monkeypatch):
    """What include/msckf_hip.h says of the gate: it factors the track's unprojected N_j.  On pivot_lab.GATE_DRAW every projected
    S_j' is positive definite and the double oracle passes all 24 tracks; two N_j' are indefinite (proven on the CPU), and the
    device gate-rejects exactly two tracks, in double, and stacks the other 22.  (The trajectory's flag is up all the same: the
    joint S' is indefinite.)"""
    n, fam, which, sub = PL.GATE_DRAW
    bt, _ = make_handle(capi, po, monkeypatch, "default", "f64", n, [(n, fam)] * 2)
    bt.set_covariance(1, PL.damage(po, n, fam, which, sub).Pd)
    bt.marginalize_range(0, 2)
    st, ref = bt.last_stats(1, strict=False), PL.run_damaged(po, n, fam, which, sub)
    assert ref.stats["n_gate_rejected"] == 0 and ref.stats["n_passed"] == 24
    assert (st["n_gate_rejected"], st["n_passed"], st["n_tri_rejected"], st["n_motion_rejected"]) == (2, 22, 0, 0), st
    assert bt.error_flags(0) == 0 and bt.last_stats(0)["n_passed"] == 24
    bt.close()


def test_the_literal_route_reports_through_the_same_factorizations(capi, po, routes_exe, monkeypatch):
    """Six anisotropic trajectories (v' = 4 u') on the 22-camera window, float: the literal route's Lam^ in front of the chain's
    blocked gain at 12 blocks.  The damage is built on the literal compression's own T (pivot_lab.stack_literal; proven on the CPU
    against the anisotropic double oracle); reported, isolated, sticky, recovered as everywhere else, within literal_lab's bars."""
    run_case(capi, po, routes_exe, monkeypatch, "blocked gain", "default", "f32", PL.LITERAL_SIZE, fam=PL.LITERAL)


# ------------------------------------------------------------------------------------------------ the frame loop
B3, F3, AFTER = PL.FRAME_B, PL.FRAME_F, PL.FRAME_AFTER


@contextlib.contextmanager
def _small_update(value):
    old = os.environ.get("MSCKF_HIP_SMALL_UPDATE")
    if value is not None:
        os.environ["MSCKF_HIP_SMALL_UPDATE"] = value
    elif old is not None:
        del os.environ["MSCKF_HIP_SMALL_UPDATE"]
    try:
        yield
    finally:
        os.environ.pop("MSCKF_HIP_SMALL_UPDATE", None)
        if old is not None:
            os.environ["MSCKF_HIP_SMALL_UPDATE"] = old


@pytest.mark.parametrize("N", sorted(PL.FRAME_SHAPES, reverse=True), ids=["chain-order2-n10", "small-n8"])
def test_the_flag_reaches_the_logs_and_the_neighbours_keep_their_bits(capi, po, routes_exe, N):
    small = PL.FRAME_SHAPES[N]
    trs, K = PL.frame_trajectories(N)
    NF = K + AFTER
    # the full windows of frames K .. NF - 1 reach the factorization the case is written for
    routes = assert_routes(routes_exe, "chain" if small == "0" else "default", "f32", B3, N, N, [N] * B3, f_cap=F3)
    assert (" blocked<4," in routes["K"] and " chain " in routes["V"]) if small == "0" else " small " in routes["V"], routes
    st, dm = PL.frame_damage(po, N)                      # (proven on the CPU: tests/test_pivot_inputs.py)
    u, c = dm.u[:-6].copy(), dm.c                        # the pre-augment window is one camera smaller; u is zero there
    u[:15] = 0.0
    truth = sc.imu_state_gt(trs, 0, NF)

    def run(damage):
        with _small_update(small):
            bt = capi.Batch(B3, N, F3, N, capi.F32)
        for b, tr in enumerate(trs):
            bt.initialize(b, tr.cfg, tr.imu0)
        bt.frame_log_enable(NF)
        bt.truth_set(truth)
        bt.nees_log_enable(NF)
        bt.scenario_alloc(NF, sc.IMU_PER_FRAME)
        for k in range(NF):
            for b, tr in enumerate(trs):
                fr = tr.frames[k]
                bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
        bt.scenario_commit()
        bt.run_frames(0, K); bt.sync()
        assert all(bt.error_flags(b) == 0 for b in range(B3)) and bt.num_cam_states(1) == N - 1
        if damage:
            bt.set_covariance(1, bt.covariance(1) - c * np.outer(u, u))
        bt.run_frames(K, NF); bt.sync()
        out = dict(snap=[H.snapshot(bt, b, strict=False) for b in range(B3)], tracks=[bt.last_tracks(b) for b in range(B3)], log=bt.frame_log_read(),
                   nees=bt.nees_log_read(), flags=[bt.error_flags(b) for b in range(B3)], chol=bt.frame_order_chol_count(),
                   metrics=bt.frame_log_metrics(0, NF, np.zeros((NF, B3, 3))))
        bt.close()
        return out

    got, ctl = run(True), run(False)
    assert ctl["flags"] == [0, 0, 0] and got["flags"] == [0, PL.STAT_ERR_PIVOT, 0]
    for b in (0, 2):
        assert H.same_bits(got["snap"][b], ctl["snap"][b]), b
        assert np.array_equal(got["tracks"][b], ctl["tracks"][b]), b
        assert np.array_equal(got["log"][0][:, b], ctl["log"][0][:, b]), b
        assert np.array_equal(got["nees"][0][:, b], ctl["nees"][0][:, b], equal_nan=True), b
    err = got["log"][1]["error_flags"][:, :, 0]
    assert got["log"][0].shape[0] == NF and not np.any(ctl["log"][1]["error_flags"])
    assert np.array_equal(err[:, 1], np.where(np.arange(NF) >= K, float(PL.STAT_ERR_PIVOT), 0.0)), err[:, 1]
    assert not np.any(err[:, (0, 2)])
    nflag = got["nees"][1]["flags"][:, :, 0].astype(int) & capi.NEES_FLAG_STAT_ERR
    assert np.array_equal(nflag[:, 1] != 0, np.arange(NF) >= K) and not np.any(nflag[:, (0, 2)])
    assert not np.any(ctl["nees"][1]["flags"][:, :, 0].astype(int) & capi.NEES_FLAG_STAT_ERR)
    assert got["metrics"][:, 5].tolist() == [0.0, float(AFTER), 0.0] and ctl["metrics"][:, 5].tolist() == [0.0, 0.0, 0.0]
    # order 2 on every frame of the second call but its first where k_update_small is off, never where it runs
    assert got["chol"] == ctl["chol"] and (got["chol"] >= AFTER - 1 if small == "0" else got["chol"] == 0)
