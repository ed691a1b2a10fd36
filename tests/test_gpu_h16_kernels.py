"""The fp16-Jacobian dtype (capi.F16H, MSCKF_HIP_F16H_F32P) against a reference, per track and per update (tests/h16_lab.py: the
given-H twin, the rounding law, the B^ identity, the constants measured on the CPU; tests/test_h16_inputs.py: the proof on the
CPU that each check sees the fault it is meant for).

Per track (feature_lab's 63-camera window and lists, every route launch_feature has for a float handle): the blocks the kernel
STORED, read back through last_track_blocks, obey the rounding law against the twin's unrounded double blocks at the point the
device reports; the stored B^ is the projection of those stored blocks (F32 and F64 handles too: nothing else holds B^); flags,
statistics and gamma are the twin's when it is handed the device's blocks.

Per update (update_lab's windows, test_gpu_update_kernels.py's one-handle-one-launch shape): covariance and correction within
the ordinary FLOAT bars of the given-H twin, and at least three bars away from the unrounded double oracle -- the rounding is
applied on that route and every consumer sees the same blocks."""
import os
import subprocess
import types

import numpy as np
import pytest

import feature_lab as FL
import h16_lab as HL
import helpers as H
import test_gpu_update_kernels as TU
import update_lab as UL

pytestmark = pytest.mark.gpu

# id: (dtype, m_cap, MSCKF_HIP_FEATURE_PAIR, set_compression or None, what launch_feature runs)
ROUTES = {
    "h16-m30-pair3": ("h16", 30, "3", None, "k_feature_pair, one track per wavefront (forced)"),
    "h16-m30-pair2": ("h16", 30, "2", None, "k_feature_pair, two tracks per wavefront (forced)"),
    "h16-m30-pair0": ("h16", 30, "0", None, "k_feature<float, false>"),
    "h16-m62-pair1": ("h16", 62, "1", None, "k_feature_pair for M <= 30, k_feature<float, true> with gate_chol_staged for 31 .. 62"),
    "h16-m63-pair1": ("h16", 63, "1", None, "k_feature_pair for M <= 30, k_feature<float, true> in bins (30, 47] and (47, 63]"),
    "h16-m63-pair0": ("h16", 63, "0", None, "k_feature<float, false> for M <= 30, k_feature<float, true> in bins"),
    "h16-m30-tsqr": ("h16", 30, "1", 0, "set_compression(0): k_feature<float, false>, TSQR; H_x is stored, B^ is not"),
    # the B^ identity (and the unrounded stored blocks) of the plain dtypes, pair and non-pair
    "f32-m63-pair1": ("f32", 63, "1", None, "k_feature_pair and k_feature<float, true>"),
    "f32-m63-pair0": ("f32", 63, "0", None, "k_feature<float, false> and k_feature<float, true>"),
    "f64-m63": ("f64", 63, None, None, "k_feature<double, false> and k_feature<double, true>: the f64 reflectors"),
}
# The stored B^ against the projection of the stored blocks.  The float kernels' comment claims ~1e-10 (normal equations of H_f in
# f64: its squared condition).  Measured on an MI355X for the plain F32 dtype on these lists: see B_F32_MEASURED; all three dtypes
# are held to 10 x that, and never looser than h16_lab.B_IDENTITY_CAP.
B_F32_MEASURED = 9.49e-13        # F32, m_cap 63, pairs on and off alike (F16H 6.4e-13, F64 8.0e-13: the comment's 1e-10 is generous)
B_BAR = min(10.0 * B_F32_MEASURED, HL.B_IDENTITY_CAP)
H_BAR_F64 = 1e-9                 # a double handle's stored blocks against the twin's, relative to the row's largest entry


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def win(po):
    return FL.window(po)


def _dtype(capi, name):
    return {"h16": capi.F16H, "f32": capi.F32, "f64": capi.F64}[name]


def _handle(capi, win, monkeypatch, dtype, m_cap, pair, compress, f_cap, cfg=None):
    if pair is not None:
        monkeypatch.setenv("MSCKF_HIP_FEATURE_PAIR", pair)
    bt = capi.Batch(1, FL.N_WIN, f_cap, m_cap, _dtype(capi, dtype))
    if compress is not None:
        bt.set_compression(compress)
    bt.initialize(0, cfg or win.tr.cfg, win.tr.imu0)
    return bt


def _lists(po, m_cap):
    """per pattern: (tracks of at most m_cap observations, the twin's results for them with its own blocks)"""
    out = {}
    for p in FL.PATTERNS:
        tr, infos = FL.lab(po)[p], HL.lab_blocks(po)[p][0]
        idx = [i for i, t in enumerate(tr) if t.L <= m_cap]
        out[p] = ([tr[i] for i in idx], [infos[i] for i in idx])
    return out


def _check_flags(td, rows, skip, tag):
    """helpers.check_tracks' flag part against the twin's rows; gate_pass / included are not compared where `skip` is set"""
    assert len(td) == len(rows), (tag, len(td), len(rows))
    mo = rows[:, 0] > 0
    assert np.array_equal(td[:, 0] > 0, mo), (tag, "motion_ok", np.nonzero((td[:, 0] > 0) != mo)[0])
    assert np.array_equal((td[:, 1] > 0) & mo, (rows[:, 1] > 0) & mo), (tag, "tri_valid", np.nonzero(((td[:, 1] > 0) != (rows[:, 1] > 0)) & mo)[0])
    want = mo & (rows[:, 1] > 0) & (rows[:, 2] > 0)
    for col, name in ((2, "gate_pass"), (3, "included")):
        diff = ((td[:, col] > 0) != want) & ~skip
        assert not diff.any(), (tag, name, np.nonzero(diff)[0])
    jac = mo & (rows[:, 1] > 0)
    assert not ((td[:, 2] > 0) & ~jac).any() and not ((td[:, 3] > 0) & ~jac).any(), (tag, "gate flag without a Jacobian")


def _per_track(win, bt, dtype, tracks, pre, tag, weights=(1.0, 1.0), b_stored=True, decisions=True):
    """every per-track check of one update of trajectory 0; returns the figures measured"""
    n_cam = FL.N_WIN
    td, blk = bt.last_tracks(0), bt.last_track_blocks(0)
    assert len(td) == len(tracks) == len(blk["first"]), (tag, len(td), len(tracks))
    cams, g = win.o.getCamStates()[0], win.o.getImuState()[16:19]
    wrow = np.array(weights).reshape(1, 2, 1)
    fig = dict(law=0.0, mism=0, entries=0, b=0.0, gamma=0.0, jac=0, skips=0)
    table = []
    for t, (tk, info) in enumerate(zip(tracks, pre)):
        L = tk.L
        table.append(blk["Hx"][t, :L])
        if info["own"] is None or not (td[t, 0] > 0 and td[t, 1] > 0):
            continue                                  # (a disagreement about who has a Jacobian is reported by _check_flags below)
        assert int(blk["first"][t]) == int(tk.slots.min()) and int(blk["last"][t]) == int(tk.slots.max()), (tag, t)
        stored = blk["Hx"][t, :L]
        assert np.all(np.isfinite(stored)) and np.all(np.abs(stored).sum(axis=(1, 2)) > 0), (tag, t, "empty or non-finite stored block")
        x = HL.blocks_of(cams, g, td[t, 5:8], tk.slots)[0] * wrow          # the twin's unrounded whitened blocks at the device's point
        rowmax = np.abs(x).max(axis=-1, keepdims=True)
        if dtype == "h16":
            bad, mism, n = HL.rounding_violations(stored, x)
            assert not bad, (tag, t, L, tk.kind, len(bad), bad[:4])
            fig["mism"] += mism
            fig["entries"] += n
            fig["law"] = max(fig["law"], float(((np.abs(stored - x) - 0.5 * HL.ulp16(x)) / rowmax).max()))
        else:
            e = float((np.abs(stored - x) / rowmax).max())
            fig["law"] = max(fig["law"], e)
            assert e <= (HL.H_SLACK if dtype == "f32" else H_BAR_F64), (tag, t, L, e)
        if b_stored:
            e = HL.b_identity_error(blk["B"][t], stored, blk["rw"][t, :L], tk.slots, n_cam)
            fig["b"] = max(fig["b"], e)
            assert e <= B_BAR, (tag, t, L, tk.kind, e, B_BAR)
    if not decisions:
        return fig
    M, slots, obs = FL.worklist(tracks)
    given = HL.GivenHTwin(win.o, win.tr.cfg).run(M, slots, obs, table=table, update=False, reuse=pre)
    rows, skip = HL.rows_of(given), HL.gate_skips(given)
    _check_flags(td, rows, skip, tag)
    jac = (rows[:, 0] > 0) & (rows[:, 1] > 0)
    fig["jac"], fig["skips"] = int(jac.sum()), int(skip.sum())
    sd, want = bt.last_stats(0), FL.stats_of(rows)
    for key in ("n_tracks", "n_motion_rejected", "n_tri_rejected"):
        assert sd[key] == want[key], (tag, key, sd, want)
    if not skip.any():
        for key in want:
            assert sd[key] == want[key], (tag, key, sd, want)
    e = FL.track_errors(win, td, rows, tracks)
    for t, (rp, dp, grel, _) in e.items():
        assert rp < FL.BAR_REPROJ and dp < FL.BAR_DEPTH, (tag, t, rp, dp)
        fig["gamma"] = max(fig["gamma"], grel)
        assert grel <= HL.GAMMA_BAR, (tag, t, tracks[t].L, grel, HL.GAMMA_BAR)
    return fig


@pytest.mark.parametrize("route", list(ROUTES))
def test_stored_blocks_and_decisions_per_track(capi, po, win, monkeypatch, route, capsys):
    """All lengths 2 .. m_cap in the four slot patterns, one update per pattern.  F16H: the rounding law on the stored blocks, the
    B^ identity (information form), flags, statistics and gamma against the twin handed the device's blocks.  F32 / F64: the
    stored blocks against the twin's at the device's point (float: within h16_lab.H_SLACK of the row's largest entry, the very
    allowance the rounding law makes; double: 1e-9), the B^ identity, and the same decisions.

    Measured on an MI355X (worst over the four patterns; law = (|h - x| - ulp/2) / rowmax for F16H, against a slack of 3.4e-6,
    and |h - x| / rowmax otherwise; mismatch = entries with h != float16(x), cap 2e-3; gamma against a bar of 1.7e-2):
      h16 m_cap 30, pair 3 / 2 / 0 and TSQR alike: law 1.0e-7, mismatch 96 of 79 524 (1.2e-3), B^ 6.4e-13, gamma 4.8e-3
      h16 m_cap 62: law 1.9e-7, mismatch 259 of 271 260; m_cap 63, pairs on / off alike: 267 of 282 600 (9.4e-4), B^ 6.4e-13
      f32 m_cap 63, pairs on / off alike: law 7.2e-7 (the CPU's float32 evaluation: 8.3e-7), B^ 9.5e-13, gamma 4.8e-3
      f64 m_cap 63: law 1.0e-15, B^ 8.0e-13, gamma 1.4e-12
    No track within GATE_MARGIN of its threshold on any route (0 of 765)."""
    dtype, m_cap, pair, compress, _ = ROUTES[route]
    lists = _lists(po, m_cap)
    bt = _handle(capi, win, monkeypatch, dtype, m_cap, pair, compress, max(len(v[0]) for v in lists.values()) + 1)
    seen, tot = set(), dict(law=-1.0, mism=0, entries=0, b=0.0, gamma=0.0, jac=0, skips=0)
    for p in FL.PATTERNS:
        tracks, pre = lists[p]
        H.copy_oracle_to_device(win.o, bt, 0)
        bt.set_tracks(0, *FL.worklist(tracks))
        bt.marginalize_range(0, 1)
        assert bt.error_flags(0) == 0 and all(v == 0 for v in bt.literal_info(0).values()), (route, p)
        fig = _per_track(win, bt, dtype, tracks, pre, (route, p), b_stored=compress != 0)
        seen |= set(t.L for t, i in zip(tracks, pre) if i["own"] is not None)
        for k in ("law", "b", "gamma"):
            tot[k] = max(tot[k], fig[k])
        for k in ("mism", "entries", "jac", "skips"):
            tot[k] += fig[k]
    bt.close()
    with capsys.disabled():
        print("h16-per-track %s law %.3e mismatch %d / %d B^ %.3e gamma %.3e skips %d / %d" % (route, tot["law"], tot["mism"], tot["entries"], tot["b"], tot["gamma"], tot["skips"], tot["jac"]))
    assert seen >= set(range(2, m_cap + 1)), sorted(set(range(2, m_cap + 1)) - seen)
    assert tot["skips"] <= HL.SKIP_CAP * tot["jac"], tot
    if dtype == "h16":
        assert tot["mism"] <= HL.MISMATCH_CAP * tot["entries"], tot


def test_anisotropic_noise_is_pre_whitened_before_the_rounding(capi, po, win, monkeypatch, capsys):
    """u_var' != v_var' on an F16H handle: derive_noise sends it to pre-whitening (the literal route is off for this dtype), so
    the stored rows are the roundings of the 1 / sigma_u, 1 / sigma_v weighted blocks, B^ is the projection of those, and the
    handle took no literal route.  (The weighted entries reach 663: DESIGN.md has the fp16 overflow limit beside the dtype.)
    Measured on an MI355X: law 1.3e-7 of the row's largest entry, 22 of 19 992 entries differ from float16(x), B^ 1.9e-15."""
    cfg = dict(win.tr.cfg)
    cfg["u_var_prime"], cfg["v_var_prime"] = HL.ANISO_VAR[0] * win.tr.cfg["u_var_prime"], HL.ANISO_VAR[1] * win.tr.cfg["u_var_prime"]
    weights = (1.0 / np.sqrt(cfg["u_var_prime"]), 1.0 / np.sqrt(cfg["v_var_prime"]))
    tracks, pre = _lists(po, 30)["spread"]
    bt = _handle(capi, win, monkeypatch, "h16", 30, "1", None, len(tracks) + 1, cfg=cfg)
    H.copy_oracle_to_device(win.o, bt, 0)
    bt.set_tracks(0, *FL.worklist(tracks))
    bt.marginalize_range(0, 1)
    assert bt.error_flags(0) == 0
    assert all(v == 0 for v in bt.literal_info(0).values()), bt.literal_info(0)
    fig = _per_track(win, bt, "h16", tracks, pre, "aniso", weights=weights, decisions=False)
    bt.close()
    with capsys.disabled():
        print("h16-per-track aniso law %.3e mismatch %d / %d B^ %.3e" % (fig["law"], fig["mism"], fig["entries"], fig["b"]))
    assert fig["entries"] > 10000 and fig["mism"] <= HL.MISMATCH_CAP * fig["entries"], fig


# ------------------------------------------------------------------------------------------------ the whole update
UPDATE_CASES = [("default", 10), ("default", 14), ("default", 22), ("default", 33), ("chain", 10), ("chain", 22), ("tsqr", 10), ("tsqr", 33)]
ROUNDING_BARS = 3.0              # the device's update is at least this many float bars from the unrounded double oracle


def _specs(n_cap):
    """test_gpu_update_kernels.specs_of restricted to the windows whose update the rounding moves visibly (h16_lab.h16_window)"""
    return [s for s in TU.specs_of(n_cap) if s[1] in ("empty", "rejected") or HL.h16_window(*s)]


@pytest.fixture(scope="module")
def routes_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("update_routes_h16") / "update_routes_host")
    src = os.path.join(H.ROOT, "tests", "cpp", "update_routes_host.cpp")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", "-o", exe, src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


@pytest.mark.parametrize("variant,n_cap", UPDATE_CASES, ids=["%s-n%d" % c for c in UPDATE_CASES])
def test_update_against_the_given_h_twin(capi, po, routes_exe, monkeypatch, variant, n_cap, capsys):
    """One F16H handle, one marginalize_range; trajectory b holds a window of its own size with the `tall` or `thin` list.  The
    float routes apply (the dtype is a float handle) and are asserted as test_gpu_update_kernels.py asserts them.  Per
    trajectory: the stored blocks are read back and handed to the twin; covariance and correction within update_lab.bars("f32")
    of it; counts and flags equal; P bit-symmetric; no sticky flag; and the distance to the UNROUNDED double oracle is at least
    three bars on covariance or correction.  (`tsqr`: the blocks are read back all the same: k_feature stores H_x on every route.)

    Measured on an MI355X, worst over the case's windows (covariance / correction distance from the given-H twin; bars 1.36e-4 /
    5.7e-5): default n_cap 10: 3.4e-6 / 5.5e-6, 14: 3.6e-6 / 6.3e-6, 22: 5.2e-6 / 7.3e-6, 33: 7.3e-6 / 1.2e-5; chain 10 and 22: as
    default to the digits shown; tsqr 10: 3.0e-6 / 5.3e-6, 33: 1.0e-5 / 1.2e-5.  The window nearest the unrounded oracle (14 cameras,
    `thin`) is 4.4 bars from it on every route."""
    specs = _specs(n_cap)
    B = len(specs)
    as_f32 = types.SimpleNamespace(Batch=capi.Batch, F32=capi.F16H, F64=capi.F64)
    bt, m_cap = TU.make_handle(as_f32, po, monkeypatch, variant, "f32", n_cap, specs)
    TU.assert_routes(routes_exe, variant, "f32", B, n_cap, m_cap, [n for n, _ in specs])
    before = {b: TU.state_bits(bt, b) for b, (n, fam) in enumerate(specs) if fam in ("empty", "rejected")}
    bt.marginalize_range(0, B)
    bar_c, bar_d = UL.bars("f32")
    failures, worst, far = [], [0.0, 0.0], [np.inf, 0.0]
    for b, (n, fam) in enumerate(specs):
        st = bt.last_stats(b)
        assert bt.error_flags(b) == 0, (b, n, fam)
        now = TU.state_bits(bt, b)
        assert np.array_equal(now[2], now[2].T), (b, n, fam)
        if fam in ("empty", "rejected"):
            assert st["n_tracks"] == (0 if fam == "empty" else UL.N_TALL) and st["n_passed"] == 0 and st["m_rows"] == 0, (b, n, fam, st)
            assert all(np.array_equal(x, y) for x, y in zip(now, before[b])), (b, n, fam)
            continue
        M, slots, _ = UL.tracks_of(po, n, fam)
        blk = bt.last_track_blocks(b)
        tw, given = HL.update_given(po, n, fam, [blk["Hx"][t, :int(M[t])] for t in range(len(M))])
        rows, skip = HL.rows_of(given), HL.gate_skips(given)
        assert not skip.any(), (b, n, fam, "a track of the update lists within GATE_MARGIN of its threshold")
        _check_flags(bt.last_tracks(b), rows, skip, (variant, n_cap, n, fam))
        want = FL.stats_of(rows)
        for key in want:
            assert st[key] == want[key], (b, n, fam, key, st, want)
        ref = UL.reference(po, n, fam)
        dx = bt.last_deltax(b)
        dc, dd = H.cov_scaled_err(now[2], tw.P), UL.dx_scaled(dx, tw.last["dx"], ref.P0)
        uc, ud = H.cov_scaled_err(now[2], ref.P1), UL.dx_scaled(dx, ref.dx, ref.P0)
        with capsys.disabled():
            print("h16-update %s n_cap=%d n=%d %s twin: cov %.3e dx %.3e | unrounded oracle: cov %.2f dx %.2f bars" % (variant, n_cap, n, fam, dc, dd, uc / bar_c, ud / bar_d))
        worst[0], worst[1] = max(worst[0], dc), max(worst[1], dd)
        if not (dc <= bar_c and dd <= bar_d):
            failures.append(("twin", b, n, fam, dc, dd))
        if not max(uc / bar_c, ud / bar_d) >= ROUNDING_BARS:
            failures.append(("rounding not visible", b, n, fam, uc / bar_c, ud / bar_d))
    bt.close()
    assert not failures, (variant, n_cap, (bar_c, bar_d), failures)
