"""msckf_hip_set_gate_early_accept against a reference, on each of its three implementations (the TSQR branch of k_feature, which
sums (Q_f^T r)[3:]; the information-form branch, |r|^2 - |c|^2; k_feature_pair's normal equations), in float and double, on short
and long tracks and on both sides of the 0.5 x threshold rule.

Window and lists are feature_lab's (the four patterns, every length up to m_cap), each list followed by the line cases
(feature_lab.line_cases: ub / (0.5 x threshold) = 0.98 and 1.02 per length class).  Expected values: flags, gamma and point from the
double oracle, ub = |r_o|^2 / sigma^2 from the double twin of tests/h16_lab.py (which equals the oracle: tests/test_h16_inputs.py).
Per track with a Jacobian: no decision changes (helpers.check_tracks' whole flag part); where ub < 0.5 thresh (1 - m) the reported
gamma IS ub, where ub > 0.5 thresh (1 + m) it is the real statistic, each to check_tracks' gamma tolerance of the precision, m =
1e-3 in float and 1e-6 in double; inside the band either.  Every route sees an early-accepted track, one passed by the real
statistic and a rejected one (asserted).  And the same handle geometry with the option off leaves the same bits: state, camera
states, covariance, correction."""
import numpy as np
import pytest

import feature_lab as FL
import h16_lab as HL
import helpers as H

pytestmark = pytest.mark.gpu

# id: (precision, m_cap, MSCKF_HIP_FEATURE_PAIR or None, set_compression or None)
ROUTES = {
    "f32-m30-pair2": ("f32", 30, "2", None),          # k_feature_pair's normal_eq
    "f32-m30-pair0": ("f32", 30, "0", None),          # k_feature<float, false>: rn - |c|^2 from the f64 cq
    "f32-m62-pair1": ("f32", 62, "1", None),          # pair + the staged long kernel
    "f64-m30": ("f64", 30, None, None),
    "f64-m63": ("f64", 63, None, None),
    "f32-m30-tsqr": ("f32", 30, "1", 0),              # the TSQR branch: sum of qr[] over rows >= 3
    "f64-m30-tsqr": ("f64", 30, None, 0),
}
BAND = {"f32": 1e-3, "f64": 1e-6}


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


def _handle(capi, win, monkeypatch, prec, m_cap, pair, compress, f_cap, early):
    if pair is not None:
        monkeypatch.setenv("MSCKF_HIP_FEATURE_PAIR", pair)
    bt = capi.Batch(1, FL.N_WIN, f_cap, m_cap, capi.F64 if prec == "f64" else capi.F32)
    if compress is not None:
        bt.set_compression(compress)
    bt.set_gate_early_accept(early)
    bt.initialize(0, win.tr.cfg, win.tr.imu0)
    return bt


def _lists(po, win, m_cap):
    """per pattern: (tracks, double-oracle rows, ub, thresh) of the lab's list up to m_cap followed by the line cases up to m_cap"""
    line = FL.line_cases(po, m_cap)
    n_all = len(FL.line_cases(po))
    assert [t.L for t in FL.line_cases(po)[:len(line)]] == [t.L for t in line] and len(line) <= n_all      # (the shorter classes come first)
    line_rows = FL.run_oracle(win, po.F64, line)[0]
    line_infos = HL.line_reference(po)[:len(line)]
    out = {}
    for p in FL.PATTERNS:
        tr, infos, rows = FL.lab(po)[p], HL.lab_blocks(po)[p][0], FL.reference(po, p)[0]
        idx = [i for i, t in enumerate(tr) if t.L <= m_cap]
        both = [infos[i] for i in idx] + list(line_infos)
        out[p] = ([tr[i] for i in idx] + line, np.concatenate([rows[idx], line_rows]),
                  np.array([i["ub"] for i in both]), np.array([i["thresh"] for i in both]))
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_early_accept_reports_the_bound_below_the_line_and_the_statistic_above(capi, po, win, monkeypatch, route, capsys):
    prec, m_cap, pair, compress = ROUTES[route]
    lists = _lists(po, win, m_cap)
    f_cap = max(len(v[0]) for v in lists.values()) + 1
    on = _handle(capi, win, monkeypatch, prec, m_cap, pair, compress, f_cap, 1)
    off = _handle(capi, win, monkeypatch, prec, m_cap, pair, compress, f_cap, 0)
    m = BAND[prec]
    n_early = n_real = n_rej = n_band = n_line = 0
    for p in FL.PATTERNS:
        tracks, ref, ub, thr = lists[p]
        wl = FL.worklist(tracks)
        for bt in (on, off):
            H.copy_oracle_to_device(win.o, bt, 0)
            bt.set_tracks(0, *wl)
            bt.marginalize_range(0, 1)
            assert bt.error_flags(0) == 0
        jac = (ref[:, 0] > 0) & (ref[:, 1] > 0)
        below, above = jac & (ub < 0.5 * thr * (1 - m)), jac & (ub > 0.5 * thr * (1 + m))
        assert not (below & ~(ref[:, 2] > 0)).any()               # gamma <= ub: a track below the line passes the real gate too
        want = ref.copy()
        want[below, 4] = ub[below]
        td = on.last_tracks(0)
        sd, ws = on.last_stats(0), FL.stats_of(ref)
        for key in ws:
            assert sd[key] == ws[key], (route, p, key, sd, ws)
        H.check_tracks(td, want, below | above, prec, win.tr, dict(M=wl[0], slots=wl[1]), win.o, (route, p))
        H.check_tracks(off.last_tracks(0), ref, jac, prec, win.tr, dict(M=wl[0], slots=wl[1]), win.o, (route, p, "off"))
        for t in np.nonzero(jac & ~below & ~above)[0]:            # inside the band: the bound or the statistic
            tol = (1e-3 if prec == "f32" else 1e-6) * max(ub[t], 1e-9)
            assert min(abs(td[t, 4] - ub[t]), abs(td[t, 4] - ref[t, 4])) <= tol, (route, p, t, td[t, 4], ub[t], ref[t, 4])
        is_line = np.array([t.kind == "line" for t in tracks])
        assert (is_line & jac).sum() == is_line.sum() and not (is_line & ~(below | above)).any()
        # the bound and the statistic are told apart on every line case: they differ by 2 % and more, ten float tolerances
        assert np.all(ref[is_line, 4] < 0.99 * ub[is_line])
        n_line += int(is_line.sum())
        n_early += int(below.sum())
        n_real += int((above & (ref[:, 2] > 0)).sum())
        n_rej += int((above & ~(ref[:, 2] > 0)).sum())
        n_band += int((jac & ~below & ~above).sum())
        a, b = _bits(on), _bits(off)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (route, p, [i for i, (x, y) in enumerate(zip(a, b)) if not np.array_equal(x, y)])
    on.close()
    off.close()
    with capsys.disabled():
        print("gate-early %s: early %d, passed by the statistic %d, rejected %d, in the band %d, line cases %d" % (route, n_early, n_real, n_rej, n_band, n_line))
    assert n_early > 0 and n_real > 0 and n_rej > 0, (route, n_early, n_real, n_rej)


def _bits(bt):
    return bt.imu_state(0), bt.cam_states(0)[0], bt.covariance(0), bt.last_deltax(0)
