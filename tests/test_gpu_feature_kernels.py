"""The feature kernels (k_feature<S, LONG>, k_feature_pair) track by track against the DOUBLE oracle, on every route
launch_feature can take and on both sides of every track-length edge the kernels have (tests/feature_lab.py: the window, the
hand-made tracks, the edges with their reasons; tests/test_feature_inputs.py: the proof on the CPU that these inputs and this
metric see a fault).  The device never fills a window: it is teacher-forced with the oracle's 63-camera window before every
update.  The metric is helpers.check_tracks: every flag of every track at the track's own index, the point and gamma of every
track with a Jacobian; last_stats equal.

Routes (n_cap = 63 throughout; the settings are read when the handle is created, so the environment is set before capi.Batch):
see ROUTES.  A list longer than m_cap is refused by the library before anything is staged ("track longer than m_cap"): M =
m_cap + 1 cannot reach a kernel, and every route with m_cap < 63 asserts the refusal."""
import numpy as np
import pytest

import feature_lab as FL
import helpers as H

pytestmark = pytest.mark.gpu

# id: (precision, m_cap, MSCKF_HIP_FEATURE_PAIR or None, B, f_cap or None = just above the list, what launch_feature runs)
ROUTES = {
    "f32-m30-pair3": ("f32", 30, "3", 1, None, "k_feature_pair, one track per wavefront (forced)"),
    "f32-m30-pair2": ("f32", 30, "2", 1, None, "k_feature_pair, two tracks per wavefront (forced)"),
    "f32-m30-pair0": ("f32", 30, "0", 1, None, "k_feature<float, false>"),
    "f32-m30-pair1-1024": ("f32", 30, "1", 2, 512, "default: nb * f_cap = 1024 <= 1024, the one-track form of k_feature_pair"),
    "f32-m30-pair1-1026": ("f32", 30, "1", 3, 342, "default: nb * f_cap = 1026 > 1024, pairs"),
    "f32-m30-pair1-f513": ("f32", 30, "1", 1, 513, "pairs refused by f_cap > 512: k_feature<float, false>"),
    "f32-m62-pair1": ("f32", 62, "1", 1, None, "k_feature_pair for M <= 30, k_feature<float, true> with gate_chol_staged for 31 .. 62"),
    "f32-m63-pair1": ("f32", 63, "1", 1, None, "k_feature_pair for M <= 30, k_feature<float, true> in bins (30, 47] and (47, 63]"),
    "f32-m40-pair0": ("f32", 40, "0", 1, None, "k_feature<float, false> for M <= 30, ONE k_feature<float, true> launch for 31 .. 40"),
    "f32-m63-pair0": ("f32", 63, "0", 1, None, "k_feature<float, false> for M <= 30, k_feature<float, true> in bins (30, 47] and (47, 63]"),
    "f64-m30": ("f64", 30, None, 1, None, "k_feature<double, false>"),
    "f64-m40": ("f64", 40, None, 1, None, "k_feature<double, false> for M <= 30, ONE k_feature<double, true> launch for 31 .. 40"),
    "f64-m63": ("f64", 63, None, 1, None, "k_feature<double, false>, k_feature<double, true> in bins (30, 47] and (47, 63] (M >= 47: in-place LDS factorization)"),
}


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


def _handle(capi, win, monkeypatch, prec, m_cap, pair, B, f_cap):
    if pair is not None:
        monkeypatch.setenv("MSCKF_HIP_FEATURE_PAIR", pair)
    bt = capi.Batch(B, FL.N_WIN, f_cap, m_cap, capi.F64 if prec == "f64" else capi.F32)
    for b in range(B):
        bt.initialize(b, win.tr.cfg, win.tr.imu0)
    return bt


def _force(win, bt, B):
    for b in range(B):
        H.copy_oracle_to_device(win.o, bt, b)


def _compare(win, bt, b, prec, tracks, ref, tag):
    """trajectory b's last update against the double-oracle rows `ref` of the same list"""
    M, slots, _ = FL.worklist(tracks)
    td, sd = bt.last_tracks(b), bt.last_stats(b)
    want = FL.stats_of(ref)
    for key in want:
        assert sd[key] == want[key], (tag, key, sd, want)
    ok = (ref[:, 0] > 0) & (ref[:, 1] > 0)
    H.check_tracks(td, ref, ok, prec, win.tr, dict(M=M, slots=slots), win.o, tag)


def _sub(po, pattern, keep):
    """(tracks, double-oracle rows) of the lab's list of `pattern` restricted to the tracks keep(t) accepts, order kept (per-track
    results do not depend on the rest of the list: feature_lab)"""
    tr, (rows, _) = FL.lab(po)[pattern], FL.reference(po, pattern)
    idx = [i for i, t in enumerate(tr) if keep(t)]
    return [tr[i] for i in idx], rows[idx]


@pytest.mark.parametrize("route", list(ROUTES))
def test_route_against_double_oracle_per_track(capi, po, win, monkeypatch, route):
    """All lengths 2 .. m_cap in the four slot patterns, both gate decisions on each side of every edge, the Huber, outlier and
    triangulation-rejected cases: one update per pattern (a batch of B > 1 gives every trajectory another pattern each time)."""
    prec, m_cap, pair, B, f_cap, _ = ROUTES[route]
    lists = {p: _sub(po, p, lambda t: t.L <= m_cap) for p in FL.PATTERNS}
    bt = _handle(capi, win, monkeypatch, prec, m_cap, pair, B, f_cap or max(len(v[0]) for v in lists.values()) + 1)
    if m_cap < FL.N_WIN:
        t = FL.make_track(win, lists["spread"][0][0].landmark, np.zeros((FL.N_WIN, 2)), "spread", m_cap + 1, 0.0)
        with pytest.raises(capi.HipError, match="track longer than m_cap"):
            bt.set_tracks(0, *FL.worklist([t]))
    seen = set()
    for r in range(len(FL.PATTERNS)):
        _force(win, bt, B)
        mine = [FL.PATTERNS[(b + r) % len(FL.PATTERNS)] for b in range(B)]
        for b, p in enumerate(mine):
            bt.set_tracks(b, *FL.worklist(lists[p][0]))
        bt.marginalize_range(0, B)
        for b, p in enumerate(mine):
            _compare(win, bt, b, prec, lists[p][0], lists[p][1], (route, p, b))
            seen |= set(t.L for t, row in zip(*lists[p]) if row[0] > 0 and row[1] > 0)
    assert seen >= set(range(2, m_cap + 1)), sorted(set(range(2, m_cap + 1)) - seen)     # (60 .. 63 executed AND compared at m_cap 63)
    bt.close()


# ------------------------------------------------------------------------------------------------ the paired form's structure
def _pool(po, keep):
    tr, rows = [], []
    for p in FL.PATTERNS:
        a, b = _sub(po, p, keep)
        tr += a
        rows.append(b)
    return tr, np.concatenate(rows)


def _single_obs_tracks(win, po, n):
    """n tracks of ONE observation (M < 2: flagged unresidualizable by the kernels, motion-rejected by the oracle)"""
    src = FL.lab(po)["spread"]
    return [src[i].copy(L=1, slots=src[i].slots[:1].copy(), obs=src[i].obs[:1].copy()) for i in range(n)]


def _structure_lists(win, po, case):
    short, rs = _pool(po, lambda t: t.L <= 30)
    if case in ("F1", "F2", "F7", "F64", "F65", "F128", "F129"):     # F7: odd, the middle rank is alone; 64-lane chunks of the histogram
        n = int(case[1:])
        return [(short[:n], rs[:n])]
    if case == "all30":             # no pair fits the LDS together: every wavefront factors its two matrices one after the other
        return [_pool(po, lambda t: t.L == 30)]
    if case == "ties":              # every length equal: the ranking is decided by the stable order alone
        return [_pool(po, lambda t: t.L == 14)]
    if case == "ranks_skip":        # tracks of one observation interleaved: ranks skip entries the histogram never counts
        one = _single_obs_tracks(win, po, 20)
        tr, ref = [], []
        for i in range(41):
            if i % 2 == 0 and i // 2 < 20:
                tr.append(one[i // 2]); ref.append(np.zeros(8))
            tr.append(short[i]); ref.append(rs[i])
        return [(tr, np.array(ref))]
    if case == "B3":                # F = 0, 7 and 129 in ONE launch
        return [(short[:0], rs[:0]), (short[130:137], rs[130:137]), (short[:129], rs[:129])]
    raise ValueError(case)


@pytest.mark.parametrize("case", ["F1", "F2", "F7", "all30", "ties", "F64", "F65", "F128", "F129", "ranks_skip", "B3"])
def test_paired_form_structure(capi, po, win, monkeypatch, case):
    """k_feature_pair with pairs forced (f32, m_cap = 30): how many tracks, which ranks exist, which pairs share the LDS"""
    lists = _structure_lists(win, po, case)
    B = len(lists)
    bt = _handle(capi, win, monkeypatch, "f32", 30, "2", B, max(max(len(t) for t, _ in lists), 1) + 1)
    _force(win, bt, B)
    for b, (tr, _) in enumerate(lists):
        bt.set_tracks(b, *FL.worklist(tr))
    bt.marginalize_range(0, B)
    for b, (tr, ref) in enumerate(lists):
        if len(tr):
            _compare(win, bt, b, "f32", tr, ref, (case, b))
        else:
            assert bt.last_stats(b)["n_tracks"] == 0
    if case == "ranks_skip":        # the oracle agrees that a one-observation track is motion-rejected
        rows, _ = FL.run_oracle(win, po.F64, lists[0][0][:6])
        assert np.array_equal(rows[:, :3], lists[0][1][:6, :3])
    bt.close()


def test_long_and_short_tracks_interleaved_at_m_cap_62(capi, po, win, monkeypatch):
    """the pair launch (M <= 30) and the long launch (31 .. 62, gate_chol_staged) each skip the other's tracks"""
    short, rs = _sub(po, "gapped", lambda t: t.L <= 30)
    long_, rl = _sub(po, "tail", lambda t: 30 < t.L <= 62)
    n = min(len(short), len(long_), 40)
    tr, ref = [], []
    for i in range(n):
        tr += [short[i], long_[i]]
        ref += [rs[i], rl[i]]
    bt = _handle(capi, win, monkeypatch, "f32", 62, "2", 1, 2 * n + 1)
    _force(win, bt, 1)
    bt.set_tracks(0, *FL.worklist(tr))
    bt.marginalize_range(0, 1)
    _compare(win, bt, 0, "f32", tr, np.array(ref), "interleaved")
    bt.close()


# ------------------------------------------------------------------------------------------------ one-track updates
@pytest.mark.parametrize("route", list(ROUTES))
def test_one_track_update_per_edge_length(capi, po, win, monkeypatch, route, capsys):
    """The Jacobian and the null-space projection per length: an update handed ONE track (feature_lab.one_track_cases, a `spread`
    track of 0.5 px per edge length), last_deltax and P_after - P_before against the double oracle's lastDeltaX() and its own
    covariance change, each relative to the reference's norm of that change.  Double: 1e-6.  Float: at most
    ONE_TRACK_FLOAT_FACTOR = 4 x the float ORACLE's distance from the double oracle on the same track (the device's algorithm
    differs -- normal equations of H_f, information form -- and is equally valid; the CPU suite shows that the `drop_last`
    mutant exceeds this bar by at least 10 x at every length, and that the float oracle is within 1e-2 everywhere).

    Measured on an MI355X, per length M: device/float-oracle relative error of deltaX, then of the covariance change (worst of the
    ten float routes, which agree to the digits shown; worst ratio 1.8 on deltaX, 0.6 on the covariance change; double routes
    <= 4.7e-10 on both):
       2: 9.4e-05/1.2e-04 6.0e-05/1.9e-04    3: 5.7e-05/9.7e-05 1.5e-05/5.0e-05    4: 6.2e-05/1.5e-04 1.5e-05/6.7e-05
       5: 5.1e-05/4.8e-05 2.9e-05/1.1e-04    6: 7.7e-05/5.9e-05 1.2e-05/3.1e-05    7: 1.6e-04/1.4e-04 4.6e-05/1.6e-04
      10: 1.5e-04/8.7e-05 1.4e-05/3.2e-05   11: 6.1e-05/7.0e-05 1.9e-05/6.9e-05   14: 1.5e-04/1.3e-04 3.8e-05/2.2e-04
      15: 1.9e-04/1.4e-04 1.2e-04/2.0e-04   16: 1.4e-04/9.5e-05 1.5e-05/7.0e-05   17: 5.7e-05/5.1e-05 2.7e-05/1.5e-04
      18: 4.0e-05/5.4e-05 1.4e-05/5.2e-05   19: 7.1e-05/1.1e-04 1.0e-05/3.1e-05   22: 4.0e-05/9.0e-05 7.9e-06/3.1e-05
      23: 1.8e-04/3.1e-04 1.6e-05/5.6e-05   26: 1.8e-04/3.6e-04 8.8e-06/2.4e-05   27: 1.3e-04/1.5e-04 1.5e-05/9.5e-05
      29: 4.3e-04/5.6e-04 1.4e-05/7.7e-05   30: 6.2e-05/5.9e-05 2.6e-05/2.5e-04   31: 1.9e-04/1.9e-04 2.1e-05/1.4e-04
      32: 8.8e-05/1.3e-04 1.5e-05/8.8e-05   33: 8.1e-05/9.7e-05 1.6e-05/7.4e-05   38: 6.4e-05/2.6e-04 3.8e-05/2.6e-04
      39: 1.2e-04/9.9e-05 3.4e-05/3.3e-04   40: 3.4e-04/3.4e-04 2.3e-05/7.4e-05   46: 7.8e-05/9.6e-05 8.0e-06/4.5e-05
      47: 1.2e-04/6.7e-05 3.2e-05/9.3e-05   48: 1.2e-04/1.2e-04 2.9e-05/2.4e-04   54: 9.3e-05/9.4e-05 1.2e-05/5.5e-05
      55: 1.2e-04/1.2e-04 1.7e-05/1.3e-04   60: 3.1e-04/1.8e-04 8.6e-06/3.7e-05   61: 1.3e-04/2.3e-04 1.1e-05/5.5e-05
      62: 1.6e-04/1.7e-04 1.5e-05/8.3e-05   63: 1.3e-04/2.6e-04 1.1e-05/5.3e-05"""
    prec, m_cap, pair, B, f_cap, _ = ROUTES[route]
    cases = FL.one_track_cases(po)
    r64, r32 = FL.one_track_reference(po, po.F64), FL.one_track_reference(po, po.F32)
    bt = _handle(capi, win, monkeypatch, prec, m_cap, pair, B, f_cap or 2)
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))
    failures = []
    for i, t in enumerate(cases):
        if t.L > m_cap:
            continue
        _force(win, bt, B)
        P0 = bt.covariance(0)
        bt.set_tracks(0, *FL.worklist([t]))
        for b in range(1, B):
            bt.set_tracks(b, *empty)
        bt.marginalize_range(0, B)
        rows, st, dx, dP = r64[i]
        _compare(win, bt, 0, prec, [t], rows, (route, t.L))
        e = FL.update_errors(bt.last_deltax(0), bt.covariance(0) - P0, dx, dP)
        e32 = FL.update_errors(r32[i][2], r32[i][3], dx, dP)
        bar = (1e-6, 1e-6) if prec == "f64" else tuple(FL.ONE_TRACK_FLOAT_FACTOR * x for x in e32)
        with capsys.disabled():
            print("one-track %s L=%d device dx %.3e dP %.3e | float oracle dx %.3e dP %.3e" % (route, t.L, e[0], e[1], e32[0], e32[1]))
        if not (e[0] <= bar[0] and e[1] <= bar[1]):
            failures.append((t.L, e, bar))
    bt.close()
    assert not failures, failures
