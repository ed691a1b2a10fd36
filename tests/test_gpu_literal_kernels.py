"""The literal anisotropic route on the device -- k_lit_pre, k_lit_gamma, k_lit_phase<S, 0..3> (kernels_literal.hip over
literal_core.h) and k_literal_dense -- against the DOUBLE oracle on the entry-scaled metric, at windows on both sides of every
size edge the route has, with v' = 4 u' (tests/literal_lab.py: the windows, lists, edges and bars; tests/test_literal_inputs.py:
the proof on the CPU that these inputs and this metric see a fault -- a device that computed the pre-whitened update instead is
29 bars and more away from 10 cameras on -- and the host build of literal_core.h against the oracle on every case).

A case is ONE handle of one n_cap and dtype and ONE marginalize_range over all of it: trajectory b holds a window of its own size
with one of the lab's lists, teacher-forced from the oracle's window; every handle also carries an empty work-list, a list none
of whose tracks passes, and ONE ISOTROPIC trajectory (u' = v', PRM_LIT == 0) in the same launch, which the literal kernels must
leave to k_gram's Lam^.  Per trajectory: last_stats' counts and every track's flags equal the double oracle's, covariance and
correction within the dtype's bar (double 1e-6; float 4 x the float oracle's own worst distance, measured on the CPU), no sticky
error flag, P bit-symmetric, literal_info: route, stacked rows and kept rows equal the oracle's (the float oracle keeps the same
rows as the double one on every case of the lab: no slack in float either), six or more kept handed-through rows on the lists with
an unobserved camera slot; the row-less trajectories keep state and covariance to the bit; the isotropic one meets
update_lab.bars against its own oracle.

Each case first asserts, through tests/cpp/update_routes_host.cpp --handle-lit, the launches the chain takes (no k_update_small,
the information form) and, from the device's own counts through literal_lab.staging, that the handle's largest window is on the
side of every staging edge it was written for (meant_sides below, written down by hand): a moved LIT_LDS_DOUBLES cannot silently
empty a case.

Out of this suite: the fp16-Jacobian dtype and the early-accept bound."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import literal_lab as LL
import test_gpu_update_kernels as TU
import update_lab as UL

pytestmark = pytest.mark.gpu

N_CAPS = (5, 10, 11, 16, 21, 22, 31, 32, 33, 34, 38, 39, 41, 42, 43, 53, 54, 60, 61, 62, 63)
BOTH = ("f32", "f64")
# name: environment at create time, aniso_mode, K, dtypes, n_caps, the lists per window
VARIANTS = {
    "default": dict(env={}, mode=0, K=LL.K_MAIN, precs=BOTH, n_caps=N_CAPS),
    "wide": dict(env={}, mode=0, K=LL.K_MAIN, precs=BOTH, n_caps=LL.WIDE_SIZES),
    "long": dict(env={}, mode=0, K=LL.K_MAIN, precs=BOTH, n_caps=(33, 63)),
    "inverse": dict(env={}, mode=0, K=LL.K_INV, precs=("f64",), n_caps=LL.K_INV_SIZES),
    "dense": dict(env={"MSCKF_HIP_LITERAL_ROUTE": "1"}, mode=0, K=LL.K_MAIN, precs=("f64",), n_caps=(5, 10, 16)),
    "serial": dict(env={"MSCKF_HIP_LITERAL_SERIAL": "1"}, mode=0, K=LL.K_MAIN, precs=("f64",), n_caps=(10, 22)),
    "whitened": dict(env={}, mode=1, K=LL.K_MAIN, precs=BOTH, n_caps=LL.WHITENED_SIZES),
}
CASES = [(v, p, n) for v, s in VARIANTS.items() for p in s["precs"] for n in s["n_caps"] if not (v == "long" and (p, n) == ("f64", 33))]
ENV_NAMES = TU.ENV_NAMES + ("MSCKF_HIP_LITERAL_ROUTE", "MSCKF_HIP_LITERAL_SERIAL")


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


routes_exe = TU.routes_exe


# ------------------------------------------------------------------------------------------------ what each handle was written for
def meant_sides(n, fam):
    """the sides of literal_lab.staging a window of n cameras with the list `fam` was written for -- by hand, from the edge table of
    DESIGN.md section 3.4d, NOT computed from literal_core.h"""
    m = dict(two_level=n >= 32, rows_tiles=n <= 41, stage_lds=n <= 60)
    if fam in ("tall", "gap6", "long") or fam.startswith("wide"):
        m.update(gram=n >= 5, sweep_pb=(16 if n <= 38 else 8) if n >= 5 else None)
    if fam == "tall":
        m.update(basis_tiles=n <= 31, elim_pb=16 if n <= 61 else 8)
    if fam == "gap6":
        m.update(basis_tiles=True, tiles_list=False)
    if fam in ("brim44", "brim45"):
        m.update(gram=False, sweep_pb=None)
    if fam == "brim46":
        m.update(gram=True, sweep_pb=16)
    return m


def specs_of(variant, n_cap):
    """(window size, list, K) per trajectory; K None: the isotropic trajectory"""
    K = VARIANTS[variant]["K"]
    if variant == "wide":
        s = [(n_cap, "wide%d" % c, K) for c in LL.wide_counts(n_cap)]
    elif variant == "long":
        s = [(n, "long", K) for n in sorted(LL.LONG_LENGTHS) if n <= n_cap] + [(n_cap, "tall", K)]
    elif variant == "inverse":
        s = [(n, fam, K) for n in LL.K_INV_SIZES if n <= n_cap for fam in ("tall", "thin", "gap_deep")]
    elif variant == "whitened":
        s = [(n, fam, K) for n in LL.WHITENED_SIZES if n <= n_cap for fam in ("tall", "thin")]
    else:
        s = []
        for n in (x for x in LL.SIZES if x <= n_cap):
            fams = [f for f in LL.families(n) if f in ("tall", "thin", "gap_deep", "gap6") or f.startswith("brim") or (f == "gap_front" and n == n_cap)]
            s += [(n, fam, K) for fam in fams]
    top = max(n for n, _, _ in s)
    return s + [(top, "empty", K), (top, "rejected", K), (top, "tall", None)]


def caps_of(variant, n_cap):
    return (LL.F_CAP_WIDE if variant == "wide" else LL.F_CAP), (n_cap if variant == "long" else min(max(n_cap, 4), 30))


def assert_routes(exe, variant, prec, n_cap, f_cap, m_cap, windows):
    v = VARIANTS[variant]
    lit = v["mode"] == 0
    args = ["f" if prec == "f32" else "d", len(windows), len(windows), n_cap, f_cap, m_cap, 0, 2, 0, 84, -1] + list(windows)
    out = subprocess.run([exe, "--handle-lit" if lit else "--handle"] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines())
    # with a literal trajectory in the handle: the chain alone, on the information form (TU's `chain` variant states exactly that);
    # pre-whitened rows are ordinary rows: TU's `default`, k_update_small up to 12 cameras
    want = TU.meant("chain" if lit else "default", prec, n_cap, len(windows))
    for key, text in want.items():
        if key == "F" and variant in ("wide", "long"):       # (f_cap 260 / m_cap > 30: the feature routes are tests/test_gpu_feature_kernels.py's)
            continue
        assert text in got[key[0]], (variant, prec, n_cap, key, text, got[key[0]])
    assert "none" not in out.stdout and "?" not in out.stdout and got["G"].startswith("ok"), out.stdout
    if lit:
        assert "chain split=0 nsmall=0" in got["V"] and "select_diag gram" in got["C"], got
    return got


def make_handle(capi, po, monkeypatch, variant, prec, n_cap, specs):
    v = VARIANTS[variant]
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in v["env"].items():
        monkeypatch.setenv(name, value)
    f_cap, m_cap = caps_of(variant, n_cap)
    B = len(specs)
    bt = capi.Batch(B, n_cap, f_cap, m_cap, capi.F64 if prec == "f64" else capi.F32)
    if v["mode"]:
        bt.set_anisotropic_noise(v["mode"])
    tr = UL.FL.window(po).tr
    for b, (n, fam, K) in enumerate(specs):
        bt.initialize(b, LL.config(po, K), tr.imu0)
    sizes = [n for n, _, _ in specs]
    for k in range(max(sizes)):          # every trajectory augmented to its own size: one launch per run of longer windows
        b = 0
        while b < B:
            if sizes[b] <= k:
                b += 1
                continue
            e = b
            while e < B and sizes[e] > k:
                e += 1
            bt.augment_range(b, e - b)
            b = e
    for b, (n, fam, K) in enumerate(specs):
        assert bt.num_cam_states(b) == n
        H.copy_oracle_to_device(UL.window(po, n), bt, b)
        bt.set_tracks(b, *LL.tracks_of(po, n, fam))
    return bt, f_cap, m_cap


def run_case(capi, po, routes_exe, monkeypatch, variant, prec, n_cap):
    v = VARIANTS[variant]
    specs = specs_of(variant, n_cap)
    B = len(specs)
    bt, f_cap, m_cap = make_handle(capi, po, monkeypatch, variant, prec, n_cap, specs)
    assert_routes(routes_exe, variant, prec, n_cap, f_cap, m_cap, [n for n, _, _ in specs])
    before = {b: TU.state_bits(bt, b) for b, (n, fam, K) in enumerate(specs) if fam in ("empty", "rejected")}
    bt.marginalize_range(0, B)
    failures, worst = [], {}
    for b, (n, fam, K) in enumerate(specs):
        tag = (variant, prec, n_cap, b, n, fam, K)
        st = bt.last_stats(b)                               # (raises when a sticky flag is up)
        assert bt.error_flags(b) == 0, tag
        now = TU.state_bits(bt, b)
        assert np.array_equal(now[2], now[2].T), tag
        info = bt.literal_info(b)
        if fam in ("empty", "rejected"):
            assert st["n_tracks"] == (0 if fam == "empty" else UL.N_TALL) and st["n_passed"] == 0 and st["m_rows"] == 0, (tag, st)
            assert all(np.array_equal(x, y) for x, y in zip(now, before[b])), tag
            continue
        iso, lit = K is None, K is not None and v["mode"] == 0
        ref = LL.iso_reference(po, n, fam) if iso else LL.reference(po, n, fam, K) if lit else LL.whitened(po, n, fam, K)
        bar_c, bar_d = UL.bars(prec) if iso else LL.bars(prec, whitened_route=not lit)
        for key in H.STAT_KEYS:
            assert st[key] == ref.stats[key], (tag, key, st, ref.stats)
        M, slots, _ = LL.tracks_of(po, n, fam)
        ok = (ref.rows[:, 0] > 0) & (ref.rows[:, 1] > 0)
        H.check_tracks(bt.last_tracks(b), ref.rows, ok, prec, None, dict(M=M, slots=slots), UL.window(po, n), tag)
        if lit:
            assert info["route"] == (2 if variant == "dense" else 3) and info["m_rows"] == ref.stats["m_rows"], (tag, info, ref.stats)
            assert info["kept_rows"] == ref.stats["r_rows"], (tag, info, ref.stats)
            if fam.startswith("gap") and variant != "dense":
                assert info["kept_handed_through_rows"] >= 6, (tag, info)
            if variant != "dense" and (n == n_cap or fam == "gap6" or fam.startswith("brim")):
                sides = LL.staging(n, info["m_rows"], reflected=info["reflected"], basis=info["spare"], handed=info["kept_handed_through_rows"])
                for key, want in meant_sides(n, fam).items():
                    assert sides[key] == want, (tag, key, sides, info)
        else:
            assert info["route"] == 0 and info["m_rows"] == 0, (tag, info)      # left to k_gram's Lam^
        dx = bt.last_deltax(b)
        dc, dd = H.cov_scaled_err(now[2], ref.P1), UL.dx_scaled(dx, ref.dx, ref.P0)
        print("literal-dev %s %s n_cap=%d B=%d n=%d %s K=%s cov %.3e dx %.3e kept %d" % (variant, prec, n_cap, B, n, fam, K, dc, dd, info["kept_rows"]))
        w = worst.setdefault(n, [0.0, 0.0])
        w[0], w[1] = max(w[0], dc), max(w[1], dd)
        if not (dc <= bar_c and dd <= bar_d):
            failures.append((b, n, fam, K, dc, dd, (bar_c, bar_d)))
    bt.close()
    assert not failures, (variant, prec, n_cap, failures)
    return worst


@pytest.mark.parametrize("variant,prec,n_cap", CASES, ids=["%s-%s-n%d" % c for c in CASES])
def test_literal_route_against_double_oracle_at_every_edge(capi, po, routes_exe, monkeypatch, variant, prec, n_cap):
    """Measured on an MI355X: DESIGN.md section 3.4d has the device's worst distance per window size over these cases beside the
    float oracle's."""
    run_case(capi, po, routes_exe, monkeypatch, variant, prec, n_cap)


def test_grid_reaches_both_sides_of_every_edge():
    """every pair of neighbouring window sizes of the edge table has a handle of each size, and the special lists ride in one"""
    for a, b in ((10, 11), (21, 22), (31, 32), (32, 33), (33, 34), (38, 39), (41, 42), (42, 43), (53, 54), (60, 61), (61, 62), (62, 63)):
        assert a in N_CAPS and b in N_CAPS and a in LL.SIZES and b in LL.SIZES
    fams = {(n, fam) for c in N_CAPS for n, fam, _ in specs_of("default", c)}
    assert {(5, "brim44"), (5, "brim45"), (5, "brim46"), (34, "gap6"), (63, "gap_front"), (6, "gap_deep")} <= fams
    assert max(len(specs_of("default", c)) for c in N_CAPS) <= 90
