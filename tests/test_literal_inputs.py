"""CPU only: the inputs and the metric of tests/test_gpu_literal_kernels.py can see a fault of the literal anisotropic route, and
the host build of literal_core.h (tests/cpp/literal_host.cpp) matches the oracle on every one of them -- the CPU statement of the
algorithm at every window up to 63 cameras.  Everything here runs on the CPU oracles (tests/literal_lab.py: double LEAN with
tolerance 1e-10 = the reference of the GPU suite; float LEAN with 8e-4 = what a correct float implementation looks like; the
whitened double GRAM oracle = the GLS stand-in and the reference of aniso_mode 1); the mutants and stand-ins are distances from the
reference's own RESULT, never applied to the code under test.  Zero cases excluded.

Measured over literal_lab.cases() (125 cases: 24 window sizes x their lists x K = 4, K = 1/4 at 10, 32, 39, 63 cameras), distance
from the double oracle on the entry-scaled metric (covariance, correction): see literal_lab.D32_MEASURED; the stand-ins:
    (a) GLS on the same case   0 (3 cameras: nothing is compressed), 4.9 bars at 5 cameras, 5.4 .. 6.4 at 6, >= 29 from 10 on
    (b) isotropic, sigma^2 = u'   >= 160 bars at every size        (c) isotropic, sigma^2 = v'   6.6 bars at 3 cameras, >= 100 from 5 on
    `thin` (4 rows: nothing dropped by the compression): (a) <= 4.2e-15"""
import numpy as np
import pytest

import helpers as H
import literal_lab as LL
import test_literal_core as TC
import update_lab as UL
from msckf_mono_amd import scenario as sc

lit = TC.lit          # the host build of literal_core.h (module-scoped fixture of tests/test_literal_core.py)
DENSE_MAX_ROWS = 800

_HOST = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def host(lit, po, n, fam, K):
    """the host build on one lab case: {route: (info8, relative Frobenius distance of its information matrix from the
    oracle's)}, the oracle's kept rows, and the staging sides of the compact route"""
    key = (n, fam, K)
    if key not in _HOST:
        o = LL.captured(po, n, fam, K)
        ref = LL.reference(po, n, fam, K)
        F, M, inc, slots, hx, r = TC._track_inputs(o)
        L_or, nr_or = TC.oracle_information(o, n)
        cfg = LL.config(po, K)
        out = {}
        for route in ((0, 1) if ref.stats["m_rows"] <= DENSE_MAX_ROWS else (0,)):
            L, info, _ = TC.host_compress(lit, n, M, inc, slots, hx, r, cfg["u_var_prime"], cfg["v_var_prime"], LL.TOL64, route=route)
            out[route] = ([int(x) for x in info], float(np.linalg.norm(L - L_or) / np.linalg.norm(L_or)))
        i0 = out[0][0]
        _HOST[key] = (out, nr_or, LL.staging(n, i0[0], reflected=i0[2], basis=i0[7], handed=i0[6]))
    return _HOST[key]


def test_every_size_has_a_reason_and_the_edges_are_where_the_code_has_them():
    lds = LL.lds_doubles()
    assert lds == 12000
    for n in LL.SIZES:
        assert len(LL.E[n]) > 10
    # the sizes of update_lab.E that decide what the chain does with Lam^
    for a, b in ((10, 11), (21, 22), (31, 32), (32, 33), (42, 43), (53, 54), (62, 63)):
        assert a in LL.E and b in LL.E and a in UL.E and b in UL.E
    full = lambda n: LL.staging(n, 15 + 6 * n + 100, reflected=6 * n, basis=15 + 6 * n)
    assert full(38)["sweep_pb"] == 16 and full(39)["sweep_pb"] == 8 and 288 * 38 + 784 <= lds < 288 * 39 + 784
    assert full(41)["rows_tiles"] and not full(42)["rows_tiles"]
    assert full(60)["stage_lds"] and not full(61)["stage_lds"]
    assert full(60)["elim_pb"] == 16 and full(61)["elim_pb"] == 8 and LL.staging(61, 500, reflected=350, basis=370)["elim_pb"] == 16
    assert not full(31)["two_level"] and full(32)["two_level"]
    assert full(26)["basis_tiles"] and not full(31)["basis_tiles"]       # a full basis: up to 26 cameras; at 31 it needs nb <= 184
    assert LL.staging(31, 400, reflected=184, basis=184)["basis_tiles"] and not LL.staging(32, 400, reflected=184, basis=184)["basis_tiles"]
    assert not LL.staging(5, 45)["gram"] and LL.staging(5, 46)["gram"] and LL.staging(5, 44)["sweep_pb"] is None
    for n in range(LL.N_MIN, LL.N_WIN + 1):      # the restatement's panel widths are those of the code: 16, 8 -- never narrower at 12000 doubles
        assert full(n)["sweep_pb"] in (16, 8) and full(n)["elim_pb"] in (16, 8)


def test_the_lists_are_what_they_say(po):
    for n in LL.WIDE_SIZES:
        for c in LL.wide_counts(n):
            M, slots, _ = LL.tracks_of(po, n, "wide%d" % c)
            s = slots.reshape(-1, 3)
            assert len(M) == c and np.all(M == 3) and np.all(np.diff(s, axis=1) > 0) and s.min() == 0 and s.max() == n - 1
            # slot ranges that straddle a 32-column tile edge of k_lit_gamma, and some that do not
            assert len(set((6 * a // 32, (6 * b + 5) // 32) for a, _, b in s)) >= 2
    for n, Ls in LL.LONG_LENGTHS.items():
        M, slots, _ = LL.tracks_of(po, n, "long")
        assert tuple(M[:len(Ls)]) == Ls and max(M) == n and len(M) <= LL.F_CAP
        off = np.concatenate([[0], np.cumsum(M)])
        ranges = [int(slots[off[i + 1] - 1] - slots[off[i]] + 1) for i in range(len(M))]
        assert ranges[len(Ls):len(Ls) + 4] == [10, 11, 10, 11] and list(M[len(Ls):len(Ls) + 4]) == [10, 11, 5, 5]
    for m, Ls in LL.BRIM.items():
        assert sum(2 * L - 3 for L in Ls) == m and max(Ls) <= LL.BRIM_N
    assert sorted(LL.BRIM) == [15 + 6 * LL.BRIM_N - 1, 15 + 6 * LL.BRIM_N, 15 + 6 * LL.BRIM_N + 1]
    for n in LL.SIZES:
        if n < LL.GAP_MIN_N:
            continue
        tall = LL.tracks_of(po, n, "tall")
        for where in ("front", "deep"):
            g = LL.gap_slot(n, where, tall[1])
            t = LL.tracks_of(po, n, "gap_" + where)
            assert g in tall[1] and g not in t[1] and 0 < g <= n - 3 and len(t[0]) >= LL.UL.N_TALL - 4, (n, where, g)
        assert LL.gap_slot(n, "deep", tall[1]) >= n - 5 and LL.gap_slot(n, "front", tall[1]) <= max(2, n // 3)
    t = LL.tracks_of(po, LL.GAP6_N, "gap6")
    assert not set(LL.GAP6_SLOTS) & set(int(s) for s in t[1])


@pytest.mark.parametrize("n", LL.SIZES)
def test_conditions_and_mutants_hold_with_zero_exclusions(po, n):
    """Per list of the window and per K: double and float oracle agree on every track's flags, on the six counts, on m_rows AND on
    r_rows; n_passed > 0; no gamma within 1 % of its threshold; the float oracle within FLOAT_ILL; on the lists with rows to compress
    every stand-in and every damage of update_lab.mutate at MUTANT_FACTOR float bars or more (but MUTANT_EXEMPT, asserted to be what
    it says); stand-in (a) from GLS_MIN_N cameras on, and zero to 1e-12 on `thin`.  Flags and counts are those of the isotropic
    lab: the gate keeps u'."""
    bc, bd = LL.bars("f32")
    low = []
    for fam in LL.families(n):
        M = LL.tracks_of(po, n, fam)[0]
        for K in LL.ks_of(n):
            ref = LL.reference(po, n, fam, K)
            assert LL.case_violations(po, n, fam, K, M) == [], (n, fam, K)
            iso = LL.iso_reference(po, n, fam)
            assert np.array_equal(iso.rows[:, :3] > 0, ref.rows[:, :3] > 0) and all(iso.stats[k] == ref.stats[k] for k in H.STAT_KEYS), (n, fam, K)
            if n >= 5:
                assert ref.stats["n_passed"] == len(M) and ref.stats["m_rows"] == int(np.sum(2 * M - 3)), (n, fam, ref.stats)
            scores = {w: LL.stand_in_score(po, n, fam, K, w) for w in LL.STAND_INS}
            scores.update({m: UL.mutant_score(ref, m) for m in UL.MUTANTS})
            d = LL.distances(LL.float_oracle(po, n, fam, K), ref)
            print("literal-lab n=%d %s K=%g passed %d m_rows %d r_rows %d | d32 %.3e %.3e | %s" % (
                n, fam, K, ref.stats["n_passed"], ref.stats["m_rows"], ref.stats["r_rows"], d[0], d[1], " ".join("%s %.2e" % kv for kv in scores.items())))
            if fam == "thin":
                assert scores["gls"] <= 1e-12 and ref.stats["m_rows"] == (4 if n >= 4 else ref.stats["m_rows"]), (n, K, scores["gls"])
            if not LL.needs_rows(fam):
                continue
            for m, s in scores.items():
                bar = LL.MUTANT_FACTOR * (bd if m in ("dx_newest", "dx_last") else bc)
                if m == "gls" and n < LL.GLS_MIN_N:
                    assert s < bar, (n, fam, K, s)            # GLS_MIN_N is the SMALLEST such window: below it the stand-in is under ten bars
                elif (n, fam, K, m) in LL.MUTANT_EXEMPT:
                    want = LL.MUTANT_EXEMPT[(n, fam, K, m)]
                    assert s < bar and abs(s - want) <= 0.05 * want, (n, fam, K, m, s, want)
                elif not s >= bar:
                    low.append((n, fam, K, m, s, s / bar * LL.MUTANT_FACTOR))
    assert not low, low
    assert all(k[0] in LL.SIZES and k[1] in LL.families(k[0]) and k[2] in LL.ks_of(k[0]) for k in LL.MUTANT_EXEMPT)


def test_float_bars_are_the_measured_ones(po):
    """ONE bar per metric: FLOAT_FACTOR x the largest distance of the float LEAN oracle (tolerance 8e-4) from the double one over
    every case of the lab; the recorded maxima reproduce to 2 %, no case exceeds the constants the bars are built on nor the
    ill-conditioning line.  The same for aniso_mode 1: the whitened float GRAM oracle against the whitened double one."""
    w, where = np.zeros(2), [None, None]
    for n, fam, K in LL.cases():
        d = LL.distances(LL.float_oracle(po, n, fam, K), LL.reference(po, n, fam, K))
        assert max(d) <= LL.FLOAT_ILL, (n, fam, K, d)
        for i in range(2):
            if d[i] > w[i]:
                w[i], where[i] = d[i], (n, fam, K)
    print("literal-lab float maxima %.3e %s %.3e %s" % (w[0], where[0], w[1], where[1]))
    assert np.all(w <= [LL.D32_COV, LL.D32_DX]), w
    assert np.allclose(w, LL.D32_MEASURED, rtol=0.02), (w, LL.D32_MEASURED)
    assert LL.FLOAT_ILL <= 3 * max(LL.D32_COV, LL.D32_DX) + 1e-12 and LL.bars("f64") == (1e-6, 1e-6) and LL.bars("f32") == (4 * LL.D32_COV, 4 * LL.D32_DX)
    ww = np.zeros(2)
    for n in LL.WHITENED_SIZES:
        for fam in ("tall", "thin"):
            a, b = LL.whitened(po, n, fam), LL.whitened(po, n, fam, dtype=po.F32)
            assert np.array_equal(a.rows[:, :3] > 0, b.rows[:, :3] > 0) and all(a.stats[k] == b.stats[k] for k in H.STAT_KEYS), (n, fam)
            ww = np.maximum(ww, LL.distances(b, a))
    print("literal-lab whitened float maxima %.3e %.3e" % (ww[0], ww[1]))
    assert np.all(ww <= [LL.D32W_COV, LL.D32W_DX]) and np.allclose(ww, LL.D32W_MEASURED, rtol=0.02), (ww, LL.D32W_MEASURED)
    assert LL.bars("f32", True) == (4 * LL.D32W_COV, 4 * LL.D32W_DX)


def _gls_against_literal(po, n, cfg_uv):
    """(worst entry of helpers.state_errors, scaled covariance distance, scaled correction distance) of the GLS update from the
    literal one on the `tall` list of the window, with the noise (u', v') given"""
    t = LL.tracks_of(po, n, "tall")
    K = cfg_uv[1] / cfg_uv[0]
    ref = LL.run_oracle(po, n, t, K, po.F64, po.LEAN, tol=LL.TOL64)
    gls = LL.run_oracle(po, n, t, K, po.F64, po.GRAM, whiten=True)
    fro = H.worst(H.state_errors(gls.imu, ref.imu, gls.cams, ref.cams, gls.P1, ref.P1))
    return (fro,) + LL.distances(gls, ref)


def test_the_shipped_noise_cannot_show_a_literal_route_fault_in_float(po):
    """The documented gap, both halves.  With the ratio v' / u' of the shipped EuRoC intrinsics (scenario.filter_config(isotropic =
    False): 0.6 %) a device that computed GLS instead of the literal compression would pass the float bars of this suite on the
    covariance at 10, 30 and 39 cameras by a factor of 40 and more (found: 9.2e-8 .. 6.9e-7 against 1.28e-4), the correction bar
    (3.5e-5 .. 9.7e-5 against 1.17e-4) and the 1e-3 of helpers.state_errors on every field (4.7e-4 .. 7.3e-4; the covariance alone
    5e-9 .. 2e-8).  With K = 4 the same stand-in fails the scaled covariance bar by the factors GAP_FACTORS (found: 32, 255, 201), the
    correction bar by 70 and more, and state_errors by 90."""
    euroc = sc.filter_config(10, isotropic=False)
    ratio = euroc["v_var_prime"] / euroc["u_var_prime"]
    assert 0.003 < abs(ratio - 1.0) < 0.02
    u = LL.config(po, None)["u_var_prime"]
    bc, bd = LL.bars("f32")
    for n in LL.GAP_TABLE_SIZES:
        fro, dc, dd = _gls_against_literal(po, n, (u, ratio * u))
        fro4, dc4, dd4 = _gls_against_literal(po, n, (u, LL.K_MAIN * u))
        t = LL.tracks_of(po, n, "tall")
        refe = LL.run_oracle(po, n, t, ratio, po.F64, po.LEAN, tol=LL.TOL64)
        glse = LL.run_oracle(po, n, t, ratio, po.F64, po.GRAM, whiten=True)
        froP = H.rel(glse.P1, refe.P1, 1e-30)
        print("literal-lab gap n=%d EuRoC: state_errors %.2e (P alone %.2e) scaled %.2e %.2e | K=4: state_errors %.2e scaled %.2e %.2e = %.0f / %.0f bars" % (
            n, fro, froP, dc, dd, fro4, dc4, dd4, dc4 / bc, dd4 / bd))
        assert fro < 1e-3 and froP < 1e-6 and dc < bc / 40 and dd < bd, (n, fro, froP, dc, dd)
        assert dc4 >= LL.GAP_FACTORS[n] * bc and dd4 >= 10 * bd and fro4 > 50e-3, (n, fro4, dc4, dd4)


@pytest.mark.parametrize("n", LL.SIZES)
def test_host_build_of_the_literal_core_matches_the_oracle_on_every_lab_case(lit, po, n):
    """tests/cpp/literal_host.cpp with the default staging area of 12000 doubles, compact route on every case and the sweep over
    the dense stack on those of up to 800 rows: stacked rows, kept rows and reflected steps equal the oracle's (and each other's),
    the kept handed-through rows cover every unobserved camera slot, the information matrix within 1e-9 (relative Frobenius, as
    tests/test_literal_core.py measures it)."""
    for fam in LL.families(n):
        slots = LL.tracks_of(po, n, fam)[1]
        for K in LL.ks_of(n):
            out, nr_or, st = host(lit, po, n, fam, K)
            ref = LL.reference(po, n, fam, K)
            ic, ec = out[0]
            print("literal-lab host n=%d %s K=%g info %s err %.1e%s | %s" % (n, fam, K, ic, ec, " dense %s %.1e" % out[1] if 1 in out else "", st))
            assert ic[0] == ref.stats["m_rows"] and ic[4] == 3 and ic[1] == nr_or == ref.stats["r_rows"], (n, fam, K, ic, nr_or, ref.stats)
            assert ec < 1e-9, (n, fam, K, ec)
            if 1 in out:
                ig, eg = out[1]
                assert ig[0] == ic[0] and ig[4] == 2 and ig[1] == nr_or and ig[2] == ic[2] and eg < 1e-9, (n, fam, K, ig, ic, eg)
            if fam.startswith("gap"):
                unseen = n - len(set(int(s) for s in slots))
                assert unseen >= (6 if fam == "gap6" else 1) and ic[6] >= (36 if fam == "gap6" else 6), (n, fam, ic, unseen)
            assert st["basis_tiles"] is not None, (n, fam, K, ic)      # the restatement knows which side the case is on


def test_every_literal_edge_has_a_case_on_each_side(lit, po):
    """from the host build's own counts (stacked rows, reflected steps, rows of the basis, kept handed-through rows) through
    literal_lab.staging: both sides of every staging decision of the compact route are reached by a lab case"""
    seen = {key: {} for key, _, _ in LL.EDGES}
    for n, fam, K in LL.cases():
        st = host(lit, po, n, fam, K)[2]
        for key in seen:
            seen[key].setdefault(st[key], (n, fam, K))
    print("literal-lab edges", seen)
    for key, a, b in LL.EDGES:
        assert a in seen[key] and b in seen[key], (key, seen[key])
    assert set(seen["sweep_pb"]) <= {None, 16, 8} and set(seen["elim_pb"]) == {16, 8}
    # the window sizes the sides change at, on the `tall` list
    side = lambda n, key: host(lit, po, n, "tall", LL.K_MAIN)[2][key]
    assert (side(38, "sweep_pb"), side(39, "sweep_pb")) == (16, 8) and (side(41, "rows_tiles"), side(42, "rows_tiles")) == (True, False)
    assert (side(60, "stage_lds"), side(61, "stage_lds")) == (True, False) and (side(31, "two_level"), side(32, "two_level")) == (False, True)
    st = host(lit, po, LL.GAP6_N, "gap6", LL.K_MAIN)
    assert st[2]["basis_tiles"] and st[2]["tiles_list"] is False and st[0][0][0][7] > 208, st


def test_empty_and_rejected_lists(po):
    """the row-less trajectories of the GPU suite under anisotropic noise: no track of the 40 px list passes (the gate keeps u'),
    the covariance stays untouched"""
    for n in LL.SIZES:
        r = LL.run_oracle(po, n, LL.tracks_of(po, n, "rejected"), LL.K_MAIN, po.F64, po.LEAN, tol=LL.TOL64)
        assert r.stats["n_tracks"] == UL.N_TALL and r.stats["n_passed"] == 0 and r.stats["m_rows"] == 0 and np.array_equal(r.P0, r.P1), (n, r.stats)
    r = LL.run_oracle(po, 63, LL.tracks_of(po, 63, "empty"), LL.K_MAIN, po.F64, po.LEAN, tol=LL.TOL64)
    assert np.array_equal(r.P0, r.P1)
