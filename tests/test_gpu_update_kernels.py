"""Everything an update runs after k_feature -- k_select_diag, k_gram, k_chol_mfma in its six modes, k_trsm_rows, the GEMMs
OP_PHT / OP_PHTT / OP_S / OP_W / OP_K / OP_DOWN, k_gain, k_gain_w, k_chol_inv, k_dx_w, k_dx_wz, k_inject, k_update_small --
against the DOUBLE oracle on an entry-scaled metric, at windows on both sides of every edge these kernels have
(tests/update_lab.py: the windows, the two track lists per window, the edges with their reasons, the bars;
tests/test_update_inputs.py: the proof on the CPU that these inputs and this metric see a fault that helpers.state_errors
passes).

A case is ONE handle and ONE marginalize_range over all of it: trajectory b holds a window of its own size -- every size of
update_lab.SIZES up to the handle's n_cap with the `tall` and the `thin` list, and at the largest size one trajectory with an
empty work-list and one whose 24 tracks carry 40 px of noise (none passes).  The device never fills a window: every trajectory
is augmented to its size and teacher-forced with the oracle's window.  Per trajectory: last_stats' counts and every track's
flags equal the double oracle's (helpers.check_tracks; r_rows is a count of pivots on the information form and is not compared),
covariance and correction within the dtype's bar (double 1e-6; float 4 x the float oracle's own worst distance, measured on the
CPU), no sticky error flag, P bit-symmetric; the row-less trajectories keep state and covariance to the bit.

Each case first asserts, through the pure functions of csrc/update_routes.h (tests/cpp/update_routes_host.cpp --handle), that
its handle and windows reach the launches the case was written for (MEANT below): a later change of a threshold cannot
silently empty a case.  The settings are read when the handle is created, so the environment is set before capi.Batch.

Found while writing this suite: the one-launch update fits windows of at most 12 cameras (routes::small_limit(84) = 72 columns),
not the 14 the setting asks for; 13 and 14 cameras take the chain.  Hence 12 among the sizes, and `mixed` from n_cap 14 on.

Out of scope: the fp16-Jacobian dtype (tests/test_gpu_h16_kernels.py holds it to a given-H twin on these windows), the early-accept
bound (tests/test_gpu_gate_early.py), tracks longer than 30 (the feature routes: tests/test_gpu_feature_kernels.py); the anisotropic and literal routes and aniso_mode == 1 are tests/test_gpu_literal_kernels.py's.
The `tsqr` variant below holds the Householder TSQR route on THESE lists only (every track from slot 0, all or none passing, at
most 720 rows); everything else about that route -- every k_qr_update instantiation, the chunk counts, staggered first slots,
compactions with holes, blind cameras, stacks deeper than the pipeline and longer than the progress ring, the route taken by
geometry -- is tests/test_gpu_tsqr_kernels.py's (inputs: tests/tsqr_lab.py, tests/test_tsqr_inputs.py)."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import update_lab as UL
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu

C = (10, 11, 14, 15, 21, 22, 23, 24, 31, 32, 33, 42, 43, 53, 54, 63)      # 23 | 24: k_chol_inv<double> with S in LDS | in global memory
BOTH = ("f32", "f64")
# name: environment at create time, set_covariance_update, set_compression, dtypes, n_caps
VARIANTS = {
    "default": dict(env={}, form=0, compress=-1, precs=BOTH, n_caps=C),
    "chain": dict(env={"MSCKF_HIP_SMALL_UPDATE": "0"}, form=0, compress=-1, precs=BOTH, n_caps=C),
    "form2": dict(env={}, form=2, compress=-1, precs=("f32",), n_caps=tuple(c for c in C if c <= 33)),
    "parts2": dict(env={"MSCKF_HIP_GAIN_PARTS": "2"}, form=0, compress=-1, precs=("f32",), n_caps=(22, 31, 32)),
    # (without MSCKF_HIP_SMALL_UPDATE=0 the handle of n_cap 10 would take k_update_small for every window and never launch OP_S)
    "unfused": dict(env={"MSCKF_HIP_FUSED_S": "0", "MSCKF_HIP_SMALL_UPDATE": "0"}, form=0, compress=-1, precs=("f32",), n_caps=(10, 21, 32)),
    "joseph": dict(env={}, form=1, compress=-1, precs=BOTH, n_caps=(10, 11, 21, 22, 32, 33)),
    "tsqr": dict(env={}, form=0, compress=0, precs=BOTH, n_caps=(10, 22, 33, 63)),
}
CASES = [(v, p, n) for v, s in VARIANTS.items() for p in s["precs"] for n in s["n_caps"]]
ENV_NAMES = ("MSCKF_HIP_SMALL_UPDATE", "MSCKF_HIP_GAIN_PARTS", "MSCKF_HIP_FUSED_S", "MSCKF_HIP_FEATURE_PAIR")
F_CAP = 32


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def routes_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("update_routes") / "update_routes_host")
    src = os.path.join(H.ROOT, "tests", "cpp", "update_routes_host.cpp")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", "-o", exe, src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


# ------------------------------------------------------------------------------------------------ the routes that were meant
def _level(n_cap, bounds, values):
    return values[sum(n_cap > b for b in bounds)]


def meant(variant, prec, n_cap, nb):
    """{stage letter: text the stage's line of --handle must contain} -- written down here from the table of this suite's
    specification, NOT computed from update_routes.h"""
    v = VARIANTS[variant]
    f32, form = prec == "f32", v["form"]
    S = "float" if f32 else "double"
    m = {"G": "ok "}
    info = v["compress"] != 0
    m["F"] = "pair lm=" if f32 and info else "k_feature<0> lm="
    if not info:
        m["C"] = "compress=0 select tsqr"
    elif n_cap <= 31:
        m["C"] = "select_diag gram parts=3 CH_GRAM<%d>" % _level(n_cap, (10, 21), (4, 8, 12))
    else:
        nb_b = _level(n_cap, (42, 53), (4, 8, 12))
        m["C"] = "select_diag gram parts=1 CH_GRAM_A<12> TR_GRAM items=%d CH_GRAM_B<%d>" % (nb_b // 4, nb_b)
    small = info and form == 0 and v["env"].get("MSCKF_HIP_SMALL_UPDATE") != "0"
    if not small:
        m["V"] = "chain split=0 nsmall=0 segb=0"
    elif n_cap <= 12:
        m["V"] = "small split=0 nsmall=%d segb=%d" % (6 * n_cap, 4 if n_cap <= 10 else 8)      # k_update_small alone, segb 4 | 8
    else:
        m["V"] = "mixed split=72 nsmall=72 segb=8"                                               # SMALL_AND_CHAIN in one range
    npart = 8 if nb <= 64 else 4 if nb <= 128 else 2
    large = "large CH_S_A<12> TR_S21 items=%d CH_S_B<%d> TR_W<%d>" % ((_level(n_cap, (42, 53), (4, 8, 12)) // 4,) + _level(n_cap, (42, 53), ((4, 16), (8, 20), (12, 24))))
    if form == 1:
        if n_cap <= (32 if f32 else 21):
            m["K"] = "fused=0 k_gain<%s,%d> k_inject<true>" % (S, _level(n_cap, (10, 21), (4, 8, 12)))
        else:
            m["K"] = "k_chol_inv<%s,%s> " % (S, "true" if (not f32 and n_cap <= 23) else "false")
            m["K2"] = " OP_W OP_K k_inject<false>"
    elif f32 and form == 0:
        if n_cap <= 32:
            blocked = _level(n_cap, (10, 21), ("4,2,3", "8,3,3", "12,7,2" if variant == "parts2" else "12,4,4"))
            m["K"] = "fused=%d blocked<%s>" % (0 if variant == "unfused" else 1, blocked)
        else:
            m["K"] = "fused=0 " + large
    elif f32:           # form 2: the register-resident solve, NBN = 12 in float only
        m["K"] = "fused=0 k_gain_w<float,%d,%d>" % (_level(n_cap, (10, 21), (4, 8, 12)), npart) if n_cap <= 32 else "fused=0 k_chol_inv<float,false> lds=0 OP_W k_dx_w"
    elif n_cap <= 21:
        m["K"] = "fused=0 k_gain_w<double,%d,%d>" % (_level(n_cap, (10,), (4, 8)), npart)
    elif n_cap <= 32:
        m["K"] = "fused=0 k_chol_inv<double,%s> " % ("true" if n_cap <= 23 else "false")
        m["K2"] = " OP_W k_dx_w"
    else:
        m["K"] = "fused=0 " + large
    return m


def assert_routes(exe, variant, prec, B, n_cap, m_cap, windows, f_cap=F_CAP, skip=()):
    v = VARIANTS[variant]
    args = ["f" if prec == "f32" else "d", B, len(windows), n_cap, f_cap, m_cap, v["form"], v["env"].get("MSCKF_HIP_FUSED_S", 2),
            v["env"].get("MSCKF_HIP_GAIN_PARTS", 0), v["env"].get("MSCKF_HIP_SMALL_UPDATE", 84), v["compress"]] + list(windows)
    out = subprocess.run([exe, "--handle"] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines())
    want = meant(variant, prec, n_cap, len(windows))
    for key, text in want.items():
        if key in skip:
            continue
        assert text in got[key[0]], (variant, prec, n_cap, key, text, got[key[0]])
    assert (m_cap > 30 or "k_feature<1>" not in got["F"]) and "none" not in out.stdout and "?" not in out.stdout, out.stdout
    return got


# ------------------------------------------------------------------------------------------------ one handle, one launch sequence
def specs_of(n_cap):
    """(window size, list) per trajectory, window sizes ascending; the two row-less trajectories at the largest size"""
    sizes = [n for n in UL.SIZES if n <= n_cap]
    return [(n, fam) for n in sizes for fam in UL.FAMILIES] + [(sizes[-1], "empty"), (sizes[-1], "rejected")]


def tracks_for(po, n, fam):
    return UL.EMPTY if fam == "empty" else UL.rejected_tracks(po, n) if fam == "rejected" else UL.tracks_of(po, n, fam)


def hard_specs():
    """the `thin` lists the float GRAM oracle cannot do (update_lab.HARD_THIN), one trajectory each"""
    return [(n, "thin:%d" % sub) for n, sub in UL.HARD_THIN]


def make_handle(capi, po, monkeypatch, variant, prec, n_cap, specs):
    v = VARIANTS[variant]
    for name in ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    for name, value in v["env"].items():
        monkeypatch.setenv(name, value)
    B, m_cap = len(specs), min(max(n_cap, 4), 30)
    bt = capi.Batch(B, n_cap, F_CAP, m_cap, capi.F64 if prec == "f64" else capi.F32)
    if v["compress"] >= 0:
        bt.set_compression(v["compress"])
    if v["form"]:
        bt.set_covariance_update(v["form"])
    tr = UL.FL.window(po).tr
    for b in range(B):
        bt.initialize(b, tr.cfg, tr.imu0)
    for k in range(max(n for n, _ in specs)):          # every trajectory augmented to its own size: one launch per run of longer windows
        b = 0
        while b < B:
            if specs[b][0] <= k:
                b += 1
                continue
            e = b
            while e < B and specs[e][0] > k:
                e += 1
            bt.augment_range(b, e - b)
            b = e
    for b, (n, fam) in enumerate(specs):
        assert bt.num_cam_states(b) == n
        H.copy_oracle_to_device(UL.window(po, n), bt, b)
        bt.set_tracks(b, *tracks_for(po, n, fam))
    return bt, m_cap


def state_bits(bt, b):
    return bt.imu_state(b), bt.cam_states(b)[0], bt.covariance(b)


def run_case(capi, po, routes_exe, monkeypatch, variant, prec, n_cap, specs=None):
    """the case's launch sequence and every per-trajectory assertion; returns (state bits + correction per trajectory, the
    worst distances per window size)"""
    specs = specs_of(n_cap) if specs is None else specs
    B = len(specs)
    bt, m_cap = make_handle(capi, po, monkeypatch, variant, prec, n_cap, specs)
    assert_routes(routes_exe, variant, prec, B, n_cap, m_cap, [n for n, _ in specs])
    before = {b: state_bits(bt, b) for b, (n, fam) in enumerate(specs) if fam in ("empty", "rejected")}
    bt.marginalize_range(0, B)
    bar_c, bar_d = UL.bars(prec)
    failures, out, worst = [], [], {}
    for b, (n, fam) in enumerate(specs):
        st = bt.last_stats(b)                               # (raises when a sticky flag is up)
        assert bt.error_flags(b) == 0, (b, n, fam)
        now = state_bits(bt, b)
        assert np.array_equal(now[2], now[2].T), (b, n, fam)
        if fam in ("empty", "rejected"):
            assert st["n_tracks"] == (0 if fam == "empty" else UL.N_TALL) and st["n_passed"] == 0 and st["m_rows"] == 0, (b, n, fam, st)
            assert all(np.array_equal(x, y) for x, y in zip(now, before[b])), (b, n, fam)
            out.append(now + (None,))
            continue
        ref = UL.reference(po, n, fam)
        for key in H.STAT_KEYS:
            assert st[key] == ref.stats[key], (b, n, fam, key, st, ref.stats)
        M, slots, _ = UL.tracks_of(po, n, fam)
        ok = (ref.rows[:, 0] > 0) & (ref.rows[:, 1] > 0)
        H.check_tracks(bt.last_tracks(b), ref.rows, ok, prec, None, dict(M=M, slots=slots), UL.window(po, n), (variant, prec, n_cap, n, fam))
        dx = bt.last_deltax(b)
        dc, dd = H.cov_scaled_err(now[2], ref.P1), UL.dx_scaled(dx, ref.dx, ref.P0)
        print("update-dev %s %s n_cap=%d B=%d n=%d %s cov %.3e dx %.3e" % (variant, prec, n_cap, B, n, fam, dc, dd))
        w = worst.setdefault(n, [0.0, 0.0])
        w[0], w[1] = max(w[0], dc), max(w[1], dd)
        if not (dc <= bar_c and dd <= bar_d):
            failures.append((b, n, fam, dc, dd))
        out.append(now + (dx,))
    bt.close()
    assert not failures, (variant, prec, n_cap, (bar_c, bar_d), failures)
    return out, worst


@pytest.mark.parametrize("variant,prec,n_cap", CASES, ids=["%s-%s-n%d" % c for c in CASES])
def test_update_against_double_oracle_at_every_window_edge(capi, po, routes_exe, monkeypatch, variant, prec, n_cap):
    """Measured on an MI355X: DESIGN.md section 3.4c has the device's worst distance per window size over these cases beside the
    float oracle's."""
    run_case(capi, po, routes_exe, monkeypatch, variant, prec, n_cap)


@pytest.mark.parametrize("variant", ["default", "chain", "tsqr"])
@pytest.mark.parametrize("prec", BOTH)
def test_rank_4_updates_the_float_gram_oracle_cannot_do(capi, po, routes_exe, monkeypatch, variant, prec):
    """Fourteen two-track updates on which the CPU oracle's own float Gram restatement is 2e-4 .. 2.3e-2 from the double oracle or
    finds a fifth pivot (update_lab.HARD_THIN): the device is held to the ordinary bars on them, against the double oracle --
    k_update_small (4 .. 12 cameras) and the chain's k_chol_mfma (24, 43, 63) in one range of an n_cap = 63 handle, the chain alone,
    and the TSQR route.  Measured on an MI355X, information form: float <= 1.1e-5 / 3.5e-6, double <= 1.8e-10 / 1.8e-11."""
    run_case(capi, po, routes_exe, monkeypatch, variant, prec, 63, hard_specs())


def test_k_gain_w_parts_change_no_bit(capi, po, routes_exe, monkeypatch):
    """k_gain_w runs 8 workgroups per trajectory up to 64 trajectories in the launch, 4 up to 128, 2 beyond: the double default
    at n_cap 21, its range as it is (26 trajectories), padded to 65 and to 129 by repeating the list.  Every run is held to the
    bars; the trajectories present in all three carry the same bits (state, covariance, correction)."""
    base = specs_of(21)
    runs = []
    for B in (len(base), 65, 129):
        specs = (base * (B // len(base) + 1))[:B]
        got = assert_routes(routes_exe, "default", "f64", B, 21, 21, [n for n, _ in specs])
        assert "k_gain_w<double,8,%d>" % {len(base): 8, 65: 4, 129: 2}[B] in got["K"], got
        runs.append(run_case(capi, po, routes_exe, monkeypatch, "default", "f64", 21, specs)[0])
    for b in range(len(base)):
        for other in runs[1:]:
            for x, y in zip(runs[0][b], other[b]):
                assert (x is None and y is None) or np.array_equal(x, y), (b, base[b])


# ------------------------------------------------------------------------------------------------ the prune riding on the downdate
@pytest.mark.parametrize("prec,N", [("f32", 22), ("f64", 22), ("f32", 36)])
def test_prune_on_the_chain_s_downdate_equals_the_separate_prune(capi, routes_exe, prec, N):
    """tests/test_gpu_configs.py::test_prune_on_the_downdate_equals_the_separate_prune holds the fused prune at 8 cameras, which
    is k_update_small's downdate.  Here the chain's OP_DOWN (22 cameras, float and double) and GAIN_LARGE's (36 cameras): a frame
    range run frame by frame (the separate prune launch throughout) and in one call (the prune rides on every downdate but the
    last) gives the same bits -- states, camera states, covariance, window size, statistics."""
    B, F, nf = 2, 40, N + 4
    dtype = capi.F32 if prec == "f32" else capi.F64
    got = assert_routes(routes_exe, "default", prec, B, N, N, [N] * B, f_cap=F, skip=("V",))      # (V is meant for the windows of specs_of)
    assert got["V"].startswith("limit=72 chain") and ("large" in got["K"]) == (N == 36), got
    trajs = [sc.Trajectory(2, 300 + b, N, F, nf) for b in range(B)]

    def run(cuts):
        bt = capi.Batch(B, N, F, N, dtype)
        for b, tr in enumerate(trajs):
            bt.initialize(b, tr.cfg, tr.imu0)
        bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
        for k in range(nf):
            for b, tr in enumerate(trajs):
                fr = tr.frames[k]
                bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
        bt.scenario_commit()
        a = 0
        for c in cuts:
            bt.run_frames(a, a + c)
            a += c
        bt.sync()
        snap = [H.snapshot(bt, b) for b in range(B)]
        bt.close()
        return snap

    ref, one = run([1] * nf), run([nf])
    for b in range(B):
        assert ref[b][3] == N - 1 and ref[b][4]["n_passed"] > 0, (b, ref[b][3], ref[b][4])      # full window, one state dropped per frame, still updating
        assert H.same_bits(one[b], ref[b]), (prec, N, b)
