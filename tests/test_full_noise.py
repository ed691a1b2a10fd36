"""Whole noiseParams::Q_imu (12 x 12) and initial_imu_covar (15 x 15) (types.h:90-91, msckf.h:86, :134) through every layer:
msckf_hip_initialize_full, k_propagate's full-Q instantiation, its per-trajectory routing in batched launches, the shim's
full-matrix members, capi / scenario.  The reference for the numbers is the numpy twin oracle/np_oracle.py (it propagates with
G Q G^T for whatever Q it holds), given the whole matrices."""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

ROOT = H.ROOT
SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "shim_full_noise.cpp")


def correlated(diag, seed, lo=0.3, hi=0.6):
    """SPD matrix with the given diagonal whose off-diagonal entries are lo .. hi (in magnitude, random signs) of the geometric
    mean of their two diagonal entries: correlation c c^T + diag(1 - c^2), |c_i| in [sqrt(lo), sqrt(hi)]"""
    rng = np.random.default_rng(seed)
    n = len(diag)
    c = rng.uniform(np.sqrt(lo), np.sqrt(hi), n) * rng.choice([-1.0, 1.0], n)
    R = np.outer(c, c)
    np.fill_diagonal(R, 1.0)
    s = np.sqrt(np.asarray(diag, dtype=np.float64))
    return R * np.outer(s, s)


def full_config(N, seed=7, **kw):
    base = sc.filter_config(N, **kw)
    return sc.filter_config(N, Q_imu=correlated(base["Q_imu_diag"], seed), P0=correlated(base["P0_diag"], seed + 1), **kw)


def without(cfg, *keys):
    c = dict(cfg)
    for k in keys:
        c.pop(k, None)
    return c


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_initialize_full_is_declared_and_exported():
    from msckf_mono_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msckf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+msckf_hip_initialize_full\s*\(", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T msckf_hip_initialize_full$", out, flags=re.M)
    assert "msckf_hip_initialize_full" in capi.SYMBOLS


def test_shim_full_matrix_members_compile(tmp_path):
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", SHIM_SRC,
                          "-o", str(tmp_path / "shim_full.o")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_configs_carry_the_whole_matrices():
    from msckf_mono_amd import capi
    d = sc.filter_config(8)
    assert "Q_imu" not in d and "P0" not in d and capi.full_noise(d) is None
    f = full_config(8)
    Q, P0 = capi.full_noise(f)
    assert np.array_equal(np.diag(Q), f["Q_imu_diag"]) and np.array_equal(np.diag(P0), f["P0_diag"])
    assert np.array_equal(Q, Q.T) and np.all(np.linalg.eigvalsh(Q) > 0) and np.all(np.linalg.eigvalsh(P0) > 0)
    off = np.abs(Q) / np.sqrt(np.outer(np.diag(Q), np.diag(Q)))
    off = off[~np.eye(12, dtype=bool)]
    assert off.min() >= 0.3 - 1e-12 and off.max() <= 0.6 + 1e-12
    # one matrix missing: the diagonal keys stand in for it
    Q1, P1 = capi.full_noise(without(f, "P0"))
    assert np.array_equal(Q1, Q) and np.array_equal(P1, np.diag(f["P0_diag"]))
    # IMU noise drawn from the [omega, a] block of Q_imu; the tracks (and the stream of a config without Q_imu) do not move
    a, b = sc.Trajectory(2, 5, 8, 10, 12, cfg=f), sc.Trajectory(2, 5, 8, 10, 12)
    assert all(np.array_equal(x["obs"], y["obs"]) and np.array_equal(x["slots"], y["slots"]) for x, y in zip(a.frames, b.frames))
    assert not np.array_equal(a.readings[:, :6], b.readings[:, :6])
    assert np.array_equal(b.readings, sc.Trajectory(2, 5, 8, 10, 12, cfg=sc.filter_config(8)).readings)


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def npo():
    import np_oracle
    return np_oracle


def twin(npo, cfg, imu0):
    n = npo.NpMSCKF(cfg, imu0)
    if "Q_imu" in cfg:
        n.Q = np.array(cfg["Q_imu"], dtype=np.float64)
    if "P0" in cfg:
        n.P = np.array(cfg["P0"], dtype=np.float64)
    return n


def _per_call_run(capi, cfg, tr, dtype, nf, on_frame):
    """the ASL runner's per-filter call order (asl_msckf.cpp:227-294) on capi.MSCKF; on_frame(k, filter) after every image"""
    st = tr.stream()
    f = capi.MSCKF(dtype, n_cap=24, f_cap=128, m_cap=24)
    f.initialize(cfg, tr.imu0)
    sid = 0
    for k in range(nf):
        for rd in tr.imu_for_frame(k):
            f.propagate(rd)
        sid += len(tr.imu_for_frame(k))
        f.augmentState(sid, tr.frame_times[k])
        f.update(*st[k]["cur"]); f.addFeatures(*st[k]["new"])
        f.marginalize(); f.pruneEmptyStates()
        on_frame(k, f)
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_per_call_filter_with_full_matrices_matches_the_twin(capi, npo, prec):
    """initialize_full, then 30 images of propagate / augmentState / update / addFeatures / marginalize / pruneEmptyStates:
    state and covariance against the numpy twin holding the same whole Q_imu and initial_imu_covar, after every image.  The
    same run with only the diagonal of Q_imu is far off the twin (the feature is what closes the gap)."""
    N, F, nf = 10, 16, 30
    dtype, tol = (capi.F64, 1e-6) if prec == "f64" else (capi.F32, 1e-3)
    cfg = full_config(N)
    tr = sc.Trajectory(2, 31, N, F, nf, cfg=cfg)
    st = tr.stream()
    n = twin(npo, cfg, tr.imu0)
    ref = []
    sid = 0
    for k in range(nf):
        for rd in tr.imu_for_frame(k):
            n.propagate(rd)
        sid += len(tr.imu_for_frame(k))
        n.augment(sid); n.update(*st[k]["cur"]); n.add_features(*st[k]["new"]); n.marginalize(); n.prune_empty()
        ref.append((n.imu29(), n.cam_array(), n.P.copy()))
    worst = [0.0, 0.0]

    def check(which):
        def on_frame(k, f):
            e = H.state_errors(f.getImuState(), ref[k][0], f.getCamStates()[0], ref[k][1], f.getCovariance(), ref[k][2])
            worst[which] = max(worst[which], H.worst(e))
            if which == 0:
                assert f.getNumCamStates() == len(ref[k][1]), k
                assert H.worst(e) < tol, (k, e)
        return on_frame

    _per_call_run(capi, cfg, tr, dtype, nf, check(0))
    _per_call_run(capi, without(cfg, "Q_imu"), tr, dtype, nf, check(1))    # whole P0, diagonal Q_imu
    assert worst[0] < tol and worst[1] > 1e-2, worst


@pytest.mark.gpu
def test_process_noise_term_is_linear_in_q(capi):
    """Propagation only (with two augmentations, so that P_IC is carried too), double: P(Q) - P(0) is linear in Q, so with Q_d
    diagonal (the diagonal kernel) and Q_o only off-diagonal (the full-Q kernel)
    P(Q_d + Q_o) - P(0) = [P(Q_d) - P(0)] + [P(Q_o) - P(0)].  No oracle needed; the four filters share one mixed launch."""
    N = 8
    Qf = correlated(sc.filter_config(N)["Q_imu_diag"], 11)
    Qd, Qo = np.diag(np.diag(Qf)), Qf - np.diag(np.diag(Qf))
    base = full_config(N, seed=3)
    tr = sc.Trajectory(2, 9, N, 0, 6, cfg=base)
    bt = capi.Batch(4, N, 8, N, capi.F64)
    for b, Q in enumerate([np.zeros((12, 12)), Qd, Qo, Qf]):
        bt.initialize(b, sc.filter_config(N, Q_imu=Q, P0=base["P0"]), tr.imu0)
    for k in range(5):
        bt.propagate_range(0, 4, np.stack([tr.imu_for_frame(k)] * 4))
        if k in (1, 3):
            bt.augment_range(0, 4)
    P = [bt.covariance(b) for b in range(4)]
    for b in range(1, 4):
        assert np.array_equal(bt.imu_state(b), bt.imu_state(0)) and np.array_equal(bt.cam_states(b)[0], bt.cam_states(0)[0])
    lhs, rhs = P[3] - P[0], (P[1] - P[0]) + (P[2] - P[0])
    assert np.linalg.norm(P[2] - P[0]) > 1e-2 * np.linalg.norm(P[1] - P[0])     # the off-diagonal part does move P
    assert np.linalg.norm(lhs - rhs) < 1e-12 * np.linalg.norm(P[3]), np.linalg.norm(lhs - rhs) / np.linalg.norm(P[3])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_zero_off_diagonals_give_the_diagonal_filter_bit_for_bit(capi, dtype_name):
    """initialize_full with diagonal matrices is msckf_hip_initialize on their diagonals: same code path, same bits."""
    N, F, nf = 8, 20, 14
    dtype = getattr(capi, dtype_name)
    cfg = sc.filter_config(N)
    cfgm = sc.filter_config(N, Q_imu=np.diag(cfg["Q_imu_diag"]), P0=np.diag(cfg["P0_diag"]))
    tr = sc.Trajectory(2, 44, N, F, nf, cfg=cfg)
    bt = capi.Batch(2, N, F, N, dtype)
    bt.initialize(0, cfg, tr.imu0)
    bt.initialize(1, cfgm, tr.imu0)
    for k in range(nf):
        for b in range(2):
            H.device_frame(bt, b, tr, k, N)
        assert np.array_equal(bt.imu_state(0), bt.imu_state(1)), k
        assert np.array_equal(bt.cam_states(0)[0], bt.cam_states(1)[0]), k
        assert np.array_equal(bt.covariance(0), bt.covariance(1)), k


MIX = dict(N=10, F=24, nf=16, B=8)


def _mixed_trajs(diag_even=False):
    """even b: whole Q_imu / P0 (each its own), odd b: diagonal; diag_even: the even ones with only their diagonals"""
    c = MIX
    out = []
    for b in range(c["B"]):
        cf = full_config(c["N"], seed=100 + b)
        tr = sc.Trajectory(2, 50 + b, c["N"], c["F"], c["nf"], cfg=cf if b % 2 == 0 else None)
        if b % 2 == 0 and diag_even:
            tr.cfg = without(cf, "Q_imu", "P0")
        out.append(tr)
    return out


def _snap(bt, b):
    return bt.imu_state(b), bt.cam_states(b)[0], bt.covariance(b)


def _same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


@pytest.mark.gpu
def test_mixed_batch_routes_per_trajectory(capi):
    """B = 8, even trajectories with a whole Q_imu, odd ones diagonal, through propagate_range (+ augment / marginalize /
    prune ranges), run_frames (3 streams: every slice mixed; 8 streams: one trajectory per slice) and image_cycle_range.  The odd
    trajectories are bit-identical to an all-diagonal batch, the even ones to the same filters driven one by one."""
    c = MIX
    N, F, nf, B = c["N"], c["F"], c["nf"], c["B"]
    trs, trd = _mixed_trajs(), _mixed_trajs(diag_even=True)
    even, odd = range(0, B, 2), range(1, B, 2)

    def ranged(ts):
        bt = capi.Batch(B, N, F, N, capi.F32)
        for b, tr in enumerate(ts):
            bt.initialize(b, tr.cfg, tr.imu0)
        for k in range(nf):
            bt.propagate_range(0, B, np.stack([tr.imu_for_frame(k) for tr in ts]))
            bt.augment_range(0, B)
            for b, tr in enumerate(ts):
                fr = tr.frames[k]
                bt.set_tracks(b, fr["M"], fr["slots"], fr["obs"])
            bt.marginalize_range(0, B)
            if bt.num_cam_states(0) == N:
                bt.drop_oldest_range(0, B, 1)
        return bt

    def resident(ts, streams):
        bt = capi.Batch(B, N, F, N, capi.F32)
        for b, tr in enumerate(ts):
            bt.initialize(b, tr.cfg, tr.imu0)
        bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
        for k in range(nf):
            for b, tr in enumerate(ts):
                fr = tr.frames[k]
                bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
        bt.scenario_commit()
        bt.set_streams(streams)
        bt.run_frames(0, nf); bt.sync()
        return bt

    one = capi.Batch(B, N, F, N, capi.F32)
    for b in even:
        one.initialize(b, trs[b].cfg, trs[b].imu0)
        for k in range(nf):
            H.device_frame(one, b, trs[b], k, N)
    per_call = {b: _snap(one, b) for b in even}
    for run in (ranged, lambda ts: resident(ts, 3), lambda ts: resident(ts, 8)):
        mix, dg = run(trs), run(trd)
        for b in odd:
            assert _same(_snap(mix, b), _snap(dg, b)), b
        for b in even:
            assert _same(_snap(mix, b), per_call[b]), b
            assert not np.array_equal(mix.covariance(b), dg.covariance(b)), b
        mix.close(); dg.close()
    one.close()

    # image_cycle_range: the per-image cycle in lockstep vs the per-filter calls
    sts = [tr.stream() for tr in trs]
    big, dg, one = capi.Batch(B, 24, 64, 24, capi.F32), capi.Batch(B, 24, 64, 24, capi.F32), capi.Batch(B, 24, 64, 24, capi.F32)
    for b in range(B):
        big.initialize(b, trs[b].cfg, trs[b].imu0); dg.initialize(b, trd[b].cfg, trd[b].imu0); one.initialize(b, trs[b].cfg, trs[b].imu0)
    for k in range(nf):
        rd = np.stack([tr.imu_for_frame(k) for tr in trs])
        args = ([k] * B, [tr.frame_times[k] for tr in trs], [sts[b][k]["cur"] for b in range(B)], [sts[b][k]["new"] for b in range(B)])
        big.propagate_range(0, B, rd); big.image_cycle_range(0, B, *args)
        dg.propagate_range(0, B, np.stack([tr.imu_for_frame(k) for tr in trd])); dg.image_cycle_range(0, B, *args)
        for b in even:
            one.propagate_range(b, 1, trs[b].imu_for_frame(k))
            one.augment_state(b, k, trs[b].frame_times[k])
            one.update(b, *sts[b][k]["cur"]); one.add_features(b, *sts[b][k]["new"])
            one.marginalize(b); one.prune_redundant_states(b); one.prune_empty_states(b)
        for b in odd:
            assert _same(_snap(big, b), _snap(dg, b)), ("image_cycle_range", k, b)
        for b in even:
            assert _same(_snap(big, b), _snap(one, b)), ("image_cycle_range", k, b)
    big.close(); dg.close(); one.close()


@pytest.mark.gpu
def test_copies_carry_q_and_bad_matrices_are_refused(capi):
    N, F, nf = 8, 16, 10
    cfg = full_config(N, seed=21)
    tr = sc.Trajectory(2, 61, N, F, nf, cfg=cfg)
    src, dst = capi.Batch(2, N, F, N, capi.F64), capi.Batch(2, N, F, N, capi.F64)
    src.initialize(0, cfg, tr.imu0); src.initialize(1, without(cfg, "Q_imu"), tr.imu0)
    dst.initialize(0, without(cfg, "Q_imu"), tr.imu0); dst.initialize(1, cfg, tr.imu0)   # the opposite flags before the copy
    for k in range(3):
        for b in range(2):
            H.device_frame(src, b, tr, k, N)
    dst.copy_state_from(src)
    for k in range(3, nf):
        for bt in (src, dst):
            for b in range(2):
                H.device_frame(bt, b, tr, k, N)
    for b in range(2):
        assert _same(_snap(src, b), _snap(dst, b)), b
    assert not np.array_equal(src.covariance(0), src.covariance(1))
    # capi.MSCKF.copy goes through the same entry
    f = capi.MSCKF(capi.F64, n_cap=N, f_cap=F, m_cap=N)
    f.initialize(cfg, tr.imu0); f.propagate(tr.imu_for_frame(0))
    g = f.copy()
    for x in (f, g):
        x.propagate(tr.imu_for_frame(1)); x.augmentState(1)
    assert np.array_equal(f.getCovariance(), g.getCovariance()) and np.array_equal(f.getImuState(), g.getImuState())

    # a later plain initialize of the same b drops the full Q_imu
    a, d = capi.Batch(1, N, F, N, capi.F64), capi.Batch(1, N, F, N, capi.F64)
    a.initialize(0, cfg, tr.imu0); a.initialize(0, without(cfg, "Q_imu", "P0"), tr.imu0)
    d.initialize(0, without(cfg, "Q_imu", "P0"), tr.imu0)
    for k in range(4):
        H.device_frame(a, 0, tr, k, N); H.device_frame(d, 0, tr, k, N)
    assert _same(_snap(a, 0), _snap(d, 0))

    # only the symmetric part of Q_imu is kept: the upper triangle doubled and the lower one zero is the same Q
    Q = np.asarray(cfg["Q_imu"])
    Qa = np.triu(Q, 1) * 2 + np.diag(np.diag(Q))
    s1, s2 = capi.Batch(1, N, F, N, capi.F64), capi.Batch(1, N, F, N, capi.F64)
    s1.initialize(0, cfg, tr.imu0)
    s2.initialize(0, dict(cfg, Q_imu=Qa), tr.imu0)
    for k in range(4):
        H.device_frame(s1, 0, tr, k, N); H.device_frame(s2, 0, tr, k, N)
    assert _same(_snap(s1, 0), _snap(s2, 0))

    # refused: asymmetric initial_imu_covar, non-finite entries
    P0 = np.array(cfg["P0"]); P0[2, 7] *= 1.001
    Qn = np.array(cfg["Q_imu"]); Qn[4, 1] = np.nan
    for bad, what in ((dict(cfg, P0=P0), "symmetric"), (dict(cfg, Q_imu=Qn), "non-finite")):
        with pytest.raises(capi.HipError) as ei:
            s1.initialize(0, bad, tr.imu0)
        assert "(-22)" in str(ei.value) and what in str(ei.value)
    for x in (src, dst, a, d, s1, s2):
        x.close()


@pytest.mark.gpu
def test_shim_with_full_matrix_members_matches_the_twin(tmp_path, npo):
    """tests/cpp/shim_full_noise.cpp: the Eigen-free shim with Q_imu / initial_imu_covar given whole, the ASL runner's call
    order, against the twin; a copy taken half-way ends bit-identical."""
    from msckf_mono_amd import capi
    exe = str(tmp_path / "shim_full_noise")
    libdir = os.path.dirname(capi.LIB_PATH)
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), SHIM_SRC, "-o", exe, "-L" + libdir,
                          "-lmsckf_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    N, F, nf = 8, 12, 14
    cfg = full_config(N, seed=31)
    tr = sc.Trajectory(2, 23, N, F, nf, cfg=cfg)
    st = tr.stream()
    cam, noise, prm = capi.pack_config(cfg)
    vals = np.concatenate([cam, noise[:2], np.asarray(cfg["Q_imu"]).ravel(), np.asarray(cfg["P0"]).ravel(), prm, tr.imu0])   # row by row
    lines = [" ".join(repr(float(x)) for x in vals), str(nf)]
    n = twin(npo, cfg, tr.imu0)
    sid = 0
    for k in range(nf):
        rd = tr.imu_for_frame(k)
        lines.append(str(len(rd)) + " " + " ".join(repr(float(x)) for x in rd.ravel()))
        for kind in ("cur", "new"):
            obs, ids = st[k][kind]
            lines.append(str(len(ids)) + " " + " ".join("%r %r %d" % (float(z[0]), float(z[1]), i) for z, i in zip(obs, ids)))
        for r in rd:
            n.propagate(r)
        sid += len(rd)
        n.augment(sid); n.update(*st[k]["cur"]); n.add_features(*st[k]["new"]); n.marginalize(); n.prune_empty()
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stderr)
    rows = run.stdout.strip().splitlines()
    imu = np.array([float(x) for x in rows[0].split()])
    ncam = int(rows[1])
    P = np.array([float(x) for x in rows[2].split()])
    D = 15 + 6 * ncam
    assert ncam == len(n.cams) and P.size == D * D
    P = P.reshape(D, D, order="F")
    ref = n.imu29()
    assert H.quat_angle(imu[:4], ref[:4]) < 1e-6 and H.rel(imu[4:16], ref[4:16]) < 1e-6
    assert H.rel(P, n.P, 1e-30) < 1e-6
    assert rows[3].strip() == "1"
