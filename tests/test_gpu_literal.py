"""Anisotropic pixel noise (u_var' != v_var', the configuration both shipped callers run: asl_msckf.cpp:77-78) on the
device's LITERAL route (default): R_o_j = A_j^T R_j A_j per track, HouseholderQR of the stack in the reference's row and
column order with the zero-tail rule, R_n = Q_1^T R_o Q_1 (msckf.h:423-431, 1343-1366; kernels_literal.hip).

Held against (1) the oracle's restatement of the same lines with the same zero-tail tolerance -- 1e-6 in double on state
AND covariance, biases included -- and (2) the reference's own source under its two roundings (lib_ref.so, lib_ref_alt.so),
whose mutual distance is the only yardstick the reference offers for the biases there (tests/test_ref_vs_oracle.py)."""
import numpy as np
import pytest

import helpers as H
import literal_lab as LL
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def _errs(bt, b, r):
    return H.state_errors(bt.imu_state(b), r.getImuState(), bt.cam_states(b)[0], r.getCamStates()[0], bt.covariance(b), r.getCovariance())


def _oerrs(a, b):
    return H.state_errors(a.getImuState(), b.getImuState(), a.getCamStates()[0], b.getCamStates()[0], a.getCovariance(), b.getCovariance())


def _force(dst, src):
    cams, _ = src.getCamStates()
    dst.setCovariance(src.getCovariance()); dst.setImuState(src.getImuState())
    for i, c in enumerate(cams):
        dst.setCamPose(i, c)
    dst.setNumResidualized(src.numResidualized())


def _aniso(N, F, nf, traj, cfgid=2):
    cfg = sc.filter_config(N, isotropic=False)
    cfg["translation_threshold"] = 0.01
    assert cfg["u_var_prime"] != cfg["v_var_prime"]
    return sc.Trajectory(cfgid, traj, N, F, nf, cfg=cfg)


@pytest.mark.parametrize("N,F,nf,traj", [(8, 24, 14, 5), (8, 24, 14, 6), (10, 50, 16, 7), (6, 6, 12, 3)])
def test_literal_route_double_vs_restatement_every_frame(capi, po, N, F, nf, traj):
    """free-running, double: device (literal, default tolerance 1e-10; the compact route: no stack) vs the restatement with
    the same tolerance, 1e-6 on every field after every frame; the kept rows of R agree (msckf.h:1347).  Trajectory 6 has an
    update whose stack has a dependent column in the middle of the sweep, (6, 6) stacks with fewer rows than columns."""
    tr = _aniso(N, F, nf, traj)
    o = po.Oracle(po.F64, po.LEAN); o.setTinyRowTol(1e-10); o.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N, F, max(N, 4), capi.F64); bt.initialize(0, tr.cfg, tr.imu0)
    updates = 0
    handed = 0
    for k in range(nf):
        H.oracle_frame(o, tr, k, N); H.device_frame(bt, 0, tr, k, N)
        e = _errs(bt, 0, o)
        assert H.worst(e) < 1e-6, (k, e)
        assert H.cov_scaled_err(bt.covariance(0), o.getCovariance()) < 1e-6, k       # entry by entry: the norm above cannot see a wrong block
        if o.lastStats()["m_rows"]:
            info = bt.literal_info(0)
            assert info["m_rows"] == o.lastStats()["m_rows"] and info["kept_rows"] == o.lastStats()["r_rows"] and info["route"] == 3, (k, info, o.lastStats())
            updates += 1
            handed = max(handed, info["kept_handed_through_rows"])
    assert updates >= nf - 4
    # the basis of range(Q_1) then holds Q columns of rows that a dependent column handed through (literal_core.h: q_h), not only
    # kept unit vectors and reflected columns: these two scenarios must exercise that path
    if traj in (6, 3):
        assert handed > 0
    bt.close()


def test_literal_general_route_alone_on_the_device(capi, po, monkeypatch):
    """MSCKF_HIP_LITERAL_ROUTE=1: the reflector sweep over the dense stack (the definition: literal_general) instead of the
    default compact route, against the restatement at 1e-6 like the default above."""
    monkeypatch.setenv("MSCKF_HIP_LITERAL_ROUTE", "1")
    N, F, nf = 10, 50, 16
    tr = _aniso(N, F, nf, 7)
    o = po.Oracle(po.F64, po.LEAN); o.setTinyRowTol(1e-10); o.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N, F, N, capi.F64); bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(nf):
        H.oracle_frame(o, tr, k, N); H.device_frame(bt, 0, tr, k, N)
        assert H.worst(_errs(bt, 0, o)) < 1e-6, (k, _errs(bt, 0, o))
        if o.lastStats()["m_rows"]:
            info = bt.literal_info(0)
            assert info["route"] == 2 and info["kept_rows"] == o.lastStats()["r_rows"]
    bt.close()


def test_a_copy_takes_the_literal_route_over_or_refuses(capi, monkeypatch):
    """msckf_hip_copy_state hands the source's literal route (MSCKF_HIP_LITERAL_ROUTE at ITS creation) to the copy.  A destination
    without literal work space allocates it for that route and continues bit for bit (literal_info: route 2 = the sweep over the
    dense stack, 3 = the compact route).  The dense stack is only allocated for route 1, and a copy does not reallocate: a
    destination whose work space exists without it refuses a source on route 1 (-EINVAL) and stays as it was; the other way
    round it adopts the compact route."""
    N, F, nf = 8, 24, 8
    tr = _aniso(N, F, nf, 5)
    make = lambda: capi.Batch(1, N, F, N, capi.F64)
    monkeypatch.setenv("MSCKF_HIP_LITERAL_ROUTE", "1")
    a = make(); a.initialize(0, tr.cfg, tr.imu0)
    monkeypatch.delenv("MSCKF_HIP_LITERAL_ROUTE")
    fresh = make()                                            # never initialised: no literal work space yet
    used = make(); used.initialize(0, tr.cfg, tr.imu0)        # anisotropic noise: work space of the compact route
    for k in range(5):
        H.device_frame(a, 0, tr, k, N)
    assert a.literal_info(0)["route"] == 2 and a.literal_info(0)["m_rows"] > 0
    fresh.copy_state_from(a)
    with pytest.raises(capi.HipError, match=r"\(-22\): copy_state: handles differ in shape or dtype"):
        used.copy_state_from(a)
    for k in range(5, nf):
        H.device_frame(a, 0, tr, k, N); H.device_frame(fresh, 0, tr, k, N)
    assert fresh.literal_info(0)["route"] == 2 and fresh.literal_info(0)["m_rows"] > 0
    assert H.same_bits(H.snapshot(fresh, 0), H.snapshot(a, 0))
    a.copy_state_from(used)                                   # the refused destination is untouched: still at its initial state
    for k in range(5):
        H.device_frame(a, 0, tr, k, N); H.device_frame(used, 0, tr, k, N)
    assert a.literal_info(0)["route"] == 3 and used.literal_info(0)["route"] == 3 and a.literal_info(0)["m_rows"] > 0
    assert H.same_bits(H.snapshot(a, 0), H.snapshot(used, 0))
    for bt in (a, fresh, used):
        bt.close()


def test_literal_route_float_vs_restatement(capi, po):
    N, F, nf = 10, 50, 16
    tr = _aniso(N, F, nf, 7)
    o = po.Oracle(po.F32, po.LEAN); o.setTinyRowTol(8e-4); o.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N, F, N, capi.F32); bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(nf):
        if k:
            H.copy_oracle_to_device(o, bt, 0)
        H.oracle_frame(o, tr, k, N); H.device_frame(bt, 0, tr, k, N)
        e = _errs(bt, 0, o)
        assert H.worst(e) < 1e-3, (k, e)
    bt.close()


def _ref_at(po, tr, teacher, impl):
    r = po.Oracle(po.F64, impl=impl)
    r.initialize(tr.cfg, tr.imu0)
    while r.getNumCamStates() < teacher.getNumCamStates():
        r.augmentState(r.getNumCamStates(), 0.0)
    _force(r, teacher)
    return r


@pytest.mark.parametrize("tol", [-1.0, 0.0])
def test_literal_route_vs_reference_source_two_roundings(capi, po, tol):
    """Teacher-forced, double, over 4 trajectories x ~12 updates: device vs lib_ref.so and lib_ref_alt.so.  Everything
    observable (q, v, p, P, camera poses) at 2e-6; the biases measured in units of the distance between the reference's two
    roundings on the same update: the median ratio stays near 1 (the device is as close to either rounding as they are to
    each other), with the pre-whitened route at ~5x for comparison (tests/test_gpu_vs_reference.py holds that one to 10x).
    tol = 0: msckf.h's zero-tail rule to the letter (the device's own rounding noise picks the gauge rows)."""
    N, F, nf = 8, 24, 14
    ratios = {"bg": [], "ba": []}
    worst = {}
    for traj in (5, 6, 7, 8):
        tr = _aniso(N, F, nf, traj)
        teacher = po.Oracle(po.F64, po.LEAN); teacher.setTinyRowTol(1e-10); teacher.initialize(tr.cfg, tr.imu0)
        bt = capi.Batch(1, N, F, N, capi.F64); bt.set_anisotropic_noise(0, tol); bt.initialize(0, tr.cfg, tr.imu0)
        for k in range(nf):
            if k == 0:
                H.oracle_frame(teacher, tr, k, N); H.device_frame(bt, 0, tr, k, N)
                continue
            a, b = _ref_at(po, tr, teacher, "ref"), _ref_at(po, tr, teacher, "ref_alt")
            H.copy_oracle_to_device(teacher, bt, 0)
            H.oracle_frame(teacher, tr, k, N); H.device_frame(bt, 0, tr, k, N)
            if teacher.lastStats()["n_motion_rejected"] > 0 or teacher.lastStats()["m_rows"] == 0:
                continue
            H.oracle_frame(a, tr, k, N); H.oracle_frame(b, tr, k, N)
            mutual = _oerrs(a, b)
            ea, eb = _errs(bt, 0, a), _errs(bt, 0, b)
            for key in ("q", "v", "p", "P", "Pii", "cam_q", "cam_p"):
                worst[key] = max(worst.get(key, 0.0), ea[key], eb[key])
            for key in ("bg", "ba"):
                if mutual[key] > 1e-7:
                    ratios[key].append(max(ea[key], eb[key]) / mutual[key])
        bt.close()
    for key, v in worst.items():
        assert v < 2e-6, (key, worst)
    for key in ("bg", "ba"):
        r = np.array(ratios[key])
        assert len(r) >= 30
        assert np.median(r) < 1.5 and np.percentile(r, 90) < 4.0, (key, np.median(r), np.percentile(r, 90), r.max())


def test_literal_route_cfg3_window_float(capi, po):
    """30-camera window, 200 tracks (BASELINE configs[2] geometry, cfg4's noise), float: two steady-state updates against
    the float restatement (explicit Q_1 of a ~5 800-row stack on the CPU), teacher-forced, 1e-3."""
    N, F, nf = 30, 200, 33
    tr = _aniso(N, F, nf, 0, cfgid=3)
    fast = po.Oracle(po.F32, po.GRAM); fast.setWhiten(True); fast.initialize(tr.cfg, tr.imu0)     # brings the window to steady state cheaply
    bt = capi.Batch(1, N, F, 32, capi.F32); bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(nf - 2):
        H.oracle_frame(fast, tr, k, N)
    o = po.Oracle(po.F32, po.LEAN); o.setTinyRowTol(8e-4); o.initialize(tr.cfg, tr.imu0)
    while o.getNumCamStates() < fast.getNumCamStates():
        o.augmentState(o.getNumCamStates(), 0.0)
    _force(o, fast)
    bt2 = bt
    for _ in range(fast.getNumCamStates()):
        bt2.augment_range(0, 1)
    n = 0
    for k in range(nf - 2, nf):
        H.copy_oracle_to_device(o, bt2, 0)
        H.oracle_frame(o, tr, k, N); H.device_frame(bt2, 0, tr, k, N)
        if o.lastStats()["n_motion_rejected"]:
            continue
        e = _errs(bt2, 0, o)
        assert H.worst(e) < 1e-3, (k, e)
        info = bt2.literal_info(0)
        assert info["m_rows"] == o.lastStats()["m_rows"] > 4000 and abs(info["kept_rows"] - o.lastStats()["r_rows"]) <= 2 and info["route"] == 3
        n += 1
    assert n >= 1
    bt.close()


def _frame_without_slot(fr, slot):
    """the frame's work-list without its observations in one camera slot (tracks left with fewer than three leave the list)"""
    M, sl, ob = [], [], []
    o = 0
    for m in fr["M"]:
        keep = [o + i for i in range(int(m)) if fr["slots"][o + i] != slot]
        o += int(m)
        if len(keep) >= 3:
            M.append(len(keep)); sl.extend(int(fr["slots"][i]) for i in keep); ob.extend(fr["obs"][i] for i in keep)
    out = dict(fr)
    out["M"] = np.array(M, dtype=fr["M"].dtype); out["slots"] = np.array(sl, dtype=fr["slots"].dtype); out["obs"] = np.array(ob, dtype=fr["obs"].dtype).reshape(-1, 2)
    return out


@pytest.mark.parametrize("slot,double", [(20, False), (6, False), (20, True)])
def test_literal_route_handed_through_rows_deep_in_the_sweep(capi, po, slot, double):
    """A camera state that none of the update's tracks observes: six zero columns 6 x slot steps into the sweep, whose rows are
    handed through and kept -- the part of the compact route that builds columns of Q (literal_core.h: blocked column
    operations, par_gemm4, the register-resident reflector chain, extras_products; the host build of the same code is held
    against the dense sweep in tests/test_literal_core.py).  30-camera window, 200 tracks, teacher-forced, against the
    restatement: float at 1e-3 like test_literal_route_cfg3_window_float, double at 1e-6."""
    N, F, nf = 30, 200, 33
    tr = _aniso(N, F, nf, 0, cfgid=3)
    prec, dprec, tol, bar = (po.F64, capi.F64, 1e-10, 1e-6) if double else (po.F32, capi.F32, 8e-4, 1e-3)
    fast = po.Oracle(prec, po.GRAM); fast.setWhiten(True); fast.initialize(tr.cfg, tr.imu0)
    bt = capi.Batch(1, N, F, 32, dprec); bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(nf - 2):
        H.oracle_frame(fast, tr, k, N)
    o = po.Oracle(prec, po.LEAN); o.setTinyRowTol(tol); o.initialize(tr.cfg, tr.imu0)
    while o.getNumCamStates() < fast.getNumCamStates():
        o.augmentState(o.getNumCamStates(), 0.0)
    _force(o, fast)
    for _ in range(fast.getNumCamStates()):
        bt.augment_range(0, 1)
    n = 0
    for k in range(nf - 2, nf):
        tr.frames[k] = _frame_without_slot(tr.frames[k], slot)
        H.copy_oracle_to_device(o, bt, 0)
        H.oracle_frame(o, tr, k, N); H.device_frame(bt, 0, tr, k, N)
        if o.lastStats()["n_motion_rejected"]:
            continue
        e = _errs(bt, 0, o)
        assert H.worst(e) < bar, (k, e)
        sc_err = H.cov_scaled_err(bt.covariance(0), o.getCovariance())              # entry by entry: 1e-6 in double, the lab's float bar in float
        assert sc_err < (LL.BAR_F64 if double else LL.bars("f32")[0]), (k, sc_err)
        info = bt.literal_info(0)
        assert info["m_rows"] == o.lastStats()["m_rows"] > 4000 and abs(info["kept_rows"] - o.lastStats()["r_rows"]) <= (0 if double else 2) and info["route"] == 3
        assert info["kept_handed_through_rows"] >= 6, info
        n += 1
    assert n >= 1
    bt.close()


def test_literal_route_inside_run_frames_equals_the_single_call_path(capi, po):
    """the resident-scenario path (compact work-lists, slices, prune on the downdate) runs the same literal compression: same
    bits as frame-by-frame calls"""
    N, F, nf, B = 8, 24, 12, 3
    trs = [_aniso(N, F, nf, 20 + b) for b in range(B)]
    b1 = capi.Batch(B, N, F, N, capi.F64); b2 = capi.Batch(B, N, F, N, capi.F64)
    b2.scenario_alloc(nf, sc.IMU_PER_FRAME)
    for b, tr in enumerate(trs):
        b1.initialize(b, tr.cfg, tr.imu0); b2.initialize(b, tr.cfg, tr.imu0)
        for k in range(nf):
            fr = tr.frames[k]
            b2.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
            H.device_frame(b1, b, tr, k, N)
    b2.scenario_commit()
    b2.set_streams(2)
    b2.run_frames(0, nf); b2.sync()
    for b in range(B):
        assert np.array_equal(b1.covariance(b), b2.covariance(b)) and np.array_equal(b1.imu_state(b), b2.imu_state(b))
    b1.close(); b2.close()


def test_literal_route_cfg3_window_float_vs_reference_source(capi, po):
    """BASELINE configs[3]'s geometry and noise (30-camera window, 200 tracks, EuRoC f_u != f_v) in FLOAT against the
    reference's own source under BOTH its roundings (lib_ref.so / lib_ref_alt.so: msckf.h unmodified, its full Q of a
    ~5 800-row stack, seconds per update, on host threads): SIX consecutive steady-state updates of FOUR trajectories,
    teacher-forced from the float restatement (zero-tail tolerance 8e-4, as the device).  Everything the measurements
    determine -- attitude, velocity, position, camera poses, covariance -- at the section-3.4 bar of 1e-3 against either
    rounding.  The biases, which the reference itself only defines to its rounding envelope under anisotropic noise (DESIGN
    3.3), are measured as the double test above measures them: in units of the distance between the reference's two
    roundings ON THE SAME UPDATE -- the device is as close to either as they are to each other (median ratio, 90th
    percentile) -- with a flat 2e-2 only as the outer fence; against the float restatement (a third rounding of the same
    algorithm) they are held at 1e-3 or twice that spread.  The device keeps exactly the rows the restatement keeps."""
    if not po.ref_available():
        pytest.skip("oracle/_ref/lib_ref.so not built (needs /root/reference at build time)")
    import threading
    N, F, nf, n_upd = 30, 200, 38, 6
    trs = [_aniso(N, F, nf, g, cfgid=3) for g in (0, 1, 2, 3)]
    B = len(trs)
    teachers = []
    for tr in trs:
        t = po.Oracle(po.F32, po.GRAM); t.setWhiten(True); t.initialize(tr.cfg, tr.imu0)      # cheap way to a steady-state window
        teachers.append(t)
    first = nf - n_upd
    for k in range(first):
        for t, tr in zip(teachers, trs):
            H.oracle_frame(t, tr, k, N)
    lean = []
    for t, tr in zip(teachers, trs):
        o = po.Oracle(po.F32, po.LEAN); o.setTinyRowTol(8e-4); o.initialize(tr.cfg, tr.imu0)
        while o.getNumCamStates() < t.getNumCamStates():
            o.augmentState(o.getNumCamStates(), 0.0)
        _force(o, t)
        lean.append(o)
    bt = capi.Batch(B, N, F, 32, capi.F32)
    for b, tr in enumerate(trs):
        bt.initialize(b, tr.cfg, tr.imu0)
        for _ in range(lean[b].getNumCamStates()):
            bt.augment_range(b, 1)
    env, compared, kept = {}, 0, []
    ratios = {"bg": [], "ba": []}
    for k in range(first, nf):
        refs = []
        for tr, t in zip(trs, lean):
            pair = []
            for impl in ("ref", "ref_alt"):
                r = po.Oracle(po.F32, impl=impl); r.initialize(tr.cfg, tr.imu0)
                while r.getNumCamStates() < t.getNumCamStates():
                    r.augmentState(r.getNumCamStates(), 0.0)
                _force(r, t)
                pair.append(r)
            refs.append(pair)
        for b, t in enumerate(lean):
            H.copy_oracle_to_device(t, bt, b)
        th = [threading.Thread(target=H.oracle_frame, args=(r, tr, k, N)) for pair, tr in zip(refs, trs) for r in pair]
        for x in th:
            x.start()
        for b, (t, tr) in enumerate(zip(lean, trs)):
            H.oracle_frame(t, tr, k, N); H.device_frame(bt, b, tr, k, N)
        for x in th:
            x.join()
        for b, (t, pair) in enumerate(zip(lean, refs)):
            if t.lastStats()["n_motion_rejected"] > 0:       # D1: the reference is undefined on this frame
                continue
            info = bt.literal_info(b)
            assert info["route"] == 3 and info["m_rows"] == t.lastStats()["m_rows"] > 4000
            kept.append((info["kept_rows"], t.lastStats()["r_rows"]))
            ea, eb, mutual = _errs(bt, b, pair[0]), _errs(bt, b, pair[1]), _oerrs(pair[0], pair[1])
            for key in ea:
                env[key] = max(env.get(key, 0.0), ea[key], eb[key])
            for key in ("bg", "ba"):
                if mutual[key] > 1e-6:
                    ratios[key].append(max(ea[key], eb[key]) / mutual[key])
            e2 = _errs(bt, b, t)                                # and the restatement itself: every observable field at 1e-3, the biases at
            for key, v in e2.items():                          # 1e-3 or twice the reference's own spread on this update, whichever is larger
                assert v < (max(1e-3, 2.0 * mutual[key]) if key in ("bg", "ba") else 1e-3), (k, b, key, e2, mutual)
            compared += 1
    bt.close()
    assert compared >= 10, compared
    assert all(a == b for a, b in kept), kept
    for key in ("q", "v", "p", "P", "Pii", "cam_q", "cam_p"):
        assert env[key] < 1e-3, (key, env)
    assert env["bg"] < 2e-2 and env["ba"] < 2e-2, env
    for key in ("bg", "ba"):
        r = np.array(ratios[key])
        assert len(r) >= 8, (key, r)
        assert np.median(r) < 2.0 and np.percentile(r, 90) < 5.0, (key, np.median(r), np.percentile(r, 90), r.max(), r)


def test_literal_route_batched_at_the_benchmarked_size_vs_restatement(capi, po):
    """The BATCHED literal route as bench.py --config cfg4 runs it -- 64 trajectories, 30-camera window, 200 tracks, EuRoC
    f_u != f_v, float, resident scenario, FOUR slices (streams) -- against the float restatement of msckf.h:423-431,
    1343-1366 (explicit Q_1 of a ~5 800-row stack on the CPU, zero-tail tolerance 8e-4 as the device): after the window is
    full, 8 sampled trajectories hand state + covariance to a restatement each (teacher forcing, device -> oracle), both
    run the next update on the same inputs, and every state field and the covariance agree to 1e-3, the gate's counts and
    the stacked rows exactly, the kept rows of R to the restatement's; two consecutive updates."""
    import threading
    N, F, B, nf = 30, 200, 64, 33
    trs = [_aniso(N, F, nf, 100 + b, cfgid=3) for b in range(B)]
    bt = capi.Batch(B, N, F, 32, capi.F32)
    for b, tr in enumerate(trs):
        bt.initialize(b, tr.cfg, tr.imu0)
    bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    for k in range(nf):
        for b, tr in enumerate(trs):
            fr = tr.frames[k]
            bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    bt.set_streams(4)
    k0 = nf - 2
    bt.run_frames(0, k0); bt.sync()
    sample = [0, 9, 17, 26, 35, 44, 53, 63]
    compared = 0
    for k in (k0, k0 + 1):
        oracles = {}
        for b in sample:
            o = po.Oracle(po.F32, po.LEAN); o.setTinyRowTol(8e-4)
            o.initialize(trs[b].cfg, trs[b].imu0)
            H.copy_device_to_oracle(bt, b, o)
            oracles[b] = o
        th = [threading.Thread(target=H.oracle_frame, args=(oracles[b], trs[b], k, N)) for b in sample]
        for x in th:
            x.start()
        bt.run_frames(k, k + 1); bt.sync()
        for x in th:
            x.join()
        for b in sample:
            o = oracles[b]
            so, sd = o.lastStats(), bt.last_stats(b)
            for key in ("n_tracks", "n_motion_rejected", "n_tri_rejected", "n_gate_rejected", "n_passed", "m_rows"):
                assert so[key] == sd[key], (k, b, key, so, sd)
            info = bt.literal_info(b)
            assert info["route"] == 3 and info["m_rows"] == so["m_rows"] > 4000 and abs(info["kept_rows"] - so["r_rows"]) <= 2, (k, b, info, so)
            e = _errs(bt, b, o)
            assert H.worst(e) < 1e-3, (k, b, e)
            compared += 1
    bt.close()
    assert compared == 2 * len(sample)


def test_literal_letter_rule_in_float_at_the_benchmarked_window_recorded(capi, po):
    """What the zero-tail tolerance is worth at the benchmarked window, as a number: the same float updates (30-camera window,
    200 tracks, EuRoC noise, teacher-forced from the restatement) on the device with the default tolerance 8e-4 (the
    exact-arithmetic limit of the rule, what bench.py --config cfg4 runs) and with tolerance 0 (msckf.h / Eigen's
    makeHouseholder to the letter: a tail of rounding noise is reflected along).  RECORDED, not gated: under the letter rule
    the float filter's own rounding picks the gauge rows; the distance is printed and written to
    gpurun_out/literal_tol0_float.json when that directory exists.  Held: both runs finish with finite states and the
    observable fields stay within 1e-2 of each other."""
    import json, os
    N, F, nf, n_upd = 30, 200, 36, 4
    tr = _aniso(N, F, nf, 2, cfgid=3)
    fast = po.Oracle(po.F32, po.GRAM); fast.setWhiten(True); fast.initialize(tr.cfg, tr.imu0)
    first = nf - n_upd
    for k in range(first):
        H.oracle_frame(fast, tr, k, N)
    o = po.Oracle(po.F32, po.LEAN); o.setTinyRowTol(8e-4); o.initialize(tr.cfg, tr.imu0)
    while o.getNumCamStates() < fast.getNumCamStates():
        o.augmentState(o.getNumCamStates(), 0.0)
    _force(o, fast)
    bts = []
    for tol in (-1.0, 0.0):
        bt = capi.Batch(1, N, F, 32, capi.F32); bt.set_anisotropic_noise(0, tol); bt.initialize(0, tr.cfg, tr.imu0)
        for _ in range(o.getNumCamStates()):
            bt.augment_range(0, 1)
        bts.append(bt)
    rec = []
    for k in range(first, nf):
        for bt in bts:
            H.copy_oracle_to_device(o, bt, 0)
        H.oracle_frame(o, tr, k, N)
        for bt in bts:
            H.device_frame(bt, 0, tr, k, N)
        if o.lastStats()["n_motion_rejected"] or o.lastStats()["m_rows"] == 0:
            continue
        a, z = bts
        e = H.state_errors(z.imu_state(0), a.imu_state(0), z.cam_states(0)[0], a.cam_states(0)[0], z.covariance(0), a.covariance(0))
        assert all(np.isfinite(v) for v in e.values()), e
        for key in ("q", "v", "p", "cam_q", "cam_p"):
            assert e[key] < 1e-2, (k, e)
        rec.append(dict(frame=k, kept_rows_default=a.literal_info(0)["kept_rows"], kept_rows_letter=z.literal_info(0)["kept_rows"],
                        **{key: float(v) for key, v in e.items()}))
    for bt in bts:
        bt.close()
    assert len(rec) >= 1
    print("literal route, float, N=30 / F=200: tolerance 0 (letter rule) vs 8e-4 (default), per update:", json.dumps(rec))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        json.dump(dict(what="device, literal anisotropic route, float, 30-camera window / 200 tracks: zero-tail tolerance 0 (msckf.h's rule to the letter) against "
                            "the default 8e-4, same teacher-forced updates; section-3.4 error metric per field", updates=rec), open(os.path.join(out, "literal_tol0_float.json"), "w"), indent=1)
