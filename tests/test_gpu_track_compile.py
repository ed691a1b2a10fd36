"""Compiled recordings on the device: the lab recordings A-D (tests/compile_lab.py) compiled on the host (capi.TrackCompiler),
staged through asl.stage_scenario / asl.stage_replay and run by the three frame loops, against the double oracle driven by ids
in asl.run's call order (no pruneRedundantStates).

Handles of B = 3: two seeds of one recording and one of another -- (A, A, B) and (C, C, D) -- so that the trajectories'
sequences differ in length (the shorter one's last frames are skipped cells) and in tracks per image.

  1. double: ONE run_frames call with the frame log on; every record against the free-running oracle at 1e-6 (state, P_II
     diagonal, position block through helpers' conventions; window, n_tracks, passed equal; cam7 of slot 0), the full covariance
     and camera states at the end.  run_frames_streamed and run_frames_replay (all sigmas 0) give the same bits.
  2. float at 1e-3: the filter is re-seeded every image as the project's float tests are (teacher forcing, device -> oracle:
     DESIGN 3.4) -- here into the SAME double oracle, whose id bookkeeping runs on untouched; a frame-by-frame run_frames run is
     compared image by image, and the one-call runs of the three loops give its bits.
  3. the same recording through capi.MSCKF + asl.run (the per-call path) and through asl.compile_sequence + the frame loop.

Measured on an MI355X (the tests print the figures, -s): double free-running worst 1.9e-9 (b_g), full
covariance 4.2e-10; float re-seeded worst 9.7e-4 on b_g on (C, C, D), 8.3e-5 on (A, A, B), every other field below 8e-5; per-call
path against the compiled loop 8e-16 (double), 7e-7 (float)."""
import numpy as np
import pytest

import compile_lab as CL
import helpers as H
from msckf_mono_amd import asl, scenario as sc

pytestmark = pytest.mark.gpu
GROUPS = (("A", "A", "B"), ("C", "C", "D"))
SEEDS = (11, 12, 13)


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c_
    c_.lib()
    return c_


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def _cd(capi, prec):
    return capi.F64 if prec == "f64" else capi.F32


def _batch(capi, prec, names):
    bt = capi.Batch(len(names), CL.N_CAP, CL.F_CAP, CL.M_CAP, _cd(capi, prec))
    for b, n in enumerate(names):
        bt.initialize(b, CL.recording(n).cfg, CL.recording(n).imu0)
    return bt


def _stage_replay(bt, names):
    """the distinct recordings of `names` as sequences (asl.stage_replay), trajectory b on its recording's with seed SEEDS[b] and
    no noise at all"""
    seqs = sorted(set(names))
    nf = max(len(CL.compiled(n)) for n in seqs)
    bt.replay_alloc(len(seqs), nf, CL.K)
    for s, n in enumerate(seqs):
        asl.stage_replay(bt, CL.as_compiled(n), s)
        for f in range(len(CL.compiled(n)), nf):
            bt.replay_set_cell(f, s, np.zeros((0, 7)), [], [], np.zeros((0, 2)), 0, skip=True)
    bt.replay_assign([seqs.index(n) for n in names], SEEDS[:len(names)], (0.0, 0.0, 0.0, 0.0))
    bt.replay_commit()
    return nf


def _logged(capi, prec, names, loop):
    """one call of `loop` over the staged recordings with the frame log on: (records [nf][B][48], snapshots)"""
    bt = _batch(capi, prec, names)
    nf = _stage_replay(bt, names) if loop == "run_frames_replay" else CL.stage_scenario(bt, names)
    bt.frame_log_enable(nf)
    getattr(bt, loop)(0, nf)
    bt.sync()
    assert bt.frame_log_count() == nf
    out = bt.frame_log_read()[0], [H.snapshot(bt, b, strict=False) for b in range(bt.B)]
    bt.close()
    return out


def _record_errors(rec, o):
    """helpers.state_errors' conventions on what a frame-log record holds (as tests/test_gpu_frame_log.py reads it), and cam7 of slot 0"""
    imu, P, cams = o.getImuState(), o.getCovariance(), o.getCamStates()[0]
    ppp = np.array([P[12, 12], P[12, 13], P[12, 14], P[13, 13], P[13, 14], P[14, 14]])
    err = dict(q=H.quat_angle(rec[0:4], imu[0:4]), bg=H.rel(rec[4:7], imu[4:7]), v=H.rel(rec[7:10], imu[7:10]),
               ba=H.rel(rec[10:13], imu[10:13]), p=H.rel(rec[13:16], imu[13:16]),
               Pii_diag=H.rel(rec[16:31], np.diag(P)[:15], 1e-30), Ppp=H.rel(rec[31:37], ppp, 1e-30))
    if len(cams):
        err["cam0_q"], err["cam0_p"] = H.quat_angle(rec[41:45], cams[0, :4]), H.rel(rec[45:48], cams[0, 4:7])
    return err


def _check_record(rec, o, n_tracks, tol, where, worst):
    so = o.lastStats()
    assert rec[37] == o.getNumCamStates(), where
    assert (rec[38], rec[39]) == ((so["n_tracks"], so["n_passed"]) if n_tracks else (0, 0)), (where, so)
    err = _record_errors(rec, o)
    for key, val in err.items():
        worst[key] = max(worst.get(key, 0.0), val)
    assert H.worst(err) < tol, (where, err)


def _final_errors(snap, o):
    return H.state_errors(snap[0], o.getImuState(), snap[1], o.getCamStates()[0], snap[2], o.getCovariance())


def _same_runs(x, y, where):
    assert np.array_equal(x[0], y[0]), where
    for b, (p, q) in enumerate(zip(x[1], y[1])):
        assert H.same_bits(p, q), (where, b)


# ------------------------------------------------------------------------------------------------ 1. double, free-running
@pytest.mark.parametrize("names", GROUPS, ids=["AAB", "CCD"])
def test_compiled_recordings_double_against_the_id_driven_oracle(capi, po, names):
    log, snaps = _logged(capi, "f64", names, "run_frames")
    worst, passed = {}, 0
    for b in (0, 2):
        rec, cells = CL.recording(names[b]), CL.compiled(names[b])
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(rec.cfg, rec.imu0)
        for k, im in enumerate(rec.images):
            n0, n1 = CL.id_driven_frame(o, im)
            assert (n0, n0 - n1) == (cells[k]["window"], cells[k]["n_drop"])
            _check_record(log[k, b], o, len(cells[k]["M"]), 1e-6, (names[b], k), worst)
            passed += int(log[k, b, 39])
        for k in range(len(rec.images), log.shape[0]):                   # the skipped cells behind the recording's end change nothing
            assert np.array_equal(log[k, b, :38], log[len(rec.images) - 1, b, :38]), (names[b], k)
        fin = _final_errors(snaps[b], o)
        worst["P"] = max(worst.get("P", 0.0), fin["P"])
        assert H.worst(fin) < 1e-6 and snaps[b][3] == o.getNumCamStates(), (names[b], fin)
    assert passed > 100
    assert np.array_equal(log[:len(CL.compiled(names[0])), 0], log[:len(CL.compiled(names[0])), 1])    # two copies of one recording
    print("compiled %s, f64 free-running, worst:" % "".join(names), {k: "%.2e" % x for k, x in worst.items()})
    for loop in ("run_frames_streamed", "run_frames_replay"):
        _same_runs(_logged(capi, "f64", names, loop), (log, snaps), loop)


# ------------------------------------------------------------------------------------------------ 2. float, teacher-forced
@pytest.mark.parametrize("names", GROUPS, ids=["AAB", "CCD"])
def test_compiled_recordings_float_against_the_id_driven_oracle(capi, po, names):
    step = _batch(capi, "f32", names)
    nf = CL.stage_scenario(step, names)
    step.frame_log_enable(nf)
    oracles = {}
    for b in (0, 2):
        oracles[b] = po.Oracle(po.F64, po.LEAN)
        oracles[b].initialize(CL.recording(names[b]).cfg, CL.recording(names[b]).imu0)
    worst, passed = {}, 0
    for k in range(nf):
        live = [b for b in (0, 2) if k < len(CL.recording(names[b]).images)]
        for b in live:
            assert step.num_cam_states(b) == oracles[b].getNumCamStates()
            H.copy_device_to_oracle(step, b, oracles[b])                 # numbers only: the oracle's tracks and ids stay its own
        step.run_frames(k, k + 1)
        step.sync()
        for b in live:
            cell = CL.compiled(names[b])[k]
            CL.id_driven_frame(oracles[b], CL.recording(names[b]).images[k])
            rec = step.frame_log_read(k, 1, b, 1)[0][0, 0]
            _check_record(rec, oracles[b], len(cell["M"]), 1e-3, (names[b], k), worst)
            passed += int(rec[39])
            if k == len(CL.recording(names[b]).images) - 1:
                fin = _final_errors(H.snapshot(step, b, strict=False), oracles[b])
                assert H.worst(fin) < 1e-3, (names[b], fin)
    assert passed > 100
    got = step.frame_log_read()[0], [H.snapshot(step, b, strict=False) for b in range(step.B)]
    step.close()
    print("compiled %s, f32 teacher-forced, worst:" % "".join(names), {k: "%.2e" % x for k, x in worst.items()})
    for loop in ("run_frames", "run_frames_streamed", "run_frames_replay"):
        _same_runs(_logged(capi, "f32", names, loop), got, loop)


# ------------------------------------------------------------------------------------------------ 3. the per-call path
def _dataset(rec):
    """the recording as the dict asl.read_dataset returns: one IMU sample per 5 ms, an image stamped with its last sample, ground
    truth that makes asl.initial_state the recording's imu0"""
    rd = np.concatenate([im["readings"] for im in rec.images])
    imu_t = (np.arange(len(rd), dtype=np.int64) + 1) * 5_000_000
    ends = np.cumsum([len(im["readings"]) for im in rec.images])
    cam_t = imu_t[ends - 1]
    s = rec.imu0
    gt = dict(t=np.array([0], dtype=np.int64), q_IG=s[None, 0:4], b_g=s[None, 4:7], v=s[None, 7:10], b_a=s[None, 10:13], p=s[None, 13:16])
    tracks = {int(t): dict(cur=(im["cur"][0].tolist(), [int(i) for i in im["cur"][1]]), new=(im["new"][0].tolist(), [int(i) for i in im["new"][1]]))
              for t, im in zip(cam_t, rec.images)}
    return dict(imu_t=imu_t, readings=rd, cam_t=cam_t, gt=gt, tracks=tracks)


@pytest.mark.parametrize("prec,tol", [("f64", 1e-6), ("f32", 1e-3)])
@pytest.mark.parametrize("name", ["A", "B"])
def test_the_per_call_path_and_the_compiled_frame_loop_agree(capi, name, prec, tol):
    """capi.MSCKF driven by asl.run(prune_redundant=False) against asl.compile_sequence + asl.stage_scenario + run_frames on the
    same dataset: the same window size and gate counts on every image, states within the bars, the same covariance at the end"""
    rec = CL.recording(name)
    ds = _dataset(rec)
    assert np.array_equal(asl.initial_state(ds), rec.imu0)
    flt = capi.MSCKF(_cd(capi, prec), CL.N_CAP, CL.F_CAP, CL.M_CAP)
    per = []
    out = asl.run(ds, flt, rec.cfg, on_frame=lambda t, s: per.append((flt.getNumCamStates(), flt.batch.last_stats(0, strict=False))))
    comp = asl.compile_sequence(ds, rec.cfg)
    assert len(comp["images"]) == len(out) == len(rec.images)
    for cell, want in zip(comp["images"], CL.compiled(name)):
        assert all(np.array_equal(cell[key], want[key]) for key in ("M", "slots", "obs", "ids")) and cell["n_drop"] == want["n_drop"]
    assert comp["K"] <= CL.K and comp["n_cap"] <= CL.N_CAP and comp["f_cap"] <= CL.F_CAP and comp["m_cap"] <= CL.M_CAP
    bt = capi.Batch(1, CL.N_CAP, CL.F_CAP, CL.M_CAP, _cd(capi, prec))
    bt.initialize(0, rec.cfg, rec.imu0)
    nf = len(comp["images"])
    bt.scenario_alloc(nf, comp["K"])
    asl.stage_scenario(bt, comp, 0, comp["K"])
    bt.scenario_commit()
    bt.frame_log_enable(nf)
    bt.run_frames(0, nf)
    bt.sync()
    log = bt.frame_log_read()[0][:, 0]
    worst = 0.0
    for k, ((stamp, s), (n_cam, st), cell) in enumerate(zip(out, per, comp["images"])):
        assert stamp == cell["stamp"] and log[k, 37] == n_cam == cell["window"] - cell["n_drop"], k
        if len(cell["M"]):
            assert (log[k, 38], log[k, 39]) == (st["n_tracks"], st["n_passed"]), (k, st)
        err = max(H.quat_angle(log[k, 0:4], s[0:4]), H.rel(log[k, 4:7], s[4:7]), H.rel(log[k, 7:10], s[7:10]), H.rel(log[k, 10:13], s[10:13]), H.rel(log[k, 13:16], s[13:16]))
        worst = max(worst, err)
        assert err < tol, (k, err)
    fin = H.state_errors(bt.imu_state(0), flt.getImuState(), bt.cam_states(0)[0], flt.getCamStates()[0], bt.covariance(0), flt.getCovariance())
    assert H.worst(fin) < tol, fin
    print("per-call path against the compiled frame loop (%s, %s): worst %.2e, at the end %.2e" % (name, prec, worst, H.worst(fin)))
    bt.close()
