"""GPU parity tests at BASELINE.json's configurations and launch modes: the benched cfg3 batch (64 trajectories, 30-camera
window, 200 tracks, float) on 1/2/4/8 streams and against the oracle, the cfg5 geometry (60-camera window, 500 tracks)
against the oracle, and an ill-conditioned (low-parallax) double case on both compression routes."""
import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from msckf_mono_amd import capi as c
    c.lib()
    return c


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


# ------------------------------------------------------------------------------------------------ cfg3, the benched batch
CFG3 = dict(N=30, F=200, B=64, nf=34)


@pytest.fixture(scope="module")
def cfg3_trajs():
    c = CFG3
    return [sc.Trajectory(3, b, c["N"], c["F"], c["nf"]) for b in range(c["B"])]


def _resident_batch(capi, trajs, N, F, nf, m_cap, dtype, streams=1, route=-1):
    B = len(trajs)
    bt = capi.Batch(B, N, F, m_cap, dtype)
    if route >= 0:
        bt.set_compression(route)
    for b, tr in enumerate(trajs):
        bt.initialize(b, tr.cfg, tr.imu0)
    bt.scenario_alloc(nf, sc.IMU_PER_FRAME)
    for k in range(nf):
        for b, tr in enumerate(trajs):
            fr = tr.frames[k]
            bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    bt.set_streams(streams)
    return bt


def _snapshot(bt, B):
    return [(bt.imu_state(b), bt.cam_states(b)[0], bt.covariance(b)) for b in range(B)]


def test_cfg3_streams_give_bit_identical_results(capi, cfg3_trajs):
    """bench.py runs on several streams (threaded enqueue, one slice of the batch per stream: 3 streams = 21 / 21 / 22
    trajectories).  Trajectories are independent, so 1, 2, 3 (uneven slices), 4 and 8 streams must give BIT-identical states
    and covariances for all 64 trajectories."""
    c = CFG3
    ref = None
    for ns in (1, 2, 3, 4, 8):
        bt = _resident_batch(capi, cfg3_trajs, c["N"], c["F"], c["nf"], 32, capi.F32, streams=ns)
        bt.run_frames(0, c["nf"]); bt.sync()
        snap = _snapshot(bt, c["B"])
        stats = [bt.last_stats(b) for b in range(c["B"])]
        bt.close()
        assert all(s["n_passed"] > 150 for s in stats)
        if ref is None:
            ref = snap
            continue
        for b in range(c["B"]):
            for x, y in zip(snap[b], ref[b]):
                assert np.array_equal(x, y), (ns, b)
    # inputs uploaded per frame inside the run (msckf_hip_run_frames_streamed: compact per-frame blocks from page-locked
    # memory, copy stream, ring of staging sets; host or device-event hand-over): same bits.  A ring of 2 wraps 16 times.
    for ns, ring, mode in ((1, 6, 0), (3, 6, 0), (3, 2, 0), (2, 3, 1), (4, 4, 0)):
        bt = _resident_batch(capi, cfg3_trajs, c["N"], c["F"], c["nf"], 32, capi.F32, streams=ns)
        bt.set_upload_ring(ring, mode)
        bt.scenario_pin(0, 11)                       # explicit for the first call, on demand for the second
        bt.run_frames_streamed(0, 11); bt.run_frames_streamed(11, c["nf"]); bt.sync()
        snap = _snapshot(bt, c["B"])
        bt.close()
        for b in range(c["B"]):
            for x, y in zip(snap[b], ref[b]):
                assert np.array_equal(x, y), ("streamed", ns, ring, mode, b)


@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_prune_on_the_downdate_equals_the_separate_prune(capi, dtype_name):
    """Inside run_frames the prune of every frame but a call's last rides on the covariance downdate (written to its pruned
    position in the handle's second covariance buffer, window size committed by the next frame's propagate), the last frame
    of a call prunes with its own launch.  However a frame range is cut into calls -- all at once, frame by frame (no
    fused frame at all), in pieces of 2 and 3 (odd and even numbers of buffer swaps per call), streamed or resident --
    states, camera states, covariance, window size and statistics must be the SAME BITS, and the getters must read the
    buffer that is current after an odd number of swaps."""
    N, F, B = 8, 40, 6
    nf = N + 9
    dtype = capi.F32 if dtype_name == "f32" else capi.F64
    trajs = [sc.Trajectory(2, 300 + b, N, F, nf) for b in range(B)]

    def run(cuts, streamed=False, streams=1):
        bt = _resident_batch(capi, trajs, N, F, nf, 12, dtype, streams=streams)
        a = 0
        for c in cuts:
            (bt.run_frames_streamed if streamed else bt.run_frames)(a, a + c)
            a += c
        assert a == nf
        bt.sync()
        out = _snapshot(bt, B), [bt.num_cam_states(b) for b in range(B)], [bt.last_stats(b) for b in range(B)]
        bt.close()
        return out

    ref = run([1] * nf)                              # every frame its own call: the separate prune launch throughout
    assert all(n == N - 1 for n in ref[1])           # the window is full and one state is dropped per frame
    for cuts, kw in (([nf], {}), ([2] * (nf // 2) + [nf % 2] * (nf % 2), {}), ([3, 4, 3, nf - 10], {}),
                     ([nf], dict(streams=3)), ([4, nf - 4], dict(streamed=True, streams=2))):
        snap, ncam, stats = run([c for c in cuts if c], **kw)
        assert ncam == ref[1], (cuts, kw)
        for b in range(B):
            for x, y in zip(snap[b], ref[0][b]):
                assert np.array_equal(x, y), (dtype_name, cuts, kw, b)
            assert stats[b] == ref[2][b], (cuts, kw, b)


def test_gain_solve_forms_s_the_same_alone_shared_or_after_a_missed_rendezvous(capi, cfg3_trajs, monkeypatch):
    """S = T_H (P T_H^T)[15:,:] + sigma^2 I is formed inside the blocked gain solve.  By default the four workgroups of a
    trajectory share the product (each forms a quarter of the blocks, agent-scope stores, counter barrier, read the rest);
    MSCKF_HIP_FUSED_S=1 makes every workgroup form all of it; =3 is the shared form with a zero wait at the barrier, so that
    workgroups give up on their siblings and form the missing blocks themselves (what happens when the siblings are not
    resident).  All three must give the same bits: the same MFMA sequence per block whoever runs it."""
    c = CFG3
    nf, B = 33, 16
    ref = None
    for mode in ("2", "1", "3"):
        monkeypatch.setenv("MSCKF_HIP_FUSED_S", mode)
        bt = _resident_batch(capi, cfg3_trajs[:B], c["N"], c["F"], nf, 32, capi.F32, streams=2)
        bt.run_frames(0, nf); bt.sync()
        snap = _snapshot(bt, B)
        bt.close()
        if ref is None:
            ref = snap
            continue
        for b in range(B):
            for x, y in zip(snap[b], ref[b]):
                assert np.array_equal(x, y), (mode, b)


def test_stage_timers_and_the_reading_of_an_empty_event_pair(capi, cfg3_trajs):
    """msckf_hip_profile_*: HIP-event pairs around every stage's launches on the library's stream (bench.py's roofline takes its
    kernel time from them), and msckf_hip_profile_event_overhead: what such a pair reads with nothing between its records,
    which bench.py takes off.  Two profiled frames give two pairs per stage; every single-kernel stage reads more than the
    empty pair (to measurement noise) and less than a millisecond at this size."""
    c = CFG3
    bt = _resident_batch(capi, cfg3_trajs[:8], c["N"], c["F"], 33, 32, capi.F32)
    bt.run_frames(0, 31); bt.sync()
    bt.profile_enable(True)
    bt.run_frames(31, 33); bt.sync()
    prof = bt.profile_read()
    bt.profile_enable(False)
    oh = bt.profile_event_overhead()
    bt.close()
    assert 0.0 < oh < 0.1, oh
    for stage in ("propagate", "augment", "feature", "compress_stage1", "compress_merge", "kalman", "prune", "select"):
        ms, cnt = prof[stage]
        assert cnt == 2, (stage, prof)
        assert 0.8 * oh < ms / cnt < 1.0, (stage, ms / cnt, oh)   # (the 4 us augment launch reads ~7 us against ~5 for the empty pair)


def test_cfg3_batch_of_64_vs_oracle(capi, po, cfg3_trajs):
    """The benched configuration against the oracle: after the window is full, 8 sampled trajectories of the 64 hand their
    state + covariance to a float oracle (teacher forcing, device -> oracle), both run the next filter update on the same
    inputs -- the device as ONE batched launch sequence on 2 streams, exactly as bench.py does -- and every state field
    and the covariance agree to 1e-3."""
    c = CFG3
    N, F, nf, B = c["N"], c["F"], c["nf"], c["B"]
    bt = _resident_batch(capi, cfg3_trajs, N, F, nf, 32, capi.F32, streams=2)
    k0 = nf - 2
    bt.run_frames(0, k0); bt.sync()
    sample = [0, 7, 13, 21, 30, 42, 55, 63]
    for k in (k0, k0 + 1):
        oracles = {}
        for b in sample:
            o = po.Oracle(po.F32, po.LEAN)
            o.initialize(cfg3_trajs[b].cfg, cfg3_trajs[b].imu0)
            H.copy_device_to_oracle(bt, b, o)
            oracles[b] = o
        bt.run_frames(k, k + 1); bt.sync()
        for b in sample:
            o, tr = oracles[b], cfg3_trajs[b]
            H.oracle_frame(o, tr, k, N)
            so, sd = o.lastStats(), bt.last_stats(b)
            for key in ("n_tracks", "n_motion_rejected", "n_tri_rejected", "n_gate_rejected", "n_passed", "m_rows"):
                assert so[key] == sd[key], (k, b, key, so, sd)
            e = H.state_errors(bt.imu_state(b), o.getImuState(), bt.cam_states(b)[0], o.getCamStates()[0], bt.covariance(b), o.getCovariance())
            assert H.worst(e) < 1e-3, (k, b, e)
    bt.close()


# ------------------------------------------------------------------------------------------------ cfg5 geometry
def test_cfg5_geometry_vs_oracle(capi, po):
    """BASELINE.json configs[4] geometry: 60-camera window, 500 tracks per update, float covariance, B = 2.  The window
    is filled on the device, then each trajectory's next update is compared with the float oracle (teacher-forced)."""
    N, F, nf, B = 60, 500, 63, 2
    trajs = [sc.Trajectory(5, b, N, F, nf) for b in range(B)]
    bt = _resident_batch(capi, trajs, N, F, nf, 60, capi.F32)
    k0 = nf - 1
    bt.run_frames(0, k0); bt.sync()
    oracles = []
    for b in range(B):
        o = po.Oracle(po.F32, po.LEAN)
        o.initialize(trajs[b].cfg, trajs[b].imu0)
        H.copy_device_to_oracle(bt, b, o)
        oracles.append(o)
    bt.run_frames(k0, k0 + 1); bt.sync()
    for b in range(B):
        o = oracles[b]
        H.oracle_frame(o, trajs[b], k0, N)
        so, sd = o.lastStats(), bt.last_stats(b)
        assert sd["n_passed"] > 400
        for key in ("n_tracks", "n_motion_rejected", "n_tri_rejected", "n_gate_rejected", "n_passed", "m_rows"):
            assert so[key] == sd[key], (b, key, so, sd)
        e = H.state_errors(bt.imu_state(b), o.getImuState(), bt.cam_states(b)[0], o.getCamStates()[0], bt.covariance(b), o.getCovariance())
        assert H.worst(e) < 1e-3, (b, e)
    bt.close()


@pytest.mark.parametrize("N,F", [(32, 70), (33, 70), (36, 80), (47, 100), (60, 140)])
def test_two_level_information_form_equals_householder_route_large_windows(capi, N, F):
    """Windows of more than 31 cameras (6N + 1 > 192): the information form factors the Gram matrix in two levels
    (kernels_chol.hip: leading 192 columns, L21 on the matrix cores, Schur complement; 256 / 320 / 384 padded columns
    here; 32 cameras = 193 columns: only the H_o^T r_o row lies beyond the split, 33 = the first real second level) and must stay with the Householder TSQR route (what the reference does, msckf.h:1338-1366) to rounding, in
    double, free-running from the first frame -- the frames during which the window is still below 192 columns included."""
    nf = N + 6
    tr = sc.Trajectory(5, 11, N, F, nf)
    res = {}
    for route in (0, 3):
        bt = capi.Batch(1, N, F, N, capi.F64)
        bt.set_compression(route)
        bt.initialize(0, tr.cfg, tr.imu0)
        for k in range(nf):
            H.device_frame(bt, 0, tr, k, N)
        res[route] = (bt.imu_state(0), bt.cam_states(0)[0], bt.covariance(0), bt.last_stats(0))
        bt.close()
    e = H.state_errors(res[3][0], res[0][0], res[3][1], res[0][1], res[3][2], res[0][2])
    # rounding level: the two routes share no arithmetic after k_feature (the information form's first <= 14-camera frames also take
    # the one-launch update k_update_small), and the weakly observable accelerometer bias amplifies the difference over N + 6
    # free-running frames: 1.1e-8 on b_a at 36 cameras, everything else below 3e-9 (the double filter is held to the oracle at 1e-6)
    assert H.worst(e) < 3e-8, e
    assert max(v for k, v in e.items() if k != "ba") < 1e-8, e
    assert res[3][3]["m_rows"] == res[0][3]["m_rows"] > 0
    assert res[3][3]["r_rows"] < res[0][3]["r_rows"] == 6 * N            # gauge directions skipped


def test_cfg5_geometry_householder_route_vs_information_form_float(capi):
    """cfg5 geometry in float, B = 2, resident scenario: the default route (two-level information form) against the TSQR
    route on the same frames; both are separately held against the oracle (test_cfg5_geometry_vs_oracle runs the default)."""
    N, F, nf, B = 60, 300, 63, 2
    trajs = [sc.Trajectory(5, 20 + b, N, F, nf) for b in range(B)]
    res = {}
    for route in (0, 3):
        bt = _resident_batch(capi, trajs, N, F, nf, 60, capi.F32)
        bt.set_compression(route)
        bt.run_frames(0, nf); bt.sync()
        res[route] = [(bt.imu_state(b), bt.cam_states(b)[0], bt.covariance(b), bt.last_stats(b)) for b in range(B)]
        bt.close()
    for b in range(B):
        a, c = res[3][b], res[0][b]
        e = H.state_errors(a[0], c[0], a[1], c[1], a[2], c[2])
        assert H.worst(e) < 1e-3, (b, e)
        assert a[3]["n_passed"] == c[3]["n_passed"] > 0.9 * F


def test_fp16_jacobian_dtype(capi, po):
    """MSCKF_HIP_F16H_F32P (BASELINE.json configs[4]: fp16 Jacobian / fp32 covariance): the measurement Jacobian blocks are
    rounded to fp16 (11-bit significand: ~5e-4 relative per entry) where they are formed, everything else stays f32.
    (1) the rounding is active and bounded: against the plain float filter on the same inputs, per update, attitude /
    position / velocity move by < 3e-3, the covariance and the accelerometer bias by < 3e-2, the gyro bias by < 1e-1
    (measured at the 10-camera window: 1e-4, 5e-5, 2e-4, 9e-4, 3e-3, 5e-2; at the 60-camera window P moves by 1.0e-2); (2) cfg5 geometry (60-camera window, 500 tracks): the same envelope
    against the float oracle with equal gate decisions, AND SURVEY 8d's 1e-2 on q, v, p, camera poses and the IMU block of the covariance as
    a gate, 1.5e-2 on the full covariance (measured 1.0e-2) (the survey says "reported, not gated"; the biases keep the envelope: their floor is the fp16 significand).
    The envelope contains the rounding itself; tests/test_gpu_h16_kernels.py holds the dtype to the float bars against a twin that is handed the stored fp16 blocks."""
    def envelope(e):
        assert max(e["q"], e["p"], e["v"], e["cam_q"], e["cam_p"]) < 3e-3 and max(e["P"], e["Pii"], e["ba"]) < 3e-2 and e["bg"] < 1e-1, e
    N, F, nf = 10, 50, 20
    tr = sc.Trajectory(2, 4, N, F, nf)
    a, b = capi.Batch(1, N, F, N, capi.F32), capi.Batch(1, N, F, N, capi.F16H)
    a.initialize(0, tr.cfg, tr.imu0); b.initialize(0, tr.cfg, tr.imu0)
    worst = 0.0
    for k in range(nf):
        if k:   # teacher-forced from the float filter
            b.set_covariance(0, a.covariance(0)); b.set_imu_state(0, a.imu_state(0))
            for i, c in enumerate(a.cam_states(0)[0]):
                b.set_cam_pose(0, i, c)
            b.set_num_residualized(0, a.num_residualized(0))
        H.device_frame(a, 0, tr, k, N); H.device_frame(b, 0, tr, k, N)
        e = H.state_errors(b.imu_state(0), a.imu_state(0), b.cam_states(0)[0], a.cam_states(0)[0], b.covariance(0), a.covariance(0))
        envelope(e)
        worst = max(worst, H.worst(e))
    assert worst > 1e-6, worst        # the rounding is really applied
    a.close(); b.close()
    N, F, nf, B = 60, 500, 63, 2
    trajs = [sc.Trajectory(5, b2, N, F, nf) for b2 in range(B)]
    bt = _resident_batch(capi, trajs, N, F, nf, 60, capi.F16H)
    k0 = nf - 1
    bt.run_frames(0, k0); bt.sync()
    oracles = []
    for b2 in range(B):
        o = po.Oracle(po.F32, po.LEAN)
        o.initialize(trajs[b2].cfg, trajs[b2].imu0)
        H.copy_device_to_oracle(bt, b2, o)
        oracles.append(o)
    bt.run_frames(k0, k0 + 1); bt.sync()
    for b2 in range(B):
        o = oracles[b2]
        H.oracle_frame(o, trajs[b2], k0, N)
        so, sd = o.lastStats(), bt.last_stats(b2)
        assert so["n_passed"] == sd["n_passed"] > 400, (so, sd)
        e = H.state_errors(bt.imu_state(b2), o.getImuState(), bt.cam_states(b2)[0], o.getCamStates()[0], bt.covariance(b2), o.getCovariance())
        envelope(e)
        # SURVEY 8d's bar for this configuration, as a gate: 1e-2 against the float oracle on attitude, velocity, position
        # (IMU and camera states) and on the covariance (full and IMU block)
        for key in ("q", "v", "p", "cam_q", "cam_p", "Pii"):
            assert e[key] < 1e-2, (b2, key, e)
        assert e["P"] < 1.5e-2, (b2, e)     # measured 1.02e-2 / 0.98e-2 on the two trajectories: the full covariance sits AT the survey's figure, not under it
    bt.close()


# ------------------------------------------------------------------------------------------------ ill-conditioned stack
def test_low_parallax_double_both_routes_vs_oracle(capi, po):
    """Landmarks 150-600 m away (sub-pixel parallax per frame): the stacked Jacobian is as ill-conditioned as tracks that
    still pass the reference's own triangulation checks (msckf.h:1257-1276) can make it -- cond(H_o) over its column
    space, measured with the numpy twin, is ~1e4 against ~70 in the 2-10 m scenes (it grows with depth; further out the
    tracks are rejected, so 1e6 is not reachable with valid input).  That is where chol(H_o^T H_o) (information form,
    condition squared, f64) and a Householder QR (what the reference does, msckf.h:1343) could part ways.  Both routes
    stay with the double oracle to 1e-6, teacher-forced, state and covariance."""
    import np_oracle
    N, F, nf = 10, 40, 16
    cfg = sc.filter_config(N)
    cfg["translation_threshold"] = 0.01
    tr = sc.Trajectory(2, 3, N, F, nf, cfg=cfg, depth_range=(150.0, 600.0))
    conds = []

    class Capture(np_oracle.NpMSCKF):
        def measurement_update(self, Hm, r, R):
            s = np.linalg.svd(np.asarray(Hm)[:, 15:], compute_uv=False)
            s = s[s > 1e-11 * s[0]]
            conds.append(s[0] / s[-1])
            return super().measurement_update(Hm, r, R)

    for route in (3, 0):
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        bt = capi.Batch(1, N, F, N, capi.F64)
        bt.set_compression(route)
        bt.initialize(0, tr.cfg, tr.imu0)
        for k in range(nf):
            if k:
                H.copy_oracle_to_device(o, bt, 0)
            H.oracle_frame(o, tr, k, N); H.device_frame(bt, 0, tr, k, N)
            so, sd = o.lastStats(), bt.last_stats(0)
            assert so["n_passed"] == sd["n_passed"] and so["m_rows"] == sd["m_rows"], (route, k, so, sd)
            e = H.state_errors(bt.imu_state(0), o.getImuState(), bt.cam_states(0)[0], o.getCamStates()[0], bt.covariance(0), o.getCovariance())
            assert H.worst(e) < 1e-6, (route, k, e)
        assert so["n_passed"] > F // 2
        bt.close()
    # condition number of the stack (numpy twin on the same scenario, free-running for the first updates)
    tw = Capture(tr.cfg, tr.imu0)
    for k in range(12):
        for rd in tr.imu_for_frame(k):
            tw.propagate(rd)
        tw.augment(k)
        fr = tr.frames[k]
        if len(fr["M"]):
            tw.set_tracks(fr["M"], fr["slots"], fr["obs"]); tw.marginalize()
        if len(tw.cam_array()) == N:
            tw.drop_oldest(1)
    assert conds and max(conds) > 5e3, conds


def test_failed_streamed_run_makes_the_handle_unusable(capi, monkeypatch):
    """A run_frames_streamed call that fails after some of its frames were enqueued (here: the copy of frame 11 is made to
    fail, msckf_mono_amd/csrc/msckf_hip.hip: MSCKF_HIP_TEST_FAIL_UPLOAD) leaves the slices at different frames -- which
    covariance buffer is current differs per slice.  The call returns -EIO, and so does everything that would read or advance
    the filters afterwards; a fresh handle is unaffected.  Also: a scenario patched and re-committed several times streams
    from re-pinned blocks (the page-locked chunks are released with the last of their frames)."""
    N, F, nf, B = 8, 24, 16, 2
    trajs = [sc.Trajectory(2, 30 + b, N, F, nf) for b in range(B)]
    monkeypatch.setenv("MSCKF_HIP_TEST_FAIL_UPLOAD", "11")
    bad = _resident_batch(capi, trajs, N, F, nf, N, capi.F32, streams=2)
    monkeypatch.delenv("MSCKF_HIP_TEST_FAIL_UPLOAD")
    bad.run_frames(0, 8); bad.sync()
    with pytest.raises(capi.HipError, match=r"\(-5\).*undefined"):
        bad.run_frames_streamed(8, 14)
    for call in (lambda: bad.imu_state(0), lambda: bad.covariance(1), lambda: bad.run_frames(14, 15), lambda: bad.run_frames_streamed(14, 15)):
        with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
            call()
    bad.close()
    good = _resident_batch(capi, trajs, N, F, nf, N, capi.F32, streams=2)
    ref = _resident_batch(capi, trajs, N, F, nf, N, capi.F32, streams=2)
    ref.run_frames(0, nf); ref.sync()
    good.run_frames(0, 8)
    for rnd in range(3):                      # patch a frame that was already pinned (same contents), commit, stream on
        good.run_frames_streamed(8 + 2 * rnd, 10 + 2 * rnd)
        for k in (8 + 2 * rnd, 9 + 2 * rnd, 14):      # the two frames of the block just streamed (-> its chunk is released) and one ahead
            for b, tr in enumerate(trajs):
                fr = tr.frames[k]
                good.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
        good.scenario_commit()
    good.run_frames_streamed(14, nf); good.sync()
    for b in range(B):
        assert np.array_equal(good.imu_state(b), ref.imu_state(b)) and np.array_equal(good.covariance(b), ref.covariance(b))
    good.close(); ref.close()


def test_streamed_run_under_the_stage_timers_equals_the_resident_run(capi, cfg3_trajs):
    """With the stage timers on (msckf_hip_profile_enable: one stream, augmentState and the prune as launches of their own)
    run_frames_streamed goes through the same frame step as run_frames: same bits for every trajectory, and profile_read
    counts the same number of launches per stage -- one propagate, augment, update sequence and prune per frame."""
    c = CFG3
    B, nf = 8, 33

    def run(streamed):
        bt = _resident_batch(capi, cfg3_trajs[:B], c["N"], c["F"], nf, 32, capi.F32, streams=3)
        bt.profile_enable(True)
        go = bt.run_frames_streamed if streamed else bt.run_frames
        go(0, 20); go(20, nf); bt.sync()
        prof = bt.profile_read()
        bt.profile_enable(False)
        snap = _snapshot(bt, B)
        bt.close()
        return snap, {stage: cnt for stage, (ms, cnt) in prof.items()}

    ref, ref_cnt = run(False)
    snap, cnt = run(True)
    for stage in ("propagate", "augment", "feature", "select", "prune"):
        assert ref_cnt[stage] == nf, (stage, ref_cnt)
    assert cnt == ref_cnt, (cnt, ref_cnt)
    for b in range(B):
        for x, y in zip(snap[b], ref[b]):
            assert np.array_equal(x, y), b
