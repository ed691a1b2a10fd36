"""What the aligned trajectory error costs on the device, beside the host round trip it replaces (recorded,
not asserted).

Float, isotropic, N = 8, F = 40 (the reduction does not depend on the filter's shape); 5 noise-free sequences x 128 seeds = 640
trajectories under the Q_imu model, 200 frames with the frame log on.  Timed, each as the median of --calls calls: frame_log_align
(per mode) and frame_log_rpe (5 lags) -- the whole call, upload of the ground truth, kernel and read-back of the rows, between
two HIP events on the legacy default stream (the handle's stream is idle before the first and synchronised before the second),
and by the host clock; then frame_log_read of the same records plus the numpy twin, trajectory by trajectory, by the host clock.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from msckf_mono_amd import capi, scenario as sc, trajeval as te  # noqa: E402

LAGS = (1, 2, 5, 10, 50)


def hip_runtime():
    """the HIP runtime this process already has (the library's own, or torch's): found in the process map, not loaded anew"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime in this process")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=128)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--no-twin", action="store_true")
    args = ap.parse_args()
    N, F, S, B, nf = 8, 40, args.sequences, args.sequences * args.seeds, args.frames
    cfg = sc.filter_config(N, isotropic=True)
    seqs = [sc.Trajectory(2, p, N, F, nf, cfg=cfg, imu_noise_scale=0.0, obs_noise_px=0.0, path_id=p % len(sc.PATHS)) for p in range(S)]
    seq_of = [b % S for b in range(B)]
    bt = capi.Batch(B, N, F, 12, capi.F32)
    for b in range(B):
        bt.initialize(b, cfg, seqs[seq_of[b]].imu0)
    bt.replay_alloc(S, nf, sc.IMU_PER_FRAME)
    for f in range(nf):
        for s, tr in enumerate(seqs):
            fr = tr.frames[f]
            bt.replay_set_cell(f, s, tr.imu_for_frame(f), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.replay_assign_q(seq_of, [0x5EED4000 + b for b in range(B)], np.diag(np.asarray(cfg["Q_imu_diag"], dtype=np.float64)), 0.05, (0.5 / cfg["f_u"], 0.5 / cfg["f_v"]))
    bt.replay_commit()
    bt.frame_log_enable(nf)
    bt.run_frames_replay(0, nf)
    bt.sync()
    gt = np.ascontiguousarray(te.gt_pose7(seqs, 0, nf)[:, seq_of])

    hip = hip_runtime()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def timed(fn):
        dev, host, res = [], [], None
        for _ in range(args.calls + 1):                     # the first call warms up and is not reported
            hip.hipEventRecord(ev[0], None)
            t0 = time.perf_counter()
            res = fn()
            host.append(time.perf_counter() - t0)
            hip.hipEventRecord(ev[1], None); hip.hipEventSynchronize(ev[1])
            ms = C.c_float()
            hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])
            dev.append(ms.value)
        return dict(event_ms=statistics.median(dev[1:]), host_ms=1e3 * statistics.median(host[1:])), res

    out = {"shape": dict(dtype="f32", trajectories=B, records=nf, lags=list(LAGS), calls=args.calls), "device": {}}
    rows = {}
    for mode in (0, 1, 2):
        out["device"]["frame_log_align_mode%d" % mode], rows[mode] = timed(lambda: bt.frame_log_align(0, nf, gt, mode))
    out["device"]["frame_log_rpe_5_lags"], rpe = timed(lambda: bt.frame_log_rpe(0, nf, gt, LAGS))
    n = rows[2][:, 0].sum()
    out["ate_m"] = {"unaligned": float(np.sqrt(rows[0][:, 14].sum() / n)), "yaw": float(np.sqrt(rows[1][:, 14].sum() / n)), "se3": float(np.sqrt(rows[2][:, 14].sum() / n))}
    out["rpe_m"] = {str(lag): float(np.sqrt(rpe[:, k, 1].sum() / rpe[:, k, 0].sum())) for k, lag in enumerate(LAGS)}
    if not args.no_twin:
        t0 = time.perf_counter()
        arr, _ = bt.frame_log_read()
        t1 = time.perf_counter()
        est = te.pose7_from_truth16(arr[:, :, 0:16])
        tw = np.stack([te.align(est[:, b], gt[:, b], 2) for b in range(B)])
        t2 = time.perf_counter()
        np.stack([te.rpe(est[:, b], gt[:, b], LAGS) for b in range(B)])
        t3 = time.perf_counter()
        out["host"] = dict(frame_log_read_ms=1e3 * (t1 - t0), twin_align_one_mode_ms=1e3 * (t2 - t1), twin_rpe_5_lags_ms=1e3 * (t3 - t2))
        out["device_vs_twin_max_rel_sum_sq"] = float(np.max(np.abs(tw[:, 14] - rows[2][:, 14]) / tw[:, 14]))
    print(json.dumps(out))
    bt.close()


if __name__ == "__main__":
    main()
