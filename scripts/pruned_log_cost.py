#!/usr/bin/env python3
"""What the pruned-state log costs at cfg3 (B = 64, four slices, streamed inputs): windows of K steps after the window fill and
W warm-up steps, timed with a host clock around run_frames_streamed + sync, alternating log-off and log-on windows in one
process on the same handle (the frames differ per window, as in bench.py; alternation keeps drift out of the comparison).
With the log on no frame's prune rides on the covariance downdate: a log-on step has one k_prune_inplace launch and one
k_pruned_log launch per slice more than a log-off step.
--mode off runs log-off windows only and never touches the pruned-log entry points, so it also runs an older library
(MSCKF_HIP_LIB=...) for the A/B against the parent commit on the same lease.
One JSON line: per mode the windows' updates/s, their median and min/median (the window-to-window spread); with the log on
also the records found per window (all trajectories: one state per trajectory and frame leaves the full window).
Usage: pruned_log_cost.py [--mode alternate|off|on] [--steps 20] [--warmup 5] [--windows 8] [--tag NAME]"""
import argparse, json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("alternate", "off", "on"), default="alternate")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=8, help="windows per mode")
    ap.add_argument("--streams", type=int, default=4)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    import bench
    c = dict(bench.CONFIGS["cfg3"])
    N, F, B = c["N"], c["F"], c["B"]
    K, W = a.steps, a.warmup
    modes = ["off", "on"] if a.mode == "alternate" else [a.mode]
    R = a.windows * len(modes)
    nfr = N + W + K * R
    trajs = bench.make_trajectories(c, 0, nfr)
    import torch
    from msckf_mono_amd import capi
    bt = capi.Batch(B, N, F, N, capi.F32, 0)
    bt.scenario_alloc(nfr, bench.K_IMU)
    for b, tr in enumerate(trajs):
        bt.initialize(b, tr.cfg, tr.imu0)
        for f in range(nfr):
            fr = tr.frames[f]
            bt.scenario_set(f, b, tr.imu_for_frame(f), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    bt.scenario_pin(N, nfr)
    bt.set_streams(a.streams)
    bt.run_frames(0, N); bt.run_frames_streamed(N, N + W); bt.sync()
    vals = {m: [] for m in modes}
    found = []
    f = N + W
    for i in range(R):
        m = modes[i % len(modes)]
        if a.mode != "off":
            bt.pruned_log_enable(K if m == "on" else 0)       # (waits for the stream; outside the timed region)
        torch.cuda.synchronize(); bt.sync()
        t0 = time.perf_counter()
        bt.run_frames_streamed(f, f + K); bt.sync()
        vals[m].append(B * K / (time.perf_counter() - t0)); f += K
        if m == "on":
            assert bt.pruned_log_frames() == K
            found.append(int(bt.pruned_log_counts()[1].sum()))
    out = dict(tag=a.tag, lib=os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH), mode=a.mode, steps=K, warmup=W, streams=a.streams, B=B)
    for m in modes:
        v = vals[m]
        out["log_" + m] = dict(windows=[round(x) for x in v], median=round(float(np.median(v))), min=round(min(v)), max=round(max(v)),
                               min_over_median=round(min(v) / float(np.median(v)), 4), ms_per_step=round(1e3 * B / float(np.median(v)), 4))
    if found:
        out["records_found_per_window"] = found
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
