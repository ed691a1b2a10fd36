"""What the NEES log costs per frame at the Monte-Carlo replay's configuration (recorded, not asserted).

Float, isotropic, N = 30, F = 200; 5 noise-free sequences x 128 seeds = 640 trajectories under the Q_imu model (the filter's
diagonal Q_imu with both walks, scale 0.05); 30 fill frames + 40 timed.  Two replay handles on the same sequences, one with
the NEES log on (truth rows by sequence, the walk added on the device), one with it off; timed windows alternate in one process,
every window from freshly initialised filters brought through the fill frames.  Prints one JSON line: all window times, the
medians, ms per frame, the time of one ensemble reduction over the timed records, and the ANEES of the last frame per sequence.

--log off: the log-off handle alone, through entry points that a library from before the log has as well (MSCKF_HIP_LIB names
such a library for the comparison with the parent commit).  --windows / --timed shorten a run under a profiler."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from msckf_mono_amd import capi, scenario as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--tracks", type=int, default=200)
    ap.add_argument("--sequences", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=128)
    ap.add_argument("--fill", type=int, default=30)
    ap.add_argument("--timed", type=int, default=40)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--log", choices=("both", "off"), default="both")
    args = ap.parse_args()
    N, F, S, B, fill, nf = args.window, args.tracks, args.sequences, args.sequences * args.seeds, args.fill, args.fill + args.timed
    K = sc.IMU_PER_FRAME
    cfg = sc.filter_config(N, isotropic=True)
    seqs = [sc.Trajectory(4, p, N, F, nf, cfg=cfg, imu_noise_scale=0.0, obs_noise_px=0.0, path_id=p % len(sc.PATHS)) for p in range(S)]
    seq_of = [b % S for b in range(B)]
    seeds = [0x5EED4000 + b for b in range(B)]
    Q = np.diag(np.asarray(cfg["Q_imu_diag"], dtype=np.float64))
    sigma_uv = (0.5 / cfg["f_u"], 0.5 / cfg["f_v"])

    def reinit(bt):
        for b in range(B):
            bt.initialize(b, cfg, seqs[seq_of[b]].imu0)

    def handle(log):
        bt = capi.Batch(B, N, F, N, capi.F32)
        reinit(bt)
        bt.replay_alloc(S, nf, K)
        for f in range(nf):
            for s, tr in enumerate(seqs):
                fr = tr.frames[f]
                bt.replay_set_cell(f, s, tr.imu_for_frame(f), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
        bt.replay_assign_q(seq_of, seeds, Q, 0.05, sigma_uv)
        bt.replay_commit()
        if log:
            bt.truth_set(sc.imu_state_gt(seqs, 0, nf), row_of=seq_of, add_walk=True)
            bt.nees_log_enable(nf)
        return bt

    paths = {"off": handle(False)}
    if args.log == "both":
        paths["on"] = handle(True)
    times = {k: [] for k in paths}
    for w in range(args.windows + 1):                       # window 0 warms both handles up and is not reported
        for name, bt in paths.items():
            reinit(bt)
            if name == "on":
                bt.nees_log_reset()
            bt.run_frames_replay(0, fill)
            bt.sync()
            t0 = time.perf_counter()
            bt.run_frames_replay(fill, nf)
            bt.sync()
            if w:
                times[name].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "shape": dict(dtype="f32", window=N, tracks=F, sequences=S, trajectories=B, fill_frames=fill, timed_frames=args.timed, windows=args.windows),
        "library": os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH),
        "slices": {k: bt.effective_streams(False) for k, bt in paths.items()},
        "window_s": times, "median_window_s": med, "ms_per_frame": {k: 1e3 * v / args.timed for k, v in med.items()},
    }
    if "on" in paths:
        on = paths["on"]
        out["on_over_off_time"] = med["on"] / med["off"]
        out["log_us_per_frame"] = 1e6 * (med["on"] - med["off"]) / args.timed
        t0 = time.perf_counter()
        sums, anees = on.nees_log_ensemble(fill, nf, seq_of, S)
        out["ensemble_ms"] = 1e3 * (time.perf_counter() - t0)
        out["last_frame"] = dict(members=sums[-1, :, 0].tolist(), flagged=sums[-1, :, 1].tolist(), anees_15=anees[-1, :, 0].tolist(),
                                 anees_blocks_mean=np.nanmean(anees[-1, :, 1:], axis=0).tolist())
        same = all(np.array_equal(paths["off"].imu_state(b), on.imu_state(b)) for b in range(0, B, max(B // 16, 1)))
        out["same_final_states"] = bool(same)
    print(json.dumps(out))
    for bt in paths.values():
        bt.close()


if __name__ == "__main__":
    main()
