"""What the calibrated expansion of the Monte-Carlo replay costs per frame, and a small sensitivity sweep over two calibration
errors (Calibration; recorded, not asserted).

Float, isotropic, N = 30, F = 200; 5 noise-free sequences x 128 seeds = 640 trajectories under the Q_imu model; 30 fill frames +
40 timed; one slice -- scripts/replay_timing_cost.py's configuration.  Variants, on one handle, their timed windows alternating in
one process:
  off      no record of any kind (k_replay_expand)
  timing   replay_set_timing((5 ms, 30 ms readout over 480 rows, 1 ms jitter)) (k_replay_expand_timed)
  calib    both calibration records: scale, misalignment, g-sensitivity, saturation, quantisation; all eight camera fields
           (k_replay_expand_calib)
  all      calibration, timing and faults (0.1, 0.1, 3 px, 3 px) together (k_replay_expand_calib)
Per variant: ms per frame (median of the windows) and the expansion's stage time per launch (stage 11, from the library's stage
timers in a run of its own).

--parent-lib PATH: a libmsckf_hip.so built from the parent commit.  The script then starts one child process per library and
round, parent and this tree alternating, the parent running `off` alone, and reports both `off` figures side by side together
with the run-to-run spread of the same A/B: per library the largest relative difference between two rounds' `off` figures.

--sweep: the last round's child also runs the whole sequence under a gyro scale error and under a principal-point error of
growing size, every trajectory at the same record, and records the SE(3)-aligned ATE (frame_log_align) and the mean ANEES over
the timed frames (nees_log_ensemble) of each point.  A demonstration of the feature, not a check.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SWEEP_GYRO_SCALE = (0.0, 1e-3, 3e-3, 1e-2, 3e-2)
SWEEP_PP_PX = (0.0, 0.5, 1.0, 2.0, 4.0)


def child(args):
    from msckf_mono_amd import capi, scenario as sc, trajeval as te
    N, F, S, B, fill, nf = args.window, args.tracks, args.sequences, args.sequences * args.seeds, args.fill, args.fill + args.timed
    K = sc.IMU_PER_FRAME
    cfg = sc.filter_config(N, isotropic=True)
    seqs = [sc.Trajectory(4, p, N, F, nf, cfg=cfg, imu_noise_scale=0.0, obs_noise_px=0.0, path_id=p % len(sc.PATHS)) for p in range(S)]
    seq_of = [b % S for b in range(B)]
    seeds = [0x5EED4000 + b for b in range(B)]
    bt = capi.Batch(B, N, F, N, capi.F32)

    def reinit():
        for b in range(B):
            bt.initialize(b, cfg, seqs[seq_of[b]].imu0)

    reinit()
    bt.set_streams(1)
    bt.replay_alloc(S, nf, K)
    for f in range(nf):
        for s, tr in enumerate(seqs):
            fr = tr.frames[f]
            bt.replay_set_cell(f, s, tr.imu_for_frame(f), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.replay_assign_q(seq_of, seeds, np.diag(np.asarray(cfg["Q_imu_diag"], dtype=np.float64)), 0.05, (0.5 / cfg["f_u"], 0.5 / cfg["f_v"]))
    bt.replay_commit()
    fault4 = (0.1, 0.1, 3.0 / cfg["f_u"], 3.0 / cfg["f_v"])
    timing4 = (5e-3, 0.030 * cfg["f_v"] / 480.0, (240.0 - cfg["c_v"]) / cfg["f_v"], 1e-3)
    imucal = sc.imu_calib_record(scale_g=[3e-3, -2e-3, 4e-3], misalign_g=1e-3, scale_a=[-5e-3, 2e-3, 3e-3], misalign_a=-1e-3, g_sens=2e-4,
                                 sat_g=np.deg2rad(250.0), sat_a=16 * 9.80665, lsb_g=np.deg2rad(250.0) / 32768.0, lsb_a=9.80665e-3)
    camcal = sc.cam_calib_record(e_u=-3e-3, e_v=2e-3, d_u=1.5 / cfg["f_u"], d_v=-2.0 / cfg["f_v"], k1=6e-3, k2=-1.5e-3, p1=3e-4, p2=-2e-4)
    variants = args.variants.split(",")
    has_timing, has_calib = hasattr(bt.L, "msckf_hip_replay_set_timing"), hasattr(bt.L, "msckf_hip_replay_set_imu_calib")

    def select(v):
        bt.replay_set_faults(fault4 if v == "all" else None)
        if has_timing:
            bt.replay_set_timing(timing4 if v in ("timing", "all") else None)
        if has_calib:
            bt.replay_set_imu_calib(imucal if v in ("calib", "all") else None)
            bt.replay_set_cam_calib(camcal if v in ("calib", "all") else None)

    times = {v: [] for v in variants}
    for w in range(args.windows + 1):                       # window 0 warms every variant up and is not reported
        for v in variants:
            select(v)
            reinit()
            bt.run_frames_replay(0, fill)
            bt.sync()
            t0 = time.perf_counter()
            bt.run_frames_replay(fill, nf)
            bt.sync()
            if w:
                times[v].append(time.perf_counter() - t0)
    out = {}
    for v in variants:
        select(v)
        reinit()
        bt.run_frames_replay(0, fill)
        bt.profile_enable(True)
        bt.run_frames_replay(fill, nf)
        ms, cnt = bt.profile_read()["replay_expand"]
        bt.profile_enable(False)
        out[v] = dict(window_s=times[v], ms_per_frame=1e3 * statistics.median(times[v]) / args.timed, expand_ms_per_launch=ms / max(cnt, 1), expand_launches=cnt)
    out["slices"] = bt.effective_streams(False)
    if args.sweep and has_calib:
        select("off")
        gt = np.ascontiguousarray(te.gt_pose7(seqs, 0, nf)[:, seq_of])
        bt.truth_set(sc.imu_state_gt(seqs, 0, nf), row_of=seq_of, add_walk=True)

        def point(ic, cc):
            bt.replay_set_imu_calib(ic)
            bt.replay_set_cam_calib(cc)
            reinit()
            bt.frame_log_enable(nf)
            bt.nees_log_enable(nf)
            bt.run_frames_replay(0, nf)
            bt.sync()
            rows = bt.frame_log_align(0, nf, gt, capi.ALIGN_SE3)
            sums, _ = bt.nees_log_ensemble(fill, nf, [0] * B, 1)
            n = float(sums[:, 0, 0].sum())
            counts = bt.replay_calib_counts()
            return dict(ate_se3_m=float(np.sqrt(rows[:, 14].sum() / rows[:, 0].sum())), anees_full=float(sums[:, 0, 2].sum() / n) if n else None,
                        anees_p=float(sums[:, 0, 7].sum() / n) if n else None, nees_records=n, nees_flagged=float(sums[:, 0, 1].sum()),
                        clipped_samples=int(counts[:, 7].sum()))

        out["sweep"] = dict(
            gyro_scale=[dict(scale=e, **point(sc.imu_calib_record(scale_g=e), None)) for e in SWEEP_GYRO_SCALE],
            principal_point_px=[dict(px=p, **point(None, sc.cam_calib_record(d_u=p / cfg["f_u"], d_v=p / cfg["f_v"]))) for p in SWEEP_PP_PX])
    bt.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--tracks", type=int, default=200)
    ap.add_argument("--sequences", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=128)
    ap.add_argument("--fill", type=int, default=30)
    ap.add_argument("--timed", type=int, default=40)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variants", default="off,timing,calib,all")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    shape = ["--window", args.window, "--tracks", args.tracks, "--sequences", args.sequences, "--seeds", args.seeds, "--fill", args.fill, "--timed", args.timed, "--windows", args.windows]

    def run(lib, variants, sweep=False):
        env = dict(os.environ)
        if lib:
            env["MSCKF_HIP_LIB"] = os.path.abspath(lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--variants", variants] + (["--sweep"] if sweep else []) + [str(x) for x in shape],
                           env=env, capture_output=True, text=True)
        if p.returncode != 0:
            raise SystemExit("child failed (%d):\n%s" % (p.returncode, p.stdout[-2000:] + p.stderr[-2000:]))
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    rounds = []
    for i in range(args.rounds):
        r = {}
        if args.parent_lib:
            r["parent"] = run(args.parent_lib, "off")
        r["this"] = run(None, args.variants, sweep=args.sweep and i == args.rounds - 1)
        rounds.append(r)
        print("round %d of %d done" % (i + 1, args.rounds), file=sys.stderr, flush=True)
    med = statistics.median
    spread = lambda xs: (max(xs) - min(xs)) / min(xs)
    summary = {v: dict(ms_per_frame=med([r["this"][v]["ms_per_frame"] for r in rounds]), expand_ms_per_launch=med([r["this"][v]["expand_ms_per_launch"] for r in rounds]))
               for v in args.variants.split(",")}
    if "off" in summary:
        summary["off"]["round_spread"] = spread([r["this"]["off"]["ms_per_frame"] for r in rounds])
    if args.parent_lib:
        summary["parent_off"] = dict(ms_per_frame=med([r["parent"]["off"]["ms_per_frame"] for r in rounds]), expand_ms_per_launch=med([r["parent"]["off"]["expand_ms_per_launch"] for r in rounds]),
                                     round_spread=spread([r["parent"]["off"]["ms_per_frame"] for r in rounds]))
        if "off" in summary:
            summary["off_vs_parent"] = summary["off"]["ms_per_frame"] / summary["parent_off"]["ms_per_frame"] - 1.0
    sweep = rounds[-1]["this"].pop("sweep", None)
    out = dict(shape=dict(dtype="f32", window=args.window, tracks=args.tracks, sequences=args.sequences, trajectories=args.sequences * args.seeds, fill_frames=args.fill,
                          timed_frames=args.timed, windows=args.windows, rounds=args.rounds, model="q_imu", slices=1), summary=summary, rounds=rounds)
    if sweep is not None:
        out["sweep_not_asserted"] = sweep
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
