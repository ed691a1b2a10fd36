"""What the faulted and the timed expansion of the Monte-Carlo replay cost per frame (recorded, not asserted).

Float, isotropic, N = 30, F = 200; 5 noise-free sequences x 128 seeds = 640 trajectories under the Q_imu model; 30 fill frames +
40 timed; one slice.  Variants, on one handle, their timed windows alternating in one process:
  off      no fault record, no timing record (k_replay_expand)
  faults   replay_set_faults((0.1, 0.1, 3 px, 3 px)) (k_replay_expand_faults)
  timing   replay_set_timing((5 ms, 30 ms readout over 480 rows, 1 ms jitter)) (k_replay_expand_timed)
  both     both records (k_replay_expand_timed)
Per variant: ms per frame (median of the windows) and the expansion's stage time per launch (stage 11, from the library's stage
timers in a run of its own).

--parent-lib PATH: a libmsckf_hip.so built from the parent commit.  The script then starts one child process per library and
round, parent and this tree alternating (two machines, or two visits to one, differ by up to 8 %: DESIGN section 9), the parent
running `off` alone, and reports both `off` figures side by side.  Prints one JSON line; --out writes it to a file as well."""
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


def child(args):
    from msckf_mono_amd import capi, scenario as sc
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
    variants = args.variants.split(",")

    def select(v):
        bt.replay_set_faults(fault4 if v in ("faults", "both") else None)
        if v in ("timing", "both"):
            bt.replay_set_timing(timing4)
        elif hasattr(bt.L, "msckf_hip_replay_set_timing"):
            bt.replay_set_timing(None)

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
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--variants", default="off,faults,timing,both")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    shape = ["--window", args.window, "--tracks", args.tracks, "--sequences", args.sequences, "--seeds", args.seeds, "--fill", args.fill, "--timed", args.timed, "--windows", args.windows]

    def run(lib, variants):
        env = dict(os.environ)
        if lib:
            env["MSCKF_HIP_LIB"] = os.path.abspath(lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--variants", variants] + [str(x) for x in shape], env=env, capture_output=True, text=True)
        if p.returncode != 0:
            raise SystemExit("child failed (%d):\n%s" % (p.returncode, p.stdout[-2000:] + p.stderr[-2000:]))
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])

    rounds = []
    for i in range(args.rounds):
        r = {}
        if args.parent_lib:
            r["parent"] = run(args.parent_lib, "off")
        r["this"] = run(None, args.variants)
        rounds.append(r)
        print("round %d of %d done" % (i + 1, args.rounds), file=sys.stderr, flush=True)
    med = lambda xs: statistics.median(xs)
    summary = {v: dict(ms_per_frame=med([r["this"][v]["ms_per_frame"] for r in rounds]), expand_ms_per_launch=med([r["this"][v]["expand_ms_per_launch"] for r in rounds]))
               for v in args.variants.split(",")}
    if args.parent_lib:
        summary["parent_off"] = dict(ms_per_frame=med([r["parent"]["off"]["ms_per_frame"] for r in rounds]), expand_ms_per_launch=med([r["parent"]["off"]["expand_ms_per_launch"] for r in rounds]))
    out = dict(shape=dict(dtype="f32", window=args.window, tracks=args.tracks, sequences=args.sequences, trajectories=args.sequences * args.seeds, fill_frames=args.fill,
                          timed_frames=args.timed, windows=args.windows, rounds=args.rounds, model="q_imu", slices=1), summary=summary, rounds=rounds)
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
