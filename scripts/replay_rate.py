"""Monte-Carlo replay against the streamed path, at BASELINE configs[3]'s share per GPU (recorded, not asserted).

Float, isotropic, N = 30, F = 200; 5 noise-free sequences x 128 seeds = 640 trajectories; 30 fill frames + 40 timed.
  streamed   run_frames_streamed on an ordinary scenario whose 640 x 70 cells are the replay's own expansions, read back
  replay     run_frames_replay on the five sequences
Both handles run the same frames on the same inputs (checked: the final IMU states agree bit for bit).  Three timed windows
each, alternating in one process; every window starts from freshly initialised filters brought through the fill frames on the
path that is timed.  Prints one JSON line: median and all window times, frames/s, the bytes per frame each path keeps on the
host, page-locks and sends over PCIe (computed from the shapes), and the expansion kernel's time per frame from the library's
stage timers (a run of its own: profiling forces one slice).

--model q: the Q_imu noise model against the sigma4 one instead (no streamed handle): two replay handles on the same sequences,
one assigned through replay_assign (sigma4), one through replay_assign_q (the filter's diagonal Q_imu with both walks, scale
0.05), windows alternating in one process; the expansion's stage time for each, and the one-off walk scan's (stage 12).
--faults P (with --model q): both handles under replay_set_faults((P, P, 3 px, 3 px)), the faulted form of the expansion; the
JSON line then carries the fault counts of the timed frames and the lane group G the form was launched with."""
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


def up(x, a=256):
    return (x + a - 1) // a * a


def block_bytes(B, K, f_cap, nf, esz):
    """a frame's streamed block (csrc/input_layouts.h, FrameLayout): [rd | n | drop | k | M | off | slots | obs] at 256-byte offsets"""
    o = 0
    for per in (7 * K * esz, 4, 4, 4, 4 * f_cap, 4 * f_cap):
        o = up(o + B * per)
    return up(up(o + 4 * nf) + 2 * nf * esz)


def store_bytes(cells, K, f_cap, entries, esz):
    """the host store of `cells` cells with `entries` entries in all: the fixed sections and the compact work-lists"""
    return cells * (7 * K * esz + 12 + 8 * f_cap) + entries * (4 + 2 * esz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=30)
    ap.add_argument("--tracks", type=int, default=200)
    ap.add_argument("--sequences", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=128)
    ap.add_argument("--fill", type=int, default=30)
    ap.add_argument("--timed", type=int, default=40)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--model", choices=("sigma4", "q"), default="sigma4")
    ap.add_argument("--faults", type=float, default=0.0)
    args = ap.parse_args()
    N, F, S, B, fill, nf = args.window, args.tracks, args.sequences, args.sequences * args.seeds, args.fill, args.fill + args.timed
    K, esz = sc.IMU_PER_FRAME, 4
    cfg = sc.filter_config(N, isotropic=True)
    seqs = [sc.Trajectory(4, p, N, F, nf, cfg=cfg, imu_noise_scale=0.0, obs_noise_px=0.0, path_id=p % len(sc.PATHS)) for p in range(S)]
    seq_of = [b % S for b in range(B)]
    seeds = [0x5EED4000 + b for b in range(B)]
    q = cfg["Q_imu_diag"]
    sigma = (0.05 * np.sqrt(q[0] * sc.IMU_RATE), 0.05 * np.sqrt(q[6] * sc.IMU_RATE), 0.5 / cfg["f_u"], 0.5 / cfg["f_v"])   # Trajectory's default noise

    def handle():
        bt = capi.Batch(B, N, F, N, capi.F32)
        for b in range(B):
            bt.initialize(b, cfg, seqs[seq_of[b]].imu0)
        return bt

    def reinit(bt):
        for b in range(B):
            bt.initialize(b, cfg, seqs[seq_of[b]].imu0)

    t0 = time.time()
    rp = handle()
    rp.replay_alloc(S, nf, K)
    for f in range(nf):
        for s, tr in enumerate(seqs):
            fr = tr.frames[f]
            rp.replay_set_cell(f, s, tr.imu_for_frame(f), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    rp.replay_assign(seq_of, seeds, sigma)
    rp.replay_commit()
    t_replay_setup = time.time() - t0
    if args.model == "q":
        return model_q(args, rp, handle, reinit, seqs, seq_of, seeds, sigma, cfg)
    t0 = time.time()
    st = handle()
    st.scenario_alloc(nf, K)
    for f in range(nf):
        for b in range(B):
            ex = rp.replay_expand(f, b)
            st.scenario_set(f, b, ex["rd"][:max(ex["k"], 0)], ex["M"][:ex["n"]], ex["slots"], ex["obs"], ex["drop"])
    st.scenario_commit()
    st.scenario_pin(0, nf)
    t_streamed_setup = time.time() - t0

    paths = {"streamed": (st, st.run_frames_streamed), "replay": (rp, rp.run_frames_replay)}
    times = {k: [] for k in paths}
    for w in range(args.windows + 1):                       # window 0 warms both paths up and is not reported
        for name, (bt, run) in paths.items():
            reinit(bt)
            run(0, fill)
            bt.sync()
            t0 = time.perf_counter()
            run(fill, nf)
            bt.sync()
            if w:
                times[name].append(time.perf_counter() - t0)
    same = all(np.array_equal(st.imu_state(b), rp.imu_state(b)) for b in range(0, B, max(B // 16, 1)))

    # the expansion kernel alone, from the stage timers (one slice; event pairs carry their own overhead, reported beside it)
    reinit(rp)
    rp.run_frames_replay(0, fill)
    rp.profile_enable(True)
    rp.run_frames_replay(fill, nf)
    prof = rp.profile_read()
    overhead = rp.profile_event_overhead()
    rp.profile_enable(False)
    ms, cnt = prof["replay_expand"]

    seq_entries = [sum(int(tr.frames[f]["M"].sum()) for tr in seqs) for f in range(nf)]
    exp_entries = [sum(int(seqs[s].frames[f]["M"].sum()) for s in seq_of) for f in range(nf)]
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "shape": dict(dtype="f32", window=N, tracks=F, sequences=S, trajectories=B, fill_frames=fill, timed_frames=args.timed, windows=args.windows),
        "slices": {"streamed": st.effective_streams(True), "replay": rp.effective_streams(False)},
        "window_s": times, "median_window_s": med,
        "frames_per_s": {k: args.timed / v for k, v in med.items()},
        "ms_per_frame": {k: 1e3 * v / args.timed for k, v in med.items()},
        "replay_over_streamed_time": med["replay"] / med["streamed"],
        "same_final_states": bool(same),
        "expand_kernel_ms_per_frame": ms / max(cnt, 1), "expand_launches": cnt, "event_pair_overhead_ms": overhead,
        "bytes_per_frame": {
            "streamed": dict(host_store=store_bytes(B * nf, K, F, sum(exp_entries), esz) / nf,
                             page_locked=sum(block_bytes(B, K, F, e, esz) for e in exp_entries) / nf,
                             h2d=sum(block_bytes(B, K, F, e, esz) for e in exp_entries) / nf),
            "replay": dict(host_store=store_bytes(S * nf, K, F, sum(seq_entries), 8) / nf, page_locked=0, h2d=0,
                           h2d_once_at_commit=store_bytes(S * nf, K, F, sum(seq_entries), 8) + 4 * B * nf + 44 * B,
                           device_block_per_slice=block_bytes(B, K, F, max(exp_entries), esz)),
        },
        "setup_s": {"replay": t_replay_setup, "streamed_from_read_backs": t_streamed_setup},
    }
    print(json.dumps(out))
    st.close()
    rp.close()


def model_q(args, rp, handle, reinit, seqs, seq_of, seeds, sigma, cfg):
    """the sigma4 replay handle rp against a second one under the Q_imu model"""
    fill, nf, K = args.fill, args.fill + args.timed, sc.IMU_PER_FRAME
    Q = np.diag(np.asarray(cfg["Q_imu_diag"], dtype=np.float64))
    rq = handle()
    rq.replay_alloc(len(seqs), nf, K)
    for f in range(nf):
        for s, tr in enumerate(seqs):
            fr = tr.frames[f]
            rq.replay_set_cell(f, s, tr.imu_for_frame(f), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == args.window else 0)
    rq.replay_assign_q(seq_of, seeds, Q, 0.05, sigma[2:])
    rq.replay_commit()
    paths = {"replay": rp, "replay_q": rq}
    faults = {}
    if args.faults > 0.0:
        for bt in paths.values():
            bt.replay_set_faults((args.faults, args.faults, 3.0 / cfg["f_u"], 3.0 / cfg["f_v"]))
        cnt = rp.replay_fault_counts(fill, nf).sum(0)
        G = 16 if args.window <= 16 else 32 if args.window <= 32 else 64
        faults = dict(p_miss=args.faults, p_out=args.faults, counts_timed_frames=dict(zip(capi.REPLAY_FAULT_COUNTS, (int(x) for x in cnt))), lane_group=G,
                      wavefronts_per_trajectory=dict(tracks=(args.tracks * G + 63) // 64, fixed_sigma4=(4 * K + args.tracks + 1 + 63) // 64))
    times = {k: [] for k in paths}
    for w in range(args.windows + 1):                       # window 0 warms both paths up and is not reported
        for name, bt in paths.items():
            reinit(bt)
            bt.run_frames_replay(0, fill)
            bt.sync()
            t0 = time.perf_counter()
            bt.run_frames_replay(fill, nf)
            bt.sync()
            if w:
                times[name].append(time.perf_counter() - t0)
    stages = {}
    for name, bt in paths.items():
        reinit(bt)
        bt.run_frames_replay(0, fill)
        bt.profile_enable(True)
        if name == "replay_q":
            rq.replay_assign_q(seq_of, seeds, Q, 0.05, sigma[2:])     # the same assignment again: the next run tabulates the walk anew
        bt.run_frames_replay(fill, nf)
        prof = bt.profile_read()
        stages[name] = dict(expand_ms_per_frame=prof["replay_expand"][0] / max(prof["replay_expand"][1], 1), expand_launches=prof["replay_expand"][1],
                            walk_scan_ms=prof["replay_walk_scan"][0], walk_scan_launches=prof["replay_walk_scan"][1], event_pair_overhead_ms=bt.profile_event_overhead())
        bt.profile_enable(False)
    walk = rq.replay_walk()
    med = {k: statistics.median(v) for k, v in times.items()}
    entries = sum(int(seqs[s].frames[nf - 1]["M"].sum()) for s in seq_of)
    print(json.dumps({
        "shape": dict(dtype="f32", window=args.window, tracks=args.tracks, sequences=len(seqs), trajectories=len(seq_of), fill_frames=fill, timed_frames=args.timed, windows=args.windows),
        "slices": {k: bt.effective_streams(False) for k, bt in paths.items()},
        "window_s": times, "median_window_s": med, "ms_per_frame": {k: 1e3 * v / args.timed for k, v in med.items()},
        "model_over_sigma4_time": med["replay_q"] / med["replay"], "stages": stages, "faults": faults,
        "items_per_frame": {"entries": entries, "imu_sigma4": 3 * K * len(seq_of), "imu_model": K * len(seq_of)},
        "walk_table_bytes": int(walk.nbytes), "walk_rms_last_row": float(np.sqrt(np.mean(walk[-1] ** 2))),
    }))
    rp.close()
    rq.close()


if __name__ == "__main__":
    main()
