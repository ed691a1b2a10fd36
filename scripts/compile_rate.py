"""A compiled recording in the frame loop beside the per-image id path (recorded, not asserted).

The recording is lab recording B of the track compiler's tests: the id stream of scenario.Trajectory(3, 1, 10, 8, 30), compiled
with max_cam_states 5, min_track_length 3, max_track_length 6 -- windows of up to 6 cameras, up to 12 tracks per image -- tiled to
the benchmark's 128 trajectories (float, handle of n_cap 16, f_cap 64, m_cap 16).
  compile      the host time of capi.TrackCompiler over the recording's images (no device), 128 times over
  frame_loop   run_frames over the compiled cells, all 30 images in one call
  id_path      per image propagate_range + msckf_hip_image_cycle_range with flags = 2 (pruneEmptyStates, no pruneRedundantStates)
               on the same ids: the host bookkeeping runs inside the loop
  imu_sums     msckf_hip_replay_imu_sums over all frames of the recording staged as one replay sequence with 128 seeds (wall
               time of the call, plan already on the device)
Windows alternate in one process; window 0 warms up and is not reported.  Both paths end in the same window sizes (checked).
Prints one JSON line."""
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

from msckf_mono_amd import asl, capi, scenario as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=128)
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    B = args.trajectories
    N, F, nf, params = 10, 8, 30, (5, 3, 6)
    n_cap, f_cap, m_cap, K = 16, 64, 16, sc.IMU_PER_FRAME
    tr = sc.Trajectory(3, 1, N, F, nf)
    cfg = dict(tr.cfg, max_cam_states=params[0], min_track_length=params[1], max_track_length=params[2])
    st = tr.stream()
    arr = lambda p: (np.asarray(p[0], dtype=np.float64).reshape(-1, 2), np.asarray(p[1], dtype=np.uint64).reshape(-1))
    images = [dict(cur=arr(st[k]["cur"]), new=arr(st[k]["new"])) for k in range(nf)]

    def compile_once():
        tc = capi.TrackCompiler(*params)
        cells = [tc.image(im["cur"], im["new"]) for im in images]
        tc.close()
        return cells

    compile_once()
    t0 = time.perf_counter()
    for _ in range(B):
        cells = compile_once()
    t_compile = time.perf_counter() - t0
    comp = dict(images=[dict(c, stamp=k, state_k=k, readings=tr.imu_for_frame(k)) for k, c in enumerate(cells)])

    def handle():
        bt = capi.Batch(B, n_cap, f_cap, m_cap, capi.F32)
        reinit(bt)
        return bt

    def reinit(bt):
        for b in range(B):
            bt.initialize(b, cfg, tr.imu0)

    fl = handle()
    fl.scenario_alloc(nf, K)
    for b in range(B):
        asl.stage_scenario(fl, comp, b, K)
    fl.scenario_commit()
    ip = handle()
    packed = [capi.Batch.pack_image_inputs(B, [k] * B, [float(tr.frame_times[k])] * B, [images[k]["cur"]] * B, [images[k]["new"]] * B) for k in range(nf)]
    rd = [np.tile(tr.imu_for_frame(k), (B, 1, 1)) for k in range(nf)]

    def run_frame_loop():
        fl.run_frames(0, nf)
        fl.sync()

    def run_id_path():
        for k in range(nf):
            ip.propagate_range(0, B, rd[k])
            ip.image_cycle_range_packed(0, B, packed[k], prune_redundant=False, prune_empty=True)
        ip.sync()

    paths = {"frame_loop": (fl, run_frame_loop), "id_path": (ip, run_id_path)}
    times = {k: [] for k in paths}
    for w in range(args.windows + 1):
        for name, (bt, run) in paths.items():
            reinit(bt)
            bt.sync()
            t0 = time.perf_counter()
            run()
            if w:
                times[name].append(time.perf_counter() - t0)
    same = all(fl.num_cam_states(b) == ip.num_cam_states(b) for b in range(B))
    updates = sum(1 for c in cells if len(c["M"])) * B

    # the sums kernel: the recording as one noise-free sequence, 128 seeds
    fl.replay_alloc(1, nf, K)
    asl.stage_replay(fl, comp, 0)
    fl.replay_assign([0] * B, [0x5EED5000 + b for b in range(B)], (7e-3, 7e-2, 1e-3, 1e-3))
    fl.replay_commit()
    fl.replay_imu_sums(0, nf)
    t_sums = []
    for _ in range(5):
        t0 = time.perf_counter()
        sums = fl.replay_imu_sums(0, nf)
        t_sums.append(time.perf_counter() - t0)

    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "shape": dict(dtype="f32", recording="B", images=nf, trajectories=B, params=params, n_cap=n_cap, f_cap=f_cap, m_cap=m_cap,
                      max_window=max(c["window"] for c in cells), max_tracks_per_image=max(len(c["M"]) for c in cells), tracks=sum(len(c["M"]) for c in cells)),
        "compile_s": dict(all_trajectories=t_compile, per_recording=t_compile / B, per_image=t_compile / B / nf),
        "window_s": times, "median_window_s": med, "ms_per_frame": {k: 1e3 * v / nf for k, v in med.items()},
        "updates_per_s": {k: updates / v for k, v in med.items()},
        "id_path_over_frame_loop_time": med["id_path"] / med["frame_loop"], "same_window_sizes": bool(same),
        "slices": fl.effective_streams(False),
        "imu_sums_call_ms": dict(median=1e3 * statistics.median(t_sums), all=[1e3 * x for x in t_sums], samples_per_trajectory=float(sums[0, 0])),
    }))
    fl.close()
    ip.close()


if __name__ == "__main__":
    main()
