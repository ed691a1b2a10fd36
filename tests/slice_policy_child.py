"""Child process of tests/test_gpu_slice_policy.py: the hardware-queue budget belongs to a process (the runtime reads
GPU_MAX_HW_QUEUES once), so every budget is a fresh process with the variable in its environment (capi.Batch passes its value on to the handle it creates).  Runs the frame loops of
the small cases and writes every dump and the effective slice counts to the .npz named on the command line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from msckf_mono_amd import capi, scenario as sc   # noqa: E402

N, F, NF, RING = 6, 24, 12, 3     # 6-camera window, 24 tracks, 12 frames: a ring of 3 wraps four times, the last frame prunes with its own launch
BATCHES = (8, 3, 1)
EXACT = "--exact" in sys.argv[2:]   # every handle runs exactly the slices it is asked for (msckf_hip_set_slices_exact)


def batch(trajs, with_state=True):
    bt = capi.Batch(len(trajs), N, F, N, capi.F32)
    if with_state:
        for b, tr in enumerate(trajs):
            bt.initialize(b, tr.cfg, tr.imu0)
    bt.scenario_alloc(NF, sc.IMU_PER_FRAME)
    for k in range(NF):
        for b, tr in enumerate(trajs):
            fr = tr.frames[k]
            bt.scenario_set(k, b, tr.imu_for_frame(k), fr["M"], fr["slots"], fr["obs"], 1 if fr["Nw"] == N else 0)
    bt.scenario_commit()
    bt.set_upload_ring(RING, 0)
    bt.set_slices_exact(EXACT)
    return bt


def dump(bt, B):
    """IMU states, camera poses, covariances and gate statistics of every trajectory after the last frame"""
    bt.sync()
    stats = [bt.last_stats(b) for b in range(B)]
    keys = sorted(stats[0])
    return dict(imu=np.stack([bt.imu_state(b) for b in range(B)]), cams=np.stack([bt.cam_states(b)[0] for b in range(B)]),
                cov=np.stack([bt.covariance(b) for b in range(B)]), stats=np.array([[float(s[k]) for k in keys] for s in stats]))


def main():
    out = {}
    counts = {}
    for B in BATCHES:
        trajs = [sc.Trajectory(2, 500 + b, N, F, NF) for b in range(B)]
        for name, streams, streamed in (("one", 1, False), ("resident", 4, False), ("streamed", 4, True)):
            bt = batch(trajs)
            bt.set_streams(streams)
            counts["%s_B%d" % (name, B)] = bt.effective_streams(streamed)
            (bt.run_frames_streamed if streamed else bt.run_frames)(0, NF)
            for k, v in dump(bt, B).items():
                out["%s_B%d_%s" % (name, B, k)] = v
            bt.close()          # "one": a handle on which only run_frames with 1 stream ever ran -- its other streams were never used
        # a copy made before any frame loop ran on either handle, then 4 slices on the copy: streams that nothing had used yet
        src = batch(trajs)
        dst = batch(trajs, with_state=False)
        dst.copy_state_from(src)
        src.close()
        dst.set_streams(4)
        counts["copy_B%d" % B] = dst.effective_streams(False)
        dst.run_frames(0, NF)
        for k, v in dump(dst, B).items():
            out["copy_B%d_%s" % (B, k)] = v
        dst.close()
    np.savez(sys.argv[1], **out)
    print(json.dumps(counts))


if __name__ == "__main__":
    main()
