"""The lab recordings of the track compiler's tests (tests/test_track_compile.py on the CPU, tests/test_gpu_track_compile.py on
the device): id streams cut from scenario.Trajectory(3, 1, N, F, nf).stream() and compiled with their own (max_cam_states,
min_track_length, max_track_length), which are NOT the generator's -- the generator's tracks know when they end, the compiler
has to find out.

  A  N 12, F 6, 24 images; (6, 2, 1000)   the oldest camera keeps tracking: the window grows past max_cam_states, drops of 0 .. 4
  B  N 10, F 8, 30 images; (5, 3, 6)      tracks end by length (with an observation in the newest camera) and by loss
  C  N 8, F 6, 24 images; (7, 3, 4)
  D  B with hand edits: an inserted image with no features and no IMU samples, a duplicated id in a `cur` list, `cur` ids that
     are not tracked, tracks shorter than min_track_length, IMU counts of 9, 10 and 11
Handles of n_cap 16, f_cap 64, m_cap 16 hold all of them.  Everything is built once; nobody writes to it."""
import functools

import numpy as np

from msckf_mono_amd import scenario as sc

N_CAP, F_CAP, M_CAP, K = 16, 64, 16, 11
SPECS = {"A": (12, 6, 24, (6, 2, 1000)), "B": (10, 8, 30, (5, 3, 6)), "C": (8, 6, 24, (7, 3, 4)), "D": (10, 8, 30, (5, 3, 6))}
D_EMPTY_AT = 14          # D: an image inserted before B's image 14, without features and without IMU samples
D_SHORT_AT = (8, 20)     # D: a feature that is new on these images, tracked on the next one and then lost (2 < min_track_length)
D_DUP_AT = 11            # D: the first id of this image's `cur` list once more at its end, with other coordinates
D_STRAY_AT = (3, 17)     # D: `cur` ids nobody tracks
D_COUNTS = {4: 9, 5: 11, 22: 11, 23: 9}   # D: IMU samples of these images (the others 10; sums unchanged, so the stamps stay)


class Recording:
    """images[k] = dict(cur=(meas [n][2], ids [n]), new=(..), readings [k][7], state_id, time); cfg with the compile parameters"""

    def __init__(self, name):
        N, F, nf, (mcs, lo, hi) = SPECS[name]
        tr = sc.Trajectory(3, 1, N, F, nf)
        self.name, self.traj, self.params = name, tr, (mcs, lo, hi)
        self.cfg = dict(tr.cfg, max_cam_states=mcs, min_track_length=lo, max_track_length=hi)
        self.imu0 = tr.imu0
        st = tr.stream()
        arr = lambda p: (np.asarray(p[0], dtype=np.float64).reshape(-1, 2), np.asarray(p[1], dtype=np.uint64).reshape(-1))
        self.images = [dict(cur=arr(st[k]["cur"]), new=arr(st[k]["new"]), readings=tr.imu_for_frame(k), time=float(tr.frame_times[k])) for k in range(nf)]
        if name == "D":
            self._hand_edits()
        for k, im in enumerate(self.images):
            im["state_id"] = k

    def _hand_edits(self):
        im, tr = self.images, self.traj
        cat = lambda p, z, i: (np.concatenate([p[0], np.asarray(z, dtype=np.float64).reshape(-1, 2)]), np.concatenate([p[1], np.asarray(i, dtype=np.uint64)]))
        for j, k in enumerate(D_SHORT_AT):
            fid = 900000 + j
            im[k]["new"] = cat(im[k]["new"], [0.01 * (j + 1), -0.02], [fid])
            im[k + 1]["cur"] = cat(im[k + 1]["cur"], [0.012 * (j + 1), -0.021], [fid])
        cur = im[D_DUP_AT]["cur"]
        assert len(cur[1]) > 0
        im[D_DUP_AT]["cur"] = cat(cur, cur[0][0] + 0.05, [cur[1][0]])
        for j, k in enumerate(D_STRAY_AT):
            im[k]["cur"] = cat(im[k]["cur"], [[0.1, 0.1], [-0.1, 0.2]], [990000 + 2 * j, 990001 + 2 * j])
        # the IMU stream cut again: consecutive runs of the counts
        counts = [D_COUNTS.get(k, sc.IMU_PER_FRAME) for k in range(len(im))]
        assert sum(counts) == len(tr.readings)
        o = 0
        for k, c in enumerate(counts):
            im[k]["readings"] = tr.readings[o:o + c]
            o += c
        none = (np.zeros((0, 2)), np.zeros(0, dtype=np.uint64))
        im.insert(D_EMPTY_AT, dict(cur=none, new=none, readings=np.zeros((0, 7)), time=im[D_EMPTY_AT - 1]["time"]))


@functools.lru_cache(maxsize=None)
def recording(name):
    return Recording(name)


@functools.lru_cache(maxsize=None)
def compiled(name):
    """the recording's cells, one per image: capi.TrackCompiler.image's dicts (host code, no device)"""
    from msckf_mono_amd import capi
    rec = recording(name)
    tc = capi.TrackCompiler(*rec.params)
    return tuple(tc.image(im["cur"], im["new"]) for im in rec.images)


def id_driven_frame(o, im, prune=True):
    """one image through a filter with the reference's member names (the oracle, capi.MSCKF), by ids: asl.run's call order
    without pruneRedundantStates.  Returns (window before pruneEmptyStates, window after)."""
    o.propagate(im["readings"])
    o.augmentState(im["state_id"], im["time"])
    o.update(im["cur"][0], im["cur"][1])
    o.addFeatures(im["new"][0], im["new"][1])
    o.marginalize()
    n0 = o.getNumCamStates()
    o.pruneEmptyStates()
    return n0, o.getNumCamStates()


def cell_driven_frame(o, im, cell):
    """the same image through an oracle by position: the compiled cell alone"""
    o.propagate(im["readings"])
    o.augmentState(im["state_id"], im["time"])
    if len(cell["M"]):
        o.setTracks(cell["M"], cell["slots"], cell["obs"])
        o.marginalize()
    if cell["n_drop"]:
        o.dropOldest(cell["n_drop"])


def stage_scenario(bt, names):
    """recordings names[b] as trajectory b of a resident scenario on handle bt (asl.stage_scenario), committed; a trajectory
    whose recording is shorter skips the frames behind its end"""
    from msckf_mono_amd import asl
    nf = max(len(compiled(n)) for n in names)
    bt.scenario_alloc(nf, K)
    for b, n in enumerate(names):
        asl.stage_scenario(bt, as_compiled(n), b, K)
        for f in range(len(compiled(n)), nf):
            bt.scenario_set(f, b, np.zeros((0, 7)), [], [], np.zeros((0, 2)), 0, skip=True)
    bt.scenario_commit()
    return nf


def as_compiled(name):
    """the recording's cells in asl.compile_sequence's shape (stamp: the image's index)"""
    rec = recording(name)
    return dict(images=[dict(c, stamp=k, state_k=k, readings=rec.images[k]["readings"]) for k, c in enumerate(compiled(name))])
