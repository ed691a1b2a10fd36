"""k_feature_pair under co-residency: what a trajectory's wavefronts leave per track must not depend on what runs beside them.

One trajectory at a full 30-camera window with 8 hand-made tracks of 2, 3, 4, 16, 27, 28, 29 and 30 observations -- the pair form
puts the longest with the shortest (30 + 2, 29 + 3, 28 + 4, 27 + 16), so the wavefronts with the 8-block gate factorization, the
kernel's register peak, are the ones that also carry a second track.  The update runs once alone and once as each of 20 identical
trajectories of one launch, pairs forced (MSCKF_HIP_FEATURE_PAIR=2) both times.  Per track the flags, gamma, the point, first and
last camera slot, the whitened H_x blocks and residuals and the rows of B^ must be the same bits alone and in every one of the 20
copies.  On a correct build this holds by construction (a trajectory's wavefronts read nothing of their neighbours'): it guards
the addressing of scratch and LDS with sixteen wavefronts on a compute unit."""
import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc

pytestmark = pytest.mark.gpu

N = 30
LENGTHS = (2, 3, 4, 16, 27, 28, 29, 30)
COPIES = 20
NOISE_PX = 0.5


def _fill_window(capi):
    """a float device filter run until its window holds N = 30 camera states; returns the trajectory and its state"""
    tr = sc.Trajectory(5, 21, N, 8, N + 4)
    bt = capi.Batch(1, N, 8, N, capi.F32)
    bt.initialize(0, tr.cfg, tr.imu0)
    for k in range(N + 2):
        H.device_frame(bt, 0, tr, k, N)
    bt.propagate_range(0, 1, tr.imu_for_frame(N + 2))
    bt.augment_range(0, 1)
    cams, _ = bt.cam_states(0)
    # N + 2 whole frames, each dropping the oldest camera of a full window, then frame N + 2's camera: slot s holds frame 3 + s
    state = dict(P=bt.covariance(0), imu=bt.imu_state(0), cams=cams, frames=np.arange(3, N + 3), nres=bt.num_residualized(0))
    bt.close()
    assert len(cams) == N and state["nres"] > 3, (len(cams), state["nres"])
    return tr, state


def _tracks(tr, frames):
    """one landmark per length that all N ground-truth cameras of the window see in front of them, observed with 0.5 px of noise
    in L slots spread over the window"""
    C, p = tr.C_CG[frames], tr.p_C[frames]
    rng = sc.SplitMix64(0xF3A70030)
    lms = []
    while len(lms) < len(LENGTHS):
        u = rng.uniform(3)
        d = 3.0 + 5.0 * u[2]
        pc = np.array([d * np.tan(0.5 * (2 * u[0] - 1)), d * np.tan(0.5 * (2 * u[1] - 1)), d])
        pw = pc @ C[N // 2] + p[N // 2]
        q = np.einsum("sij,sj->si", C, pw[None, :] - p)
        if np.all((q[:, 2] > 0.5) & (np.abs(q[:, 0]) < 3 * q[:, 2]) & (np.abs(q[:, 1]) < 3 * q[:, 2])):
            lms.append(pw)
    M, slots, obs = [], [], []
    for L, pw in zip(LENGTHS, lms):
        s = np.round(np.linspace(0, N - 1, L)).astype(np.int32)
        q = np.einsum("sij,sj->si", C[s], pw[None, :] - p[s])
        z = q[:, :2] / q[:, 2:3] + (NOISE_PX / tr.cfg["f_u"]) * rng.normal(2 * L).reshape(L, 2)
        M.append(L); slots.append(s); obs.append(z)
    return np.array(M, np.int32), np.concatenate(slots).astype(np.int32), np.concatenate(obs), slots


def _run(capi, tr, state, wl, B):
    bt = capi.Batch(B, N, len(LENGTHS) + 1, N, capi.F32)
    for b in range(B):
        bt.initialize(b, tr.cfg, tr.imu0)
        bt.set_covariance(b, state["P"])
        bt.set_imu_state(b, state["imu"])
        for i, c in enumerate(state["cams"]):
            bt.set_cam_pose(b, i, c)
        bt.set_num_residualized(b, state["nres"])
        bt.set_tracks(b, *wl)
    bt.marginalize_range(0, B)
    out = []
    for b in range(B):
        blk = bt.last_track_blocks(b)
        blk["tracks"], blk["stats"] = bt.last_tracks(b), bt.last_stats(b)
        out.append(blk)
    bt.close()
    return out


def _stored(blk, slot_lists):
    """what the kernel stored of every track, stale entries of the buffers left out: rows of the track's observations, columns of
    B^ inside its slot range, the column of c"""
    parts = [blk["tracks"].ravel(), blk["first"].astype(np.float64), blk["last"].astype(np.float64)]
    for t, s in enumerate(slot_lists):
        L, lo, hi = len(s), int(s.min()), int(s.max())
        parts += [blk["Hx"][t, :L].ravel(), blk["rw"][t, :L].ravel(), blk["B"][t, :, 6 * lo:6 * hi + 6].ravel(), blk["B"][t, :, 6 * N].ravel()]
    return np.concatenate(parts)


def test_pair_wavefronts_alone_and_among_twenty_trajectories(monkeypatch):
    from msckf_mono_amd import capi
    capi.lib()
    tr, state = _fill_window(capi)
    M, slots, obs, slot_lists = _tracks(tr, state["frames"])
    monkeypatch.setenv("MSCKF_HIP_FEATURE_PAIR", "2")
    alone = _run(capi, tr, state, (M, slots, obs), 1)[0]
    many = _run(capi, tr, state, (M, slots, obs), COPIES)
    F = len(LENGTHS)
    assert len(alone["tracks"]) == F and alone["stats"]["n_tracks"] == F
    print("flags [motion_ok tri_valid gate_pass included] gamma per track:", alone["tracks"][:, :5].tolist())
    # 0.5 px tracks: the float and the double oracle accept all eight on this window, every gamma a tenth of its threshold or less
    # (0.009 against 0.35 at two observations, 0.41 against 19.3 at thirty)
    assert np.all(alone["tracks"][:, :4] == 1), alone["tracks"][:, :5]
    # the stored slot range is the list's, every stored value is a number, and the Jacobian of an observed row is not empty
    assert [int(x) for x in alone["first"]] == [int(s.min()) for s in slot_lists]
    assert [int(x) for x in alone["last"]] == [int(s.max()) for s in slot_lists]
    want = _stored(alone, slot_lists)
    assert np.all(np.isfinite(want))
    for t, s in enumerate(slot_lists):
        assert np.all(np.abs(alone["Hx"][t, :len(s)]).sum(axis=(1, 2)) > 0), t
    for b, blk in enumerate(many):
        got = _stored(blk, slot_lists)
        assert blk["stats"] == alone["stats"], (b, blk["stats"], alone["stats"])
        assert got.shape == want.shape and np.array_equal(got, want), (b, np.nonzero(got != want)[0][:8], np.abs(got - want).max())
