"""The shapes and bounds of the tests of the Monte-Carlo replay's Q_imu model (tests/test_replay_model_plan.py and
tests/test_replay_model_inputs.py on the CPU, tests/test_gpu_replay_model.py on the device): noise drawn from the filter's own
12 x 12 Q_imu, with the two bias random walks (csrc/replay_plan.h, MODEL).

The smallest shapes at which the model can still go wrong: S = 2 sequences, B = 3 trajectories (0 and 2 replay sequence 1 with
different seeds), K = 4 samples per cell at most, a window of 6 cameras and at most 3 tracks.  A sequence's cells come from a
noise-free scenario.Trajectory whose ten equal samples per frame are merged into k_f samples of unequal dT (means over 3 | 3 | 2 |
2 of them, 4 | 3 | 3, or all ten), so the filter still follows the path; sequence 1 has a cell with k = 0 and a skipped one.
Nearly all frames carry no track: the frame counts straddle the scan's chunk and the filter's work stays negligible.

Bounds (double).  eps0 = 1e-13 is the project's per-unit-draw figure: the device's and numpy's ln, sqrt,
cos and sin differ by that much per unit draw at the most, every other operation of the model is the same rounded operation in
the same order on both sides.  A draw z_c enters w_r with weight L_rc, so |dw_r| <= eps0 sum_c |L_rc|; one increment is scale w_r
sqrt(dT), and a walk row after n samples has collected n of them:
    walk_tol = eps0 scale sqrt(dT_max) (sum_c |L_rc|) n + ulp(value)
A stored reading adds its own white noise, scale w_r / sqrt(dT_i), to the walk at its sample:
    imu_tol  = eps0 scale (sum_c |L_rc|) / sqrt(dT_i) + walk_tol(samples before it) + ulp(value)
An observation is value + sigma n with one draw: eps0 sigma + ulp(value)."""
import functools

import numpy as np

from msckf_mono_amd import scenario as sc

EPS0 = 1e-13
N, F = 6, 3
N_CAP = M_CAP = 6
F_CAP = 3
K = 4
B, S = 3, 2
SEQ_OF = [1, 0, 1]
SEEDS = [0xB1A5ED00, 0xB1A5ED01, 0xB1A5ED02]
SIGMA_UV = (0.5 / 458.654, 0.5 / 458.654)
SCALE = [0.05, 0.08, 0.05]
TRACK_FRAMES = (6, 7, 8, 9, 10, 30)          # the frames that carry tracks (all others: none)
ZERO_FRAME, SKIP_FRAME = 20, 22              # sequence 1: a cell with k = 0, a skipped cell
GROUPS = {4: (3, 3, 2, 2), 3: (4, 3, 3), 1: (10,)}
WHITE, WALK_G, WALK_A = [0, 1, 2, 6, 7, 8], [3, 4, 5], [9, 10, 11]
WALK_ROWS = WALK_G + WALK_A


def _correlation(seed, n):
    g = sc.SplitMix64(seed).normal(n * n).reshape(n, n)
    c = g @ g.T / n + np.eye(n)
    d = np.sqrt(np.diag(c))
    return c / np.outer(d, d)


def _q_diag():
    return np.asarray(sc.filter_config(N)["Q_imu_diag"], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def q_dense():
    """a dense correlated Q_imu on filter_config's diagonal"""
    d = np.sqrt(_q_diag())
    return d[:, None] * _correlation(0x0D15E, 12) * d[None, :]


@functools.lru_cache(maxsize=None)
def q_no_walk():
    """correlated white noise, both walk blocks zero (positive semi-definite: six zero columns in L)"""
    q = np.zeros((12, 12))
    d = np.sqrt(_q_diag()[WHITE])
    q[np.ix_(WHITE, WHITE)] = d[:, None] * _correlation(0x0D15F, 6) * d[None, :]
    return q


@functools.lru_cache(maxsize=None)
def q_white_diag():
    """diag(white only): no correlation, no walk"""
    q = np.zeros((12, 12))
    q[WHITE, WHITE] = _q_diag()[WHITE]
    return q


def q_of():
    """Q per trajectory: dense, zero walk blocks, dense"""
    return [q_dense(), q_no_walk(), q_dense()]


@functools.lru_cache(maxsize=None)
def factors():
    return tuple(sc.replay_noise_factor(q) for q in q_of())


def k_of(s, f):
    """samples of sequence s's cell on frame f; -1: skipped"""
    if s == 1 and f == ZERO_FRAME:
        return 0
    if s == 1 and f == SKIP_FRAME:
        return -1
    return (4, 3, 1, 4)[(f + s) % 4]


def merged(rd10, k):
    """ten equal samples as k samples: per group the mean reading and the summed dT"""
    out, at = np.zeros((k, 7)), 0
    for i, g in enumerate(GROUPS[k]):
        out[i, :6] = rd10[at:at + g, :6].mean(0)
        out[i, 6] = rd10[at:at + g, 6].sum()
        at += g
    return out


@functools.lru_cache(maxsize=None)
def _paths(nf):
    return tuple(sc.Trajectory(7, p, N, F, nf, imu_noise_scale=0.0, obs_noise_px=0.0, path_id=p) for p in (0, 1))


@functools.lru_cache(maxsize=None)
def sequences(nf):
    """per sequence and frame the noise-free cell (readings [k][7], M, slots, obs, n_drop, skip); built once per frame count"""
    seqs = []
    for s, tr in enumerate(_paths(nf)):
        cells = []
        for f in range(nf):
            k, fr = k_of(s, f), tr.frames[f]
            drop = 1 if fr["Nw"] == N else 0
            if k < 0:
                cells.append((np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), 0, True))
            elif f in TRACK_FRAMES and k > 0:
                cells.append((merged(tr.imu_for_frame(f), k), fr["M"], fr["slots"], fr["obs"], drop, False))
            else:
                rd = merged(tr.imu_for_frame(f), k) if k else np.zeros((0, 7))
                cells.append((rd, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)), drop, False))
        seqs.append(tuple(cells))
    return tuple(seqs)


def init_of(nf, b):
    """(cfg, imu0) trajectory b's filter starts from"""
    tr = _paths(nf)[SEQ_OF[b]]
    return tr.cfg, tr.imu0


def stage_sequences(bt, nf):
    bt.replay_alloc(S, nf, K)
    for f in range(nf):
        for s in range(S):
            rd, M, slots, obs, drop, skip = sequences(nf)[s][f]
            bt.replay_set_cell(f, s, rd, M, slots, obs, drop, skip=skip)


def stage_replay(bt, nf, seeds=SEEDS, scale=SCALE, Q=None, sigma_uv=SIGMA_UV):
    """the sequences as a replay on handle bt under the model, assigned and committed"""
    stage_sequences(bt, nf)
    bt.replay_assign_q(SEQ_OF, seeds, q_of() if Q is None else Q, scale, sigma_uv)
    bt.replay_commit()


def readings_of(nf, b, seq_of=SEQ_OF):
    return [sequences(nf)[seq_of[b]][f][0] for f in range(nf)]


def twin_walk(nf, b, seeds=SEEDS, scale=SCALE):
    return sc.replay_walk(readings_of(nf, b), seeds[b], factors()[b], scale[b])


def twin_cell(nf, f, b, walk, seeds=SEEDS, scale=SCALE):
    """trajectory b's cell of frame f by the numpy twin: (readings [K][7], obs [n][2])"""
    rd, _, _, obs, _, _ = sequences(nf)[SEQ_OF[b]][f]
    return sc.replay_model_cell(rd, obs, f, seeds[b], factors()[b], scale[b], SIGMA_UV, walk[f], K=K)[:2]


# ------------------------------------------------------------------------------------------------------------------ the bounds
def row_weight(L):
    """sum_c |L_rc| per row"""
    return np.abs(np.asarray(L)).sum(1)


def samples_before(cells):
    """n[f]: the samples of the frames before f (frames + 1 values)"""
    return np.concatenate([[0], np.cumsum([len(c) for c in cells])])


def dt_max(cells):
    return max([float(c[:, 6].max()) for c in cells if len(c)] + [0.0])


def walk_tol(L, scale, dtmax, n, value):
    """[.., 6] for walk values `value` [.., 6] that have collected n [..] samples"""
    n = np.asarray(n, dtype=np.float64)[..., None]
    return EPS0 * scale * np.sqrt(dtmax) * row_weight(L)[WALK_ROWS] * n + np.spacing(np.abs(value))


def imu_tol(L, scale, dtmax, n_before, dT, value, walk_value):
    """[k][6] for the stored readings `value` [k][6] of a cell whose frame starts after n_before samples; dT [k] (> 0)"""
    k = len(dT)
    white = EPS0 * scale * row_weight(L)[WHITE][None, :] / np.sqrt(np.asarray(dT, dtype=np.float64))[:, None]
    walk = EPS0 * scale * np.sqrt(dtmax) * row_weight(L)[WALK_ROWS][None, :] * (n_before + np.arange(k))[:, None] + np.spacing(np.abs(walk_value))
    return white + walk + np.spacing(np.abs(value))


def obs_tol(value):
    return EPS0 * np.asarray(SIGMA_UV)[None, :] + np.spacing(np.abs(value))
