"""The shapes, references and bounds of the tests of the full-state NEES log (tests/test_nees_inputs.py on the CPU,
tests/test_gpu_nees_log.py on the device): k_nees_log / k_nees_ensemble of csrc/kernels_log.hip and their numpy twin
scenario.nees_record.

Two geometries.  SMALL is the frame-log tests' (N = 8, F = 40, B = 6, 17 frames): the window fills and then drops one state per
frame.  The replay geometry is tests/replay_model_lab.py's (3 trajectories on 2 sequences under the Q_imu model, a cell with
k = 0 and a skipped one) over NF_REPLAY = 24 frames, which reach both of those cells.

The bar.  A NEES column is |L^-1 D^-1/2 e|^2 with D^-1/2 P_II D^-1/2 = C = L L^T, everything in double on both sides; what the
device and numpy do differently is the order of the sums of a 15 x 15 factorisation and solve, whose relative error is a small
multiple of kappa(C) 2^-53.  gpu_bar(kappa) = 100 kappa 2^-53 is the bar the frame-log and pruned-log NEES sums already use.
On the CPU the double oracle supplies states and covariances of the same geometries, so that the condition numbers the bar
rests on, and what a wrong definition would move, are known before a device is asked."""
import functools

import numpy as np

import replay_model_lab as ML
from msckf_mono_amd import scenario as sc

SMALL = dict(N=8, F=40, B=6, nf=8 + 9, m_cap=12)
ORACLE_TRAJS = (0, 4)              # the SMALL trajectories the double oracle walks (as the frame-log tests do)
NF_REPLAY = 24
EPS = 2.0 ** -53
COND_LIMIT = 1e-6                  # gpu_bar(kappa) of every record of the lab stays below this


def gpu_bar(kappa):
    return 100.0 * kappa * EPS


@functools.lru_cache(maxsize=None)
def small_trajs():
    g = SMALL
    return tuple(sc.Trajectory(2, 300 + b, g["N"], g["F"], g["nf"]) for b in range(g["B"]))


def sym_upper(P):
    """P_II as the kernel reads it: the upper triangle, mirrored"""
    U = np.triu(np.asarray(P, dtype=np.float64)[:15, :15])
    return U + np.triu(U, 1).T


def correlation(P):
    P = sym_upper(P)
    s = 1.0 / np.sqrt(np.diag(P))
    return P * s[:, None] * s[None, :], s


def corr_cond(P):
    """kappa(C) of C = D^-1/2 P_II D^-1/2, by numpy"""
    return float(np.linalg.cond(correlation(P)[0]))


def solve_columns(e, P):
    """the six columns from an error vector, independent of the twin's loops: z^T solve(C, z) (LU) for the 15-state and
    e_k^T solve(P_kk, e_k) for the five blocks"""
    C, s = correlation(P)
    P = sym_upper(P)
    z = e * s
    cols = [z @ np.linalg.solve(C, z)]
    for o in range(0, 15, 3):
        cols.append(e[o:o + 3] @ np.linalg.solve(P[o:o + 3, o:o + 3], e[o:o + 3]))
    return np.array(cols)


def plain_error_angle(q, q_gt):
    """e_th by the plain product q * q_gt^-1 (no difference form): -2 vec / norm, scalar part made non-negative"""
    g = np.asarray(q_gt, dtype=np.float64)
    u = sc.quat_mul(np.asarray(q, dtype=np.float64), np.concatenate([[g[0]], -g[1:]]) / (g @ g))
    if u[0] < 0:
        u = -u
    return -2.0 * u[1:] / np.linalg.norm(u)


# ------------------------------------------------------------------------------------------------------------------ the mutants
def diagonal_only(e, P):
    """column 0 with the correlations dropped: sum e_i^2 / P_ii"""
    cols = solve_columns(e, P)
    cols[0] = float(np.sum(e * e / np.diag(sym_upper(P))))
    return cols


def swapped_bg_v(e, P):
    m = e.copy()
    m[3:6], m[6:9] = e[6:9], e[3:6]
    return solve_columns(m, P)


def opposite_angle(e, P):
    m = e.copy()
    m[0:3] = -e[0:3]
    return solve_columns(m, P)


# ------------------------------------------------------------------------------------------------------------------ the oracle's records
def _record(o, truth16, **extra):
    return dict(imu16=np.array(o.getImuState()[:16]), P=np.array(o.getCovariance()[:15, :15]), truth16=np.array(truth16), **extra)


def small_records(po):
    """per ORACLE_TRAJS trajectory and frame of SMALL: dict(b, f, imu16, P, truth16) from the double oracle, free-running from
    ground truth"""
    import helpers as H
    g, trajs = SMALL, small_trajs()
    truth = sc.imu_state_gt(trajs, 0, g["nf"])
    out = []
    for b in ORACLE_TRAJS:
        tr = trajs[b]
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        for f in range(g["nf"]):
            H.oracle_frame(o, tr, f, g["N"])
            out.append(_record(o, truth[f, b], b=b, f=f))
    return out


def replay_truth(nf=NF_REPLAY):
    """the replay's truth table, rows by sequence: [nf][S][16] (constant biases: the walk is added on the device)"""
    return sc.imu_state_gt(ML._paths(nf), 0, nf)


def replay_records(po, nf=NF_REPLAY):
    """per trajectory and frame of the replay geometry: dict(b, f, imu16, P, truth16 -- the sequence's row, constant biases --,
    walk [nf + 1][6], skipped) from the double oracle on the twin's cells (replay_model_lab.twin_cell)"""
    truth = replay_truth(nf)
    out = []
    for b in range(ML.B):
        s, path = ML.SEQ_OF[b], ML._paths(nf)[ML.SEQ_OF[b]]
        walk = ML.twin_walk(nf, b)
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(*ML.init_of(nf, b))
        for f in range(nf):
            rd0, M, slots, _, drop, skip = ML.sequences(nf)[s][f]
            if not skip:
                rd, obs = ML.twin_cell(nf, f, b, walk)
                if len(rd0):
                    o.propagate(rd[:len(rd0)])
                o.augmentState(f, path.frame_times[f])
                if len(M):
                    o.setTracks(M, slots, obs)
                    o.marginalize()
                if drop:
                    o.dropOldest(drop)
            out.append(_record(o, truth[f, s], b=b, f=f, walk=walk, skipped=bool(skip)))
    return out


def with_walk(truth16, walk_row):
    """the truth row with a walk row added to b_g and b_a"""
    t = np.array(truth16, dtype=np.float64)
    t[4:7] += walk_row[0:3]
    t[10:13] += walk_row[3:6]
    return t
