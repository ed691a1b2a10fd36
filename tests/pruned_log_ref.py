"""numpy reference of the pruned-state log's pose error and of k_pruned_metrics' ten columns, shared by
test_pruned_log_host.py (which checks the error convention against np_oracle.update_quat) and test_gpu_pruned_log.py."""
import numpy as np

from msckf_mono_amd.capi import PRUNED_LOG_FIELDS as F    # the record's layout is the binding's table


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])


def qinv(q):
    q = np.asarray(q, dtype=np.float64)
    return np.array([q[0], -q[1], -q[2], -q[3]]) / np.dot(q, q)


def angle_error(q_hat, q_gt):
    """e_th with q_hat = buildUpdateQuat(e_th) * q_gt (msckf.h:851-872: the unit quaternion (sqrt(1 - |e/2|^2), -e/2)):
    e_th = -2 vec(q_hat * q_gt^-1), with the sign that makes the scalar part non-negative"""
    q_hat, q_gt = np.asarray(q_hat, dtype=np.float64), np.asarray(q_gt, dtype=np.float64)
    s = -1.0 if q_hat @ q_gt < 0 else 1.0
    u = qmul(s * q_hat - q_gt, qinv(q_gt))        # q_hat * q_gt^-1 = s (1 + (s q_hat - q_gt) * q_gt^-1): products of the small difference
    u[0] += 1.0
    return -2.0 * u[1:4] / np.linalg.norm(u)


def block6(tri):
    """the symmetric 6 x 6 block from its upper triangle, row by row (21 values)"""
    P = np.zeros((6, 6))
    P[np.triu_indices(6)] = tri
    return P + np.triu(P, 1).T


def triangle(P, k):
    """the 21 logged values of camera slot k from a full covariance matrix: entries (r, c), r <= c, of P[15 + 6 k ..][15 + 6 k ..]"""
    o = 15 + 6 * k
    return P[o:o + 6, o:o + 6][np.triu_indices(6)]


def numpy_metrics(rec, aug, b, q0, q1, gt):
    """the ten columns of pruned_log_metrics for trajectory b from its read-back (records [n][32], augment ordinals [n]) and
    gt [n_ord][B][7] (None: none); also the largest condition number of the blocks that entered the NEES sum"""
    out, kappa = np.zeros(10), 1.0
    n_ord = 0 if gt is None else len(gt)
    for r, o in zip(rec, aug):
        if not (q0 <= r[F["frame"]][0] < q1):
            continue
        out[0] += 1
        if o < 0 or o >= n_ord:
            out[9] += 1
            continue
        g = gt[o, b]
        e = np.concatenate([angle_error(r[F["q"]], g[0:4]), r[F["p"]] - g[4:7]])
        t2, p2 = e[0:3] @ e[0:3], e[3:6] @ e[3:6]
        out[1] += 1; out[2] += p2; out[3] = max(out[3], np.sqrt(p2)); out[4] += t2; out[5] = max(out[5], np.sqrt(t2))
        P = block6(r[F["cov"]])
        try:
            L = np.linalg.cholesky(P)
        except np.linalg.LinAlgError:
            out[8] += 1
            continue
        y = np.linalg.solve(L, e)
        out[6] += y @ y; out[7] += 1
        kappa = max(kappa, np.linalg.cond(P))
    return out, kappa
