"""The aligned trajectory error, in numpy: the twin of csrc/kernels_traj.hip (k_traj_align, k_traj_rpe) and of the closing maths
of csrc/traj_plan.h, one trajectory at a time.

ATE after a yaw-plus-translation alignment (the gauge of a VIO: gravity is (0, 0, -9.81) throughout), after an SE(3) alignment,
and the gauge-free relative pose error over a lag -- Zhang & Scaramuzza's trajectory-evaluation tutorial; no scale.  A pose is
7 numbers, q (w, x, y, z) whose rotation matrix C(q) takes global vectors into the body frame (q_IG), then p.  Notation: p the
estimate, g the ground truth, _c centred on its own mean; the alignment sought is g ~ R p + t.

dtype=np.longdouble gives the reference the device is measured against (the eigenvector is then found by a Jacobi iteration in
that type; in float64 by np.linalg.eigh)."""
import numpy as np

from . import scenario as sc

ALIGN_NONE, ALIGN_YAW, ALIGN_SE3 = 0, 1, 2
ALIGN_ROW, RPE_ROW = 20, 4


# ------------------------------------------------------------------ quaternions, in the type of their arguments
def quat_rot(q):
    """Eigen's toRotationMatrix of (w, x, y, z) quaternions [..., 4]: [..., 3, 3]"""
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def quat_mul(a, b):
    """Hamilton product [..., 4]"""
    aw, ax, ay, az = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bw, bx, by, bz = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx], -1)


def quat_inv(q):
    """conjugate / squared norm, Eigen's inverse()"""
    return q * np.array([1, -1, -1, -1], dtype=q.dtype) / np.sum(q * q, axis=-1, keepdims=True)


def error_angle(q, g):
    """scenario.error_angle on rows [n, 4], in their type: e_th with q = update_quat(e_th) * g, from the small difference"""
    s = np.where(np.sum(q * g, axis=-1, keepdims=True) < 0, -1, 1).astype(q.dtype)
    u = quat_mul(s * q - g, quat_inv(g))
    u[..., 0] += 1
    return -2 * u[..., 1:] / np.sqrt(np.sum(u * u, axis=-1, keepdims=True))


# ------------------------------------------------------------------ the closing maths (csrc/traj_plan.h, section 4)
def horn_matrix(S):
    """Horn 1987's symmetric 4 x 4 matrix N of S = sum p_c g_c^T: its eigenvector of largest eigenvalue is the Hamilton quaternion
    (w, x, y, z) of the rotation R with g ~ R p"""
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]], dtype=S.dtype)


def jacobi_eigh(N, sweeps=30):
    """(eigenvalues, eigenvectors in columns) of a small symmetric matrix by the cyclic Jacobi iteration, in N's own type"""
    A, n = N.copy(), N.shape[0]
    V = np.eye(n, dtype=N.dtype)
    eps = np.finfo(N.dtype).eps
    fro2 = np.sum(A * A)
    for _ in range(sweeps):
        off2 = 2 * sum(A[p, q] * A[p, q] for p in range(n) for q in range(p + 1, n))     # (summed directly: no cancellation)
        if off2 <= eps * eps * fro2:
            break
        for p in range(n):
            for q in range(p + 1, n):
                if A[p, q] == 0:
                    continue
                tau = (A[q, q] - A[p, p]) / (2 * A[p, q])
                t = (1 if tau >= 0 else -1) / (abs(tau) + np.hypot(1, tau))
                c = 1 / np.sqrt(1 + t * t)
                s = t * c
                J = np.eye(n, dtype=N.dtype)
                J[p, p] = J[q, q] = c; J[p, q] = s; J[q, p] = -s
                A = J.T @ A @ J
                V = V @ J
                A[p, q] = A[q, p] = 0
    return np.diag(A).copy(), V


def close_yaw(S, pxy, gxy, dtype):
    """(R, q, cond): theta = atan2(W10 - W01, W00 + W11) of W = S^T, cond = hypot(.) / sqrt(pxy gxy); flat without horizontal extent"""
    R, q = np.eye(3, dtype=dtype), np.array([1, 0, 0, 0], dtype=dtype)
    A, B = S[0, 0] + S[1, 1], S[0, 1] - S[1, 0]
    h = np.sqrt(A * A + B * B)
    den = np.sqrt(pxy * gxy)
    if not (pxy > 0 and gxy > 0 and h > 0 and den > 0):
        return R, q, dtype(0)
    c, s = A / h, B / h
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = c, -s, s, c
    th = np.arctan2(B, A)
    q = np.array([np.cos(th / 2), 0, 0, np.sin(th / 2)], dtype=dtype)     # |th| <= pi: the scalar part is >= 0
    return R, q, min(h / den, dtype(1))


def close_se3(S, dtype):
    """(R, q, cond): the eigenvector of largest eigenvalue of Horn's N, cond = (l1 - l2) / l1; always a proper rotation"""
    N = horn_matrix(S)
    if not np.any(N):
        return np.eye(3, dtype=dtype), np.array([1, 0, 0, 0], dtype=dtype), dtype(0)
    if dtype == np.float64:
        lam, V = np.linalg.eigh(N)
    else:
        lam, V = jacobi_eigh(N)
    k = int(np.argmax(lam))                                          # the first of equal ones
    l1, l2 = lam[k], np.max(np.delete(lam, k))
    if not l1 > 0:
        return np.eye(3, dtype=dtype), np.array([1, 0, 0, 0], dtype=dtype), dtype(0)
    q = V[:, k].astype(dtype)
    q = q / np.sqrt(np.sum(q * q))
    if q[0] < 0:
        q = -q
    return quat_rot(q), q, min(max((l1 - l2) / l1, dtype(0)), dtype(1))


def closing(mode, n, pbar, gbar, S, pp, gg, pxy, gxy, dtype=np.float64):
    """(R, q, t, cond) from the record count, the means and the centred sums.  Flat -- R = I, cond = 0 -- when n <= 1, all p_c or
    all g_c are zero, or (yaw) there is no horizontal extent; t = gbar - R pbar in both aligned modes"""
    R, q, cond = np.eye(3, dtype=dtype), np.array([1, 0, 0, 0], dtype=dtype), dtype(0)
    if mode == ALIGN_NONE or n == 0:
        return R, q, np.zeros(3, dtype=dtype), cond
    if n > 1 and pp > 0 and gg > 0:
        R, q, cond = close_yaw(S, pxy, gxy, dtype) if mode == ALIGN_YAW else close_se3(S, dtype)
    return R, q, gbar - R @ pbar, cond


# ------------------------------------------------------------------ the two reductions
def align(est7, gt7, mode, dtype=np.float64, centred=True):
    """One trajectory, est7 and gt7 [n][7]: the row of 20 of msckf_hip_traj_align (capi.ALIGN_FIELDS) -- n, R row by row, t, cond,
    sum |e|^2, max |e|, |e| at the last record (e = R p + t - g, formed as R p_c - g_c), sum |e_th|^2 and max |e_th| of the
    aligned attitude C(q) R^T = C(q * q_R^-1) against the truth, and sum |p - g|^2 before alignment.
    centred=False expands the cross matrix and the extents from raw moments -- what the kernel must not do: the tests use it to
    show that their bar catches it."""
    if mode not in (ALIGN_NONE, ALIGN_YAW, ALIGN_SE3):
        raise ValueError("mode is ALIGN_NONE, ALIGN_YAW or ALIGN_SE3")
    e7, g7 = np.asarray(est7, dtype=np.float64).astype(dtype).reshape(-1, 7), np.asarray(gt7, dtype=np.float64).astype(dtype).reshape(-1, 7)
    if e7.shape != g7.shape:
        raise ValueError("est7 and gt7 must have the same shape [n][7]")
    n = e7.shape[0]
    row = np.zeros(ALIGN_ROW, dtype=dtype)
    row[1:10] = np.eye(3).ravel()
    if n == 0:
        return row
    p, g = e7[:, 4:7], g7[:, 4:7]
    zero = np.zeros(3, dtype=dtype)
    pbar, gbar = (zero, zero) if mode == ALIGN_NONE else (p.sum(0) / dtype(n), g.sum(0) / dtype(n))
    pc, gc = p - pbar, g - gbar
    if centred:
        S = (pc[:, :, None] * gc[:, None, :]).sum(0)
        sq_p, sq_g = (pc * pc).sum(0), (gc * gc).sum(0)
    else:
        S = (p[:, :, None] * g[:, None, :]).sum(0) - dtype(n) * np.outer(pbar, gbar)
        sq_p, sq_g = (p * p).sum(0) - dtype(n) * pbar * pbar, (g * g).sum(0) - dtype(n) * gbar * gbar
    R, qr, t, cond = closing(mode, n, pbar, gbar, S, sq_p.sum(), sq_g.sum(), sq_p[0] + sq_p[1], sq_g[0] + sq_g[1], dtype)
    e = pc @ R.T - gc
    d2 = np.sum(e * e, axis=1)
    th = error_angle(quat_mul(e7[:, 0:4], quat_inv(qr)[None, :]), g7[:, 0:4])
    t2 = np.sum(th * th, axis=1)
    row[0], row[1:10], row[10:13], row[13] = n, R.ravel(), t, cond
    row[14], row[15], row[16], row[17], row[18] = d2.sum(), np.sqrt(d2.max()), np.sqrt(d2[-1]), t2.sum(), np.sqrt(t2.max())
    row[19] = np.sum((p - g) ** 2, axis=1).sum()
    return row


def rpe(est7, gt7, lags, dtype=np.float64):
    """One trajectory: the rows [len(lags)][4] of msckf_hip_traj_rpe (capi.RPE_FIELDS) -- per lag the pairs (r, r + lag), sum |e_t|^2,
    sum |e_th|^2, max |e_t|; e_t = C(q_r) (p_{r+lag} - p_r) - C(g_r) (g_{r+lag} - g_r), e_th the error angle of q_{r+lag} * q_r^-1
    against the truth's.  A lag longer than the trajectory gives zeros."""
    e7, g7 = np.asarray(est7, dtype=np.float64).astype(dtype).reshape(-1, 7), np.asarray(gt7, dtype=np.float64).astype(dtype).reshape(-1, 7)
    if e7.shape != g7.shape:
        raise ValueError("est7 and gt7 must have the same shape [n][7]")
    out = np.zeros((len(lags), RPE_ROW), dtype=dtype)
    for k, lag in enumerate(lags):
        if lag < 1:
            raise ValueError("a lag is at least 1 record")
        m = e7.shape[0] - int(lag)
        if m <= 0:
            continue
        e0, e1, g0, g1 = e7[:m], e7[lag:], g7[:m], g7[lag:]
        de = np.einsum("nij,nj->ni", quat_rot(e0[:, 0:4]), e1[:, 4:7] - e0[:, 4:7])
        dg = np.einsum("nij,nj->ni", quat_rot(g0[:, 0:4]), g1[:, 4:7] - g0[:, 4:7])
        d2 = np.sum((de - dg) ** 2, axis=1)
        th = error_angle(quat_mul(e1[:, 0:4], quat_inv(e0[:, 0:4])), quat_mul(g1[:, 0:4], quat_inv(g0[:, 0:4])))
        out[k] = m, d2.sum(), np.sum(th * th), np.sqrt(d2.max())
    return out


# ------------------------------------------------------------------ poses
def pose7_from_truth16(truth16):
    """[..., 16] rows q_IG b_g v b_a p (scenario.imu_state_gt, a frame-log record's first 16 scalars) -> [..., 7] poses q_IG p"""
    t = np.asarray(truth16, dtype=np.float64)
    return np.concatenate([t[..., 0:4], t[..., 13:16]], axis=-1)


def gt_pose7(trajs, f0, f1):
    """Ground-truth IMU poses of the frames [f0, f1) of a batch, as Batch.frame_log_align / frame_log_rpe take them: [f1 - f0][B][7]"""
    return pose7_from_truth16(sc.imu_state_gt(trajs, f0, f1))


def transformed(pose7, R0, t0):
    """The poses [..., 7] seen from another global frame, x' = R0 x + t0: p' = R0 p + t0 and C(q') = C(q) R0^T"""
    x = np.asarray(pose7, dtype=np.float64)
    R0 = np.asarray(R0, dtype=np.float64)
    q0 = sc.rot_to_quat(R0)
    out = np.empty_like(x)
    out[..., 0:4] = quat_mul(x[..., 0:4], np.broadcast_to(quat_inv(q0), x[..., 0:4].shape))
    out[..., 4:7] = x[..., 4:7] @ R0.T + np.asarray(t0, dtype=np.float64)
    return out
