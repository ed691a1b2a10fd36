"""The fp16-Jacobian dtype (MSCKF_HIP_F16H_F32P) held to a reference: a numpy twin that takes the 2 x 6 Jacobian blocks of every
observation from a table -- the blocks the device stored, read back through last_track_blocks -- and does everything else in its
own double arithmetic; the rounding law the stored blocks must obey; the identity that ties the stored B^ to the stored blocks;
and the mutants that show on the CPU that each check sees the fault it is meant for (tests/test_h16_inputs.py).  Used on the
device by tests/test_gpu_h16_kernels.py and tests/test_gpu_gate_early.py.  TEST INFRASTRUCTURE ONLY.

Why a given-H twin: the dtype rounds H_x to binary16 where it is formed.  That rounding alone moves a 24-track update by
3 to 15 float bars (covariance) and 8 to 82 (correction) on update_lab's entry-scaled metric, so against the UNROUNDED oracle
only an envelope as wide as the rounding can hold (tests/test_gpu_configs.py::test_fp16_jacobian_dtype).  Handed the device's own blocks, the twin
reproduces what every consumer of those blocks must compute, and the ordinary float bars apply again; the blocks themselves
are held separately, entry by entry, by the rounding law."""
import numpy as np
import scipy.linalg as sla

import feature_lab as FL
import helpers as H
import np_oracle

F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14
F16_SUB_ULP = 2.0 ** -24

# ---- constants measured on the CPU; tests/test_h16_inputs.py reproduces every one of them (never taken from the device)
FLOAT_FACTOR = 4.0                   # update_lab.FLOAT_FACTOR: the allowance for another valid operation order
# The float kernel's own error in an entry before it rounds: worst |H_float32 - H_float64| / rowmax|H| over the lab's tracks with
# a Jacobian, both evaluations of the twin's block formula at the SAME point (the float oracle's), the float one on the window
# rounded to float.  The law is stated at the point the device itself reports (last_tracks: the very registers the kernel formed
# its blocks from), because the triangulation's float error is not the rounding's business and would drown it: with the double
# evaluation at the double oracle's point instead, the same figure is 1.10e-4 (a third of binary16's half-ulp) and 662 of the
# lab's 282 600 entries round to another binary16 value, 2.3e-3 -- over MISMATCH_CAP before any kernel has run.
H_SLACK_MEASURED = 8.30e-7           # measured 8.293e-07
H_SLACK = 3.4e-6                     # FLOAT_FACTOR x the figure above, rounded up
H_MISMATCH_MEASURED = (278, 282600)  # float16(H_float32) != float16(H_float64) at the same point: 9.8e-4 of the entries
MISMATCH_CAP = 2e-3                  # share of entries whose stored value is not float16(x): a condition of the issue
# worst relative distance of the float oracle's gamma from the double oracle's over the lab's tracks with a Jacobian
GAMMA_D32_MEASURED = 4.22e-3         # measured 4.213e-03 (`spread`; the other patterns 1.2e-4 .. 3.1e-4, the median track 3e-6)
GAMMA_BAR = 1.7e-2                   # FLOAT_FACTOR x the figure above, rounded up
# The rounding moves the median track's gamma by 1.5e-5 .. 2.0e-5 (worst 1.2e-2): GAMMA_BAR is NOT below it, so gamma cannot tell a
# rounded Jacobian from an unrounded one.  The bar is kept as the issue defines it; the rounding law, the B^ identity and the
# decisions carry the dtype (tests/test_h16_inputs.py asserts this reading of the figures, so that it cannot go stale).
GAMMA_SEPARATES = False
SKIP_CAP = 0.02                      # tracks whose given-H gamma is within FL.GATE_MARGIN of the threshold: at most this share
B_IDENTITY_CAP = 1e-7                # the B^ identity is never held looser than this, whatever the device's float figure
ANISO_VAR = (1.0, 4.0)               # u_var', v_var' of the anisotropic case, in units of the window's u_var'
H_MAX_MEASURED = 10.13               # largest |H| of the lab, unweighted (measured 10.124)
# largest |H| x weight: the anisotropic case pre-whitens by 1 / sigma_u = 65.5 (u_var' = 2.33e-4): 10.124 x 65.5 = 663.4, against
# F16_MAX / 16 = 4094.  The kernels have no guard against an fp16 overflow (beside the dtype).
HW_MAX_MEASURED = 664.0
# update_lab's windows the fp16 cases of the whole update use: those where rounding the twin's own blocks moves the update by at
# least H16_MIN_BARS float bars on covariance or correction.  The issue asks for 3 on the CPU and for 3 again on the device; the
# device may sit one bar from the given-H twin, hence 4 here.  Every `tall` list from 4 cameras on has it (4.8 .. 14.5 bars on
# the covariance alone); of the `thin` lists (4 rows) only these (measured, covariance / correction bars: 5: 4.4 / 1.0, 8: 3.6 / 4.8,
# 14: 4.4 / 1.6, 22: 1.3 / 5.6, 32: 6.7 / 1.7, 33: 5.3 / 2.7).
H16_MIN_BARS = 4.0
H16_TALL_MIN, H16_THIN_SIZES = 4, (5, 8, 14, 22, 32, 33)


def h16_window(n, fam):
    return n >= H16_TALL_MIN if fam == "tall" else n in H16_THIN_SIZES


# ------------------------------------------------------------------------------------------------------------ binary16
def ulp16(x):
    """spacing of binary16 at |x|: 2^(e - 10) in the binade 2^e <= |x| < 2^(e + 1), the subnormal spacing 2^-24 below 2^-14"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, F16_MIN_NORMAL)))
    return np.exp2(np.maximum(e, -14.0) - 10.0)


def round16(x):
    """round-to-nearest-even to binary16, widened (what __float2half_rn of the float value gives; a double whose float rounding
    sits exactly on a binary16 tie is the one case where the two differ: the law's slack covers it)"""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def floor16(x):
    f = np.asarray(x, dtype=np.float64).astype(np.float16)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float16(-np.inf)), f).astype(np.float64)


def ceil16(x):
    f = np.asarray(x, dtype=np.float64).astype(np.float16)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float16(np.inf)), f).astype(np.float64)


def rounding_violations(stored, ref, slack=None):
    """The rounding law, per entry x of the unrounded blocks `ref` [.., 2, 6] against the stored value h of `stored`:
      (a) h is a binary16 value;
      (b) |h - x| <= ulp16(x) / 2 + s, with s = slack x the largest |entry| of x's row (the float kernel's own error before it rounds);
      (c) h lies between the binary16 neighbours of the interval [x - s, x + s] (for s = 0: one of the two neighbours of x, or x).
    Returns (list of violations (kind, index, h, x), number of entries with h != float16(x), number of entries)."""
    slack = H_SLACK if slack is None else slack
    h, x = np.asarray(stored, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert h.shape == x.shape and x.shape[-1] == 6
    s = slack * np.abs(x).max(axis=-1, keepdims=True) * np.ones_like(x)
    bad = []
    with np.errstate(over="ignore"):
        rep = np.isfinite(h) & (np.abs(h) <= F16_MAX) & (round16(np.where(np.isfinite(h), np.clip(h, -F16_MAX, F16_MAX), 0.0)) == h)
    for kind, mask in (("not_binary16", ~rep), ("half_ulp", ~(np.abs(h - x) <= 0.5 * ulp16(x) + s)),
                       ("neighbour", ~((h >= floor16(x - s)) & (h <= ceil16(x + s))))):
        for idx in zip(*np.nonzero(mask)):
            bad.append((kind, tuple(int(i) for i in idx), float(h[idx]), float(x[idx])))
    return bad, int((h != round16(x)).sum()), int(x.size)


# ------------------------------------------------------------------------------------------------------------ the twin
def blocks_of(cams, g, p_f, slots, dtype=np.float64):
    """the 2 x 6 measurement Jacobian block (observability-constrained, unwhitened) and the predicted measurement per observation,
    every operation in `dtype`: np_oracle.NpMSCKF.jac's arithmetic.  cams [n][7] (q_CG w x y z, p_C_G).  Returns [L][2][6], [L][2]."""
    T = dtype
    cams, g, p_f = np.asarray(cams).astype(T), np.asarray(g).astype(T), np.asarray(p_f).astype(T)
    Hb, z = np.zeros((len(slots), 2, 6), T), np.zeros((len(slots), 2), T)
    for c, s in enumerate(slots):
        w, x, y, zq = cams[s, :4]
        one, two = T(1), T(2)
        C = np.array([[one - two * (y * y + zq * zq), two * (x * y - zq * w), two * (x * zq + y * w)],
                      [two * (x * y + zq * w), one - two * (x * x + zq * zq), two * (y * zq - x * w)],
                      [two * (x * zq - y * w), two * (y * zq + x * w), one - two * (x * x + y * y)]], dtype=T)
        d = p_f - cams[s, 4:7]
        pc = C @ d
        X, Y, Z = pc
        Ji = np.array([[one, 0, -X / Z], [0, one, -Y / Z]], dtype=T) / Z
        A = np.hstack([Ji @ _skew(pc, T), -(Ji @ C)])
        u = np.concatenate([C @ g, _skew(d, T) @ g])
        Hb[c] = A - np.outer(A @ u, u) / (u @ u)
        z[c] = pc[:2] / Z
    assert Hb.dtype == T
    return Hb, z


def _skew(v, T):
    o = T(0)
    return np.array([[o, -v[2], v[1]], [v[2], o, -v[0]], [-v[1], v[0], o]], dtype=T)


class GivenHTwin(np_oracle.NpMSCKF):
    """np_oracle.NpMSCKF loaded from an oracle's state (IMU state, camera states, covariance, numResidualized, config).  run()
    is marginalize() with the Jacobian blocks of every observation taken from a table when one is given -- H_f = -H[:, 3:6] of
    those same blocks -- and the twin's own double arithmetic everywhere else: motion check, triangulation, residual, null space
    of H_f, gate, stacking, measurement_update.  The gate table is the project's (oracle/chi2_table.h)."""

    def __init__(self, o, cfg):
        imu = o.getImuState()
        super().__init__(cfg, imu, nullspace="householder")
        self.q_null, self.v_null, self.p_null = imu[19:23].copy(), imu[23:26].copy(), imu[26:29].copy()
        cams, ids = o.getCamStates()
        self.cams = [dict(q=c[:4].copy(), p=c[4:7].copy(), id=int(i), feats=[]) for c, i in zip(cams, ids)]
        self.P = o.getCovariance()
        self.n_resid = int(o.numResidualized())
        assert self.P.shape[0] == 15 + 6 * len(self.cams)

    def triangulate(self, cams, obs):
        """np_oracle.NpMSCKF.triangulate (msckf.h:1147-1285) with the loops over the track's cameras as array operations: the same
        sequence of steps (tests/test_h16_inputs.py holds the result to the double oracle's point)"""
        C0, p0 = np_oracle.q2R(cams[0]["q"]), cams[0]["p"]
        Cs = np.array([np_oracle.q2R(c["q"]) for c in cams])
        Rs = Cs @ C0.T
        ts = np.einsum("nij,nj->ni", Cs, p0[None, :] - np.array([c["p"] for c in cams]))
        z = np.array(obs, dtype=float).reshape(-1, 2)
        n = len(cams)

        def h(x):
            return Rs @ np.array([x[0], x[1], 1.0]) + x[2] * ts

        def cost(x):
            hh = h(x)
            return float(np.sum((hh[:, :2] / hh[:, 2:3] - z) ** 2))
        m = Rs[-1] @ np.array([z[0, 0], z[0, 1], 1.0])
        A = np.array([m[0] - z[-1, 0] * m[2], m[1] - z[-1, 1] * m[2]])
        b = np.array([z[-1, 0] * ts[-1][2] - ts[-1][0], z[-1, 1] * ts[-1][2] - ts[-1][1]])
        x = np.array([z[0, 0], z[0, 1], (A @ A) / (A @ b)])
        lam, total, outer = 1e-3, cost(x), 0
        W = np.stack([Rs[:, :, 0], Rs[:, :, 1], ts], axis=2)                 # [n][3][3]: columns R e_x, R e_y, t
        while True:
            hh = h(x)
            J = np.stack([W[:, 0] / hh[:, 2:3] - (hh[:, 0] / hh[:, 2] ** 2)[:, None] * W[:, 2],
                          W[:, 1] / hh[:, 2:3] - (hh[:, 1] / hh[:, 2] ** 2)[:, None] * W[:, 2]], axis=1)      # [n][2][3]
            r = hh[:, :2] / hh[:, 2:3] - z
            e = np.linalg.norm(r, axis=1)
            w2 = np.where(e <= 0.01, 1.0, 0.01 / (2 * np.maximum(e, 1e-300))) ** 2
            AA = np.einsum("n,nki,nkj->ij", w2, J, J)
            bb = np.einsum("n,nki,nk->i", w2, J, r)
            inner = 0
            while True:
                delta = np.linalg.solve(AA + lam * np.eye(3), bb)
                xn = x - delta
                dn = np.linalg.norm(delta)
                nc = cost(xn)
                if nc < total:
                    reduced, x, total = True, xn, nc
                    lam = max(lam / 10, 1e-10)
                else:
                    reduced = False
                    lam = min(lam * 10, 1e12)
                go = inner < 10 and not reduced
                inner += 1
                if not go:
                    break
            go = outer < 10 and dn > 5e-7
            outer += 1
            if not go:
                break
        fin = np.array([x[0] / x[2], x[1] / x[2], 1 / x[2]])
        valid = bool(np.all((Rs @ fin + ts)[:, 2] > 0)) and not total / (2 * n ** 2) > self.cfg["max_gn_cost_norm"]
        return C0.T @ fin + p0, valid

    def run(self, M, slots, obs, table=None, update=True, reuse=None):
        """table: None (the twin's own unrounded blocks) or [F][>= L][2][6], row t the blocks of track t's observations in the
        list's order.  Returns one dict per track: motion_ok, tri_valid, gate_pass, gamma, ub = |r_o|^2 / sigma^2, thresh, p_f_G,
        own ([L][2][6]: the twin's unrounded blocks; None without a Jacobian), used (the blocks the statistics were formed from).
        With update the passing tracks are stacked and applied: self.P, self.last["dx"].  reuse: the result of an earlier run of
        the same list on the same state, whose motion checks, points and own blocks are taken over (none depends on the table)."""
        assert self.cfg["u_var_prime"] == self.cfg["v_var_prime"], "the given-H twin is isotropic: anisotropic noise is pre-whitened by the caller"
        sig2 = float(self.cfg["u_var_prime"])
        D, off = self.P.shape[0], np.concatenate([[0], np.cumsum(M)]).astype(int)
        cam_arr = self.cam_array()
        out, Hs, rs = [], [], []
        for t in range(len(M)):
            sl = [int(s) for s in slots[off[t]:off[t + 1]]]
            z = [np.asarray(obs[off[t] + i], dtype=float) for i in range(len(sl))]
            info = dict(L=len(sl), motion_ok=1, tri_valid=0, gate_pass=0, gamma=0.0, ub=0.0, thresh=float(FL.chi2_threshold(len(sl))), p_f_G=np.zeros(3), own=None, used=None)
            out.append(info)
            cams = [self.cams[s] for s in sl]
            if reuse is not None:
                if not reuse[t]["motion_ok"]:
                    info["motion_ok"] = 0
                    continue
                p_f, valid = reuse[t]["p_f_G"], reuse[t]["tri_valid"]
            else:
                if self.n_resid > 3 and not self.check_motion(z[0], cams):
                    info["motion_ok"] = 0
                    continue
                p_f, valid = self.triangulate(cams, z)
            info["p_f_G"], info["tri_valid"] = p_f, int(valid)
            if not valid:
                continue
            self.n_resid += 1
            own, zhat = blocks_of(cam_arr, self.g, p_f, sl) if reuse is None else (reuse[t]["own"], reuse[t]["zhat"])
            info["zhat"] = zhat
            used = own if table is None else np.asarray(table[t], dtype=np.float64)[:len(sl)]
            info["own"], info["used"] = own, used
            r = (np.array(z) - zhat).ravel()
            Hf = -used[:, :, 3:6].reshape(2 * len(sl), 3)
            Hx = np.zeros((2 * len(sl), D))
            for c, s in enumerate(sl):
                Hx[2 * c:2 * c + 2, 15 + 6 * s:21 + 6 * s] = used[c]
            A = sla.qr(Hf, mode="full")[0][:, 3:]
            Ho, ro = A.T @ Hx, A.T @ r
            info["ub"] = float(ro @ ro) / sig2
            info["gamma"] = float(ro @ np.linalg.solve(Ho @ self.P @ Ho.T + sig2 * np.eye(len(ro)), ro))
            if info["gamma"] < info["thresh"]:
                info["gate_pass"] = 1
                Hs.append(Ho); rs.append(ro)
        self.last = dict(n_tracks=len(M), m_rows=int(sum(len(r) for r in rs)))
        if update and Hs:
            self.measurement_update(np.vstack(Hs), np.concatenate(rs), sig2)
        return out

    def measurement_update(self, Hm, r, sig2):
        """np_oracle's measurement_update (msckf.h:1325-1423) for R = sigma^2 I, with the economic QR: the same T_H, r_n"""
        Q, Rq = sla.qr(Hm, mode="economic")
        nz = np.any(np.triu(Rq) != 0, axis=1)
        T_H, r_n = np.triu(Rq)[nz], (Q.T @ r)[nz]
        P, D = self.P, self.P.shape[0]
        K = P @ T_H.T @ np.linalg.inv(T_H @ P @ T_H.T + sig2 * np.eye(len(r_n)))
        self.last["dx"] = K @ r_n
        A = np.eye(D) - K @ T_H
        Pc = A @ P @ A.T + sig2 * (K @ K.T)
        self.P = (Pc + Pc.T) / 2


def rows_of(infos):
    """the twin's per-track results as rows of last_tracks / lastTracks: motion_ok tri_valid gate_pass 2M-3 gamma p_f_G"""
    return np.array([[i["motion_ok"], i["tri_valid"], i["gate_pass"], (2 * i["L"] - 3) * i["gate_pass"], i["gamma"]] + list(i["p_f_G"]) for i in infos]).reshape(-1, 8)


def gate_skips(infos):
    """tracks with a Jacobian whose gamma is within FL.GATE_MARGIN of the threshold: the only ones a decision may differ on"""
    return np.array([bool(i["own"] is not None and abs(i["gamma"] - i["thresh"]) < FL.GATE_MARGIN * i["thresh"]) for i in infos])


# ------------------------------------------------------------------------------------------------------------ B^
def bhat_gram(W, F):
    """W^T F (F^T F)^-1 F^T W in numpy double: the Gram matrix every valid B^ of a track has (W = [H_x | r], F = H_f)"""
    G = F.T @ W
    return G.T @ np.linalg.solve(F.T @ F, G)


def stack_w(Hx, rw, slots, ncols):
    """W = [H_x | r_w] of one track: its L stored blocks scattered to the track's camera columns (6 per slot), the whitened
    residual in column `ncols - 1`; and F = -Hx[:, :, 3:6].  Hx [L][2][6], rw [L][2]."""
    L = len(slots)
    W = np.zeros((2 * L, ncols))
    for c, s in enumerate(slots):
        W[2 * c:2 * c + 2, 6 * int(s):6 * int(s) + 6] = Hx[c]
    W[:, ncols - 1] = np.asarray(rw).ravel()
    return W, -np.asarray(Hx)[:, :, 3:6].reshape(2 * L, 3)


def track_columns(slots, n_cam):
    """the columns of B^ a track owns: six per observed slot, and the c column 6 n_cam"""
    return np.concatenate([np.arange(6 * int(s), 6 * int(s) + 6) for s in slots] + [[6 * n_cam]]).astype(int)


def b_identity_error(B, Hx, rw, slots, n_cam):
    """distance of the stored B^ ([3][>= 6 n_cam + 1], c in column 6 n_cam) from the projection of the stored blocks:
    max |B^T B - W^T F (F^T F)^-1 F^T W| over the track's columns and the c column, relative to the largest entry of the
    right-hand side"""
    cols = track_columns(slots, n_cam)
    W, F = stack_w(np.asarray(Hx, dtype=np.float64), rw, slots, 6 * n_cam + 1)
    want = bhat_gram(W[:, cols], F)
    Bc = np.asarray(B, dtype=np.float64)[:, cols]
    return float(np.abs(Bc.T @ Bc - want).max() / np.abs(want).max())


def bhat_of(W, F):
    """a valid B^ (3 rows) of the track: L^-1 F^T W with F^T F = L L^T"""
    return sla.solve_triangular(np.linalg.cholesky(F.T @ F), F.T @ W, lower=True)


# ------------------------------------------------------------------------------------------------------------ mutants
MUTANTS = ("trunc", "ftz16", "hf_unrounded", "stale_consumer")
BLOCK_MUTANTS, B_MUTANTS = MUTANTS[:2], MUTANTS[2:]


def mutate_blocks(own, which):
    """what a kernel with ONE deliberate mistake in its rounding would store for the unrounded blocks `own` -- pure, applied to
    the reference's numbers only, never to code under test"""
    x32 = np.asarray(own, dtype=np.float64).astype(np.float32)
    if which == "trunc":            # the float's low 13 mantissa bits masked: round-toward-zero where round-to-nearest is meant
        return (x32.view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32).astype(np.float64)
    if which == "ftz16":            # binary16 subnormals flushed to zero
        h = round16(x32)
        return np.where(np.abs(h) < F16_MIN_NORMAL, 0.0, h)
    raise ValueError(which)


def mutate_b(own, rw, slots, n_cam, which):
    """(stored H_x, stored B^) a kernel with ONE deliberate mistake among its consumers would leave for the unrounded blocks
    `own`: H_x is rounded as it should be, B^ is not the projection of it"""
    own = np.asarray(own, dtype=np.float64)
    h = round16(own)
    Wr, Fr = stack_w(h, rw, slots, 6 * n_cam + 1)
    Wu, Fu = stack_w(own, rw, slots, 6 * n_cam + 1)
    if which == "hf_unrounded":     # H_f taken from the unrounded registers while H_x is rounded
        return h, bhat_of(Wr, Fu)
    if which == "stale_consumer":   # one consumer reads blocks the others do not see: B^ from the unrounded blocks
        return h, bhat_of(Wu, Fu)
    raise ValueError(which)


# ------------------------------------------------------------------------------------------------------------ the lab's figures
_CACHE = {}


def lab_blocks(po):
    """per pattern of feature_lab's lists: the twin's results with its own unrounded blocks (no update), the float oracle's rows,
    and per track with a Jacobian the float32 and the double evaluation of the blocks at the FLOAT oracle's point (the float one
    from the window rounded to float, as a float handle holds it).  Cached."""
    if "blocks" not in _CACHE:
        win = FL.window(po)
        out = {}
        for p in FL.PATTERNS:
            tracks = FL.lab(po)[p]
            infos = GivenHTwin(win.o, win.tr.cfg).run(*FL.worklist(tracks), update=False)
            r32, _ = FL.run_oracle(win, po.F32, tracks)
            cams32, imu = win.o.getCamStates()[0], win.o.getImuState()
            f32 = []
            for t, (tk, i) in enumerate(zip(tracks, infos)):
                if i["own"] is None:
                    f32.append(None)
                    continue
                pf = r32[t, 5:8].astype(np.float32)
                f32.append((blocks_of(cams32, imu[16:19], pf, tk.slots, np.float32)[0].astype(np.float64), blocks_of(cams32, imu[16:19], pf.astype(np.float64), tk.slots)[0]))
            out[p] = (infos, f32, r32)
        _CACHE["blocks"] = out
    return _CACHE["blocks"]


def measure_h(po, same_point=True):
    """(worst |H_f32 - H_f64| / rowmax|H_f64|, entries with float16(H_f32) != float16(H_f64), entries, entries of H_f64 with
    2^-25 + H_SLACK rowmax < |x| < 2^-14 (the ones `ftz16` is caught on), largest |H_f64|) over the lab.  same_point: both
    evaluations at the float oracle's point (the float arithmetic alone: what the rounding law allows for); otherwise the double
    one is the twin's own, at the double oracle's point (the triangulation's float error included)."""
    worst, mism, total, sub, big = 0.0, 0, 0, 0, 0.0
    for p in FL.PATTERNS:
        infos, f32, _ = lab_blocks(po)[p]
        for i, pair in zip(infos, f32):
            if pair is None:
                continue
            h32, x = pair[0], (pair[1] if same_point else i["own"])
            rowmax = np.abs(x).max(axis=-1, keepdims=True)
            worst = max(worst, float((np.abs(h32 - x) / rowmax).max()))
            mism += int((round16(h32) != round16(x)).sum())
            total += x.size
            sub += int(((np.abs(x) < F16_MIN_NORMAL) & (np.abs(x) > 0.5 * F16_SUB_ULP + (H_SLACK or 0.0) * rowmax)).sum())
            big = max(big, float(np.abs(x).max()))
    return worst, mism, total, sub, big


def update_twin(po, n, fam):
    """(twin, results) of update_lab's list `fam` on its n-camera window with the twin's own unrounded blocks, update applied
    (cached: the motion checks, points and own blocks serve every given-H run of the same list)"""
    import update_lab as UL
    key = ("upd", n, fam)
    if key not in _CACHE:
        tw = GivenHTwin(UL.window(po, n), FL.window(po).tr.cfg)
        _CACHE[key] = (tw, tw.run(*UL.tracks_of(po, n, fam)))
    return _CACHE[key]


def update_given(po, n, fam, table):
    """the twin's update of the same list with the blocks of `table`"""
    import update_lab as UL
    tw = GivenHTwin(UL.window(po, n), FL.window(po).tr.cfg)
    return tw, tw.run(*UL.tracks_of(po, n, fam), table=table, reuse=update_twin(po, n, fam)[1])


def line_reference(po):
    """the double twin's results for feature_lab.line_cases (all of them; cached): ub, gamma, threshold per track"""
    if "line" not in _CACHE:
        win = FL.window(po)
        _CACHE["line"] = GivenHTwin(win.o, win.tr.cfg).run(*FL.worklist(FL.line_cases(po)), update=False)
    return _CACHE["line"]
