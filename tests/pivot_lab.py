"""Covariances that make the JOINT innovation matrix S = T_H P T_H^T + sigma^2 I of an update firmly indefinite while every
per-track gate matrix stays positive definite, with the first non-positive pivot of the unpivoted Cholesky at a chosen row: the
inputs of tests/test_pivot_inputs.py (CPU: proves every property below on the double oracle and the given-H twin) and of
tests/test_gpu_pivot_report.py (every factorization of S on the device reports STAT_ERR_PIVOT, isolates the failure and leaves the
handle reusable).  TEST INFRASTRUCTURE ONLY.

The recipe, on update_lab's windows and `tall` lists:
  1. H_o: the stacked, null-space projected Jacobian of the passing tracks, as h16_lab.GivenHTwin hands it to its
     measurement_update (KeepTwin below keeps it).  Its 15 IMU columns are zero.  T (r rows) is the upper STAIRCASE factor of its
     camera columns: what a Cholesky of the Gram matrix that skips its semidefinite pivots leaves, formed from H_o itself
     (staircase()).  The device's Gram-Cholesky factor equals T up to row signs, which change no leading minor, and keeps a zero
     row per skipped pivot: row i of T is the device's row lead[i].  Asserted on the CPU: T^T T = H_o^T H_o to GRAM_TOL.  (The
     rows of triu(qr(H_o)) with a diagonal above 1e-7 of the largest are NOT that factor where a dependent column is followed
     by independent ones: at 43 and 63 cameras columns 8 .. 11 / 6 .. 11 are dependent and that T^T T misses the Gram matrix by
     9e-3 of its largest entry; on the `thin` lists by 0.2.)  S = T P T^T + sigma^2 I.
  2. w: normal entries from a seeded generator on the support [a, b), zero elsewhere; u = lstsq(T, w) (T has full row rank: the
     residual is below LSTSQ_TOL, asserted); g = w^T S^-1 w, c = 2 / g, P' = P - c u u^T.
  3. S' = S - c w w^T: w^T S'^-1 w = g / (1 - c g) = -g < 0, so S' is indefinite; its leading a x a minor is S's.  That the FIRST
     non-positive pivot sits at row a exactly, and not later in the support, is a property of the drawn w: about one draw in
     thirty of an 8-row support has it, hence the sub-seeds below.

Three supports per window: `first` (row 0 alone: nothing to re-seed, the case is invariant under the scale of w), `mid` (8 rows
from a row that is no multiple of 16, at least 16 and at most r - 24, and at most CH_SPLIT - 32 on the two-level windows: level
A), `tail` (the last 8 rows; level B where r > 192).  At 5 cameras r = 23 has no row that `mid` asks for: there `mid` is the
rows [r // 2, r // 2 + 8).  The trailing 16-block of the device's S holds the window's seven unobservable directions (the last
seven columns are skipped pivots at every size), so `tail` ends in the last block that has a pivot at all; where its first row a
falls is recorded per case by tests/test_pivot_inputs.py.  At 33 cameras r = 191: every row is level A; 43 and 63 cameras
(r = 243, 359) carry level B.

The `thin` lists (two tracks, 4 rows: S of rank 4 behind 6 n - 4 skipped pivots) do not carry the damage with c = 2 / g:
c (g_1 + g_2) >= 2 / lambda_max = 1.60 .. 1.70 for every w at 5, 10 and 12 cameras (lambda_max the largest lambda of
S^-1 v = lambda D^-1 v, D the block diagonal of the two tracks' own gate matrices: thin_floor() below), so one gate matrix loses
more than 0.80 where 0.75 is allowed.  S' is indefinite for every c > 1 / g, though: the `thin` cases take c = 1.2 / g
(C_FACTOR) on the support [0, 4) and hold every condition of the other cases, with the first bad pivot in row 0 (`first`).  A
first bad pivot in row 1, 2 or 3 within the margin was not found (3000 draws each at c g = 1.2, 1.1, 1.05: the unprojected
quantity stays at 0.96 or more), so a `thin` handle has one damaged trajectory.

One more family, LITERAL: the 22-camera window's `tall` list under anisotropic noise v' = 4 u', where the literal route compresses
(T_H, r_n, R_n = Q_1^T R_o Q_1) into Lam^ = T_H^T R_n^-1 T_H and the chain's kernels factor S = T^ P T^^T + I; stack_literal()
builds that T^ and the tracks' own R_o,j = A_j^T R_j A_j, and the reference is literal_lab's anisotropic double oracle.

The unprojected margin: the gate of kernels_feature.hip factors the track's unprojected 2 M x 2 M matrix
N_j = H_x,j P H_x,j^T + sigma^2 I, not S_j = A_j^T N_j A_j (gamma = min_x |r - H_f x|^2_{N^-1}, an identity for a positive
definite N_j only).  Where c (H_j u)^T S_j^-1 (H_j u) <= 0.75 but the same quantity of N_j exceeds 1, N_j' is indefinite while S_j'
is not, and the device gate-rejects a track that the reference passes.  Every case therefore holds TRACK_MARGIN for both
matrices; GATE_DRAW is a draw that holds it for S_j only (two indefinite N_j': asserted on the CPU, and on the device that
exactly those two tracks are gate-rejected)."""
import numpy as np
import scipy.linalg as sla

import feature_lab as FL
import h16_lab as HL
import update_lab as UL
from msckf_mono_amd import scenario as sc

ROW_TOL = 1e-7            # a column opens a row of T when its remainder exceeds ROW_TOL of its own norm
GRAM_TOL = 1e-9           # |T^T T - H_o^T H_o| / |H_o^T H_o| (max norm)
LSTSQ_TOL = 1e-12         # |T u - w| / |w|
EPS_F32 = 2.0 ** -23
PIVOT_MARGIN = 2.0 ** 10 * EPS_F32       # the bad pivot is at most -PIVOT_MARGIN max diag(S'): float rounding cannot flip it
TRACK_MARGIN = 0.75       # c (H_j u)^T S_j^-1 (H_j u) of every passing track: its gate matrix keeps a quarter of its margin -- and
                          # the same of the unprojected N_j the device's gate factors (track_quantity_unprojected)
CH_SPLIT = 192
SUPPORTS = ("first", "mid", "tail")
STAT_ERR_PIVOT = 2

# (window, list) of every case of tests/test_gpu_pivot_report.py
TALL_SIZES = (5, 10, 12, 21, 22, 23, 24, 32, 33, 43, 63)
THIN_SIZES = (5, 10, 12)
WINDOWS = tuple((n, "tall") for n in TALL_SIZES)
C_FACTOR = {"thin": 1.2}   # c = C_FACTOR / g (default 2): the `thin` lists, see above
LITERAL, LITERAL_K, LITERAL_SIZE = "literal", 4, 22      # the literal anisotropic route: v' = 4 u' on the 22-camera window's `tall` list
LEVEL_B_SIZES = (43, 63)  # r > CH_SPLIT: `tail` lies in the second level (at 33 cameras r = 191)

# sub-seed of w per (window size, list, support) (default 0): found by trying 0, 1, 2, ... on the CPU until violations() is empty;
# tests/test_pivot_inputs.py asserts it for every case with none excluded.
SUB_SEEDS = {(5, "tall", "mid"): 3, (5, "tall", "tail"): 1, (10, "tall", "mid"): 77, (10, "tall", "tail"): 39, (12, "tall", "mid"): 36, (12, "tall", "tail"): 113,
             (21, "tall", "mid"): 4, (21, "tall", "tail"): 43, (22, "tall", "mid"): 31, (22, "tall", "tail"): 104, (23, "tall", "mid"): 9, (23, "tall", "tail"): 55,
             (24, "tall", "mid"): 153, (24, "tall", "tail"): 4, (32, "tall", "mid"): 107, (32, "tall", "tail"): 44, (33, "tall", "mid"): 71, (33, "tall", "tail"): 2,
             (22, "literal", "mid"): 131, (22, "literal", "tail"): 94, (43, "tall", "mid"): 14, (5, "thin", "first"): 1629, (10, "thin", "first"): 594, (12, "thin", "first"): 88,
             (63, "tall", "mid"): 73, (63, "tall", "tail"): 25}

# site of tests/test_gpu_pivot_report.py: (line of update_routes_host --handle, text it must hold), cases (variant, dtype, n_cap)
SITES = {
    "k_update_small": (("V", " small "), [("default", p, n) for p in ("f32", "f64") for n in (5, 10, 12)]),
    "blocked gain": (("K", " blocked<"), [("chain", "f32", n) for n in (10, 21, 22, 32)] + [("parts2", "f32", 22), ("unfused", "f32", 21)]),
    "two-level": (("K", " large CH_S_A<12> TR_S21 "), [("default", p, n) for p in ("f32", "f64") for n in (33, 43, 63)]),
    "k_gain": (("K", " k_gain<"), [("joseph", "f32", n) for n in (10, 21, 32)] + [("joseph", "f64", n) for n in (10, 21)]),
    "k_chol_inv": (("K", " k_chol_inv<"), [("joseph", "f64", 23), ("joseph", "f64", 24), ("joseph", "f32", 33), ("form2", "f32", 33), ("default", "f64", 32)]),
    "k_gain_w": (("K", " k_gain_w<"), [("form2", "f32", n) for n in (10, 21, 32)] + [("chain", "f64", n) for n in (10, 21)]),
    "tsqr": (("C", " tsqr"), [("tsqr", "f32", 22)]),
}
# every (window, family, support) a GPU case uses; tests/test_pivot_inputs.py proves each
CASES = ([(n, "tall", w) for n in TALL_SIZES for w in SUPPORTS] + [(n, "thin", "first") for n in THIN_SIZES]
         + [(LITERAL_SIZE, LITERAL, w) for w in SUPPORTS])
# window sizes whose `tail` has its FIRST bad pivot (row a) in the last 16-block of the device's S that holds a pivot; at the
# other sizes row a is in the block before it and the support runs on into the last (asserted on the CPU, per site)
TAIL_IN_LAST_BLOCK = (22, 24, 32, 33, 63)
# the draw that shows what the device's gate does when N_j is indefinite while S_j is not (test_pivot_inputs.py, and one device test)
GATE_DRAW = (10, "tall", "mid", 12)

_CACHE = {}


class KeepTwin(HL.GivenHTwin):
    """the given-H twin, keeping the stacked H_o and r_o it is handed"""

    def measurement_update(self, Hm, r, sig2):
        self.H_o, self.r_o, self.sig2 = Hm.copy(), r.copy(), float(sig2)
        super().measurement_update(Hm, r, sig2)


class Stack:
    """the stacked Jacobian of one update with what the recipe derives from it: H_o [m][D], rows [(lo, hi)] per passing track,
    P (before the update), sig2, T [r][D], S [r][r], lead [r] (the device's row of each row of T), Hx [(2 L x D)] per passing track:
    its unprojected Jacobian; Ro, Rx: per passing track the noise of its projected / unprojected rows (None: sigma^2 I); G: the
    matrix T^T T must equal (None: H_o^T H_o)"""
    __slots__ = ("H_o", "rows", "P", "sig2", "T", "S", "r", "lead", "Hx", "Ro", "Rx", "G")


def stack_of(twin_o, cfg, tracks, P=None):
    """Stack of the list `tracks` on the oracle `twin_o`'s window (P: the covariance S is formed with; default the window's own)"""
    P0 = twin_o.getCovariance() if P is None else np.asarray(P, dtype=np.float64)
    tw = KeepTwin(twin_o, cfg)
    infos = tw.run(*tracks)
    st = Stack()
    st.H_o, st.P, st.sig2 = tw.H_o, P0, tw.sig2
    st.Ro = st.Rx = st.G = None
    st.rows, st.Hx, lo = [], [], 0
    off = np.concatenate([[0], np.cumsum(tracks[0])]).astype(int)
    for t, i in enumerate(infos):
        if i["gate_pass"]:
            st.rows.append((lo, lo + 2 * i["L"] - 3))
            lo += 2 * i["L"] - 3
            Hx = np.zeros((2 * i["L"], P0.shape[0]))
            for c, sl in enumerate(tracks[1][off[t]:off[t + 1]]):
                Hx[2 * c:2 * c + 2, 15 + 6 * int(sl):21 + 6 * int(sl)] = i["used"][c]
            st.Hx.append(Hx)
    assert lo == st.H_o.shape[0] and not np.any(st.H_o[:, :15])
    Tc, st.lead = staircase(st.H_o[:, 15:])
    st.T = np.hstack([np.zeros((Tc.shape[0], 15)), Tc])
    st.r = st.T.shape[0]
    st.S = st.T @ P0 @ st.T.T + st.sig2 * np.eye(st.r)
    return st


def staircase(A, with_q=False):
    """the factor a Cholesky of A^T A that skips its semidefinite pivots leaves, formed from A itself: Gram-Schmidt (twice) down
    the columns, a column whose remainder is below ROW_TOL of its own norm opens no row.  Returns Q^T A [r][n], upper staircase,
    and the column each row opens at."""
    m, n = A.shape
    Q, lead = np.zeros((m, 0)), []
    for j in range(n):
        v = A[:, j].copy()
        for _ in range(2):
            v -= Q @ (Q.T @ v)
        nv = np.linalg.norm(v)
        if Q.shape[1] < m and nv > ROW_TOL * np.linalg.norm(A[:, j]):
            Q = np.hstack([Q, (v / nv)[:, None]])
            lead.append(j)
    T = Q.T @ A
    for i, j in enumerate(lead):
        T[i, :j] = 0.0
    return (T, np.array(lead, dtype=int), Q) if with_q else (T, np.array(lead, dtype=int))


def stack_literal(po, n, K):
    """Stack of the window's `tall` list under anisotropic noise v' = K u', as the literal route compresses it (msckf.h:423-431,
    1343-1366): R_o,j = A_j^T R_j A_j per track, T_H = Q_1^T H_o, R_n = Q_1^T R_o Q_1 for a basis Q_1 of the stack's range (any
    basis gives the same Lam^ = T_H^T R_n^-1 T_H), and T the staircase factor of Lam^: the device's kernels factor
    S = T P T^T + I from there (sigma^2 = 1).  The passing tracks are the anisotropic double oracle's."""
    import literal_lab as LL
    cfg, tracks = FL.window(po).tr.cfg, UL.tracks_of(po, n, "tall")
    infos = KeepTwin(UL.window(po, n), cfg).run(*tracks, update=False)
    ref = LL.reference(po, n, "tall", K)
    u2 = float(cfg["u_var_prime"])
    off = np.concatenate([[0], np.cumsum(tracks[0])]).astype(int)
    st = Stack()
    st.P, st.sig2 = UL.window(po, n).getCovariance(), 1.0
    st.rows, st.Hx, st.Ro, st.Rx, Ho, lo = [], [], [], [], [], 0
    for t, i in enumerate(infos):
        if not ref.rows[t, 2] > 0:
            continue
        L = i["L"]
        Hx = np.zeros((2 * L, st.P.shape[0]))
        for c, sl in enumerate(tracks[1][off[t]:off[t + 1]]):
            Hx[2 * c:2 * c + 2, 15 + 6 * int(sl):21 + 6 * int(sl)] = i["own"][c]
        A = sla.qr(-i["own"][:, :, 3:6].reshape(2 * L, 3), mode="full")[0][:, 3:]
        R = np.diag(np.tile([u2, K * u2], L))
        Ho.append(A.T @ Hx)
        st.Ro.append(A.T @ R @ A)
        st.Rx.append(R)
        st.Hx.append(Hx)
        st.rows.append((lo, lo + 2 * L - 3))
        lo += 2 * L - 3
    st.H_o = np.vstack(Ho)
    T_H, _, Q = staircase(st.H_o[:, 15:], with_q=True)
    R_n = Q.T @ sla.block_diag(*st.Ro) @ Q
    Tc, st.lead = staircase(sla.solve_triangular(np.linalg.cholesky(R_n), T_H, lower=True))
    G = T_H.T @ np.linalg.solve(R_n, T_H)
    st.G = np.zeros((st.P.shape[0], st.P.shape[0]))
    st.G[15:, 15:] = G
    st.T = np.hstack([np.zeros((Tc.shape[0], 15)), Tc])
    st.r = st.T.shape[0]
    st.S = st.T @ st.P @ st.T.T + np.eye(st.r)
    return st


def gram_error(st):
    G = st.H_o.T @ st.H_o if st.G is None else st.G
    return float(np.abs(st.T.T @ st.T - G).max() / np.abs(G).max())


def support_of(r, which, two_level):
    """[a, b) of the support `which` in a stack of r rows"""
    if which == "first":
        return 0, 1
    if which == "tail":
        return r - min(8, r), r
    if r < 41:
        return r // 2, min(r // 2 + 8, r)
    hi = min(r - 24, CH_SPLIT - 32) if two_level else r - 24      # (the device keeps a row per COLUMN: a few skipped pivots shift a row up)
    a = min(max(r // 2, 16), hi)
    if a % 16 == 0:
        a += 5 if a + 5 <= hi else -5
    assert 16 <= a <= hi and a % 16 != 0
    return a, a + 8


def draw_w(r, a, b, seed):
    w = np.zeros(r)
    w[a:b] = sc.SplitMix64(seed).normal(b - a)
    return w


class Damage:
    """u [D], c, w [r], g, a, b, resid (lstsq), Pd = P - c u u^T, Sd = S - c w w^T"""
    __slots__ = ("u", "c", "w", "g", "a", "b", "resid", "Pd", "Sd")


def damage_of(st, a, b, seed, k=2.0):
    """the recipe's damage with c = k / g: S' is indefinite for every k > 1 (w^T S'^-1 w = g / (1 - k))"""
    dm = Damage()
    dm.a, dm.b = a, b
    dm.w = draw_w(st.r, a, b, seed)
    dm.u = np.linalg.lstsq(st.T, dm.w, rcond=None)[0]
    dm.resid = float(np.linalg.norm(st.T @ dm.u - dm.w) / np.linalg.norm(dm.w))
    dm.g = float(dm.w @ np.linalg.solve(st.S, dm.w))
    dm.c = float(k) / dm.g
    dm.Pd = st.P - dm.c * np.outer(dm.u, dm.u)
    dm.Sd = st.S - dm.c * np.outer(dm.w, dm.w)
    return dm


def first_bad_pivot(S):
    """(row, pivot) of the first non-positive pivot of the unpivoted Cholesky of S in double; (-1, the smallest pivot) if none"""
    A = np.array(S, dtype=np.float64)
    n, small = A.shape[0], np.inf
    for k in range(n):
        p = A[k, k]
        if not p > 0:
            return k, float(p)
        small = min(small, float(p))
        l = A[k + 1:, k] / p
        A[k + 1:, k + 1:] -= np.outer(l, A[k + 1:, k])
    return -1, small


def track_quantity_unprojected(st, dm):
    """the same for the 2 L x 2 L matrix N_j = H_x,j P H_x,j^T + sigma^2 I of the track's UNPROJECTED Jacobian, which the device's
    gate factors in place of S_j (kernels_feature.hip: gamma = y^T y - b^T C^-1 b from one Cholesky of N_j; a pivot of N_j that is
    not positive rejects the track).  S_j = A^T N_j A is a compression of N_j: this quantity is never below track_quantity."""
    worst = 0.0
    for k, Hx in enumerate(st.Hx):
        v = Hx @ dm.u
        R = st.sig2 * np.eye(Hx.shape[0]) if st.Rx is None else st.Rx[k]
        worst = max(worst, dm.c * float(v @ np.linalg.solve(Hx @ st.P @ Hx.T + R, v)))
    return worst


def indefinite_tracks(st, dm):
    """(passing tracks whose projected S_j' is not positive definite, those whose unprojected N_j' is not)"""
    ns = nn = 0
    for k, ((lo, hi), Hx) in enumerate(zip(st.rows, st.Hx)):
        Hj = st.H_o[lo:hi]
        Ro = st.sig2 * np.eye(hi - lo) if st.Ro is None else st.Ro[k]
        Rx = st.sig2 * np.eye(Hx.shape[0]) if st.Rx is None else st.Rx[k]
        ns += int(np.linalg.eigvalsh(Hj @ dm.Pd @ Hj.T + Ro)[0] <= 0)
        nn += int(np.linalg.eigvalsh(Hx @ dm.Pd @ Hx.T + Rx)[0] <= 0)
    return ns, nn


def track_quantity(st, dm):
    """c max_j (H_j u)^T S_j^-1 (H_j u) over the passing tracks, S_j = H_j P H_j^T + sigma^2 I: below 1 the gate matrix of track j
    formed with P' is positive definite, with 1 - that left of its smallest margin along H_j u"""
    worst = 0.0
    for k, (lo, hi) in enumerate(st.rows):
        Hj = st.H_o[lo:hi]
        v = Hj @ dm.u
        R = st.sig2 * np.eye(hi - lo) if st.Ro is None else st.Ro[k]
        worst = max(worst, dm.c * float(v @ np.linalg.solve(Hj @ st.P @ Hj.T + R, v)))
    return worst


def thin_floor(st):
    """min over every w of c (g_1 + ... + g_J) = 2 / lambda_max, lambda_max the largest lambda of S^-1 v = lambda D^-1 v with D the
    block diagonal of the tracks' own S_j (in the rows of H_o; needs r = m, so that T is H_o up to an orthogonal factor): the
    largest per-track quantity is at least this over J"""
    assert st.r == st.H_o.shape[0]
    Sf = st.H_o @ st.P @ st.H_o.T + st.sig2 * np.eye(st.r)
    D = np.zeros_like(Sf)
    for lo, hi in st.rows:
        D[lo:hi, lo:hi] = Sf[lo:hi, lo:hi]
    return 2.0 / float(sla.eigh(np.linalg.inv(Sf), np.linalg.inv(D), eigvals_only=True)[-1])


def seed_of(n, fam, which, sub):
    return 0x91507000 + 7919 * n + 104729 * UL.FAMILIES.index(list_of(fam)) + 1299709 * SUPPORTS.index(which) + 15485863 * int(sub) + (fam == LITERAL)


def list_of(fam):
    """update_lab's list a family of this lab runs on"""
    return "tall" if fam == LITERAL else fam.partition(":")[0]


def _oracle(po, n, fam):
    """a fresh double oracle of the window as the family's reference runs it"""
    if fam != LITERAL:
        return UL.window(po, n)
    import literal_lab as LL
    return LL.window(po, n, LITERAL_K, po.F64, po.LEAN, tol=LL.TOL64)


def reference(po, n, fam):
    if fam != LITERAL:
        return UL.reference(po, n, fam)
    import literal_lab as LL
    return LL.reference(po, n, "tall", LITERAL_K)


def stack(po, n, fam):
    key = ("st", n, fam)
    if key not in _CACHE:
        _CACHE[key] = stack_literal(po, n, LITERAL_K) if fam == LITERAL else stack_of(UL.window(po, n), FL.window(po).tr.cfg, UL.tracks_of(po, n, fam))
    return _CACHE[key]


def damage(po, n, fam, which, sub=None):
    """the lab's damage of the window's list at support `which` (cached)"""
    sub = SUB_SEEDS.get((n, fam, which), 0) if sub is None else sub
    key = ("dm", n, fam, which, sub)
    if key not in _CACHE:
        st = stack(po, n, fam)
        a, b = (0, st.r) if fam == "thin" else support_of(st.r, which, n > 32)
        assert fam != "thin" or which == "first"
        _CACHE[key] = damage_of(st, a, b, seed_of(n, fam, which, sub), C_FACTOR.get(fam, 2.0))
    return _CACHE[key]


def run_damaged(po, n, fam, which, sub=None):
    """the double oracle's update of the window's list from P' (update_lab.Result; cached)"""
    key = ("run", n, fam, which, sub)
    if key not in _CACHE:
        dm = damage(po, n, fam, which, sub)
        o = _oracle(po, n, fam)
        o.setCovariance(dm.Pd)
        r = UL.Result()
        r.P0 = o.getCovariance()
        o.setTracks(*UL.tracks_of(po, n, list_of(fam)))
        o.marginalize()
        r.P1, r.dx, r.stats, r.rows = o.getCovariance(), o.lastDeltaX(), o.lastStats(), o.lastTracks()
        r.imu, r.cams = o.getImuState(), o.getCamStates()[0]
        _CACHE[key] = r
    return _CACHE[key]


def figures(po, n, fam, which, sub=None):
    """what the CPU file asserts of one case, as numbers"""
    st, dm = stack(po, n, fam), damage(po, n, fam, which, sub)
    row, piv = first_bad_pivot(dm.Sd)
    ev = np.linalg.eigvalsh(dm.Sd)
    return dict(r=st.r, a=dm.a, b=dm.b, resid=dm.resid, row=row, pivot=piv, pivot_rel=piv / float(np.max(np.diag(dm.Sd))), cg=track_quantity(st, dm), cn=track_quantity_unprojected(st, dm),
                lam=float(ev[0] / ev[-1]), diag_min=float(np.min(np.diag(dm.Pd))), clean=first_bad_pivot(st.S)[0])


def violations(po, n, fam, which, sub=None, oracle=True):
    """[] when the case holds everything tests/test_pivot_inputs.py asks of it (oracle=False: only what needs no oracle run)"""
    f = figures(po, n, fam, which, sub)
    bad = []
    if not f["resid"] < LSTSQ_TOL:
        bad.append(("lstsq", f["resid"]))
    if f["clean"] != -1:
        bad.append(("healthy S has a bad pivot", f["clean"]))
    if f["row"] != f["a"]:
        bad.append(("first bad pivot", f["row"], f["a"]))
    if not f["pivot_rel"] <= -PIVOT_MARGIN:
        bad.append(("pivot margin", f["pivot_rel"]))
    if not f["cg"] <= TRACK_MARGIN:
        bad.append(("track margin", f["cg"]))
    if not f["cg"] <= f["cn"] * (1 + 1e-9) <= TRACK_MARGIN:
        bad.append(("track margin, unprojected", f["cn"]))
    if bad or not oracle:
        return bad
    ref, got = reference(po, n, fam), run_damaged(po, n, fam, which, sub)
    if not np.array_equal(got.rows[:, :3] > 0, ref.rows[:, :3] > 0):
        bad.append(("flags",))
    for k in ("n_tracks", "n_motion_rejected", "n_tri_rejected", "n_gate_rejected", "n_passed", "m_rows"):
        if got.stats[k] != ref.stats[k]:
            bad.append((k, got.stats[k], ref.stats[k]))
    M = UL.tracks_of(po, n, list_of(fam))[0]
    for i in np.nonzero((got.rows[:, 0] > 0) & (got.rows[:, 1] > 0))[0]:
        thr = FL.chi2_threshold(int(M[i]))
        if abs(got.rows[i, 4] - thr) < UL.GATE_MARGIN * thr:
            bad.append(("gate_margin", int(i), got.rows[i, 4], thr))
    return bad


# ------------------------------------------------------------------------------------------------------------ the frame loop
FRAME_B, FRAME_F, FRAME_AFTER = 3, 16, 5
FRAME_SHAPES = {10: "0", 8: None}      # window size -> MSCKF_HIP_SMALL_UPDATE (None: the default, k_update_small)
FRAME_SUB_SEEDS = {10: 39, 8: 180}                  # window size -> sub-seed of w, the first that holds (asserted on the CPU)


def frame_trajectories(N):
    K = N + 3
    key = ("ftr", N)
    if key not in _CACHE:
        _CACHE[key] = [sc.Trajectory(2, 500 + b, N, FRAME_F, K + FRAME_AFTER) for b in range(FRAME_B)]
    return _CACHE[key], K


def frame_damage(po, N, sub=None):
    """(Stack, Damage) at the state of the double oracle after frame K's augment of trajectory 1, from frame K's list with the
    `mid` support; the pre-augment window is one camera smaller: the caller drops u's trailing six entries"""
    sub = FRAME_SUB_SEEDS.get(N, 0) if sub is None else sub
    key = ("fdm", N, sub)
    if key not in _CACHE:
        import helpers as H
        trs, K = frame_trajectories(N)
        tr = trs[1]
        if ("fst", N) not in _CACHE:
            o = po.Oracle(po.F64, po.LEAN)
            o.initialize(tr.cfg, tr.imu0)
            for k in range(K):
                H.oracle_frame(o, tr, k, N)
            o.propagate(tr.imu_for_frame(K))
            o.augmentState(K, tr.frame_times[K])
            assert o.getNumCamStates() == N
            fr = tr.frames[K]
            _CACHE[("fst", N)] = stack_of(o, tr.cfg, (fr["M"], fr["slots"], fr["obs"]))
        st = _CACHE[("fst", N)]
        a, b = support_of(st.r, "mid", False)
        _CACHE[key] = (st, damage_of(st, a, b, seed_of(N, "tall", "mid", sub) + K))
    return _CACHE[key]


def frame_violations(po, N, sub=None):
    st, dm = frame_damage(po, N, sub)
    row, piv = first_bad_pivot(dm.Sd)
    bad = []
    if not dm.resid < LSTSQ_TOL:
        bad.append(("lstsq", dm.resid))
    if row != dm.a:
        bad.append(("first bad pivot", row, dm.a))
    if not piv <= -PIVOT_MARGIN * np.max(np.diag(dm.Sd)):
        bad.append(("pivot margin", piv))
    if not track_quantity_unprojected(st, dm) <= TRACK_MARGIN:
        bad.append(("track margin, unprojected", track_quantity_unprojected(st, dm)))
    return bad
