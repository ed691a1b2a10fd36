"""Hand-made feature tracks on one real 63-camera window: the inputs of tests/test_feature_inputs.py (CPU: proves on the oracles
that inputs and metric can see a fault) and tests/test_gpu_feature_kernels.py (the feature kernels, track by track, on every
route of launch_feature).  TEST INFRASTRUCTURE ONLY.

The window is filled once per session on the double oracle (scenario.Trajectory(5, WINDOW_SEED, 63, 8, 66): 65 whole frames,
then propagate + augmentState, so that 63 camera states are present); the device is teacher-forced with
helpers.copy_oracle_to_device.  The tracks are made here, not taken from the trajectory: a landmark 3 - 8 m in front of the
mid-window camera that every one of the 63 ground-truth cameras sees in front of it (z > 0.5, |x/z|, |y/z| < 3: the kernels do
not care about a field of view), projected through the ground-truth cameras, plus Gaussian noise of the track's own size.  A
track of length L keeps L of its 63 observations in one of four slot patterns (PATTERNS).

Per-track results of an update (flags, gamma, point) depend on the state before it only, never on the other tracks of the list
(checkMotion runs for every track once more than 3 tracks have been residualized; the fill residualizes hundreds): a reference
row computed in one list holds in every sub-list."""
import os
import re

import numpy as np

import helpers as H
from msckf_mono_amd import scenario as sc

N_WIN = 63
WINDOW_SEED = 21
PATTERNS = ("spread", "tail", "head", "gapped")
GAP_SLOTS = (20, 41)      # `gapped`: two interior cameras no track sees (the kernels' packed slot range has holes: sInv < 0 columns)

# Track lengths on both sides of every edge the feature kernels have (kernels_feature.hip); reason per edge:
EDGES = {
    2: "shortest track checkMotion accepts (M < 2 is flagged unresidualizable in both kernels); 2M + 4 = 8: gate_chol<., 1>",
    3: "min_track_length; 2M - 3 = 3 rows; 2M + 4 = 10 crosses 8: gate_chol<., 2>",
    4: "feature_pair_lds_bytes sizes s_cap for the longest track + a 4-observation partner",
    5: "one past the 4-observation partner: a pair (30, 5) does not fit s_cap together and is factored one after the other",
    6: "2M + 4 = 16: last length of the two-block instances (gate_chol / gate_chol_dpp <2>)",
    7: "2M + 4 = 18 crosses 16: first of the <3> instances",
    10: "2M + 4 = 24: last of the <3> instances", 11: "2M + 4 = 26 crosses 24: first of the <4> instances",
    14: "2M + 4 = 32: last of the <4> instances", 15: "2M + 4 = 34 crosses 32: first of the <5> instances",
    16: "lane 15 | 16 of a half: k_feature_pair's sums stay inside one DPP row of 16",
    17: "first track with observations in both DPP rows of its half (v_permlane16_swap)",
    18: "2M + 4 = 40: last of the <5> instances", 19: "2M + 4 = 42 crosses 40: first of the <6> instances",
    22: "2M + 4 = 48: last of the <6> instances", 23: "2M + 4 = 50 crosses 48: first of the <7> instances",
    26: "2M + 4 = 56: last of the <7> instances", 27: "2M + 4 = 58 crosses 56: first of the <8> instances",
    29: "last length below M_REG",
    30: "M_REG = 30: 2M + 4 = 64, the whole 8 x 8 lane grid of blocks; last length of k_feature_pair and k_feature<., false>",
    31: "first length of k_feature<., true>: gate_chol<., 10>, gate_chol_staged<10>; 2M + 4 = 66 crosses 64",
    32: "GS = 32 lanes per track in k_feature_pair (M > GS is refused there)", 33: "one past GS",
    38: "2M + 4 = 80: last length of the <10> long instances", 39: "2M + 4 = 82 crosses 80: first of the <12> instances",
    40: "m_cap of the one-long-launch routes (m_cap - 30 < 16: no bins)",
    46: "2M + 4 = 96: last of the <12> instances; double: last register-resident length (nr <= 96)",
    47: "2M + 4 = 98: first of the <14> instances; double: in-place LDS factorization; mid = (30 + 63 + 1) / 2: last of bin (30, mid]",
    48: "first length of bin (mid, m_cap] at m_cap = 63",
    54: "2M + 4 = 112: last of the <14> instances", 55: "2M + 4 = 114 crosses 112: first of the <16> instances",
    60: "never executed before this suite (the scenario generator's longest track in a 60-camera window is 59)",
    61: "never executed before this suite, as 60",
    62: "2M + 4 = 128: last length of gate_chol_staged (m_cap <= 62) and of the float register-resident instances (nr <= 128)",
    63: "2M + 4 = 130 crosses 128: float in-place LDS factorization; m_cap 63 leaves the staged route for the two bins; M = n_cap",
}
# M = m_cap + 1 never reaches a kernel: check_worklist (msckf_hip.hip) refuses the list with -E2BIG "track longer than m_cap"
# before anything is staged (tests/test_gpu_parity.py::test_work_list_rules_...; asserted again per route in the GPU suite).
EDGE_LENGTHS = tuple(sorted(EDGES))
NOISE_PX = (0.5, 3.5, 4.5, 5.5)       # against the assumed 7 px: 3.5 px passes the 5 % gate at most lengths, 5.5 px fails it at most
EXTRA_NOISE_PX = (0.5, 6.0)           # two more tracks per edge length, so that both decisions occur on each side of every edge
HUBER_PX, OUTLIER_PX, OUTLIER_BASE_PX = 10.0, 40.0, 6.0
# initializePosition rejects on sum |e|^2 / (2 M^2) > max_gn_cost_norm = (7 px)^2: ONE observation moved by e px is rejected for
# e > 9.9 M px, so 40 px rejects tracks of up to 4 observations only (measured: exactly those).  `gross` moves one observation by
# GROSS_PX_PER_OBS * M px instead (cost ~ 4 x the limit at every length): the triangulation-rejected case of the long routes.
GROSS_PX_PER_OBS, GROSS_BASE_PX = 20.0, 0.5
TRI_MARGIN = 0.05                     # no track's normalized triangulation cost (numpy, from the double oracle's point) within 5 % of its limit
BRANCH_MIN_L = 4
GATE_MARGIN = 0.01                    # no track's double-oracle gamma within 1 % of its threshold
# seed per pattern of landmarks + noise, found by trying seeds 1, 2, ... on the CPU oracle until lab_violations() is empty: NO track
# inside GATE_MARGIN or TRI_MARGIN, every branch case as intended; tests/test_feature_inputs.py asserts it, and that both gate
# decisions occur at every edge length
LAB_SEEDS = {"spread": 4, "tail": 2, "head": 2, "gapped": 6}


def chi2_threshold(M):
    """gate threshold of a track of M observations: the oracle's chi_squared_test_table[dof + 1] with dof = M - 1 (msckf.h:432,
    gatingTest), the 5 % quantile of chi-squared(M + 1)"""
    return _chi2()[M]


_CACHE = {}


def _chi2():
    if "chi2" not in _CACHE:
        txt = open(os.path.join(H.ROOT, "oracle", "chi2_table.h")).read()
        body = txt[txt.index("{") + 1:txt.index("}")]
        _CACHE["chi2"] = np.array([float(x) for x in re.findall(r"[-+0-9.eE]+", body)])
        assert len(_CACHE["chi2"]) == 99
    return _CACHE["chi2"]


# ------------------------------------------------------------------------------------------------------------ the window
class Window:
    """tr: the trajectory; o: double oracle holding 63 camera states (never updated again: clone it); frames[s]: the
    trajectory's frame index of camera slot s"""

    def __init__(self, po):
        self.po = po
        tr = sc.Trajectory(5, WINDOW_SEED, N_WIN, 8, 66)
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        for k in range(65):
            H.oracle_frame(o, tr, k, N_WIN)
        o.propagate(tr.imu_for_frame(65))
        o.augmentState(65, tr.frame_times[65])
        assert o.getNumCamStates() == N_WIN and o.numResidualized() > 3
        self.tr, self.o = tr, o
        self.frames = o.getCamStates()[1].astype(np.int64)
        assert list(self.frames) == list(range(3, 66))
        self.C = tr.C_CG[self.frames]          # ground-truth cameras of the 63 slots
        self.p = tr.p_C[self.frames]
        self._f32 = None

    def oracle(self, dtype):
        """a fresh oracle of `dtype` holding the window (double: a clone; float: teacher-forced from the double one)"""
        po = self.po
        if dtype == po.F64:
            return self.o.clone()
        if self._f32 is None:
            cams, ids = self.o.getCamStates()
            f = po.Oracle(po.F32, po.LEAN)
            f.initialize(self.tr.cfg, self.tr.imu0)
            for i in range(N_WIN):
                f.augmentState(int(ids[i]), 0.0)
            f.setImuState(self.o.getImuState())
            for i, c in enumerate(cams):
                f.setCamPose(i, c)
            f.setCovariance(self.o.getCovariance())
            f.setNumResidualized(self.o.numResidualized())
            self._f32 = f
        return self._f32.clone()


def window(po):
    if "win" not in _CACHE:
        _CACHE["win"] = Window(po)
    return _CACHE["win"]


# ------------------------------------------------------------------------------------------------------------ the tracks
def pattern_slots(pattern, L):
    if pattern == "spread":
        return np.round(np.linspace(0, N_WIN - 1, L)).astype(np.int32)
    if pattern == "tail":
        return np.arange(N_WIN - L, N_WIN, dtype=np.int32)
    if pattern == "head":
        return np.arange(L, dtype=np.int32)
    assert pattern == "gapped"
    free = np.array([s for s in range(N_WIN) if s not in GAP_SLOTS], dtype=np.int32)
    return free[np.round(np.linspace(0, len(free) - 1, L)).astype(np.int64)]


def pattern_max_len(pattern):
    return N_WIN - len(GAP_SLOTS) if pattern == "gapped" else N_WIN


class Track:
    __slots__ = ("L", "pattern", "kind", "noise_px", "slots", "obs", "landmark", "moved")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def copy(self, **kw):
        t = Track(**{k: getattr(self, k) for k in self.__slots__})
        t.slots, t.obs = self.slots.copy(), self.obs.copy()
        for k, v in kw.items():
            setattr(t, k, v)
        return t


def _landmarks(win, rng, n):
    out = []
    mid = N_WIN // 2
    while len(out) < n:
        u = rng.uniform(3 * 64).reshape(64, 3)
        d = 3.0 + 5.0 * u[:, 2]
        ax, ay = 0.5 * (2 * u[:, 0] - 1), 0.5 * (2 * u[:, 1] - 1)
        pc = np.stack([d * np.tan(ax), d * np.tan(ay), d], -1)
        pw = pc @ win.C[mid] + win.p[mid]                                   # C^T pc + p
        q = np.einsum("sij,nsj->nsi", win.C, pw[:, None, :] - win.p[None])
        ok = np.all((q[..., 2] > 0.5) & (np.abs(q[..., 0]) < 3 * q[..., 2]) & (np.abs(q[..., 1]) < 3 * q[..., 2]), axis=1)
        out.extend(pw[ok])
    return np.array(out[:n])


def make_track(win, landmark, unit_noise, pattern, L, noise_px, kind="base"):
    """unit_noise [63][2]: the track's N(0, 1) draws per slot (a longer or shorter track of the same landmark shares them)"""
    slots = pattern_slots(pattern, L)
    q = np.einsum("sij,sj->si", win.C[slots], landmark[None, :] - win.p[slots])
    obs = q[:, :2] / q[:, 2:3] + (noise_px / win.tr.cfg["f_u"]) * unit_noise[slots]
    moved = -1
    if kind in ("huber", "outlier", "gross"):
        moved = L // 2
        obs[moved, 0] += {"huber": HUBER_PX, "outlier": OUTLIER_PX, "gross": GROSS_PX_PER_OBS * L}[kind] / win.tr.cfg["f_u"]
    return Track(L=L, pattern=pattern, kind=kind, noise_px=noise_px, slots=slots, obs=obs, landmark=landmark, moved=moved)


def pattern_tracks(win, pattern, seed=None):
    """The lab's list of one pattern, lengths shuffled, every landmark distinct: per length 2 .. 63 one track (noise cycling
    through NOISE_PX with the length), per edge length two more (EXTRA_NOISE_PX) and, from BRANCH_MIN_L on, the branch
    cases: `huber` (0.5 px and ONE observation moved by 10 px), `outlier` (6 px and one observation moved by 40 px) and `gross`
    (0.5 px and one observation moved by 20 M px)."""
    seed = LAB_SEEDS[pattern] if seed is None else seed
    rng = sc.SplitMix64(0xFEA70000 + 7919 * PATTERNS.index(pattern) + 104729 * int(seed))
    spec = []
    for L in range(2, pattern_max_len(pattern) + 1):
        spec.append((L, NOISE_PX[(L + PATTERNS.index(pattern)) % 4], "base"))
        if L in EDGES:
            spec += [(L, px, "base") for px in EXTRA_NOISE_PX]
            if L >= BRANCH_MIN_L:
                spec += [(L, 0.5, "huber"), (L, OUTLIER_BASE_PX, "outlier"), (L, GROSS_BASE_PX, "gross")]
    lm = _landmarks(win, rng, len(spec))
    noise = rng.normal(len(spec) * N_WIN * 2).reshape(len(spec), N_WIN, 2)
    order = np.argsort(rng.u64(len(spec)), kind="stable")
    return [make_track(win, lm[i], noise[i], pattern, spec[i][0], spec[i][1], spec[i][2]) for i in order]


def lab(po):
    """{pattern: [Track]} -- the whole lab, built once"""
    if "lab" not in _CACHE:
        win = window(po)
        _CACHE["lab"] = {p: pattern_tracks(win, p) for p in PATTERNS}
    return _CACHE["lab"]


def worklist(tracks):
    M = np.array([len(t.slots) for t in tracks], dtype=np.int32)
    slots = np.concatenate([t.slots for t in tracks]).astype(np.int32) if len(tracks) else np.zeros(0, np.int32)
    obs = np.concatenate([t.obs for t in tracks]) if len(tracks) else np.zeros((0, 2))
    return M, slots, obs


# ------------------------------------------------------------------------------------------------------------ references
def run_oracle(win, dtype, tracks, want_update=False):
    """one marginalize of `tracks` on a fresh oracle of the window: lastTracks rows [F][8] (motion_ok tri_valid gate_pass rows
    gamma p_f_G), lastStats; with want_update also lastDeltaX and P_after - P_before"""
    o = win.oracle(dtype)
    M, slots, obs = worklist(tracks)
    P0 = o.getCovariance() if want_update else None
    o.setTracks(M, slots, obs)
    o.marginalize()
    rows, st = o.lastTracks(), o.lastStats()
    assert len(rows) == len(tracks)
    if not want_update:
        return rows, st
    return rows, st, o.lastDeltaX(), o.getCovariance() - P0


def reference(po, pattern):
    """double-oracle rows and stats of the lab's list of `pattern` (cached)"""
    key = ("ref", pattern)
    if key not in _CACHE:
        _CACHE[key] = run_oracle(window(po), po.F64, lab(po)[pattern])
    return _CACHE[key]


def stats_of(rows):
    """lastStats of a list whose oracle rows are `rows` (a sub-list of a reference list: the counts are sums over its tracks)"""
    mo, tv, gp = rows[:, 0] > 0, rows[:, 1] > 0, rows[:, 2] > 0
    return dict(n_tracks=len(rows), n_motion_rejected=int((~mo).sum()), n_tri_rejected=int((mo & ~tv).sum()),
                n_gate_rejected=int((mo & tv & ~gp).sum()), n_passed=int((mo & tv & gp).sum()), m_rows=int(rows[mo & tv & gp, 3].sum()))


def tri_cost(win, o_cams, track, point):
    """initializePosition's normalized cost sum |e|^2 / (2 M^2) of `point`, relative to its limit max_gn_cost_norm"""
    r = reprojection_residuals(win, o_cams, track, point)
    return float((r * r).sum() / (2.0 * len(r) ** 2) / win.tr.cfg["max_gn_cost_norm"])


def lab_violations(win, pattern, tracks, rows):
    """what the lab promises about one pattern's list, checked on its double-oracle rows: [] when all of it holds"""
    cams, _ = win.o.getCamStates()
    bad = []
    for i, t in enumerate(tracks):
        if rows[i, 0] <= 0:
            continue
        c = tri_cost(win, cams, t, rows[i, 5:8])
        if abs(c - 1.0) < TRI_MARGIN or (c < 1.0) != (rows[i, 1] > 0) and t.kind != "gross":
            bad.append(("tri_margin", t.L, t.kind, c, rows[i, 1]))
        if rows[i, 1] > 0:
            thr = chi2_threshold(t.L)
            if abs(rows[i, 4] - thr) < GATE_MARGIN * thr:
                bad.append(("gate_margin", t.L, t.kind, rows[i, 4], thr))
            if t.kind == "huber":
                r = reprojection_residuals(win, cams, t, rows[i, 5:8])
                if not (r[t.moved] > 0.01 and np.delete(r, t.moved).max() < 0.01):
                    bad.append(("huber", t.L, r[t.moved], np.delete(r, t.moved).max()))
        elif t.kind in ("base", "huber"):
            bad.append(("tri_rejected", t.L, t.kind))
        if t.kind == "gross" and rows[i, 1] > 0:
            bad.append(("gross_valid", t.L))
    return bad


def reprojection_residuals(win, o_cams, track, point):
    """|z - h(point)| per observation of `track` through the ESTIMATED cameras o_cams [63][7] (what the LM step weighs)"""
    r = np.zeros(len(track.slots))
    for i, s in enumerate(track.slots):
        a = H.q_to_rot(o_cams[s, :4]) @ (point - o_cams[s, 4:7])
        r[i] = np.linalg.norm(track.obs[i] - a[:2] / a[2])
    return r


# ------------------------------------------------------------------------------------------------------------ the float bars
def track_errors(win, rows, ref, tracks):
    """per track with a Jacobian in the reference (motion_ok and tri_valid): (worst reprojection difference of the two points
    over the track's cameras, |point difference| / max(depth, 1), relative gamma difference, absolute gamma difference)"""
    cams, _ = win.o.getCamStates()
    out = {}
    for t in np.nonzero((ref[:, 0] > 0) & (ref[:, 1] > 0))[0]:
        pd, pr = rows[t, 5:8], ref[t, 5:8]
        rp, depth = 0.0, 1e9
        for s in tracks[t].slots:
            R = H.q_to_rot(cams[s, :4])
            a, b = R @ (pd - cams[s, 4:7]), R @ (pr - cams[s, 4:7])
            rp = max(rp, float(np.abs(a[:2] / a[2] - b[:2] / b[2]).max()))
            depth = min(depth, float(b[2]))
        dg = abs(rows[t, 4] - ref[t, 4])
        out[int(t)] = (rp, float(np.linalg.norm(pd - pr)) / max(depth, 1.0), dg / max(abs(ref[t, 4]), 1e-300), dg)
    return out


# bars of helpers.check_tracks(prec="f32") per entry of track_errors; gamma: relative 1e-3, plus 1e-3 absolute only at gamma <= 0.05
BAR_REPROJ, BAR_DEPTH, BAR_GAMMA_REL, BAR_GAMMA_ABS, GAMMA_ABS_BELOW = 1e-4, 2e-3, 1e-3, 1e-3, 0.05


def gamma_bar(gamma_ref):
    return BAR_GAMMA_REL * abs(gamma_ref) + (BAR_GAMMA_ABS if abs(gamma_ref) <= GAMMA_ABS_BELOW else 0.0)


# ------------------------------------------------------------------------------------------------------------ one-track updates
ONE_TRACK_PATTERN, ONE_TRACK_PX = "spread", 0.5
ONE_TRACK_FLOAT_FACTOR = 4.0          # the device may be this many times as far from the double oracle as the float oracle is
ONE_TRACK_ILL = 1e-2                  # a track on which the float oracle itself is farther than this is replaced (none may remain)


# sub-seed per edge length (default 0), chosen on the CPU oracle so that EVERY mutant below moves the track's gamma or point by at
# least 10 x the float bars (a 0.5 px track's last observation adds ~2 / (2 M - 3) of gamma: 16 x the 1e-3 bar at M = 63 on
# average, less by chance); tests/test_feature_inputs.py asserts it
ONE_TRACK_SEEDS = {3: 1, 4: 1, 7: 1, 11: 1, 26: 1, 14: 2, 15: 1, 16: 2, 17: 1, 22: 2, 30: 1, 32: 1, 38: 1, 39: 3, 46: 1, 47: 8, 60: 1, 61: 2}


def one_track_case(win, L, sub=None):
    sub = ONE_TRACK_SEEDS.get(L, 0) if sub is None else sub
    rng = sc.SplitMix64(0x0E7AC000 + 1009 * L + 7 * int(sub))
    lm = _landmarks(win, rng, 1)
    noise = rng.normal(N_WIN * 2).reshape(N_WIN, 2)
    return make_track(win, lm[0], noise, ONE_TRACK_PATTERN, L, ONE_TRACK_PX)


def one_track_cases(po):
    """per edge length one `spread` track of 0.5 px (it passes the gate at every length: asserted on the CPU) with a landmark of
    its own"""
    if "one" not in _CACHE:
        win = window(po)
        _CACHE["one"] = [one_track_case(win, L) for L in EDGE_LENGTHS]
    return _CACHE["one"]


def mutant_score(win, track, rows, which):
    """how far mutant `which` moves the double oracle's result for `track` (rows: its unmutated result), in units of the float
    bars of helpers.check_tracks: inf when a flag changes, None when the mutant does not exist at this length"""
    tm = mutate(win, track, which)
    if tm is None:
        return None, None
    out = run_oracle(win, win.po.F64, [tm], want_update=True)
    rm = out[0]
    if not np.array_equal(rm[0, :3], rows[0, :3]):
        return float("inf"), out
    e = track_errors(win, rm, rows, [track])[0]
    return max(e[0] / BAR_REPROJ, e[1] / BAR_DEPTH, e[3] / gamma_bar(rows[0, 4])), out


def one_track_reference(po, dtype):
    """[(rows, stats, deltaX, dP)] per case of one_track_cases on the oracle of `dtype` (cached)"""
    key = ("one_ref", dtype)
    if key not in _CACHE:
        win = window(po)
        _CACHE[key] = [run_oracle(win, dtype, [t], want_update=True) for t in one_track_cases(po)]
    return _CACHE[key]


def update_errors(dx, dP, dx_ref, dP_ref):
    """(|dx - dx_ref| / |dx_ref|, |dP - dP_ref|_F / |dP_ref|_F): each relative to the reference's norm of that CHANGE"""
    return (float(np.linalg.norm(np.asarray(dx) - dx_ref) / np.linalg.norm(dx_ref)),
            float(np.linalg.norm(np.asarray(dP) - dP_ref) / np.linalg.norm(dP_ref)))


# ------------------------------------------------------------------------------------------------------------ mutants
MUTANTS = ("drop_last", "swap_slots", "move_1px", "neighbour_slot")


def mutate(win, track, which):
    """a copy of `track` with ONE deliberate mistake -- given to the reference only, never to the code under test"""
    t = track.copy()
    L = len(t.slots)
    if which == "drop_last":
        t.slots, t.obs = t.slots[:-1].copy(), t.obs[:-1].copy()
    elif which == "swap_slots":                     # two observations' slots swapped (first and last: the largest parallax)
        t.slots[[0, L - 1]] = t.slots[[L - 1, 0]]
    elif which == "move_1px":
        t.obs[L // 2, 1] += 1.0 / win.tr.cfg["f_u"]
    elif which == "neighbour_slot":                 # one slot replaced by a neighbouring camera the track does not see
        used = set(int(s) for s in t.slots)
        for i in list(range(L // 2, L)) + list(range(L // 2)):
            for s in (int(t.slots[i]) + 1, int(t.slots[i]) - 1):
                if 0 <= s < N_WIN and s not in used:
                    t.slots[i] = s
                    return t
        return None                                  # a track of all 63 cameras has no unseen neighbour
    else:
        raise ValueError(which)
    return t


# ------------------------------------------------------------------------------------------------------------ the early-accept line
# Tracks on both sides of the early-accept rule of msckf_hip_set_gate_early_accept, ub = |r_o|^2 / sigma^2 < 0.5 * threshold: per
# length class LINE_SUBS landmarks (`spread` slots, a landmark and unit noise of their own), each at the two noise sizes where the
# double twin of tests/h16_lab.py puts ub / (0.5 * threshold) at 0.98 and at 1.02 -- found by bisection on the CPU (ub grows with
# the square of the noise); tests/test_feature_inputs.py asserts that they land there.  A float kernel's ub differs by ~1e-5: both
# sides are far outside the 1e-3 band in which either report is accepted.
LINE_LENGTHS = (2, 3, 16, 30, 31, 62)
LINE_TARGETS = (0.98, 1.02)
LINE_SUBS = 2
LINE_TOL = 1e-4                       # how close to its target a line case's ratio is (asserted on the CPU)
LINE_NOISE_PX = {(2, 0, 0.98): 7.22122573, (2, 0, 1.02): 7.36258755, (2, 1, 0.98): 1.29741525, (2, 1, 1.02): 1.32307730,
                 (3, 0, 0.98): 3.01268468, (3, 0, 1.02): 3.06830646, (3, 1, 0.98): 2.19028855, (3, 1, 1.02): 2.23419040,
                 (16, 0, 0.98): 2.91333937, (16, 0, 1.02): 2.97334564, (16, 1, 0.98): 2.78549022, (16, 1, 1.02): 2.84155778,
                 (30, 0, 0.98): 2.75003289, (30, 0, 1.02): 2.80535436, (30, 1, 0.98): 3.09777572, (30, 1, 1.02): 3.16013138,
                 (31, 0, 0.98): 2.85974972, (31, 0, 1.02): 2.91741167, (31, 1, 0.98): 3.08037391, (31, 1, 1.02): 3.14223710,
                 (62, 0, 0.98): 2.70816967, (62, 0, 1.02): 2.76285612, (62, 1, 0.98): 3.06557625, (62, 1, 1.02): 3.12725493}


def line_case(win, L, sub, target):
    rng = sc.SplitMix64(0x11AE0000 + 1009 * L + 7 * int(sub))
    lm = _landmarks(win, rng, 1)
    noise = rng.normal(N_WIN * 2).reshape(N_WIN, 2)
    return make_track(win, lm[0], noise, "spread", L, LINE_NOISE_PX[(L, sub, target)], kind="line")


def line_cases(po, m_cap=N_WIN):
    """the line cases of at most m_cap observations, the 0.98 and the 1.02 case of a landmark next to each other"""
    win = window(po)
    return [line_case(win, L, sub, tg) for L in LINE_LENGTHS if L <= m_cap for sub in range(LINE_SUBS) for tg in LINE_TARGETS]
