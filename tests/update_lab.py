"""Updates of windows of every size on both sides of every edge the update kernels have: the inputs and references of
tests/test_update_inputs.py (CPU: proves on the oracles that inputs and metric can see a fault) and
tests/test_gpu_update_kernels.py (everything that runs after k_feature, on every route of csrc/update_routes.h).
TEST INFRASTRUCTURE ONLY.

A window of n cameras is feature_lab's real 63-camera window with its 63 - n oldest cameras dropped (dropOldest: a gather of
the covariance, so every window is a consistent one and none needs a trajectory of its own).  The tracks are hand-made as
feature_lab's: a landmark in front of all 63 ground-truth cameras, projected through the n that remain, 0.5 px of noise; a
track of M observations sits in the slots round(linspace(0, n - 1, M)), M <= min(n, 30) (the feature kernels stay on their
register route: they are not the subject).  Two lists per window: `tall` (24 tracks of mixed lengths: more rows than columns
from about 10 cameras on) and `thin` (two tracks of 3 and 2 observations: 4 rows, a Gram matrix of rank 4, so that the
semidefinite pivot skipping of k_chol_mfma / k_update_small does nearly all the work).

The metric is entry-scaled (helpers.cov_scaled_err, and dx_scaled below): the Frobenius norm of helpers.state_errors is
dominated by the unobservable global position and cannot see a wrong block (GAP below, asserted on the CPU)."""
import numpy as np

import feature_lab as FL
import helpers as H
from msckf_mono_amd import scenario as sc

N_WIN = FL.N_WIN
N_MIN = 3                 # at 2 cameras every track is motion-rejected
L_MAX = 30                # routes.M_REG
N_TALL = 24
FAMILIES = ("tall", "thin")
THIN_LENGTHS = (3, 2)
NOISE_PX, REJECT_PX = 0.5, 40.0
GATE_MARGIN = FL.GATE_MARGIN
# A case on which a FLOAT ORACLE itself is farther than this from the double oracle, on either metric and in either mode, cannot
# serve to measure a float bar and is re-seeded (none may remain).  It happens to `thin` lists only, and to the oracle's GRAM mode
# only: on a stack of rank 4 its Cholesky lets pivots at the rounding level of the float H_o through or drops real ones (sub-seed 0 at
# 10 cameras: 4.7e-3, at 43: 1.5e-2, with the float LEAN oracle at 4e-7 on the same lists; at 8 cameras a fifth pivot appears).
# That is the oracle's restatement, not the device: measured on those very lists (HARD_THIN) the device stays within 1.1e-5 of the
# double oracle.  The cases that remain are all below 3.4e-5.
FLOAT_ILL = 1e-4

# Window sizes on both sides of every edge of the update (csrc/update_routes.h, kernels_gram / _chol / _kalman.hip); D = 15 + 6 n
# rows of P, 6 n columns of S, 6 n + 1 columns of [T | r_n]:
E = {
    3: "smallest window with an update (N_MIN); 6 n + 1 = 19: CH_GRAM<4>, one quarter used; k_update_small, segb 4",
    4: "first window on which every track of both lists passes; 6 n = 24: S has a partial second 16-column block",
    5: "6 n = 30: two column blocks, the second partial (k_gain<., 4>, k_gain_w<., 4, .>); D = 45",
    8: "6 n = 48 = 3 x 16: the appended r_n row opens a 16-row block of its own; k_update_small's US_SEG_E = 12 divides 48",
    10: "6 n = 60: last window of 4 column blocks of S (BLOCKED_GAIN[0], k_gain_w<., 4, .>); 6 n + 1 = 61: last of ldR = 64 (CH_GRAM<4>); "
        "segb 4: 15 tasks of chol(Lam^)",
    11: "6 n = 66: first of 8 column blocks (BLOCKED_GAIN[1], NBN = 8), the fifth block with two columns; 6 n + 1 = 67: ldR = 128 (CH_GRAM<8>); "
        "n_max + 1 = 67 > 64: k_update_small's chol(Lam^) has two row chunks, segb 8",
    12: "6 n = 72: the longest window k_update_small fits, small_limit(84) = 72 (78 columns: (15 + 78) 78 > 7168 elements; 84: 21 tiles of "
        "Lam^ for 16 wavefronts) -- not in the list this suite was specified with, which took the limit for the setting's 84 columns",
    13: "6 n = 78: first window the chain takes by default; last window of 5 column blocks of S (78 | 84)",
    14: "6 n = 84: settings.small_update, the limit k_update_small is ASKED for (it fits 72: the chain runs here); six column blocks",
    15: "6 n = 90: first window beyond settings.small_update",
    16: "6 n = 96 = 6 x 16: r_n alone in a 16-row block of its own",
    21: "6 n = 126, 6 n + 1 = 127: last of 8 column blocks (BLOCKED_GAIN[1], k_gain_w<double, 8, .> = BLOCKS_REG_F64) and of ldR = 128",
    22: "6 n = 132, 6 n + 1 = 133: 9 column blocks: BLOCKED_GAIN[2 | 3], k_gain_w<float, 12, .>, double leaves the registers for k_chol_inv; ldR = 192 (CH_GRAM<12>)",
    24: "6 n = 144 = 9 x 16; double: S (n (n + 1) scalars = 167 040 bytes) no longer fits CHOL_INV_LDS: k_chol_inv on global memory",
    26: "6 n = 156: last window of 10 column blocks of S (156 | 162)",
    27: "6 n = 162: first of 11 column blocks",
    31: "6 n + 1 = 187: last window of the one-level Gram Cholesky with its split-K copies (lam_parts)",
    32: "6 n = 192 = CH_SPLIT: last window of the one-level factorization of S (12 column blocks, BLOCKS_ONE_LEVEL); 6 n + 1 = 193: "
        "ldR = 256, first two-level Gram Cholesky (CH_GRAM_A<12>, TR_GRAM, CH_GRAM_B<4>), gram_parts = 1",
    33: "6 n = 198: 13 column blocks: GAIN_LARGE (CH_S_A<12>, TR_S21, CH_S_B<4>, TR_W<16>, k_dx_wz), has_Mp2; float form 2 and Joseph: k_chol_inv<float, false>",
    40: "6 n = 240 = 15 x 16: r_n in a block of its own, in the second level",
    42: "6 n + 1 = 253: last of ldR = 256 (CH_GRAM_B<4>); 6 n = 252: last of CH_S_B<4>",
    43: "6 n + 1 = 259: ldR = 320 (CH_GRAM_B<8>, TR_GRAM items = 2); 6 n = 258: 17 column blocks, CH_S_B<8>, TR_W<20>",
    48: "6 n = 288 = 18 x 16",
    53: "6 n + 1 = 319: last of ldR = 320; 6 n = 318: last of CH_S_B<8>",
    54: "6 n + 1 = 325: ldR = 384 (CH_GRAM_B<12>, TR_GRAM items = 3); 6 n = 324: 21 column blocks, CH_S_B<12>, TR_W<24>",
    56: "6 n = 336 = 21 x 16",
    62: "one below N_CAP_MAX",
    63: "N_CAP_MAX: 6 n + 1 = 379 of the 384 columns of six panels; 24 column blocks (BLOCKS_TWO_LEVELS), the last with 10 columns",
}
SIZES = tuple(sorted(E))
# the sizes of GAP (the table of DESIGN.md section 3.4c): a block of P_after that keeps its prior passes helpers.state_errors there
GAP_BLOCK_SIZES, GAP_DOWN_SIZES = (11, 30, 33), (4, 5, 30, 33)

# sub-seed per (n, family) (default 0), found by trying 0, 1, 2, ... on the CPU oracles until case_violations() and
# mutant_violations() are empty: double, float-LEAN and float-GRAM oracle agree on every flag and on the counts, at least one
# track passes, no double-oracle gamma within GATE_MARGIN of its threshold, no float oracle beyond FLOAT_ILL, every mutant at
# MUTANT_FACTOR float bars or more; tests/test_update_inputs.py asserts it with no case excluded.  Every `tall` list holds all of
# it at sub-seed 0.  A `thin` update moves no entry of P by more than a few per cent of its scale, and 2 % of that reaches
# ten bars on about one list in three: most re-seeds are for `downdate_2pc`, seven for FLOAT_ILL, eight for a fifth pivot.
# (n, sub-seed) of the `thin` lists that FLOAT_ILL and the fifth pivot took out of SUB_SEEDS.  They are lists the float GRAM ORACLE
# cannot do; the double oracle and the float LEAN oracle agree on them as on any other (asserted on the CPU), so the device is
# still held to the same bars on them, against the double oracle: the hardest inputs the pivot skipping gets in this suite.
HARD_THIN = ((4, 2), (5, 2), (5, 5), (5, 8), (5, 10), (5, 11), (8, 0), (10, 0), (10, 2), (12, 4), (24, 4), (43, 0), (43, 1), (63, 2))
SUB_SEEDS = {(4, "thin"): 3, (5, "thin"): 20, (8, "thin"): 2, (10, "thin"): 7, (12, "thin"): 5, (14, "thin"): 5, (16, "thin"): 1, (21, "thin"): 1, (24, "thin"): 6,
             (26, "thin"): 3, (31, "thin"): 8, (40, "thin"): 1, (43, "thin"): 4, (48, "thin"): 4, (54, "thin"): 1, (56, "thin"): 4, (63, "thin"): 4}

_CACHE = {}


# ------------------------------------------------------------------------------------------------------------ windows
def window(po, n, dtype=None, mode=None):
    """a fresh oracle holding the n newest cameras of feature_lab's window; double: a clone with its oldest cameras dropped,
    float: teacher-forced from that one as feature_lab.Window.oracle does"""
    dtype = po.F64 if dtype is None else dtype
    mode = po.LEAN if mode is None else mode
    assert N_MIN <= n <= N_WIN
    if ("w", n) not in _CACHE:
        o = FL.window(po).o.clone()
        if n < N_WIN:
            o.dropOldest(N_WIN - n)
        assert o.getNumCamStates() == n
        _CACHE[("w", n)] = o
    src = _CACHE[("w", n)]
    if dtype == po.F64:
        o = src.clone()
        o.setMode(mode)
        return o
    cams, ids = src.getCamStates()
    tr = FL.window(po).tr
    f = po.Oracle(dtype, mode)
    f.initialize(tr.cfg, tr.imu0)
    for i in range(n):
        f.augmentState(int(ids[i]), 0.0)
    f.setImuState(src.getImuState())
    for i, c in enumerate(cams):
        f.setCamPose(i, c)
    f.setCovariance(src.getCovariance())
    f.setNumResidualized(src.numResidualized())
    return f


# ------------------------------------------------------------------------------------------------------------ tracks
def slots_of(n, M):
    return np.round(np.linspace(0, n - 1, M)).astype(np.int32)


def tall_lengths(n):
    lo, hi = min(3, n), min(n, L_MAX)
    return [int(x) for x in np.round(np.linspace(lo, hi, N_TALL))]


def make_tracks(po, n, family, sub=None, noise_px=NOISE_PX):
    """(M, slots, obs) of the list of `family` in the n-camera window: slots count from the oldest camera that remains"""
    win = FL.window(po)
    sub = SUB_SEEDS.get((n, family), 0) if sub is None else sub
    rng = sc.SplitMix64(0x0D47E000 + 7919 * n + 104729 * FAMILIES.index(family) + 15485863 * int(sub))
    Ls = tall_lengths(n) if family == "tall" else list(THIN_LENGTHS)
    lm = FL._landmarks(win, rng, len(Ls))
    noise = rng.normal(len(Ls) * N_WIN * 2).reshape(len(Ls), N_WIN, 2)
    if family == "tall":                      # lengths shuffled: no kernel may rely on a sorted list
        Ls = [Ls[i] for i in np.argsort(rng.u64(len(Ls)), kind="stable")]
    first = N_WIN - n                         # the window's slot 0 is the 63-camera window's slot `first`
    M, slots, obs = [], [], []
    for i, L in enumerate(Ls):
        s = slots_of(n, L)
        g = s + first
        q = np.einsum("sij,sj->si", win.C[g], lm[i][None, :] - win.p[g])
        M.append(L)
        slots.append(s)
        obs.append(q[:, :2] / q[:, 2:3] + (noise_px / win.tr.cfg["f_u"]) * noise[i][g])
    return np.array(M, dtype=np.int32), np.concatenate(slots).astype(np.int32), np.concatenate(obs)


EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2)))


def rejected_tracks(po, n):
    """the `tall` list of the window with REJECT_PX of noise: no track passes (asserted on the CPU)"""
    return make_tracks(po, n, "tall", noise_px=REJECT_PX)


# ------------------------------------------------------------------------------------------------------------ references
class Result:
    """one update of an oracle: dx = lastDeltaX(), P0 / P1 the covariance before / after, stats, rows = lastTracks(), the state after"""
    __slots__ = ("dx", "P0", "P1", "stats", "rows", "imu", "cams")


def run_oracle(po, n, tracks, dtype=None, mode=None):
    o = window(po, n, dtype, mode)
    r = Result()
    r.P0 = o.getCovariance()
    if len(tracks[0]):
        o.setTracks(*tracks)
        o.marginalize()
    r.P1, r.dx, r.stats, r.rows = o.getCovariance(), o.lastDeltaX(), o.lastStats(), o.lastTracks()
    r.imu, r.cams = o.getImuState(), o.getCamStates()[0]
    return r


def tracks_of(po, n, family):
    """the lab's list of `family` in the n-camera window (cached); "thin:7" names sub-seed 7 of `thin` whatever SUB_SEEDS says"""
    key = ("t", n, family)
    if key not in _CACHE:
        name, _, sub = family.partition(":")
        _CACHE[key] = make_tracks(po, n, name, sub=int(sub) if sub else None)
    return _CACHE[key]


def reference(po, n, family):
    """the double oracle's update (LEAN mode: the reference's own Householder sequence), cached per session"""
    key = ("ref", n, family)
    if key not in _CACHE:
        _CACHE[key] = run_oracle(po, n, tracks_of(po, n, family))
    return _CACHE[key]


def others(po, n, family):
    """{name: Result} of the oracles the reference is compared with: float in LEAN and GRAM mode, double in GRAM mode"""
    key = ("oth", n, family)
    if key not in _CACHE:
        t = tracks_of(po, n, family)
        _CACHE[key] = {"f32_lean": run_oracle(po, n, t, po.F32, po.LEAN), "f32_gram": run_oracle(po, n, t, po.F32, po.GRAM),
                       "f64_gram": run_oracle(po, n, t, po.F64, po.GRAM)}
    return _CACHE[key]


def case_violations(ref, oth, M):
    """what the lab promises about one case, checked on its oracles: [] when all of it holds"""
    bad = []
    if not ref.stats["n_passed"] > 0:
        bad.append(("n_passed", ref.stats))
    for name, r in oth.items():
        if not np.array_equal(r.rows[:, :3] > 0, ref.rows[:, :3] > 0):
            bad.append(("flags", name))
        for k in H.STAT_KEYS:
            if r.stats[k] != ref.stats[k]:
                bad.append((k, name, r.stats[k], ref.stats[k]))
    # r_rows: the Householder sequence (LEAN) keeps every non-zero row, in float as in double; GRAM mode counts the pivots above
    # 64 eps of their diagonal, fewer by the window's unobservable directions and by a handful more or less with the rounding
    # of H_o (63 cameras, `tall`: 393 rows LEAN, 360 double GRAM, 366 float GRAM) -- never more than LEAN's
    if oth["f32_lean"].stats["r_rows"] != ref.stats["r_rows"] or max(oth["f32_gram"].stats["r_rows"], oth["f64_gram"].stats["r_rows"]) > ref.stats["r_rows"]:
        bad.append(("r_rows", {k: r.stats["r_rows"] for k, r in oth.items()}, ref.stats["r_rows"]))
    for i in np.nonzero((ref.rows[:, 0] > 0) & (ref.rows[:, 1] > 0))[0]:
        thr = FL.chi2_threshold(int(M[i]))
        if abs(ref.rows[i, 4] - thr) < GATE_MARGIN * thr:
            bad.append(("gate_margin", int(i), ref.rows[i, 4], thr))
    for name in ("f32_lean", "f32_gram"):
        if len(oth[name].dx) != len(ref.dx):        # (no update on one side: reported above)
            continue
        d = distances(oth[name], ref)
        if max(d) > FLOAT_ILL:
            bad.append(("ill_conditioned", name, d))
    return bad


# ------------------------------------------------------------------------------------------------------------ the metric
def dx_scaled(dx, dx_ref, P0):
    """max_i |dx_i - dx_ref_i| / sqrt(P0_ii): every entry of the correction against the prior standard deviation of ITS state"""
    return float(np.max(np.abs(np.asarray(dx, dtype=np.float64) - dx_ref) / np.sqrt(np.diag(P0))))


def distances(r, ref):
    """(covariance, correction) distance of an update from the reference's on the entry-scaled metric"""
    return H.cov_scaled_err(r.P1, ref.P1), dx_scaled(r.dx, ref.dx, ref.P0)


# Float bars: FLOAT_FACTOR x the largest distance of the float oracle (LEAN and GRAM mode) from the double oracle over SIZES x
# FAMILIES -- ONE constant per metric (a `thin` case where the float oracle happens to be 4e-7 away must not set a bar the device
# cannot meet); the factor is DESIGN.md section 3.4a's allowance for another valid summation order (MFMA blocks against the
# oracle's loops).  D32_* are measured on the CPU (tests/test_update_inputs.py asserts that they reproduce), never on the device.
FLOAT_FACTOR = 4.0
D32_COV, D32_DX = 3.40e-5, 1.42e-5     # measured 3.390e-05 (26 cameras, `tall`, LEAN) and 1.415e-05 (26 cameras, `tall`, GRAM), rounded up
D32_MEASURED = (3.390e-5, 1.415e-5)
BAR_F64 = 1e-6            # DESIGN.md section 3.4, on this metric; d64 (double LEAN against double GRAM) shows the room it leaves
D64_ROOM = 1e-10          # measured d64 <= 8.3e-12 (covariance, 14 cameras `tall`) and 1.4e-11 (correction, 62 cameras `tall`): held from above only


def bars(prec):
    return (BAR_F64, BAR_F64) if prec == "f64" else (FLOAT_FACTOR * D32_COV, FLOAT_FACTOR * D32_DX)


# ------------------------------------------------------------------------------------------------------------ mutants
MUTANTS = ("att_block", "tail_block", "cross_block", "downdate_2pc", "dx_newest", "dx_last")
COV_MUTANTS = MUTANTS[:4]
MUTANT_FACTOR = 10.0      # every mutant scores at least this many float bars


def mutate(ref, which):
    """(P_after, dx) of the double oracle's own result with ONE deliberate damage -- never applied to code under test"""
    P, dx, P0 = ref.P1.copy(), ref.dx.copy(), ref.P0
    D = P.shape[0]
    if which == "att_block":          # the newest camera's 3 x 3 attitude block keeps its prior
        s = slice(D - 6, D - 3)
        P[s, s] = P0[s, s]
    elif which == "tail_block":       # the trailing partial 16-block of P keeps its prior (D = 15 + 6 n is odd: it always exists)
        s = slice(16 * (D // 16), D)
        P[s, s] = P0[s, s]
    elif which == "cross_block":      # theta_I x newest camera keeps its prior
        P[0:3, D - 6:D] = P0[0:3, D - 6:D]
        P[D - 6:D, 0:3] = P0[D - 6:D, 0:3]
    elif which == "downdate_2pc":     # 2 % of the downdate missing everywhere
        P = P + 0.02 * (P0 - P)
    elif which == "dx_newest":        # the newest camera is not corrected
        dx[D - 6:] = 0.0
    elif which == "dx_last":          # the last entry of the correction is lost
        dx[D - 1] = 0.0
    else:
        raise ValueError(which)
    return P, dx


# The one mutant that cannot reach MUTANT_FACTOR bars: at 3 cameras the whole update (at most 15 rows on very little parallax)
# moves no entry of P by more than 3 % of its scale, and 2 % of that is 6.2e-4 (`tall`) / 2.1e-4 (`thin`) against a bar of 1.36e-4
MUTANT_EXEMPT = {(3, "downdate_2pc")}


def mutant_violations(ref, n):
    """[] when every mutant that exists at n scores MUTANT_FACTOR float bars or more on the double oracle's own result"""
    bc, bd = bars("f32")
    out = []
    for m in MUTANTS:
        if (n, m) in MUTANT_EXEMPT:
            continue
        s = mutant_score(ref, m)
        if not s >= MUTANT_FACTOR * (bc if m in COV_MUTANTS else bd):
            out.append((m, s))
    return out


def mutant_score(ref, which):
    """the mutant's distance from the unmutated reference on the metric it damages"""
    P, dx = mutate(ref, which)
    return H.cov_scaled_err(P, ref.P1) if which in COV_MUTANTS else dx_scaled(dx, ref.dx, ref.P0)


def mutant_frobenius(ref, which):
    """worst entry of helpers.state_errors for a covariance mutant: what the existing suites see of it"""
    P, _ = mutate(ref, which)
    return H.worst(H.state_errors(ref.imu, ref.imu, ref.cams, ref.cams, P, ref.P1))
