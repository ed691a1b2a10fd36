"""The literal anisotropic route (u_var' != v_var', aniso_mode 0: kernels_literal.hip over literal_core.h) at windows on both
sides of every size edge it has: the inputs and references of tests/test_literal_inputs.py (CPU: proves on the oracles and on the
host build of literal_core.h that inputs and metric can see a fault) and tests/test_gpu_literal_kernels.py (k_lit_pre,
k_lit_gamma, k_lit_phase<S, 0..3>, k_literal_dense against the double oracle).  TEST INFRASTRUCTURE ONLY.

Built on update_lab / feature_lab: a window of n cameras is update_lab.window(po, n)'s covariance and poses, teacher-forced into
a fresh oracle initialised with the window's config plus v_var_prime = K u_var_prime.  With the EuRoC intrinsics u' and v' differ
by 0.6 % and the pre-whitened (GLS) update is 9e-8 away from the literal one: a device that computed GLS would pass every float
bar.  K = 4 (and 1/4 on a subset: the sign of u' - v') puts GLS 6e-4 .. 3e-2 away.  The gate keeps u' whatever v' is, so flags
and counts are those of the isotropic lab.

References: the double LEAN oracle with setTinyRowTol(TOL64) (THE reference), the float LEAN oracle with TOL32 (what a correct
float implementation looks like: the float bars), and for aniso_mode 1 the double GRAM oracle with setWhiten(True)."""
import os
import re

import numpy as np

import feature_lab as FL
import helpers as H
import update_lab as UL
from msckf_mono_amd import scenario as sc

N_WIN, N_MIN = UL.N_WIN, UL.N_MIN
K_MAIN, K_INV = 4.0, 0.25
TOL64, TOL32 = 1e-10, 8e-4            # the device's default zero-tail tolerances (double, float)
F_CAP, F_CAP_WIDE, M_CAP_LONG = 32, 260, 63
NOISE_PX = UL.NOISE_PX

_CSRC = os.path.join(H.ROOT, "msckf_mono_amd", "csrc")


def lds_doubles():
    """LIT_LDS_DOUBLES as kernels_literal.hip has it today: a moved constant moves every side computed below"""
    m = re.search(r"constexpr int LIT_LDS_DOUBLES = (\d+);", open(os.path.join(_CSRC, "kernels_literal.hip")).read())
    return int(m.group(1))


# ------------------------------------------------------------------------------------------------------------ the edges
# Window sizes on both sides of every edge of the literal route, with lds = LIT_LDS_DOUBLES = 12000 (kernels_literal.hip:25),
# n1 = 6 n + 1, D = 15 + 6 n, e = min(m, D) explicit rows; and the sizes of update_lab.E that decide what the chain does with Lam^.
E = {
    3: "smallest window with an update",
    5: "`brim`: m = D - 1, D, D + 1 = 44, 45, 46 stacked rows: `gram = m > e` (literal_core.h:1643, LIT_COMPACT_LAYOUT): the exact-tail path "
       "(no row below the explicit ones, sweep over E alone) | sweep_gram_blocked; 6 n = 30: one 32-column tile of k_lit_gamma",
    6: "6 n = 36: first window with a second tile row of k_lit_gamma (32 x 32 tiles, kernels_literal.hip:293-310), 4 columns in it",
    10: "6 n + 1 = 61: last of ldR = 64; first window whose `tall` list has more rows than D; a track over all 10 slots fills "
        "k_lit_pre's `col0 += 64` loop once (60 columns, kernels_literal.hip:268)",
    11: "6 n + 1 = 67: ldR = 128; a track over all 11 slots takes two rounds of `col0 += 64` (66 columns); 6 n = 66: third tile row of k_lit_gamma",
    16: "6 n = 96 = 3 x 32: k_lit_gamma's tiles all full; `wide` (255 | 256 | 257 stacked tracks, `e < 256` in track_of, kernels_literal.hip:333; "
        "odd P: the pair's second track absent) and 64 | 65, 128 | 129 tracks: per = 1 | 2, 2 | 3 in the offsets scan, kernels_literal.hip:83",
    21: "6 n + 1 = 127: last of ldR = 128 (CH_GRAM<8>)", 22: "6 n + 1 = 133: ldR = 192 (CH_GRAM<12>)",
    30: "the benchmarked window (tests/test_gpu_literal.py stops here)",
    31: "6 n + 1 = 187: last one-level Gram Cholesky with split-K copies; compact_basis' `tiles` (33 n1 + 104 + 30 ldb <= lds, ldb = (nb + 7) & ~3, "
        "literal_core.h:1942) holds for every basis: ldb <= 188",
    32: "6 n + 1 = 193 > 192: the literal Lam^ feeds the two-level Gram Cholesky (gram_parts = 1, no split-K copies to zero); `tiles` needs "
        "ldb <= 184, i.e. at most 180 reflected columns of 192",
    33: "6 n = 198: GAIN_LARGE; `tiles` needs ldb <= 176; `wide` and `long` (tracks of 31, 32, 33: beyond 32 lanes of k_lit_pre)",
    34: "`tiles` needs ldb <= 172 of 204 columns: a `tall` list that reflects (nearly) every column is past the edge",
    38: "sweep_gram_blocked: need(16) = 16 lde + 32 n1 + 672 (literal_core.h:1371), lde = (e - 15 + 4) | 1 = 6 n + 5 for m >= D: 288 n + 784 = 11 728 <= lds: last window of PB = 16",
    39: "288 n + 784 = 12 016 > lds: the sweep's panel width drops to PB = 8 (register core and rank-PB trailing passes)",
    41: "compact_rows: 33 n1 + 15 ldt <= lds, ldt = (n1 + 7) & ~3 (literal_core.h:1745): 8 151 + 3 780 = 11 931: last window of the staged-tile Gram start",
    42: "33 n1 + 15 ldt = 8 349 + 3 900 = 12 249 > lds: the stand-in of the staged-tile Gram start; 6 n + 1 = 253: last of ldR = 256",
    43: "6 n + 1 = 259: ldR = 320 (CH_GRAM_B<8>)",
    53: "6 n + 1 = 319: last of ldR = 320", 54: "6 n + 1 = 325: ldR = 384 (CH_GRAM_B<12>)",
    60: "33 n1 = 11 913 <= lds (literal_core.h:1674): last window whose staged 15 rows sE live in LDS",
    61: "33 n1 = 12 111 > lds: sE moves to global Stg; elimination panel 16 ((nz + 4) | 1) + 32 <= lds, nz = nr + 6 n + 1 "
        "(literal_core.h:556-557): PB = 16 needs nz <= 743; `tall` keeps 368 rows here, nz = 735: last window of PB = 16 (computed per case)",
    62: "one below N_CAP_MAX; `tall` keeps 374 rows, nz = 747 > 743: the elimination's panel width drops to PB = 8", 63: "N_CAP_MAX; `long` (tracks of 31 .. 63 observations, m_cap 63)",
}
SIZES = tuple(sorted(E))
K_INV_SIZES = (10, 32, 39, 63)
GAP_TABLE_SIZES = (10, 30, 39)
WIDE_SIZES, WIDE_COUNTS = (16, 33), (255, 256, 257)
SCAN_COUNTS = (64, 65, 128, 129)      # at 16 cameras only: k_lit_pre's offsets scan, per = (F + 63) / 64 = 1 | 2, 2 | 3


def wide_counts(n):
    return (SCAN_COUNTS if n == WIDE_SIZES[0] else ()) + WIDE_COUNTS
LONG_LENGTHS = {33: (31, 32, 33), 63: (31, 32, 33, 47, 48, 62, 63)}
LONG_TALL = 12
BRIM_N = 5
# `brim`: stacked rows m = sum(2 M - 3) on either side of D = 15 + 6 n = 45 (every term is odd: the parity of m is the parity of the
# track count, all three values are reachable): track lengths per list
BRIM = {44: (5, 5, 5, 5, 5, 3, 3, 3), 45: (5, 5, 5, 5, 5, 5, 3), 46: (5, 5, 5, 5, 5, 4, 3, 3)}
GAP_MIN_N = 6
# `gap6`: `tall` at 34 cameras without its observations in six slots: 36 kept handed-through rows and about 161 reflected columns: the
# basis has 15 + 204 - 7 = 212 rows -- more than the 208 ints that 104 doubles hold -- AND the tiles' copy fits (33 n1 + lsb + 30 ldb =
# 6 765 + 108 + 30 x 168 <= lds): the one combination in which compact_basis' list sB and the copy sEg overlapped (found by this suite's first
# `long` list on the host build: sB's tail read back as garbage, a row index out of bounds; literal_core.h:1938-1942)
GAP6_N, GAP6_SLOTS = 34, (4, 9, 14, 19, 24, 29)


def gap_slot(n, where, slots):
    """`gapped`: the camera slot whose observations are taken out of the `tall` list (slots: that list's): the first one after slot
    0 that a track observes (near the front), or the last one before the two newest (deep in the sweep: 6 x slot steps in).  At the
    larger windows the 24 tracks of `tall` leave other slots unobserved as well: more handed-through rows, not fewer."""
    seen = sorted(set(int(s) for s in slots) - {0})
    return seen[0] if where == "front" else max(s for s in seen if s <= n - 3)


def families(n):
    """the lists of the n-camera window (every one runs on the CPU; the GPU grid takes its pick)"""
    f = ["tall", "thin"]
    if n >= GAP_MIN_N:
        f += ["gap_front", "gap_deep"]
    if n in WIDE_SIZES:
        f += ["wide%d" % c for c in wide_counts(n)]
    if n in LONG_LENGTHS:
        f.append("long")
    if n == BRIM_N:
        f += ["brim%d" % m for m in sorted(BRIM)]
    if n == GAP6_N:
        f.append("gap6")
    return f


def ks_of(n):
    return (K_MAIN, K_INV) if n in K_INV_SIZES else (K_MAIN,)


def cases():
    return [(n, fam, K) for n in SIZES for fam in families(n) for K in ks_of(n)]


def needs_rows(fam):
    """the families that mutants and the GLS stand-in are held on (`thin` compresses nothing: literal = GLS there)"""
    return fam == "tall" or fam.startswith("gap") or fam == "long"


# sub-seed per (n, family) where update_lab's own (SUB_SEEDS there; default 0) does not hold the conditions of
# tests/test_literal_inputs.py; found by trying 0, 1, 2, ... on the CPU oracles
# (sub-seed 0 of these three: the float oracle keeps 239 of 242 and 261 of 262 rows at 39 and 43 cameras, and is 2.7e-4 / 4.9e-4 from
# the double one at 62: lists on the threshold of the zero-tail rule in float, no measure of a float bar)
SUB_SEEDS = {(39, "gap_deep"): 1, (43, "gap_deep"): 4, (62, "gap_deep"): 1}

_CACHE = {}


# ------------------------------------------------------------------------------------------------------------ windows
def config(po, K=K_MAIN, sig2=None):
    """the window's config with v' = K u' (K None: as it is, isotropic; sig2: u' = v' = sig2)"""
    cfg = dict(FL.window(po).tr.cfg)
    assert cfg["u_var_prime"] == cfg["v_var_prime"]
    if sig2 is not None:
        cfg["u_var_prime"] = cfg["v_var_prime"] = float(sig2)
    elif K is not None:
        cfg["v_var_prime"] = K * cfg["u_var_prime"]
    return cfg


def window(po, n, K=K_MAIN, dtype=None, mode=None, whiten=False, tol=None, sig2=None):
    """a fresh oracle of the n-camera window, initialised with config(K) and teacher-forced as update_lab.window's float branch"""
    dtype = po.F64 if dtype is None else dtype
    src = UL.window(po, n)
    cams, ids = src.getCamStates()
    tr = FL.window(po).tr
    f = po.Oracle(dtype, po.LEAN if mode is None else mode)
    if whiten:
        f.setWhiten(True)
    if tol is not None:
        f.setTinyRowTol(tol)
    f.initialize(config(po, K, sig2), tr.imu0)
    for i in range(n):
        f.augmentState(int(ids[i]), 0.0)
    f.setImuState(src.getImuState())
    for i, c in enumerate(cams):
        f.setCamPose(i, c)
    f.setCovariance(src.getCovariance())
    f.setNumResidualized(src.numResidualized())
    return f


# ------------------------------------------------------------------------------------------------------------ tracks
def _project(po, n, lm, noise, slot_lists, noise_px=NOISE_PX):
    """(M, slots, obs) of landmarks lm[i] seen from the slots slot_lists[i] of the n-camera window (slots count from its oldest camera)"""
    win = FL.window(po)
    first = N_WIN - n
    M, slots, obs = [], [], []
    for i, s in enumerate(slot_lists):
        s = np.asarray(s, dtype=np.int32)
        g = s + first
        q = np.einsum("sij,sj->si", win.C[g], lm[i][None, :] - win.p[g])
        M.append(len(s))
        slots.append(s)
        obs.append(q[:, :2] / q[:, 2:3] + (noise_px / win.tr.cfg["f_u"]) * noise[i][g])
    return np.array(M, dtype=np.int32), np.concatenate(slots).astype(np.int32), np.concatenate(obs)


def _hand_made(po, n, fam, slot_lists, sub):
    rng = sc.SplitMix64(0x117E0000 + 7919 * n + 104729 * (sum(ord(c) for c in fam) % 997) + 15485863 * int(sub))
    lm = FL._landmarks(FL.window(po), rng, len(slot_lists))
    noise = rng.normal(len(slot_lists) * N_WIN * 2).reshape(len(slot_lists), N_WIN, 2)
    return _project(po, n, lm, noise, slot_lists)


def without_slot(tracks, slot):
    """the list without its observations in one camera slot (tracks left with fewer than three leave the list)"""
    M, slots, obs = tracks
    Mo, so, oo = [], [], []
    o = 0
    for m in M:
        keep = [o + i for i in range(int(m)) if slots[o + i] != slot]
        o += int(m)
        if len(keep) >= 3:
            Mo.append(len(keep))
            so.extend(int(slots[i]) for i in keep)
            oo.extend(obs[i] for i in keep)
    return np.array(Mo, dtype=np.int32), np.array(so, dtype=np.int32), np.array(oo).reshape(-1, 2)


def wide_slots(n, count):
    """three observations per track: one track in three spread over the whole window (first slot in the oldest quarter, last in the
    newest), one over its older half, one over its newer half, the middle observation anywhere between -- slot ranges inside one
    32-column tile of k_lit_gamma, across one edge and across all of them; slots 0 and n - 1 are both used"""
    a = max(1, n // 4)
    out = []
    for i in range(count):
        u, v = i % a, (i // a) % a
        s0, s2 = ((u, n - 1 - v), (u, n // 2 + v), (n // 2 - 1 - u, n - 1 - v))[i % 3]
        out.append((s0, s0 + 1 + (5 * i) % (s2 - s0 - 1), s2))
    return out


def long_slots(n):
    """tracks of LONG_LENGTHS[n] observations spread over the window; four tracks whose slot range is exactly 10 and exactly 11
    cameras (k_lit_pre: 60 | 66 columns, one | two rounds of 64 lanes), each once contiguous and once with unobserved slots inside"""
    out = [UL.slots_of(n, L) for L in LONG_LENGTHS[n]]
    a = n // 3
    out += [np.arange(a, a + 10), np.arange(a + 2, a + 13), np.array([a, a + 2, a + 5, a + 7, a + 9]) + 1, np.array([a, a + 3, a + 4, a + 8, a + 10]) + 4]
    assert [int(s[-1] - s[0] + 1) for s in out[-4:]] == [10, 11, 10, 11]
    return out


def make_tracks(po, n, fam, sub=None):
    if sub is None:
        base = "tall" if fam.startswith("gap") else fam
        sub = SUB_SEEDS.get((n, fam), UL.SUB_SEEDS.get((n, base), 0))
    if fam in ("tall", "thin"):
        return UL.make_tracks(po, n, fam, sub=sub)
    if fam == "gap6":
        t = UL.make_tracks(po, n, "tall", sub=sub)
        for g in GAP6_SLOTS:
            t = without_slot(t, g)
        return t
    if fam.startswith("gap_"):
        t = UL.make_tracks(po, n, "tall", sub=sub)
        return without_slot(t, gap_slot(n, fam[4:], t[1]))
    if fam.startswith("wide"):
        return _hand_made(po, n, fam, wide_slots(n, int(fam[4:])), sub)
    if fam == "long":
        # with LONG_TALL tracks of `tall`: the handful of long tracks alone leave the 33-camera stack (233 rows on 198 columns, a quarter
        # of them unobserved) so close to the zero-tail rule's threshold that the double oracle, the float oracle and the two host
        # routes keep 205, 204, 205 and 211 rows and differ by 1e-3: no reference (measured)
        a, b = _hand_made(po, n, fam, long_slots(n), sub), UL.make_tracks(po, n, "tall", sub=UL.SUB_SEEDS.get((n, "tall"), 0))
        k = int(np.sum(b[0][:LONG_TALL]))
        return np.concatenate([a[0], b[0][:LONG_TALL]]), np.concatenate([a[1], b[1][:k]]), np.concatenate([a[2], b[2][:k]])
    if fam.startswith("brim"):
        return _hand_made(po, n, fam, [UL.slots_of(n, L) for L in BRIM[int(fam[4:])]], sub)
    raise ValueError(fam)


def tracks_of(po, n, fam):
    if fam == "empty":
        return UL.EMPTY
    if fam == "rejected":
        return UL.rejected_tracks(po, n)
    key = ("t", n, fam)
    if key not in _CACHE:
        _CACHE[key] = make_tracks(po, n, fam)
    return _CACHE[key]


def caps(fam):
    """(f_cap, m_cap floor) a handle needs for the family"""
    return (F_CAP_WIDE if fam.startswith("wide") else F_CAP), (M_CAP_LONG if fam == "long" else 0)


# ------------------------------------------------------------------------------------------------------------ references
def _run(o, tracks, capture=False):
    r = UL.Result()
    if capture:
        o.setCapture(True)
    r.P0 = o.getCovariance()
    if len(tracks[0]):
        o.setTracks(*tracks)
        o.marginalize()
    r.P1, r.dx, r.stats, r.rows = o.getCovariance(), o.lastDeltaX(), o.lastStats(), o.lastTracks()
    r.imu, r.cams = o.getImuState(), o.getCamStates()[0]
    return (r, o) if capture else r


def run_oracle(po, n, tracks, K=K_MAIN, dtype=None, mode=None, whiten=False, tol=None, sig2=None):
    return _run(window(po, n, K, dtype, mode, whiten, tol, sig2), tracks)


def reference(po, n, fam, K=K_MAIN):
    """THE reference: the double LEAN oracle with the device's double tolerance"""
    key = ("ref", n, fam, K)
    if key not in _CACHE:
        _CACHE[key], _CACHE[("cap",) + key[1:]] = _run(window(po, n, K, po.F64, po.LEAN, tol=TOL64), tracks_of(po, n, fam), capture=True)
    return _CACHE[key]


def captured(po, n, fam, K=K_MAIN):
    """the reference's oracle after its update, with the compression's inputs and results captured (for the host build)"""
    reference(po, n, fam, K)
    return _CACHE[("cap", n, fam, K)]


def float_oracle(po, n, fam, K=K_MAIN):
    key = ("f32", n, fam, K)
    if key not in _CACHE:
        _CACHE[key] = run_oracle(po, n, tracks_of(po, n, fam), K, po.F32, po.LEAN, tol=TOL32)
    return _CACHE[key]


def whitened(po, n, fam, K=K_MAIN, dtype=None):
    """the pre-whitened (GLS) update: the reference of aniso_mode 1, and stand-in (a) of the mutants"""
    key = ("gls", n, fam, K, dtype)
    if key not in _CACHE:
        _CACHE[key] = run_oracle(po, n, tracks_of(po, n, fam), K, po.F64 if dtype is None else dtype, po.GRAM, whiten=True)
    return _CACHE[key]


def isotropic(po, n, fam, K, which):
    """the isotropic oracle with sigma^2 = u' (stand-in b) or v' (stand-in c)"""
    u = config(po, None)["u_var_prime"]
    return run_oracle(po, n, tracks_of(po, n, fam), None, po.F64, po.LEAN, sig2=u if which == "u" else K * u)


def iso_reference(po, n, fam):
    """the isotropic trajectory every GPU handle carries: the same window with u' = v'"""
    key = ("iso", n, fam)
    if key not in _CACHE:
        _CACHE[key] = run_oracle(po, n, tracks_of(po, n, fam), None, po.F64, po.LEAN)
    return _CACHE[key]


distances = UL.distances


def case_violations(po, n, fam, K, M):
    """what the lab promises about one case: [] when all of it holds"""
    ref, f32 = reference(po, n, fam, K), float_oracle(po, n, fam, K)
    bad = []
    if not ref.stats["n_passed"] > 0:
        bad.append(("n_passed", ref.stats))
    if not np.array_equal(f32.rows[:, :3] > 0, ref.rows[:, :3] > 0):
        bad.append(("flags",))
    for k in H.STAT_KEYS + ("r_rows",):
        if f32.stats[k] != ref.stats[k]:
            bad.append((k, f32.stats[k], ref.stats[k]))
    for i in np.nonzero((ref.rows[:, 0] > 0) & (ref.rows[:, 1] > 0))[0]:
        thr = FL.chi2_threshold(int(M[i]))
        if abs(ref.rows[i, 4] - thr) < UL.GATE_MARGIN * thr:
            bad.append(("gate_margin", int(i), ref.rows[i, 4], thr))
    if len(f32.dx) == len(ref.dx) and max(distances(f32, ref)) > FLOAT_ILL:
        bad.append(("ill_conditioned", distances(f32, ref)))
    return bad


# ------------------------------------------------------------------------------------------------------------ bars
# Float bars: FLOAT_FACTOR x the largest distance of the float LEAN oracle (tolerance 8e-4) from the
# double one over cases(), ONE constant per metric; measured on the CPU (tests/test_literal_inputs.py asserts that they
# reproduce to 2 %), never on the device.  FLOAT_ILL as update_lab's: a case on which the float oracle itself is farther than this
# cannot serve to measure a bar and is re-seeded (none may remain); within a factor of three of the worst accepted case.
FLOAT_FACTOR = UL.FLOAT_FACTOR
D32_COV, D32_DX = 3.21e-5, 2.92e-5     # measured 3.205e-05 (53 cameras, `gap_deep`, K = 4) and 2.917e-05 (39 cameras, `tall`, K = 1/4), rounded up
D32_MEASURED = (3.205e-5, 2.917e-5)
FLOAT_ILL = 9.6e-5
BAR_F64 = UL.BAR_F64
# aniso_mode 1: the float GRAM oracle with setWhiten(True) against the double one, over WHITENED_SIZES x (tall, thin), K = 4
WHITENED_SIZES = (10, 12, 13, 22, 33, 63)
D32W_COV, D32W_DX = 7.72e-6, 9.82e-6   # measured 7.710e-06 (12 cameras, `tall`) and 9.817e-06 (63 cameras, `tall`), rounded up
D32W_MEASURED = (7.710e-6, 9.817e-6)


def bars(prec, whitened_route=False):
    if prec == "f64":
        return BAR_F64, BAR_F64
    return (FLOAT_FACTOR * D32W_COV, FLOAT_FACTOR * D32W_DX) if whitened_route else (FLOAT_FACTOR * D32_COV, FLOAT_FACTOR * D32_DX)


# ------------------------------------------------------------------------------------------------------------ mutants
STAND_INS = ("gls", "iso_u", "iso_v")
MUTANT_FACTOR = UL.MUTANT_FACTOR
GLS_MIN_N = 10            # the smallest window from which stand-in (a) scores MUTANT_FACTOR bars on every list with rows to compress
# The (case, mutant) pairs that cannot reach MUTANT_FACTOR bars, with their measured scores (asserted to reproduce to 5 %): at 3
# cameras the whole update moves no entry of P by more than 3 % of its scale (update_lab.MUTANT_EXEMPT); `dx_last` zeroes ONE entry
# of the correction, the newest camera's last position component, which on these lists happens to be a fraction of its sigma
MUTANT_EXEMPT = {
    (3, "tall", 4.0, "iso_v"): 8.50e-04,            # 6.6 bars
    (3, "tall", 4.0, "downdate_2pc"): 1.86e-04,     # 1.4 bars
    (10, "tall", 0.25, "dx_last"): 8.12e-04,        # 7.0 bars
    (10, "gap_front", 4.0, "dx_last"): 4.31e-04,    # 3.7 bars
    (32, "gap_deep", 4.0, "dx_last"): 1.74e-04,     # 1.5 bars
    (33, "tall", 4.0, "dx_last"): 1.03e-03,         # 8.8 bars
    (33, "gap_front", 4.0, "dx_last"): 1.06e-03,    # 9.1 bars
    (33, "gap_deep", 4.0, "dx_last"): 2.23e-04,     # 1.9 bars
    (62, "gap_deep", 4.0, "dx_last"): 2.07e-04,     # 1.8 bars
}
# the gap table: with K = 4 the GLS stand-in fails the scaled covariance bar by at least this factor on `tall`
GAP_FACTORS = {10: 29, 30: 230, 39: 180}


def stand_in_score(po, n, fam, K, which):
    """covariance distance of the literal reference from one stand-in ON THE SAME CASE"""
    ref = reference(po, n, fam, K)
    other = whitened(po, n, fam, K) if which == "gls" else isotropic(po, n, fam, K, which[4:])
    if other.P1.shape != ref.P1.shape:
        return float("inf")
    return H.cov_scaled_err(other.P1, ref.P1)


# ------------------------------------------------------------------------------------------------------------ staging
def staging(n, m, reflected=None, basis=None, handed=0, lds=None):
    """Which side of every staging edge of literal_core.h the compact route takes for a window of n cameras and a stack of m rows
    (reflected / basis / handed: literal_info's `reflected`, `spare` = rows of the basis and `kept_handed_through_rows`, from the
    host build or the device): a restatement of the four expressions, each with the line it restates."""
    lds = lds_doubles() if lds is None else lds
    n1, D = 6 * n + 1, 15 + 6 * n
    e = min(m, D)                                                      # literal_core.h:1641
    out = {"gram": m > e, "two_level": n1 > 192}                       # :1643; update_routes.h CH_SPLIT
    lde = (e - 15 + 4) | 1                                             # :1370
    need = lambda pb: lde * pb + 2 * pb * n1 + 2 * pb * pb + 9 * pb + 16       # :1371
    PB = 16
    while PB > 2 and need(PB) > lds:                                   # :1372
        PB >>= 1
    out["sweep_pb"] = (PB if need(PB) <= lds else 0) if (m > e and e > 15) else None       # :1373, :1803
    out["rows_tiles"] = 33 * n1 + 15 * ((n1 + 7) & ~3) <= lds          # :1744-1745
    out["stage_lds"] = 33 * n1 <= lds                                  # :1674
    if basis is not None:
        # nb = basis - na - nh with na <= 15 kept rows above the first step, nb <= reflected (:1827-1832): both ends, None when they disagree
        lsb = 104 if basis <= 208 else ((basis + 1) // 2 + 3) & ~3      # :1938-1942
        sides = {33 * n1 + lsb + 30 * ((nb + 7) & ~3) <= lds for nb in (max(basis - handed - 15, 0), min(basis - handed, reflected))}      # :1938-1942
        out["basis_tiles"] = sides.pop() if len(sides) == 1 else None
        out["tiles_list"] = (basis <= 208) if out["basis_tiles"] else None       # the list's ints within the 104 doubles | beyond them
        ldr = ((basis + n1) + 4) | 1                                   # :537, :556
        PB = 16
        while PB > 1 and ldr * PB + 2 * PB > lds:                      # :557
            PB >>= 1
        out["elim_pb"] = PB
    return out


# every literal edge: (key of staging(), value on one side, value on the other)
EDGES = (("gram", False, True), ("two_level", False, True), ("sweep_pb", 16, 8), ("rows_tiles", True, False), ("stage_lds", True, False),
         ("basis_tiles", True, False), ("tiles_list", True, False), ("elim_pb", 16, 8))
