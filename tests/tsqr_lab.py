"""Track lists for the Householder TSQR route (k_select's row layout and k_qr_update, csrc/kernels_qr.hip): the inputs and
references of tests/test_tsqr_inputs.py (CPU: proves on the oracles that these inputs can see a fault) and
tests/test_gpu_tsqr_kernels.py.  TEST INFRASTRUCTURE ONLY.

Built on update_lab: the same windows (UL.window), the same entry-scaled metric (helpers.cov_scaled_err, UL.dx_scaled), the same
reference (the double oracle in LEAN mode), the same landmarks and noise as UL.make_tracks.  What update_lab's lists cannot do
for this route is in their shape: every track of `tall` and `thin` starts at slot 0, the passed tracks are all or none, and the
stacks are short.  The lists here, each with the reason for its shape (the list ORDER is shuffled, so that the counting sort of
select_body has work to do):

  staggered   24 tracks whose first slots spread over 0 .. n - 2 (first_bins): several tracks share a first slot (the stable
              order inside a bin), from 7 cameras on empty bins lie between occupied ones (the exclusive prefix over the bins), ONE track of 2
              observations sits at (n - 2, n - 1) (kmin = 6 (n - 2): a block whose elimination starts at the last camera but one),
              one bin is slot 0, and where the window has them, first slots 10 | 11 and 21 | 22: kmin on both sides of column 64
              and of column 128, the second and third 64-column group of a lane (l_lo = max(kmin - 64 jk, 0) skips a whole group).
              The third group needs a first slot of 22 <= n - 2: from 24 cameras on (at 22 and 23 cameras no track can start
              beyond column 6 (n - 2) <= 126).  In this window the motion check rejects the track at (n - 2, n - 1), and every
              other track that starts at n - 2, at EVERY size (neighbouring cameras are closer than translation_threshold): the
              track stays, as a rejected one behind every passed one, and the bins n - 5 .. n - 3 (LATE_BINS) carry the latest
              first slots that do pass -- kmin reaches 6 (n - 3).  tests/test_tsqr_inputs.py asserts both.
  holes       `staggered` with every third track of the list at UL.REJECT_PX of noise: the passed tracks are no prefix of the
              list, order[] and row_start[] are a compaction with holes, the binary search runs over P < F.
  blind       `staggered` laid out over the cameras that remain when the oldest one and a middle one (slot n // 2) are seen by
              no track: their twelve columns of the stack are zero, the reflector of such a column has sigma <= tiny and is
              skipped, and R keeps zero rows that the Kalman stage must cope with.  Exists from 4 cameras on (at 3 one camera
              would remain).
  dense       a stack of a given length: long tracks whose first slots cycle through the oldest cameras, then one or two short
              tracks that bring m_rows to a given residue modulo the kernel's block of RW rows (a track has 2 M - 3 rows: an odd
              number, so an even remainder takes two).  deep_rows: all twelve wavefronts of the pipeline load a second block in
              stage 1; ring_rows: more blocks in every chunk than the ring of progress words has slots.
  many        1 030 tracks of 2 to 4 observations: more than routes::INFO_F_CAP = 1024 tracks, what forces a handle onto this
              route by geometry; select_body's generic path, a binary search over more than 1 000 passed tracks."""
import numpy as np

import feature_lab as FL
import update_lab as UL
from msckf_mono_amd import scenario as sc

FAMILIES = ("staggered", "holes", "blind")
N_TRACKS = 24
BLIND_MIN = 4
EDGE_FIRSTS = (10, 11, 21, 22)        # kmin = 60 | 66 and 126 | 132: both sides of columns 64 and 128
LENGTH_FRACTIONS = (1.0, 0.35, 0.7, 0.15, 0.5, 0.85)
LATE_BINS = (1, 2, 3)                 # first slots n - 3, n - 4, n - 5: the latest that pass the motion check in this window
N_MANY = 1030
SIZES = tuple(sorted(set(UL.SIZES) | {45, 46}))      # 45 | 46: the float work triangle leaves LDS (149 472 | 156 108 bytes)
QR_PIPELINE, QR_RING = 12, 512        # routes::QR_PIPELINE, routes::QR_RING (csrc/update_routes.h)


def rw_of(prec, n_cap):
    """rows per block of k_qr_update: 32 in float up to 31 cameras (three 64-column panels), else 16"""
    return 32 if prec == "f32" and n_cap <= 31 else 16


# sub-seed per (n, family) (default 0), found as UL.SUB_SEEDS were: by trying 0, 1, 2, ... on the CPU oracles until
# UL.case_violations, UL.mutant_violations and input_mutant_violations are empty; tests/test_tsqr_inputs.py asserts it with no
# case excluded.  Most re-seeds are for one mutant (`dx_last`, `lost_last_bin`: the last entry of the correction, or the last bin's
# few rows, happen to move little); those at 16 (`blind`), 24, 53 (`holes`) and 56 cameras are lists on which the float GRAM ORACLE is
# 0.26 .. 175 from the double oracle (a covariance block keeps its prior: its float Cholesky drops real pivots, as on
# UL.HARD_THIN) with the float LEAN oracle within 2e-5 on the same lists -- the oracle's restatement, not a device.
SUB_SEEDS = {(4, "blind"): 1, (10, "staggered"): 1, (16, "blind"): 1, (22, "blind"): 1, (24, "holes"): 1, (24, "blind"): 1, (26, "staggered"): 1,
             (27, "staggered"): 1, (48, "blind"): 1, (53, "holes"): 1, (56, "staggered"): 3, (56, "holes"): 3, (56, "blind"): 1, (62, "blind"): 1}

ROUND_N, ROUND_SIZES = 22, (64, 65, 256, 257)
ROUND_SEEDS = {}
DENSE_SEEDS = {"dense:16:8193:15": 3}          # per list name: re-seeded until every result mutant scores 10 bars of the list's group

_CACHE = {}


# ------------------------------------------------------------------------------------------------------------ shapes
def first_bins(nv):
    """first slots of `staggered` over nv cameras, ascending: 0, every second slot or sparser, the edge slots, nv - 2"""
    hi = nv - 2
    step = max(2, -(-hi // 6))
    return sorted(set(range(0, hi + 1, step)) | {hi} | {e for e in EDGE_FIRSTS if e <= hi} | {hi - k for k in LATE_BINS if hi - k > 0})


def staggered_shape(nv):
    """[(first slot, length)] of the 24 tracks over nv cameras, before the shuffle: ONE track in the last bin (2 observations),
    the others dealt round-robin to the bins before it, the first track of a bin the longest (up to UL.L_MAX)"""
    bins = first_bins(nv)
    head = bins[:-1] if len(bins) > 1 else bins
    out = [(bins[-1], 2)]
    for i in range(N_TRACKS - 1):
        f = head[i % len(head)]
        top = min(nv - f, UL.L_MAX)
        lo = min(3, top)
        out.append((f, int(round(lo + LENGTH_FRACTIONS[(i // len(head)) % len(LENGTH_FRACTIONS)] * (top - lo)))))
    return out


def visible(n, family):
    return [s for s in range(n) if family != "blind" or s not in (0, n // 2)]


def slots_of(vis, first, L):
    """L distinct cameras of vis from index `first` to the newest one"""
    idx = first + np.round(np.linspace(0, len(vis) - 1 - first, L)).astype(np.int64)
    return np.asarray(vis, dtype=np.int32)[idx]


def dense_shape(n, rw, min_rows, residue):
    """[(first, length)]: long tracks (first slots 0, 1, 0, 2, 0, 3, ... over the oldest quarter of the window) until the stack
    has min_rows rows, then one or two short tracks so that the row count is = residue (mod rw).  The short ones start at a
    third of the window, behind every long one in the sorted stack, and end at the newest camera (a track of a few neighbouring
    cameras does not pass the motion check in this window)"""
    out, rows, i = [], 0, 0
    late = max(n // 4, 1)
    while rows < min_rows:
        f = 0 if i % 2 == 0 else 1 + (i // 2) % late
        L = min(n - f, UL.L_MAX)
        out.append((f, L))
        rows += 2 * L - 3
        i += 1
    delta = (residue - rows) % rw
    parts = [] if delta == 0 else [delta] if delta % 2 else [1, delta - 1]
    for r in parts:
        M = (r + 3) // 2
        out.append((min(n // 3, n - M), M))
    return out


def many_shape(n, F=N_MANY):
    """F (1 030) tracks of 2, 3 or 4 observations whose first slots cycle over the older half of the window (a baseline of half a
    window: the motion check passes them)"""
    half = max(n // 2, 1)
    return [((7 * i) % half, 2 + i % 3) for i in range(F)]


# ------------------------------------------------------------------------------------------------------------ tracks
def build(po, n, shape, vis, seed, every_third_px=None, third=1):
    """(M, slots, obs) of the tracks of `shape` in the n-camera window: landmarks and noise as UL.make_tracks"""
    win = FL.window(po)
    rng = sc.SplitMix64(seed)
    lm = FL._landmarks(win, rng, len(shape))
    noise = rng.normal(len(shape) * UL.N_WIN * 2).reshape(len(shape), UL.N_WIN, 2)
    order = np.argsort(rng.u64(len(shape)), kind="stable")
    off = UL.N_WIN - n
    M, slots, obs = [], [], []
    for pos, i in enumerate(order):
        f, L = shape[i]
        s = slots_of(vis, f, L)
        g = s + off
        q = np.einsum("sij,sj->si", win.C[g], lm[i][None, :] - win.p[g])
        px = every_third_px if (every_third_px is not None and pos % 3 == third) else UL.NOISE_PX
        M.append(L)
        slots.append(s)
        obs.append(q[:, :2] / q[:, 2:3] + (px / win.tr.cfg["f_u"]) * noise[i][g])
    return np.array(M, dtype=np.int32), np.concatenate(slots).astype(np.int32), np.concatenate(obs)


def make_tracks(po, n, family, sub=None):
    assert family in FAMILIES and (family != "blind" or n >= BLIND_MIN)
    sub = SUB_SEEDS.get((n, family), 0) if sub is None else sub
    vis = visible(n, family)
    # `holes` IS `staggered` of the same sub-seed but for the noise of every third track
    seed = 0x75A70000 + 7919 * n + 104729 * (1 if family == "blind" else 0) + 15485863 * int(sub)
    return build(po, n, staggered_shape(len(vis)), vis, seed, UL.REJECT_PX if family == "holes" else None)


def families_at(n):
    return tuple(f for f in FAMILIES if f != "blind" or n >= BLIND_MIN)


def tracks_of(po, n, family):
    """the list `family` of the n-camera window (cached).  Besides FAMILIES: "dense:RW:ROWS:RESIDUE", "many", and update_lab's
    own lists ("thin", "tall")"""
    key = ("t", n, family)
    if key not in _CACHE:
        name, _, arg = family.partition(":")
        if name == "dense":
            rw, rows, res = (int(x) for x in arg.split(":"))
            _CACHE[key] = build(po, n, dense_shape(n, rw, rows, res), list(range(n)), 0xDE75E000 + 7919 * n + 31 * rows + res + 15485863 * DENSE_SEEDS.get(family, 0))
        elif name == "many":
            _CACHE[key] = build(po, n, many_shape(n), list(range(n)), 0x3A790000 + 7919 * n)
        elif name == "round":       # "round:F[:sub]": F tracks shaped as `many`, every third at UL.REJECT_PX as in `holes` (positions
            # 2, 5, ..: the tracks at 63 | 64 and 255 | 256, which close and open a 64-track round, are ordinary ones)
            F, _, sub = arg.partition(":")
            sub = int(sub) if sub else ROUND_SEEDS.get((n, int(F)), 0)
            _CACHE[key] = build(po, n, many_shape(n, int(F)), list(range(n)), 0x20D50000 + 7919 * n + 31 * int(F) + 15485863 * sub, UL.REJECT_PX, third=2)
        elif name in FAMILIES:
            _CACHE[key] = make_tracks(po, n, name, sub=int(arg) if arg else None)
        else:
            _CACHE[key] = UL.tracks_of(po, n, family)
    return _CACHE[key]


def reference(po, n, family):
    key = ("ref", n, family)
    if key not in _CACHE:
        _CACHE[key] = UL.run_oracle(po, n, tracks_of(po, n, family))
    return _CACHE[key]


def others(po, n, family, double_gram=True):
    key = ("oth", n, family)
    if key not in _CACHE:
        t = tracks_of(po, n, family)
        o = {"f32_lean": UL.run_oracle(po, n, t, po.F32, po.LEAN), "f32_gram": UL.run_oracle(po, n, t, po.F32, po.GRAM)}
        if double_gram:
            o["f64_gram"] = UL.run_oracle(po, n, t, po.F64, po.GRAM)
        _CACHE[key] = o
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ the dense cases
def deep_rows(rw):
    """a stage-1 stack in ONE chunk of which every wavefront of the pipeline loads a second block: 2 x 12 blocks"""
    return 2 * QR_PIPELINE * rw


def ring_rows(rw, nchunk=1):
    """more blocks in EVERY chunk than the ring has slots (block g goes to chunk g % nchunk)"""
    return (QR_RING * nchunk + nchunk - 1) * rw + 1


def residues(rw):
    return (0, 1, rw - 1)


def dense_name(rw, min_rows, residue):
    return "dense:%d:%d:%d" % (rw, min_rows, residue)


# ------------------------------------------------------------------------------------------------------------ input mutants
INPUT_MUTANTS = ("lost_partial_block", "lost_last_bin")
INPUT_MUTANT_MIN = 4


def sorted_passed(tracks, ref):
    """indices of the passed tracks in select_body's order (stable counting sort by first slot) and their row counts"""
    M, slots, _ = tracks
    off = np.concatenate([[0], np.cumsum(M)])
    first = np.array([slots[off[i]] for i in range(len(M))])
    ok = np.nonzero((ref.rows[:, 0] > 0) & (ref.rows[:, 1] > 0) & (ref.rows[:, 2] > 0))[0]
    order = ok[np.argsort(first[ok], kind="stable")]
    return order, 2 * M[order] - 3, first[order]


def without(tracks, drop):
    M, slots, obs = tracks
    off = np.concatenate([[0], np.cumsum(M)])
    keep = [i for i in range(len(M)) if i not in set(int(x) for x in drop)]
    return (M[keep], np.concatenate([slots[off[i]:off[i + 1]] for i in keep]).astype(np.int32), np.concatenate([obs[off[i]:off[i + 1]] for i in keep]))


def input_mutant(tracks, ref, which, rw):
    """the list without the tracks a faulty row layout would lose -- run through the double oracle, never given to code under
    test: `lost_partial_block` the tracks that own the last rw stacked rows in sorted order, `lost_last_bin` the tracks of the
    last occupied bin"""
    order, rows, first = sorted_passed(tracks, ref)
    end = np.cumsum(rows)
    if which == "lost_partial_block":
        drop = order[end > end[-1] - rw]
    elif which == "lost_last_bin":
        drop = order[first == first[-1]]
    else:
        raise ValueError(which)
    return without(tracks, drop)


def input_mutant_scores(po, n, family, which, rw=16):
    """(covariance, correction) distance of the mutant list's update from the reference's"""
    t, ref = tracks_of(po, n, family), reference(po, n, family)
    r = UL.run_oracle(po, n, input_mutant(t, ref, which, rw))
    if len(r.dx) != len(ref.dx):
        return float("inf"), float("inf")
    return UL.distances(r, ref)


def input_mutant_violations(po, n, family):
    bc, bd = bars("f32")
    out = []
    for which in INPUT_MUTANTS:
        dc, dd = input_mutant_scores(po, n, family, which)
        if not max(dc / bc, dd / bd) >= UL.MUTANT_FACTOR:       # seen on either metric: a case asserts both
            out.append((which, dc, dd))
    return out


# ------------------------------------------------------------------------------------------------------------ the bars
# Float: as update_lab's, FLOAT_FACTOR x the largest distance of the float oracle (LEAN and GRAM mode) from the double oracle, ONE
# constant per metric and GROUP of lists -- the float oracles' own distance grows with the length of the stack (a sum over
# 16 449 rows instead of 800), so the long stacks get a bar of their own and do not loosen the bar of the short ones:
#   "edge"   staggered / holes / blind at every size of SIZES, the `round` lists, the DEEP dense lists (up to 801 rows)
#   "many"   the 1 030-track lists (3 088 rows) at 10 and 31 cameras
#   "ring"   the float RING dense lists (16 447 .. 16 449 rows at 30 cameras)
# update_lab's own lists ride in every case (`thin` trajectories pad the handles), so no group's constant is below UL.D32_*.
# Measured on the CPU oracles only (tests/test_tsqr_inputs.py asserts that the maxima reproduce), never on the device.  The double
# bar is UL.BAR_F64 for every group.
D32_TSQR_MEASURED = {"edge": (3.227e-5, 1.914e-5), "many": (8.126e-5, 2.568e-5), "ring": (3.531e-4, 1.100e-4)}
D32_TSQR = {"edge": (UL.D32_COV, 1.92e-5), "many": (8.13e-5, 2.57e-5), "ring": (3.54e-4, 1.10e-4)}


def group_of(family):
    name, _, arg = family.partition(":")
    if name == "many":
        return "many"
    if name == "dense" and int(arg.split(":")[1]) > 4096:
        return "ring"
    return "edge"


def bars(prec, group="edge"):
    if prec == "f64":
        return UL.BAR_F64, UL.BAR_F64
    return tuple(UL.FLOAT_FACTOR * max(a, b) for a, b in zip(D32_TSQR[group], (UL.D32_COV, UL.D32_DX)))


def mutant_violations(ref, n, group="edge"):
    """UL.mutant_violations against this suite's float bars"""
    bc, bd = bars("f32", group)
    out = []
    for m in UL.MUTANTS:
        if (n, m) in UL.MUTANT_EXEMPT:
            continue
        s = UL.mutant_score(ref, m)
        if not s >= UL.MUTANT_FACTOR * (bc if m in UL.COV_MUTANTS else bd):
            out.append((m, s))
    return out
