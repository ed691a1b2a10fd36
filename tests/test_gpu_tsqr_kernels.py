"""The Householder TSQR route -- k_select's row layout and k_qr_update (csrc/kernels_qr.hip) -- against the DOUBLE oracle on the
entry-scaled metric of tests/update_lab.py, at every instantiation the route has and at the edges of its stack: what the `tsqr`
variant of tests/test_gpu_update_kernels.py cannot reach with lists whose tracks all start at slot 0, pass all or none, and
stack at most 720 rows (tests/tsqr_lab.py: the lists and why they are shaped as they are; tests/test_tsqr_inputs.py: the proof on
the CPU that they can see a fault).

The pattern is test_gpu_update_kernels.run_case's: ONE handle and ONE marginalize_range per case, every trajectory augmented to
its own window size and teacher-forced with the oracle's window.  Each case first asserts through the pure functions of
csrc/update_routes.h (tests/cpp/update_routes_host.cpp --handle) that it reaches the launches it was written for, the Q line
(k_qr_update's instantiation, chunk count, merge) included: meant_q below is written down from the suite's specification, not
computed from the header.  Per trajectory: last_stats' counts and every track's flags equal the double oracle's, covariance and
correction within the bars of the list's group (tsqr_lab.bars), no sticky flag, P bit-symmetric; row-less trajectories keep state
and covariance to the bit.  r_rows is not compared: this route reports 6 n whenever it has rows, the oracle min(m_rows, D).

  (a) every (dtype, NC, triangle in LDS | global) instantiation and both sides of every edge between them
  (b) nchunk 8 | 4 | 4 | 2 | 2 | 1 at B = 32 | 33 | 64 | 65 | 128 | 129; no merge launch at 129
  (c) one chunk: a stage-1 stack in which every wavefront of the 12-deep pipeline loads a second block, and one longer than the
      ring of 512 progress words; eight chunks of more than 512 blocks each
  (d) the route taken by geometry (f_cap > 1024, no set_compression): select_body's generic path, 1 030 passed tracks
  (e) select_body's 64-track rounds and its fast | generic switch, on both compression routes
  (f) a range that does not start at trajectory 0

Measured on an MI355X: DESIGN.md section 3.4c has the device's worst distance per case group beside the float oracles'."""
import subprocess

import numpy as np
import pytest

import helpers as H
import test_gpu_update_kernels as G
import tsqr_lab as TL
import update_lab as UL

pytestmark = pytest.mark.gpu

N_CAPS = (10, 11, 21, 22, 31, 32, 33, 42, 43, 45, 46, 53, 54, 63)
F_CAP = G.F_CAP
ROWLESS = ("empty", "rejected")

capi = G.capi
po = G.po
routes_exe = G.routes_exe


# ------------------------------------------------------------------------------------------------ the routes that were meant
def meant_q(prec, n_cap, B):
    """the Q line of --handle, from the instantiation table of the suite's specification"""
    f32 = prec == "f32"
    nc = G._level(n_cap, (10, 21, 31, 42, 53), (1, 2, 3, 4, 5, 6))
    rw = 32 if f32 and n_cap <= 31 else 16
    lds = n_cap <= (45 if f32 else 32)
    tri = (4 if f32 else 8) * (6 * n_cap + 1) * (6 * n_cap + 2) // 2
    nchunk = 8 if B <= 32 else 4 if B <= 64 else 2 if B <= 128 else 1
    return "tsqr NC=%d RW=%d tri=%s lds=%d nchunk=%d merge=%d" % (nc, rw, "lds" if lds else "global", 2048 + tri if lds else 2048, nchunk, 1 if nchunk > 1 else 0)


def assert_tsqr_routes(exe, prec, B, n_cap, m_cap, windows, f_cap, override):
    args = ["f" if prec == "f32" else "d", B, len(windows), n_cap, f_cap, m_cap, 0, 2, 0, 84, override] + list(windows)
    out = subprocess.run([exe, "--handle"] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines())
    want = G.meant("tsqr", prec, n_cap, len(windows))
    want.update(F="k_feature<0> lm=", C="compress=0 select tsqr")         # (no pair kernel on this route, nor beyond PAIR_F_CAP)
    if prec == "f32" and 22 <= n_cap <= 32 and B >= 96:                    # (G.meant is written for batches below GAIN_TWO_PARTS_B)
        want["K"] = "fused=1 blocked<12,7,2>"
    for key, text in want.items():
        assert text in got[key[0]], (prec, n_cap, key, text, got[key[0]])
    assert got["Q"] == meant_q(prec, n_cap, B), (prec, n_cap, B, got["Q"])
    assert "k_feature<1>" not in got["F"] and "none" not in out.stdout and "?" not in out.stdout, out.stdout
    return got


# ------------------------------------------------------------------------------------------------ one handle, one launch sequence
def tracks_for(po, n, fam):
    return UL.EMPTY if fam == "empty" else UL.rejected_tracks(po, n) if fam == "rejected" else TL.tracks_of(po, n, fam)


def reference(po, n, fam):
    return UL.reference(po, n, fam) if fam in UL.FAMILIES else TL.reference(po, n, fam)


def specs_of(n_cap):
    """(a): every size of UL.SIZES up to n_cap, and n_cap itself, with the three lists; the row-less trajectories at the largest"""
    sizes = sorted(set(n for n in UL.SIZES if n <= n_cap) | {n_cap})
    return [(n, fam) for n in sizes for fam in TL.families_at(n)] + [(n_cap, "empty"), (n_cap, "rejected")]


def padded(specs, B, n_pad):
    return specs + [(n_pad, "thin")] * (B - len(specs))


def make_handle(capi, po, monkeypatch, prec, n_cap, specs, f_cap, compress):
    for name in G.ENV_NAMES:
        monkeypatch.delenv(name, raising=False)
    B, m_cap = len(specs), min(max(n_cap, 4), 30)
    bt = capi.Batch(B, n_cap, f_cap, m_cap, capi.F64 if prec == "f64" else capi.F32)
    if compress >= 0:
        bt.set_compression(compress)
    tr = UL.FL.window(po).tr
    for b in range(B):
        bt.initialize(b, tr.cfg, tr.imu0)
    for k in range(max(n for n, _ in specs)):          # every trajectory augmented to its own size, one launch per run of longer windows
        b = 0
        while b < B:
            if specs[b][0] <= k:
                b += 1
                continue
            e = b
            while e < B and specs[e][0] > k:
                e += 1
            bt.augment_range(b, e - b)
            b = e
    for b, (n, fam) in enumerate(specs):
        assert bt.num_cam_states(b) == n
        H.copy_oracle_to_device(UL.window(po, n), bt, b)
        bt.set_tracks(b, *tracks_for(po, n, fam))
    return bt, m_cap


WORST = {}


def run_case(capi, po, routes_exe, monkeypatch, tag, prec, n_cap, specs, f_cap=F_CAP, compress=0, ranges=None, info_form=False):
    """the case's launch sequence and every per-trajectory assertion; returns (state bits + correction per trajectory, last_stats
    per trajectory)"""
    B = len(specs)
    bt, m_cap = make_handle(capi, po, monkeypatch, prec, n_cap, specs, f_cap, compress)
    windows = [n for n, _ in specs]
    if info_form:
        got = G.assert_routes(routes_exe, "default", prec, B, n_cap, m_cap, windows, f_cap=f_cap, skip=("V",))
        assert "Q" not in got
    else:
        assert_tsqr_routes(routes_exe, prec, B, n_cap, m_cap, windows, f_cap, compress)
    before = {b: G.state_bits(bt, b) for b, (n, fam) in enumerate(specs) if fam in ROWLESS}
    for b0, nb in ranges or [(0, B)]:
        bt.marginalize_range(b0, nb)
    failures, out, stats = [], [], []
    for b, (n, fam) in enumerate(specs):
        st = bt.last_stats(b)                               # (raises when a sticky flag is up)
        assert bt.error_flags(b) == 0, (b, n, fam)
        now = G.state_bits(bt, b)
        assert np.array_equal(now[2], now[2].T), (b, n, fam)
        stats.append(st)
        if fam in ROWLESS:
            assert st["n_tracks"] == (0 if fam == "empty" else UL.N_TALL) and st["n_passed"] == 0 and st["m_rows"] == 0, (b, n, fam, st)
            assert all(np.array_equal(x, y) for x, y in zip(now, before[b])), (b, n, fam)
            out.append(now + (None,))
            continue
        ref = reference(po, n, fam)
        for key in H.STAT_KEYS:
            assert st[key] == ref.stats[key], (b, n, fam, key, st, ref.stats)
        M, slots, _ = tracks_for(po, n, fam)
        ok = (ref.rows[:, 0] > 0) & (ref.rows[:, 1] > 0)
        H.check_tracks(bt.last_tracks(b), ref.rows, ok, prec, None, dict(M=M, slots=slots), UL.window(po, n), (tag, prec, n_cap, n, fam))
        dx = bt.last_deltax(b)
        dc, dd = H.cov_scaled_err(now[2], ref.P1), UL.dx_scaled(dx, ref.dx, ref.P0)
        group = TL.group_of(fam)
        bar_c, bar_d = TL.bars(prec, group)
        if fam != "thin" or b == len(specs) - 1:            # (the padding: one line)
            print("tsqr-dev %s %s n_cap=%d B=%d n=%d %s m_rows=%d cov %.3e dx %.3e" % (tag, prec, n_cap, B, n, fam, st["m_rows"], dc, dd))
        w = WORST.setdefault((tag.split("-")[0], prec, group), [0.0, 0.0])
        w[0], w[1] = max(w[0], dc), max(w[1], dd)
        if not (dc <= bar_c and dd <= bar_d):
            failures.append((b, n, fam, dc, dd, bar_c, bar_d))
        out.append(now + (dx,))
    bt.close()
    for k, w in sorted(WORST.items()):
        print("tsqr-dev worst %s %s %s cov %.3e dx %.3e" % (k + tuple(w)))
    assert not failures, (tag, prec, n_cap, failures)
    return out, stats


def same_bits(x, y):
    return all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(x, y))


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("n_cap", N_CAPS)
@pytest.mark.parametrize("prec", G.BOTH)
def test_every_instantiation_and_edge(capi, po, routes_exe, monkeypatch, prec, n_cap):
    """float: 1L 2L 3L (RW 32) | 4L 5L (45) | 5G (46) 6G; double: 1L 2L 3L 4L (32 only) | 4G (33) 5G 6G -- with staggered, holes and
    blind at every window size up to n_cap"""
    run_case(capi, po, routes_exe, monkeypatch, "a", prec, n_cap, specs_of(n_cap))


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("B", (32, 33, 64, 65, 128, 129))
@pytest.mark.parametrize("prec", G.BOTH)
def test_chunk_counts(capi, po, routes_exe, monkeypatch, prec, B):
    """nchunk follows B alone: with 2 chunks stage 2 interleaves with a divisor of 1, with 1 chunk there is no stage 2 and the
    Kalman stage reads the stage-1 triangle.  (Bits are not compared across B: the fold order differs.)"""
    specs = padded(specs_of(22)[-14:], B, 22)             # 15, 16, 21 and 22 cameras with the three lists, the row-less two, `thin` padding
    assert len(specs) == B
    got = meant_q(prec, 22, B)
    assert got.endswith({32: "nchunk=8 merge=1", 33: "nchunk=4 merge=1", 64: "nchunk=4 merge=1", 65: "nchunk=2 merge=1", 128: "nchunk=2 merge=1", 129: "nchunk=1 merge=0"}[B])
    run_case(capi, po, routes_exe, monkeypatch, "b", prec, 22, specs)


# ------------------------------------------------------------------------------------------------ (c)
N_DENSE, F_DENSE, B_ONE_CHUNK, N_PAD = 30, 320, 129, 26


@pytest.mark.parametrize("prec", G.BOTH)
def test_deep_pipeline_and_ring_in_one_chunk(capi, po, routes_exe, monkeypatch, prec):
    """B = 129: one chunk, so the whole stack of a trajectory is ONE workgroup's.  Three stacks of 24 blocks or one more (every
    wavefront takes a second block from the real loader) and three of more than 512 blocks (the ring of progress words wraps),
    with m_rows = 0, 1 and RW - 1 modulo RW: a full last block, one live row, one dead row."""
    rw = TL.rw_of(prec, N_DENSE)
    lists = [(TL.dense_name(rw, rows, res), rows, res) for rows in (TL.deep_rows(rw), TL.ring_rows(rw)) for res in TL.residues(rw)]
    specs = padded([(N_DENSE, name) for name, _, _ in lists], B_ONE_CHUNK, N_PAD)
    assert meant_q(prec, N_DENSE, B_ONE_CHUNK).startswith("tsqr NC=3 RW=%d tri=lds " % rw) and meant_q(prec, N_DENSE, B_ONE_CHUNK).endswith("nchunk=1 merge=0")
    _, stats = run_case(capi, po, routes_exe, monkeypatch, "c", prec, N_DENSE, specs, f_cap=F_DENSE)
    for (name, rows, res), st in zip(lists, stats):
        blocks = -(-st["m_rows"] // rw)
        assert st["m_rows"] >= rows and st["m_rows"] % rw == res and blocks >= 2 * TL.QR_PIPELINE, (name, st)
        assert (blocks > TL.QR_RING) == (rows > 4096), (name, st)


def test_ring_in_each_of_eight_chunks(capi, po, routes_exe, monkeypatch):
    """double, the handle on this route by geometry: more than 1 200 tracks of up to 30 observations at 31 cameras, at least
    65 649 rows = 4 104 blocks of 16 dealt to 8 chunks, 513 or more each; the second trajectory carries `many`"""
    name = TL.dense_name(16, TL.ring_rows(16, 8), 1)
    _, stats = run_case(capi, po, routes_exe, monkeypatch, "c8", "f64", 31, [(31, name), (31, "many")], f_cap=1280, compress=-1)
    blocks = -(-stats[0]["m_rows"] // 16)
    assert stats[0]["m_rows"] > 512 * 16 * 8 and stats[0]["m_rows"] % 16 == 1 and blocks // 8 > TL.QR_RING, stats[0]


# ------------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("n_cap", (10, 31))
@pytest.mark.parametrize("prec", G.BOTH)
def test_route_forced_by_geometry(capi, po, routes_exe, monkeypatch, prec, n_cap):
    """f_cap = 1040 > routes::INFO_F_CAP, no set_compression call: the way callers reach this route by necessity"""
    _, stats = run_case(capi, po, routes_exe, monkeypatch, "d", prec, n_cap, [(n_cap, "many"), (n_cap, "thin")], f_cap=1040, compress=-1)
    assert stats[0]["n_tracks"] == TL.N_MANY and stats[0]["n_passed"] > 1000


# ------------------------------------------------------------------------------------------------ (e)
@pytest.mark.parametrize("info_form", (False, True), ids=("tsqr", "information"))
@pytest.mark.parametrize("prec", G.BOTH)
def test_select_rounds(capi, po, routes_exe, monkeypatch, prec, info_form):
    """F = 64 | 65 and 256 | 257 with every third track rejected: the last and first track of a 64-track round, the fast | generic
    switch of select_body -- on both compression routes (k_select_diag runs the same body)"""
    specs = [(TL.ROUND_N, "round:%d" % F) for F in TL.ROUND_SIZES]
    run_case(capi, po, routes_exe, monkeypatch, "e-info" if info_form else "e", prec, TL.ROUND_N, specs, f_cap=320, compress=-1 if info_form else 0, info_form=info_form)


# ------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("prec,n_cap", (("f32", 22), ("f64", 33)))
def test_range_offset_changes_no_bit(capi, po, routes_exe, monkeypatch, prec, n_cap):
    """the loader indexes the work-list by b - b0: marginalize_range(0, k) then (k, B - k) on a fresh handle gives the bits of
    the single range"""
    specs = specs_of(n_cap)
    k = len(specs) // 2 + 1
    one = run_case(capi, po, routes_exe, monkeypatch, "f", prec, n_cap, specs)[0]
    two = run_case(capi, po, routes_exe, monkeypatch, "f", prec, n_cap, specs, ranges=[(0, k), (k, len(specs) - k)])[0]
    for b in range(len(specs)):
        assert same_bits(one[b], two[b]), (b, specs[b])
