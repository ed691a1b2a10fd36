"""CPU only: the inputs of tests/test_gpu_tsqr_kernels.py (tests/tsqr_lab.py) have the shapes the Householder TSQR route needs
and can see a fault.  Everything here runs on the CPU oracles, as tests/test_update_inputs.py: the double oracle in LEAN mode is
the reference, the float oracles in LEAN and GRAM mode give the float bars, the mutants are applied to the double oracle's own
RESULT or to its INPUT list, never to code under test.

Found while writing the lab: in this window the track of 2 observations at (n - 2, n - 1) the lists carry is motion-rejected at
EVERY size (two neighbouring cameras are closer than translation_threshold), and so is every track that starts at n - 2; the
latest first slot of a passed track is n - 3 .. n - 5 (LATE_BINS), so the largest kmin a block sees is 6 (n - 3), not 6 (n - 2).
The track stays in the lists (a motion-rejected track behind every passed one is a hole at the end of select_body's list); both
facts are asserted below.

Measured (distance of the float oracles from the double LEAN oracle on the entry-scaled metric: covariance, correction):
    edge lists (24 tracks, rounds, deep stacks)   <= 3.227e-05   1.914e-05   (update_lab's own lists: 3.390e-05, 1.415e-05)
    many (1 030 tracks, 3 088 rows)               <= 8.126e-05   2.568e-05
    ring (float, 16 447 .. 16 449 rows)           <= 3.531e-04   1.100e-04
For the dense, `many` and `round` lists only the result mutants are required: among hundreds of tracks the ones sorted last are
short and start late, and losing them moves little."""
import numpy as np
import pytest

import tsqr_lab as TL
import update_lab as UL

N_CAP_DENSE, N_CAP_BIG = 30, 31


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def firsts_of(tracks):
    M, slots, _ = tracks
    off = np.concatenate([[0], np.cumsum(M)])
    return np.array([slots[off[i]] for i in range(len(M))]), off


def test_shapes_without_an_oracle():
    for nv in range(2, 64):
        bins, shape = TL.first_bins(nv), TL.staggered_shape(nv)
        assert len(shape) == TL.N_TRACKS and bins[0] == 0 and bins[-1] == nv - 2
        assert shape[0] == (nv - 2, 2) and sum(f == nv - 2 for f, _ in shape) == (1 if nv > 2 else TL.N_TRACKS)
        assert all(2 <= L <= min(nv - f, UL.L_MAX) for f, L in shape)
        per_bin = [sum(f == b for f, _ in shape) for b in bins]
        assert max(per_bin) >= 2 and min(per_bin) >= 1                      # a shared first slot; no bin of first_bins stays empty
        if nv >= 7:
            assert set(range(bins[-1])) - set(bins)                         # empty bins between occupied ones (a window of up to 6 cameras has none to spare)
        assert all((e in bins) == (e <= nv - 2) for e in TL.EDGE_FIRSTS)
    for rw in (16, 32):
        for rows in (TL.deep_rows(rw), TL.ring_rows(rw)):
            for res in TL.residues(rw):
                sh = TL.dense_shape(N_CAP_DENSE, rw, rows, res)
                m = sum(2 * L - 3 for _, L in sh)
                assert m >= rows and m % rw == res and m < rows + 2 * rw + 60 and len(sh) <= 320, (rw, rows, res, m, len(sh))
    assert TL.deep_rows(16) == 384 and TL.ring_rows(32) == 16385 and TL.ring_rows(16, 8) == 65649
    sh = TL.many_shape(10)
    assert len(sh) == 1030 > 1024 and {L for _, L in sh} == {2, 3, 4}
    assert TL.rw_of("f32", 31) == 32 and TL.rw_of("f32", 32) == 16 and TL.rw_of("f64", 10) == 16


@pytest.mark.parametrize("n", TL.SIZES)
def test_conditions_and_mutants_hold_with_zero_exclusions(po, n):
    """staggered, holes and blind at every size the GPU suite uses: UL.case_violations empty, every result mutant at 10 float
    bars or more (UL.MUTANT_EXEMPT honoured), from 4 cameras on both input mutants at 10 float bars or more -- and the shapes
    as they come out of the oracle's decisions, not only as they were laid out"""
    for fam in TL.families_at(n):
        t = TL.tracks_of(po, n, fam)
        ref, oth = TL.reference(po, n, fam), TL.others(po, n, fam)
        assert UL.case_violations(ref, oth, t[0]) == [], (n, fam)
        assert TL.mutant_violations(ref, n) == [], (n, fam)
        first, off = firsts_of(t)
        order, rows, pfirst = TL.sorted_passed(t, ref)
        passed = np.zeros(len(t[0]), bool)
        passed[order] = True
        scores = {}
        if n >= TL.INPUT_MUTANT_MIN:
            assert TL.input_mutant_violations(po, n, fam) == [], (n, fam)
            scores = {w: TL.input_mutant_scores(po, n, fam, w) for w in TL.INPUT_MUTANTS}
        d = {k: UL.distances(r, ref) for k, r in oth.items()}
        print("tsqr-lab n=%d %s passed %d/%d m_rows %d firsts %s | d32 LEAN %.2e %.2e GRAM %.2e %.2e | mutants %s | input %s" % (
            n, fam, ref.stats["n_passed"], len(t[0]), ref.stats["m_rows"], sorted(set(pfirst.tolist())), *d["f32_lean"], *d["f32_gram"],
            " ".join("%.1e" % UL.mutant_score(ref, m) for m in UL.MUTANTS), " ".join("%.1e/%.1e" % s for s in scores.values())))
        assert ref.stats["m_rows"] == int(rows.sum()) and max(d["f64_gram"]) <= 1e-2 * UL.BAR_F64          # (found: <= 2.1e-9, 42 cameras)
        # the list order is no sorted one, and the sort has something to do
        assert not np.array_equal(order, np.sort(order)) or len(set(pfirst.tolist())) == 1, (n, fam)
        vis = TL.visible(n, fam)
        assert set(t[1].tolist()) <= set(vis)
        if fam == "blind":
            assert 0 not in t[1] and n // 2 not in t[1] and pfirst.min() >= 1
        last = [i for i in range(len(first)) if t[0][i] == 2 and first[i] == vis[-2]]
        if len(vis) > 2:
            assert len(last) == 1 and t[1][off[last[0]] + 1] == vis[-1]           # the track at (n - 2, n - 1) is in the list ...
        assert not passed[first == vis[-2]].any() or len(vis) <= 2, (n, fam)     # ... and the motion check rejects it, at every size
        if fam == "holes":
            assert passed.any() and (~passed).sum() > 1
            assert not passed[:np.nonzero(passed)[0][-1]].all()                   # the passed tracks are no prefix of the list
            noisy = np.arange(len(passed)) % 3 == 1
            assert (~passed[noisy]).sum() >= 3 and passed[~noisy].sum() >= 3, (n, passed)   # both kinds occur
        if fam == "staggered":
            assert 0 in pfirst
            if n >= 8:
                assert pfirst.max() >= n - 5, (n, pfirst)                          # kmin reaches 6 (n - 5) .. 6 (n - 3)
                cnt = np.bincount(pfirst)
                assert cnt.max() >= 2 and (cnt[:pfirst.max()] == 0).any()          # passed tracks share a bin; empty bins between
            if n >= 22:
                assert 10 in pfirst and 11 in pfirst                               # kmin = 60 | 66: either side of column 64
            if n >= 26:
                assert 21 in pfirst and 22 in pfirst                               # kmin = 126 | 132: either side of column 128


DENSE = [(N_CAP_DENSE, TL.dense_name(rw, rows, res), rw, rows, res) for rw in (16, 32) for rows in (TL.deep_rows(rw), TL.ring_rows(rw)) for res in TL.residues(rw)]


@pytest.mark.parametrize("n,name,rw,rows,res", DENSE, ids=[c[1] for c in DENSE])
def test_dense_stacks_have_the_rows_they_were_written_for(po, n, name, rw, rows, res):
    """every track of a dense list passes on the oracle, so m_rows is the residue the list was laid out for; the result
    mutants score 10 float bars of the list's group"""
    t = TL.tracks_of(po, n, name)
    ref, oth = TL.reference(po, n, name), TL.others(po, n, name)
    group = TL.group_of(name)
    assert ref.stats["n_passed"] == len(t[0]) and ref.stats["m_rows"] % rw == res and ref.stats["m_rows"] >= rows, ref.stats
    bad = [v for v in UL.case_violations(ref, oth, t[0]) if not (group == "ring" and v[0] == "ill_conditioned")]      # (the ring's own constants below)
    assert bad == [], (name, bad)
    assert TL.mutant_violations(ref, n, group) == [], name
    blocks = -(-ref.stats["m_rows"] // rw)
    assert blocks >= 2 * TL.QR_PIPELINE and (blocks > TL.QR_RING) == (group == "ring")
    d = np.maximum(UL.distances(oth["f32_lean"], ref), UL.distances(oth["f32_gram"], ref))
    print("tsqr-lab n=%d %s tracks %d m_rows %d blocks %d | d32 %.3e %.3e" % (n, name, len(t[0]), ref.stats["m_rows"], blocks, *d))
    if rw == 32 or group == "edge":
        assert np.all(d <= TL.D32_TSQR[group]), (name, d)


def test_the_eight_chunk_ring_list(po):
    """more than 1 200 tracks at 31 cameras: more than 512 blocks of 16 rows in each of 8 chunks; double only (no float bar)"""
    name = TL.dense_name(16, TL.ring_rows(16, 8), 1)
    t, ref = TL.tracks_of(po, N_CAP_BIG, name), TL.reference(po, N_CAP_BIG, name)
    assert ref.stats["n_passed"] == len(t[0]) > 1024 and ref.stats["m_rows"] % 16 == 1 and ref.stats["m_rows"] > 512 * 16 * 8, ref.stats
    assert -(-ref.stats["m_rows"] // 16) // 8 > TL.QR_RING          # the chunk with the fewest blocks
    assert TL.mutant_violations(ref, N_CAP_BIG, "ring") == []


@pytest.mark.parametrize("n", (10, 31))
def test_many(po, n):
    t = TL.tracks_of(po, n, "many")
    ref, oth = TL.reference(po, n, "many"), TL.others(po, n, "many")
    assert UL.case_violations(ref, oth, t[0]) == [] and TL.mutant_violations(ref, n, "many") == []
    assert ref.stats["n_tracks"] == 1030 and ref.stats["n_passed"] > 1000, ref.stats
    order = TL.sorted_passed(t, ref)[0]
    assert not np.array_equal(order, np.sort(order))
    d = np.maximum(UL.distances(oth["f32_lean"], ref), UL.distances(oth["f32_gram"], ref))
    print("tsqr-lab n=%d many passed %d m_rows %d | d32 %.3e %.3e" % (n, ref.stats["n_passed"], ref.stats["m_rows"], *d))
    assert np.all(d <= TL.D32_TSQR["many"]), d


@pytest.mark.parametrize("F", TL.ROUND_SIZES)
def test_rounds(po, F):
    """holes-style lists of 64 | 65 and 256 | 257 tracks at 22 cameras: the last and first track of a 64-track round of
    select_body, its fast | generic switch"""
    name = "round:%d" % F
    t = TL.tracks_of(po, TL.ROUND_N, name)
    ref, oth = TL.reference(po, TL.ROUND_N, name), TL.others(po, TL.ROUND_N, name)
    assert UL.case_violations(ref, oth, t[0]) == [] and TL.mutant_violations(ref, TL.ROUND_N) == []
    order = TL.sorted_passed(t, ref)[0]
    passed = np.zeros(F, bool)
    passed[order] = True
    assert ref.stats["n_tracks"] == F and 3 <= (~passed).sum() and not passed[:order.max()].all() and not np.array_equal(order, np.sort(order))
    assert passed[F - 1]             # the track that opens, or closes, a round is in the stack
    d = np.maximum(UL.distances(oth["f32_lean"], ref), UL.distances(oth["f32_gram"], ref))
    print("tsqr-lab round F=%d passed %d m_rows %d | d32 %.3e %.3e" % (F, ref.stats["n_passed"], ref.stats["m_rows"], *d))
    assert np.all(d <= TL.D32_TSQR["edge"]), d


def test_float_bars_are_the_measured_ones(po):
    """per group the largest distance of the float oracles from the double oracle reproduces (to 2 %) and stays within the
    constants the bars are built on; no bar is below update_lab's, whose lists ride in every case"""
    w = {g: np.zeros(2) for g in TL.D32_TSQR}
    cases = [(n, f) for n in TL.SIZES for f in TL.families_at(n)] + [(TL.ROUND_N, "round:%d" % F) for F in TL.ROUND_SIZES] + [(10, "many"), (31, "many")]
    cases += [(n, name) for n, name, rw, _, _ in DENSE if rw == 32 or TL.group_of(name) == "edge"]
    for n, fam in cases:
        ref, oth = TL.reference(po, n, fam), TL.others(po, n, fam)
        g = TL.group_of(fam)
        w[g] = np.maximum(w[g], np.maximum(UL.distances(oth["f32_lean"], ref), UL.distances(oth["f32_gram"], ref)))
    for g in w:
        print("tsqr-lab float maxima %s %.3e %.3e" % (g, *w[g]))
        assert np.allclose(w[g], TL.D32_TSQR_MEASURED[g], rtol=0.02), (g, w[g])
        assert np.all(np.array(TL.D32_TSQR_MEASURED[g]) <= np.maximum(TL.D32_TSQR[g], (UL.D32_COV, UL.D32_DX)))
        assert TL.bars("f32", g) >= UL.bars("f32") and TL.bars("f64", g) == UL.bars("f64")
    assert TL.bars("f32", "edge") == (4 * 3.40e-5, 4 * 1.92e-5) and TL.bars("f32", "many") == (4 * 8.13e-5, 4 * 2.57e-5) and TL.bars("f32", "ring") == (4 * 3.54e-4, 4 * 1.10e-4)


def test_rejected_list_at_the_added_sizes(po):
    """the row-less `rejected` trajectory of the GPU suite at the two sizes update_lab does not have: no track passes"""
    for n in sorted(set(TL.SIZES) - set(UL.SIZES)):
        for dtype in (po.F64, po.F32):
            r = UL.run_oracle(po, n, UL.rejected_tracks(po, n), dtype)
            assert r.stats["n_tracks"] == UL.N_TALL and r.stats["n_passed"] == 0 and r.stats["m_rows"] == 0 and np.array_equal(r.P0, r.P1), (n, r.stats)
