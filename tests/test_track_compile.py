"""The track compiler on the CPU (csrc/track_compile.h, msckf_hip_compile_*, capi.TrackCompiler, asl.compile_sequence and the
staging helpers), and the host half of the stand-still initialisation under a replay (asl.standstill_state,
scenario.replay_imu_sums).  Nothing here needs a device.

  1. tests/cpp/track_compile_host.cpp: the header alone, a recording traced by hand, plain and sanitized; and the header alone
     against the library's entry points on recording D, cell by cell
  2. round trip: a synthetic trajectory's stream compiled with its own parameters gives back its frames
  3. recordings A-D (tests/compile_lab.py) against the double oracle driven by ids, image by image, and a second oracle driven
     by the cells alone; the coverage conditions of the recordings
  4. asl.compile_sequence against what asl.run hands a filter; refusals with their texts; the staging helpers' capacity errors
  5. asl.standstill_state against the values standstill_initial_state gave before it was factored out; the twin of the sums
     against a plain loop"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compile_lab as CL
import helpers as H
from msckf_mono_amd import asl, capi, scenario as sc

FLAGS = [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]]


# ------------------------------------------------------------------------------------------------ 1. the header alone
@pytest.fixture(scope="module", params=FLAGS, ids=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("track_compile") / "track_compile_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + request.param + ["-o", path, os.path.join(H.ROOT, "tests", "cpp", "track_compile_host.cpp")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return path


def test_the_compiler_alone_on_a_recording_traced_by_hand(exe):
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "track compile ok" in run.stdout, run.stdout + run.stderr


def test_the_header_alone_and_the_library_give_the_same_cells(exe, tmp_path):
    """recording D (every hand edit) through the stand-alone program and through msckf_hip_compile_*: same summaries, ids, slots
    and coordinates, bit for bit"""
    rec, cells = CL.recording("D"), CL.compiled("D")
    path = str(tmp_path / "recording.txt")
    with open(path, "w") as fh:
        fh.write("P %d %d %d\n" % rec.params)
        for im in rec.images:
            fh.write("I %d %d\n" % (len(im["cur"][1]), len(im["new"][1])))
            for key in ("cur", "new"):
                for z, fid in zip(*im[key]):
                    fh.write("%d %s %s\n" % (int(fid), float(z[0]).hex(), float(z[1]).hex()))
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    at = 0
    for c in cells:
        head = lines[at].split(); at += 1
        assert head[0] == "C" and [int(x) for x in head[1:]] == [len(c["M"]), len(c["slots"]), c["n_drop"], c["window"], c["live"]]
        o = 0
        for t, m in enumerate(c["M"]):
            tl = lines[at].split(); at += 1
            assert tl[0] == "T" and int(tl[1]) == int(c["ids"][t]) and int(tl[2]) == m
            for _ in range(m):
                sl, x, y = lines[at].split(); at += 1
                assert int(sl) == c["slots"][o] and float.fromhex(x) == c["obs"][o, 0] and float.fromhex(y) == c["obs"][o, 1]
                o += 1
    assert lines[at:] == [""]


# ------------------------------------------------------------------------------------------------ 2. round trip
@pytest.mark.parametrize("N,F,nf", [(6, 5, 20), (10, 8, 30)])
def test_a_trajectorys_stream_compiles_back_into_its_frames(N, F, nf):
    """compile(stream(tr)) with (N - 1, 3, 1000) gives tr.frames exactly -- M, slots and coordinates bit for bit, the tracks matched
    by id (track t of frame k is id 10000 k + t) --, the window Nw, and a drop of 1 exactly when Nw == N"""
    tr = sc.Trajectory(3, 1, N, F, nf)
    tc = capi.TrackCompiler(N - 1, 3, 1000)
    st = tr.stream()
    tracks = 0
    for k, fr in enumerate(tr.frames):
        c = tc.image(st[k]["cur"], st[k]["new"])
        assert c["window"] == fr["Nw"] and c["n_drop"] == (1 if fr["Nw"] == N else 0), k
        assert sorted(int(i) for i in c["ids"]) == [10000 * k + t for t in range(len(fr["M"]))], k
        off = np.concatenate([[0], np.cumsum(fr["M"])]).astype(int)
        o = 0
        for fid, m in zip(c["ids"], c["M"]):
            t = int(fid) - 10000 * k
            assert m == fr["M"][t]
            assert np.array_equal(c["slots"][o:o + m], fr["slots"][off[t]:off[t + 1]]) and np.array_equal(c["obs"][o:o + m], fr["obs"][off[t]:off[t + 1]]), (k, t)
            o += m
        tracks += len(c["M"])
    assert tracks > 10 * F and c["live"] == 0


# ------------------------------------------------------------------------------------------------ 3. against the oracle
@pytest.fixture(scope="module")
def oracle_runs(oracle_lib):
    """per recording: the id-driven double oracle's tracks after update(), windows around pruneEmptyStates and gate counts per
    image, and the final state of it and of a second oracle fed the compiled cells alone (computed once)"""
    po = oracle_lib
    out = {}
    for name in "ABCD":
        rec, cells = CL.recording(name), CL.compiled(name)
        a, b = po.Oracle(po.F64, po.LEAN), po.Oracle(po.F64, po.LEAN)
        a.initialize(rec.cfg, rec.imu0); b.initialize(rec.cfg, rec.imu0)
        per = []
        for im, c in zip(rec.images, cells):
            a.propagate(im["readings"]); a.augmentState(im["state_id"], im["time"]); a.update(*im["cur"])
            M, sl, ob = a.getTracks()
            a.addFeatures(*im["new"]); a.marginalize()
            n0 = a.getNumCamStates(); a.pruneEmptyStates(); n1 = a.getNumCamStates()
            per.append(dict(M=M.copy(), slots=[sl[t, :M[t]].copy() for t in range(len(M))], obs=[ob[t, :M[t]].copy() for t in range(len(M))],
                            n0=n0, n1=n1, passed=a.lastStats()["n_passed"] if len(M) else 0))
            CL.cell_driven_frame(b, im, c)
        fin = lambda o: (o.getImuState(), o.getCamStates()[0], o.getCovariance())
        out[name] = dict(per=per, by_ids=fin(a), by_cells=fin(b))
    return out


@pytest.mark.parametrize("name", list("ABCD"))
def test_cells_equal_the_oracles_bookkeeping_image_by_image(oracle_runs, name):
    """the cell equals Oracle.getTracks() after update(), in contents and in order; window and n_drop equal getNumCamStates()
    around pruneEmptyStates(); and an oracle fed setTracks / marginalize / dropOldest from the cells ends bit-equal to the
    id-driven one"""
    run, cells = oracle_runs[name], CL.compiled(name)
    for k, (p, c) in enumerate(zip(run["per"], cells)):
        assert np.array_equal(p["M"], c["M"]), k
        o = 0
        for t, m in enumerate(c["M"]):
            assert np.array_equal(p["slots"][t], c["slots"][o:o + m]) and np.array_equal(p["obs"][t], c["obs"][o:o + m]), (k, t)
            o += m
        assert c["window"] == p["n0"] and c["n_drop"] == p["n0"] - p["n1"], k
    for x, y in zip(run["by_ids"], run["by_cells"]):
        assert np.array_equal(x, y)
    assert max(c["window"] for c in cells) <= CL.N_CAP and max(len(c["M"]) for c in cells) <= CL.F_CAP
    assert max(int(c["M"].max()) for c in cells if len(c["M"])) <= CL.M_CAP


def _ended(cells, hi):
    """(tracks that ended by length: max_track_length observations, the last one in the newest camera; tracks that ended by loss)"""
    by_len = by_loss = 0
    for c in cells:
        o = 0
        for m in c["M"]:
            newest = c["slots"][o + m - 1] == c["window"] - 1
            assert newest == (m >= hi)
            by_len += bool(newest); by_loss += not newest
            o += m
    return by_len, by_loss


def test_recording_a_keeps_its_edges(oracle_runs):
    """drops per image {0: 15, 1: 4, 2: 2, 3: 2, 4: 1}; the window grows to 12 because the oldest camera still tracks a feature; 126
    tracks, all passing the oracle's gate, the longest of 11 observations.  (The shortest has 3: scenario.Trajectory makes no
    shorter track, so min_track_length = 2 lists nothing the generator's own 3 would not.)"""
    cells = CL.compiled("A")
    assert collections.Counter(c["n_drop"] for c in cells) == {0: 15, 1: 4, 2: 2, 3: 2, 4: 1}
    assert max(c["window"] for c in cells) == 12 > CL.recording("A").params[0]
    lens = np.concatenate([c["M"] for c in cells])
    assert len(lens) == 126 and 2 <= lens.min() <= 3 and lens.max() == 11
    assert sum(p["passed"] for p in oracle_runs["A"]["per"]) == 126


def test_recording_b_keeps_its_edges(oracle_runs):
    """104 tracks end by length, with an observation in the newest camera; 112 end by loss; up to 12 tracks per image; 214 of 216
    pass the oracle's gate"""
    cells = CL.compiled("B")
    assert _ended(cells, CL.recording("B").params[2]) == (104, 112)
    assert max(len(c["M"]) for c in cells) == 12
    assert sum(p["passed"] for p in oracle_runs["B"]["per"]) == 214


def test_recording_c_and_d_keep_their_edges():
    """C: both ways of ending.  D: the inserted image has no features and no samples, so every track ends on it; the duplicated id's first
    occurrence is the observation kept; stray ids and the two-observation tracks appear in no cell; IMU counts 0, 9, 10, 11"""
    by_len, by_loss = _ended(CL.compiled("C"), CL.recording("C").params[2])
    assert by_len > 0 and by_loss > 0
    rec, cells = CL.recording("D"), CL.compiled("D")
    assert len(rec.images) == len(CL.recording("B").images) + 1
    e = rec.images[CL.D_EMPTY_AT]
    assert len(e["cur"][1]) == len(e["new"][1]) == len(e["readings"]) == 0
    # (an image without features loses every track: all that are long enough end here, nothing stays live)
    assert cells[CL.D_EMPTY_AT]["live"] == 0 and len(cells[CL.D_EMPTY_AT]["M"]) == max(len(c["M"]) for c in cells) > 12
    assert sorted(set(len(im["readings"]) for im in rec.images)) == [0, 9, 10, 11] and max(len(im["readings"]) for im in rec.images) <= CL.K
    listed = set(int(i) for c in cells for i in c["ids"])
    assert not any(i >= 900000 for i in listed)
    dup = rec.images[CL.D_DUP_AT]["cur"]
    fid, first = int(dup[1][0]), dup[0][0]
    assert int(dup[1][-1]) == fid and not np.array_equal(dup[0][-1], first)
    hits = [c for c in cells if fid in [int(i) for i in c["ids"]]]
    assert len(hits) == 1
    c = hits[0]
    t = [int(i) for i in c["ids"]].index(fid)
    rows = c["obs"][int(c["M"][:t].sum()):int(c["M"][:t + 1].sum())]
    assert any(np.array_equal(r, first) for r in rows) and not any(np.array_equal(r, dup[0][-1]) for r in rows)
    assert _ended(cells, rec.params[2])[0] > 0


# ------------------------------------------------------------------------------------------------ 4. compile_sequence, refusals, staging
class _Recorder:
    """a filter with the reference's member names that only records what asl.run hands it"""

    def __init__(self):
        self.calls, self.pend = [], None

    def initialize(self, cfg, imu29):
        pass

    def propagate(self, rd):
        self.pend = np.array(rd, dtype=np.float64).reshape(-1, 7)

    def augmentState(self, state_k, t):
        self.calls.append(dict(readings=self.pend, state_k=state_k)); self.pend = None

    def update(self, m, ids):
        self.calls[-1]["cur"] = list(ids)

    def addFeatures(self, m, ids):
        self.calls[-1]["new"] = list(ids)

    def marginalize(self):
        pass

    def pruneEmptyStates(self):
        pass

    def getImuState(self):
        return np.zeros(29)


def _check_against_run(ds, cfg, start_ns):
    rec = _Recorder()
    out = asl.run(ds, rec, cfg, start_ns=start_ns)
    cs = asl.compile_sequence(ds, cfg, start_ns=start_ns)
    assert len(cs["images"]) == len(out) == len(rec.calls)
    for c, (stamp, _), call in zip(cs["images"], out, rec.calls):
        assert c["stamp"] == stamp and c["state_k"] == call["state_k"]
        assert c["readings"].shape == call["readings"].shape and np.array_equal(c["readings"], call["readings"])
    trailing = rec.pend if rec.pend is not None else np.zeros((0, 7))
    assert np.array_equal(cs["trailing"], trailing)
    return cs


def test_compile_sequence_pairs_each_cell_with_the_samples_run_propagates(tmp_path):
    """on the golden EuRoC-layout dataset (one image inside the IMU stamps, no track dump: a cell without tracks, and trailing
    samples) and on a written dataset with its track dump, from the first stamp and from a start in the middle of an image's
    samples: the same images, state_k, sample counts and rows as asl.run hands propagate / augmentState"""
    ds = asl.read_dataset(os.path.join(H.ROOT, "tests", "golden", "euroc_layout", "mav0"))
    cs = _check_against_run(ds, asl.filter_config_from_dataset(ds), None)
    assert len(cs["images"]) == 1 and len(cs["images"][0]["readings"]) == 2 and len(cs["trailing"]) == 3 and len(cs["images"][0]["M"]) == 0
    assert (cs["K"], cs["n_cap"], cs["f_cap"], cs["m_cap"]) == (2, 1, 1, 1)
    N, F, nf = 7, 10, 16
    tr = sc.Trajectory(1, 3, N, F, nf)
    ds = asl.read_dataset(asl.write_dataset(str(tmp_path), tr))
    cs = _check_against_run(ds, tr.cfg, None)
    # the written dataset is the trajectory's stream: its cells are the trajectory's frames
    for k, (c, fr) in enumerate(zip(cs["images"], tr.frames)):
        assert c["window"] == fr["Nw"] and c["n_drop"] == (1 if fr["Nw"] == N else 0) and sorted(c["M"]) == sorted(fr["M"]), k
    assert cs["K"] == sc.IMU_PER_FRAME and cs["n_cap"] == N and cs["f_cap"] == F and 3 <= cs["m_cap"] <= N - 1
    cut = _check_against_run(ds, tr.cfg, int(ds["imu_t"][34]))
    assert len(cut["images"]) == nf - 3 and len(cut["images"][0]["readings"]) == 6 and cut["images"][0]["state_k"] == 6


def test_refusals_carry_their_code_and_text():
    L = capi.lib()
    err = lambda: L.msckf_hip_last_error().decode()
    h = C.c_void_p()
    for bad in ((0, 3, 6), (5, 0, 6), (5, 3, -1)):
        assert L.msckf_hip_compile_create(*bad, C.byref(h)) == -22 and not h.value and "must be positive" in err()
        with pytest.raises(capi.HipError, match="must be positive"):
            capi.TrackCompiler(*bad)
    assert L.msckf_hip_compile_create(5, 3, 6, None) == -22 and "null out pointer" in err()
    assert L.msckf_hip_compile_create(5, 3, 6, C.byref(h)) == 0 and h.value
    o5 = (C.c_int * 5)()
    z = (C.c_double * 4)(0.1, 0.2, 0.3, 0.4); ids = (C.c_uint64 * 2)(7, 8)
    assert L.msckf_hip_compile_image(None, z, ids, 0, z, ids, 0, o5) == -22 and "null argument" in err()
    assert L.msckf_hip_compile_image(h, z, ids, -1, z, ids, 0, o5) == -22 and "negative feature count" in err()
    assert L.msckf_hip_compile_image(h, z, ids, 0, z, ids, -2, o5) == -22 and "negative feature count" in err()
    assert L.msckf_hip_compile_image(h, None, ids, 1, z, ids, 0, o5) == -22 and "null feature list" in err()
    assert L.msckf_hip_compile_image(h, z, ids, 0, z, None, 2, o5) == -22 and "null feature list" in err()
    assert L.msckf_hip_compile_image(h, None, None, 0, z, ids, 2, o5) == 0 and list(o5) == [0, 0, 0, 1, 2]      # nulls with zero counts are fine
    assert L.msckf_hip_compile_cell(h, None, None, None, None, 0, 0) == 0
    assert L.msckf_hip_compile_cell(h, None, None, None, None, -1, 0) == -22 and "negative capacity" in err()
    assert L.msckf_hip_compile_destroy(h) == 0
    # -E2BIG beyond the caps: a cell with tracks into arrays too small
    tc = capi.TrackCompiler(5, 2, 1000)
    tc.image(([], []), ([[0, 0], [1, 1]], [1, 2]))
    tc.image(([[0, 0], [1, 1]], [1, 2]), ([], []))
    cell = tc.image(([], []), ([], []))
    assert list(cell["M"]) == [2, 2] and list(cell["ids"]) == [1, 2] and list(cell["slots"]) == [0, 1, 0, 1]
    M = (C.c_int * 2)(); sl = (C.c_int * 4)(); ob = (C.c_double * 8)(); fid = (C.c_uint64 * 2)()
    assert L.msckf_hip_compile_cell(tc.c, M, sl, ob, fid, 1, 4) == -7 and "capacities" in err()
    assert L.msckf_hip_compile_cell(tc.c, M, sl, ob, fid, 2, 3) == -7
    assert L.msckf_hip_compile_cell(tc.c, M, sl, ob, fid, 2, 4) == 2 and list(M) == [2, 2]


def test_a_new_id_that_is_already_tracked_ends_the_compiler():
    """-EEXIST as add_features_lists says it, with the reference's words; the compiler is unusable afterwards (-EIO)"""
    tc = capi.TrackCompiler(5, 3, 6)
    tc.image(([], []), ([[0.0, 0.0]], [42]))
    with pytest.raises(capi.HipError, match=r"\(-17\).*already being tracked"):
        tc.image(([[0.0, 0.1]], [42]), ([[0.5, 0.5], [0.0, 0.2]], [43, 42]))
    with pytest.raises(capi.HipError, match=r"\(-5\).*unusable"):
        tc.image(([], []), ([], []))


class _Caps:
    def __init__(self, n_cap, f_cap, m_cap, K):
        self.n_cap, self.f_cap, self.m_cap, self._replay_K = n_cap, f_cap, m_cap, K
        self.cells = []

    def scenario_set(self, f, b, rd, M, slots, obs, n_drop, skip=False):
        self.cells.append((f, b, len(rd), len(M), n_drop, skip))

    def replay_set_cell(self, f, s, rd, M, slots, obs, n_drop, skip=False):
        self.cells.append((f, s, len(rd), len(M), n_drop, skip))


def test_staging_refuses_a_cell_beyond_the_handles_capacities_with_its_stamp():
    comp = CL.as_compiled("A")
    ok = _Caps(CL.N_CAP, CL.F_CAP, CL.M_CAP, CL.K)
    asl.stage_scenario(ok, comp, 2, CL.K); asl.stage_replay(ok, comp, 1)
    assert len(ok.cells) == 2 * len(comp["images"]) and ok.cells[0][:2] == (0, 2) and ok.cells[-1][:2] == (len(comp["images"]) - 1, 1) and not ok.cells[0][5]
    first = lambda pred: next(c["stamp"] for c in comp["images"] if pred(c))
    for caps, K, words, stamp in (((11, CL.F_CAP, CL.M_CAP), CL.K, "12 camera states exceeds n_cap = 11", first(lambda c: c["window"] > 11)),
                                  ((CL.N_CAP, 5, CL.M_CAP), CL.K, "6 tracks exceed f_cap = 5", first(lambda c: len(c["M"]) > 5)),
                                  ((CL.N_CAP, CL.F_CAP, 10), CL.K, "11 observations exceeds m_cap = 10", first(lambda c: len(c["M"]) and c["M"].max() > 10)),
                                  ((CL.N_CAP, CL.F_CAP, CL.M_CAP), 9, "10 IMU samples exceed K = 9", 0)):
        for stage in (lambda h: asl.stage_scenario(h, comp, 0, K), lambda h: asl.stage_replay(h, comp, 0)):
            with pytest.raises(ValueError, match=r"image %d: .*%s" % (stamp, words)):
                stage(_Caps(*caps, K))


# ------------------------------------------------------------------------------------------------ 5. stand-still
def test_standstill_state_is_the_old_functions_closing_maths_bit_for_bit():
    """on the golden dataset standstill_initial_state returns the bits it returned before standstill_state was factored out of it
    (recorded here), and standstill_state of the two means gives the same"""
    ds = asl.read_dataset(os.path.join(H.ROOT, "tests", "golden", "euroc_layout", "mav0"))
    s = asl.standstill_initial_state(ds, 0, 2 ** 62)
    was = ['0x1.3063a961b17ccp-1', '0x1.3b5faa9943852p-5', '0x1.9b388d5902af2p-1', '0x0.0p+0', '-0x1.9e0ffe0cda42bp-4', '0x1.06cadb6745ed3p-3',
           '0x1.396809d6cfa24p-5', '0x0.0p+0', '0x0.0p+0', '0x0.0p+0', '-0x1.6c6010dded3acp+0', '0x1.1772625b4f308p-4', '0x1.bf5ad2317c8f0p-2']
    assert [float(x).hex() for x in s[:13]] == was
    assert np.array_equal(s[13:19], np.concatenate([np.zeros(3), sc.GRAVITY])) and np.array_equal(s[19:23], s[0:4]) and np.all(s[23:29] == 0)
    rd = ds["readings"]
    assert np.array_equal(asl.standstill_state(rd[:, 0:3].mean(0), rd[:, 3:6].mean(0)), s)
    assert np.array_equal(asl.standstill_state(list(rd[:, 0:3].mean(0)), tuple(rd[:, 3:6].mean(0))), s)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_twin_of_the_sums_is_a_plain_loop_over_the_expanded_rows(dtype):
    """scenario.replay_imu_sums under both noise models against a loop, sample by sample, over what replay_expand /
    replay_model_expand return for every frame of the range; a skipped cell and a cell without samples add nothing"""
    tr = sc.Trajectory(7, 0, 6, 0, 12, imu_noise_scale=0.0, obs_noise_px=0.0)
    seed, sigma4 = 0xABCDEF, (7.07e-3, 7.07e-2, 0.0, 0.0)
    Q = np.diag([1e-4] * 3 + [3e-5] * 3 + [1e-2] * 3 + [7e-2] * 3)
    L = sc.replay_noise_factor(Q)
    W = sc.replay_walk(tr, seed, L, 0.05)
    for f0, f1 in ((0, 12), (3, 4), (5, 5), (2, 11)):
        for model in (None, (L, 0.05)):
            want = np.zeros(8)
            for f in range(f0, f1):
                rows = sc.replay_expand(tr, f, seed, sigma4)[0] if model is None else sc.replay_model_expand(tr, f, seed, L, 0.05, (0.0, 0.0), W[f])[0]
                for r in rows:
                    want[0] += 1
                    want[1:8] += r.astype(dtype).astype(np.float64)
            got = sc.replay_imu_sums(tr, seed, f0, f1, sigma4=None if model else sigma4, model=model, dtype=dtype)
            assert got[0] == want[0] == 10 * (f1 - f0) and np.allclose(got, want, rtol=1e-13, atol=0), (f0, f1)
    cells = [tr.imu_for_frame(0), None, np.zeros((0, 7)), tr.imu_for_frame(3)[:9]]
    got = sc.replay_imu_sums(cells, seed, 0, 4, sigma4=sigma4)
    assert got[0] == 19 and np.allclose(got, sc.replay_imu_sums(cells, seed, 0, 1, sigma4=sigma4) + sc.replay_imu_sums(cells, seed, 3, 4, sigma4=sigma4), rtol=1e-14)
    with pytest.raises(ValueError):
        sc.replay_imu_sums(cells, seed, 0, 4)
