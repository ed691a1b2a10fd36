"""The update's launch routes (msckf_mono_amd/csrc/update_routes.h) as a stand-alone host program: which kernels a measurement
update launches for which handle, without a device.  The launchers carry these answers out and decide nothing themselves."""
import os
import subprocess

import pytest

import helpers as H

SRC = os.path.join(H.ROOT, "tests", "cpp", "update_routes_host.cpp")
GOLDEN = os.path.join(H.ROOT, "tests", "golden", "update_routes.txt")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]}


@pytest.fixture(scope="module", params=list(FLAGS))
def program(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("routes_" + request.param) / "update_routes_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[request.param] + ["-o", exe, SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run(exe, *args):
    out = subprocess.run([exe] + list(args), capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def table(program):
    """every case of the program's grid: table letter -> list of (keys, route text)"""
    rows = {}
    for line in run(program).splitlines():
        left, route = line.split(" : ", 1)
        tok = left.split()
        keys = {}
        for names, values in (t.split("=") for t in tok[1:]):
            keys.update(zip(names.split(","), values.split(",")))       # "B,nb=64,16": the batch and the launch's trajectories go together
        rows.setdefault(tok[0], []).append((keys, route))
    return rows


def routes(table, letter, **keys):
    want = {k: str(v) for k, v in keys.items()}
    got = [r for k, r in table[letter] if all(k[a] == b for a, b in want.items())]
    assert got, (letter, keys)
    return got


def route(table, letter, **keys):
    got = set(routes(table, letter, **keys))
    assert len(got) == 1, (letter, keys, got)
    return got.pop()


def test_the_table_is_the_committed_one(program):
    """(a) the routes of the whole grid, at every key the runs of values with equal sub-tables folded into one line (lossless)"""
    with open(GOLDEN) as f:
        want = f.read()
    got = run(program, "--runs")
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        first = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
        raise AssertionError("line %d: got %r, committed %r (%d / %d lines)" % (first + 1, g[first:first + 1], w[first:first + 1], len(g), len(w)))


def test_float_square_root_gain_routes(table):
    """(b) the blocked matrix-core solve up to 32 cameras, S formed inside it; the two-level solve beyond"""
    K = dict(scalar="f", form=0, fused_s=1)
    for parts in (0, 2, 4):
        assert route(table, "K", n_cap=8, gain_parts=parts, **K) == "fused=1 blocked<4,2,3>"
        assert route(table, "K", n_cap=10, gain_parts=parts, **K) == "fused=1 blocked<4,2,3>"
        assert route(table, "K", n_cap=11, gain_parts=parts, **K) == "fused=1 blocked<8,3,3>"
        assert route(table, "K", n_cap=21, gain_parts=parts, **K) == "fused=1 blocked<8,3,3>"
    for n in (22, 27, 32):
        for B in (1, 6, 64):
            assert route(table, "K", n_cap=n, gain_parts=0, B=B, **K) == "fused=1 blocked<12,4,4>"
        for B in (96, 128, 130):
            assert route(table, "K", n_cap=n, gain_parts=0, B=B, **K) == "fused=1 blocked<12,7,2>"
        assert route(table, "K", n_cap=n, gain_parts=2, **K) == "fused=1 blocked<12,7,2>"
        assert route(table, "K", n_cap=n, gain_parts=4, **K) == "fused=1 blocked<12,4,4>"
        assert route(table, "K", n_cap=n, gain_parts=0, B=64, scalar="f", form=0, fused_s=0) == "fused=0 blocked<12,4,4>"
    # 33 cameras: 13 column blocks.  OP_PHT and OP_S run (S is not fused), then the large solve
    assert route(table, "K", n_cap=33, **K) == "fused=0 large CH_S_A<12> TR_S21 items=1 CH_S_B<4> TR_W<16> items=4 k_dx_wz"
    assert route(table, "K", n_cap=63, **K) == "fused=0 large CH_S_A<12> TR_S21 items=3 CH_S_B<12> TR_W<24> items=7 k_dx_wz"


def test_float_register_resident_gain_routes(table):
    """(b) form 2: k_gain_w<float, 4 | 8 | 12, NPART>, NPART by the launch's trajectories; S is never fused"""
    for n, nbn in ((1, 4), (10, 4), (11, 8), (21, 8), (22, 12), (32, 12)):
        for nb, npart in ((1, 8), (2, 8), (16, 8), (64, 8), (24, 8), (128, 4), (130, 2)):
            for fused in (0, 1):
                assert route(table, "K", scalar="f", form=2, fused_s=fused, n_cap=n, nb=nb) == "fused=0 k_gain_w<float,%d,%d>" % (nbn, npart)
    assert route(table, "K", scalar="f", form=2, n_cap=33) == "fused=0 k_chol_inv<float,false> lds=0 OP_W k_dx_w"


def test_double_gain_routes(table):
    """(b) double has no blocked solve: register-resident up to 8 blocks, k_chol_inv (LDS up to 150 KB) to 12, then two levels"""
    K = dict(scalar="d", form=0, nb=16)
    assert route(table, "K", n_cap=10, **K) == "fused=0 k_gain_w<double,4,8>"
    assert route(table, "K", n_cap=11, **K) == "fused=0 k_gain_w<double,8,8>"
    assert route(table, "K", n_cap=21, **K) == "fused=0 k_gain_w<double,8,8>"
    assert route(table, "K", n_cap=22, **K) == "fused=0 k_chol_inv<double,true> lds=140448 OP_W k_dx_w"
    assert route(table, "K", n_cap=23, **K) == "fused=0 k_chol_inv<double,true> lds=153456 OP_W k_dx_w"
    for n in range(24, 33):
        assert route(table, "K", n_cap=n, **K) == "fused=0 k_chol_inv<double,false> lds=0 OP_W k_dx_w"
    for n in range(33, 64):
        assert route(table, "K", n_cap=n, **K).startswith("fused=0 large CH_S_A<12> ")
    # the Joseph form: k_gain in registers, else the inverse and two GEMMs
    assert route(table, "K", scalar="d", form=1, n_cap=21) == "fused=0 k_gain<double,8> k_inject<true>"
    assert route(table, "K", scalar="d", form=1, n_cap=22) == "fused=0 k_chol_inv<double,true> lds=140448 OP_W OP_K k_inject<false>"
    assert route(table, "K", scalar="f", form=1, n_cap=32) == "fused=0 k_gain<float,12> k_inject<true>"
    assert route(table, "K", scalar="f", form=1, n_cap=33) == "fused=0 k_chol_inv<float,false> lds=0 OP_W OP_K k_inject<false>"


def test_gram_routes(table):
    """(b) one-level Cholesky with 3 split-K copies up to 31 cameras, two levels and one copy beyond"""
    C = dict(override=-1, n_lit=0, f_cap=200)
    for n, nb in ((1, 4), (10, 4), (11, 8), (21, 8), (22, 12), (31, 12)):
        assert route(table, "C", n_cap=n, **C) == "compress=3 select_diag gram parts=3 CH_GRAM<%d>" % nb
    for n, items, nb in ((32, 1, 4), (42, 1, 4), (43, 2, 8), (53, 2, 8), (54, 3, 12), (63, 3, 12)):
        assert route(table, "C", n_cap=n, **C) == "compress=3 select_diag gram parts=1 CH_GRAM_A<12> TR_GRAM items=%d CH_GRAM_B<%d>" % (items, nb)
    assert route(table, "C", override=-1, n_lit=0, f_cap=1025, n_cap=10) == "compress=0 select tsqr"
    assert route(table, "C", override=0, n_lit=0, f_cap=200, n_cap=10) == "compress=0 select tsqr"
    assert route(table, "C", override=0, n_lit=1, f_cap=200, n_cap=10) == "compress=3 select_diag gram parts=3 CH_GRAM<4>"
    assert route(table, "C", override=3, n_lit=0, f_cap=1025, n_cap=10) == "compress=0 select tsqr"


def test_feature_routes(table):
    """(b) pair, single, register, staged or two long bins"""
    for f_cap in (8, 200, 512):
        for nb in (1, 2, 16, 24, 64, 128, 130):
            single = 1 if nb * f_cap <= 1024 else 0
            assert route(table, "F", scalar="f", compress=3, feat_pair=1, m_cap=30, f_cap=f_cap, nb=nb) == \
                "pair lm=30 (lo,hi] single=%d items=%d" % (single, f_cap if single else (f_cap + 1) // 2)
    for m in (4, 12):
        assert route(table, "F", scalar="f", compress=3, feat_pair=1, m_cap=m, f_cap=200, nb=16) == "pair lm=%d (lo,hi] single=0 items=100" % m
    assert route(table, "F", scalar="f", compress=3, feat_pair=1, m_cap=30, f_cap=513, nb=1) == "k_feature<0> lm=30 (lo,hi]"
    assert route(table, "F", scalar="f", compress=0, feat_pair=1, m_cap=30, f_cap=200, nb=1) == "k_feature<0> lm=30 (lo,hi]"
    assert route(table, "F", scalar="f", compress=3, feat_pair=2, m_cap=30, f_cap=200, nb=1) == "pair lm=30 (lo,hi] single=0 items=100"
    assert route(table, "F", scalar="f", compress=3, feat_pair=3, m_cap=30, f_cap=200, nb=130) == "pair lm=30 (lo,hi] single=1 items=200"
    # long windows
    for m in (31, 40, 60, 62):
        assert route(table, "F", scalar="f", compress=3, feat_pair=1, m_cap=m, f_cap=200, nb=16) == "pair lm=30 (lo,30] single=0 items=100 + k_feature<1> lm=%d (30,hi] staged" % m
    assert route(table, "F", scalar="f", compress=3, feat_pair=1, m_cap=63, f_cap=200, nb=16) == \
        "pair lm=30 (lo,30] single=0 items=100 + k_feature<1> lm=47 (30,47] + k_feature<1> lm=63 (47,hi]"
    assert route(table, "F", scalar="f", compress=3, feat_pair=0, m_cap=62, f_cap=200, nb=16) == \
        "k_feature<0> lm=30 (lo,30] + k_feature<1> lm=46 (30,46] + k_feature<1> lm=62 (46,hi]"
    for fp in range(4):
        assert route(table, "F", scalar="d", feat_pair=fp, m_cap=60) == "k_feature<0> lm=30 (lo,30] + k_feature<1> lm=45 (30,45] + k_feature<1> lm=60 (45,hi]"
        assert route(table, "F", scalar="d", feat_pair=fp, m_cap=40) == "k_feature<0> lm=30 (lo,30] + k_feature<1> lm=40 (30,hi]"
        assert route(table, "F", scalar="d", feat_pair=fp, m_cap=45) == "k_feature<0> lm=30 (lo,30] + k_feature<1> lm=45 (30,hi]"     # 15 lengths beyond 30: one bin
        assert route(table, "F", scalar="d", feat_pair=fp, m_cap=46) == "k_feature<0> lm=30 (lo,30] + k_feature<1> lm=38 (30,38] + k_feature<1> lm=46 (38,hi]"
        assert route(table, "F", scalar="d", feat_pair=fp, m_cap=31) == "k_feature<0> lm=30 (lo,30] + k_feature<1> lm=31 (30,hi]"
        assert route(table, "F", scalar="d", feat_pair=fp, m_cap=30) == "k_feature<0> lm=30 (lo,hi]"


def test_small_window_decision(table):
    """(b) a range on one side of the limit launches that side alone, one on both sides both; an empty window makes no range mixed"""
    V = dict(limit=72, compress=3, n_lit=0, form=0)
    for s in "fd":
        assert route(table, "L", scalar=s, f_cap=200, small_update=84) == "limit=72"
        assert route(table, "V", scalar=s, windows="all_short", **V) == "small split=0 nsmall=60 segb=4"
        assert route(table, "V", scalar=s, windows="all_long", **V) == "chain split=0 nsmall=0 segb=0"
        assert route(table, "V", scalar=s, windows="mixed", **V) == "mixed split=72 nsmall=60 segb=4"
        assert route(table, "V", scalar=s, windows="with_empty", **V) == "mixed split=72 nsmall=60 segb=4"
        assert route(table, "V", scalar=s, windows="only_empty", **V) == "chain split=0 nsmall=0 segb=0"
        assert route(table, "V", scalar=s, windows="empty_long", **V) == "chain split=0 nsmall=0 segb=0"
        assert route(table, "V", scalar=s, windows="at_limit", **V) == "mixed split=72 nsmall=72 segb=8"
        assert route(table, "V", scalar=s, windows="ahead", **V) == "small split=0 nsmall=72 segb=8"      # 10, 12 and min(13, n_cap = 12) cameras
        assert route(table, "V", scalar=s, windows="skipped", **V) == "mixed split=72 nsmall=72 segb=8"   # 12 cameras beside 13
        for off in (dict(limit=0), dict(compress=0), dict(n_lit=1), dict(form=1), dict(form=2)):
            assert route(table, "V", scalar=s, windows="mixed", **{**V, **off}) == "chain split=0 nsmall=0 segb=0"
        assert route(table, "V", scalar=s, windows="all_long", **{**V, "limit": 378}) == "chain split=0 nsmall=0 segb=0"


def test_every_accepted_geometry_has_a_route(table):
    """(c) alloc accepts n_cap <= 63 and every m_cap within the feature kernel's LDS: none of them meets "none" on a route the
    handle can select (the launchers used to ignore a false return there)"""
    accepted = {(k["scalar"], k["m_cap"]) for k, r in table["A"] if r == "ok"}
    for k, r in table["A"]:
        assert (r == "ok") == (int(k["n_cap"]) <= 63), (k, r)       # every (scalar, m_cap) of the grid fits the LDS
    for k, r in table["G"]:
        assert r.startswith("ok ") == (int(k["n_cap"]) <= 63), (k, r)
    for letter in "FCK":
        assert table[letter]
        for k, r in table[letter]:
            assert letter != "F" or (k["scalar"], k["m_cap"]) in accepted
            assert "none" not in r and "?" not in r, (letter, k, r)


def test_couplings(table):
    """(d) what the launchers used to state apart and had to keep in step by hand"""
    fused = 0
    for k, r in table["K"]:
        if r.startswith("fused=1"):
            fused += 1
            assert " blocked<" in r and k["scalar"] == "f" and k["form"] == "0" and k["fused_s"] != "0", (k, r)
        elif " blocked<" in r:
            assert k["fused_s"] == "0", (k, r)          # the blocked solve without it: only where the handle switched it off
    assert fused
    split = 0
    for k, r in table["C"]:
        if "parts=" in r and " parts=1 " not in r:
            split += 1
            assert " CH_GRAM<" in r, (k, r)             # split-K copies only where the one-level Cholesky adds them up
    assert split
    # the small-window rule is monotone in n_max: once a window does not fit, no longer one does
    for s in "fd":
        for f_cap in (8, 200, 512, 513, 1024, 1025):
            fits = [(int(k["n_cap"]), r.startswith("fits=1")) for k, r in table["S"] if k["scalar"] == s and k["f_cap"] == str(f_cap) and k["granted"] == "1"]
            assert [n for n, _ in fits] == list(range(1, 64))
            flags = [f for _, f in fits]
            assert flags == sorted(flags, reverse=True) and flags[0], (s, f_cap, flags)
            assert route(table, "S", scalar=s, f_cap=f_cap, granted=0, n_cap=10).startswith("fits=0")


# the Householder TSQR's instantiations, written down from the table of the suite's specification, NOT
# computed from update_routes.h: per dtype the windows of each (NC, triangle in LDS | global memory) pair, first and last
TSQR_PAIRS = {
    "f": (((1, 10), 1, "lds"), ((11, 21), 2, "lds"), ((22, 31), 3, "lds"), ((32, 42), 4, "lds"), ((43, 45), 5, "lds"), ((46, 53), 5, "global"), ((54, 63), 6, "global")),
    "d": (((1, 10), 1, "lds"), ((11, 21), 2, "lds"), ((22, 31), 3, "lds"), ((32, 32), 4, "lds"), ((33, 42), 4, "global"), ((43, 53), 5, "global"), ((54, 63), 6, "global")),
}


def test_tsqr_routes(table):
    """(b) k_qr_update<S, NC, RW, RLDS>: seven reachable (NC, L | G) pairs per dtype, the LDS edges at float 45 | 46 and double
    32 | 33 (4L exists in double at 32 cameras only: 151 816 bytes), RW 32 in float up to 31 cameras and 16 everywhere else, the
    chunk count by the batch size alone, no merge launch for one chunk"""
    for s, pairs in TSQR_PAIRS.items():
        seen = []
        for (lo, hi), nc, where in pairs:
            for n in range(lo, hi + 1):
                r = route(table, "Q", scalar=s, B=64, n_cap=n)
                rw = 32 if s == "f" and n <= 31 else 16
                assert r.startswith("tsqr NC=%d RW=%d tri=%s lds=" % (nc, rw, where)) and r.endswith(" nchunk=4 merge=1"), (s, n, r)
                scalar = 4 if s == "f" else 8
                tri = scalar * (6 * n + 1) * (6 * n + 2) // 2
                assert (" lds=%d " % (2048 + tri if where == "lds" else 2048)) in r and (2048 + tri <= 150 * 1024) == (where == "lds"), (s, n, r)
                seen.append(n)
        assert seen == list(range(1, 64))
    assert route(table, "Q", scalar="f", B=64, n_cap=45) == "tsqr NC=5 RW=16 tri=lds lds=149472 nchunk=4 merge=1"
    assert route(table, "Q", scalar="f", B=64, n_cap=46) == "tsqr NC=5 RW=16 tri=global lds=2048 nchunk=4 merge=1"
    assert route(table, "Q", scalar="d", B=64, n_cap=32) == "tsqr NC=4 RW=16 tri=lds lds=151816 nchunk=4 merge=1"
    assert route(table, "Q", scalar="d", B=64, n_cap=33) == "tsqr NC=4 RW=16 tri=global lds=2048 nchunk=4 merge=1"
    assert route(table, "Q", scalar="f", B=64, n_cap=31) == "tsqr NC=3 RW=32 tri=lds lds=72360 nchunk=4 merge=1"
    assert route(table, "Q", scalar="f", B=64, n_cap=32) == "tsqr NC=4 RW=16 tri=lds lds=76932 nchunk=4 merge=1"
    for s in "fd":
        for B, nchunk in ((1, 8), (32, 8), (33, 4), (64, 4), (65, 2), (128, 2), (129, 1), (130, 1)):
            assert route(table, "Q", scalar=s, B=B, n_cap=22).endswith(" nchunk=%d merge=%d" % (nchunk, 1 if nchunk > 1 else 0)), (s, B)


def test_handle_prints_the_tsqr_line_only_on_that_route(program):
    """--handle: the Q line with compress == 0 -- on request and by geometry (f_cap > 1024) -- and not on the information form"""
    args = lambda s, B, n_cap, f_cap, ov: ["--handle", s, str(B), "1", str(n_cap), str(f_cap), "30", "0", "2", "0", "84", str(ov), str(n_cap)]
    lines = lambda out: dict(line.split(" ", 1) for line in out.splitlines())
    assert lines(run(program, *args("d", 24, 32, 32, 0)))["Q"] == "tsqr NC=4 RW=16 tri=lds lds=151816 nchunk=8 merge=1"
    got = lines(run(program, *args("f", 2, 31, 1040, -1)))
    assert got["C"] == "compress=0 select tsqr" and got["Q"] == "tsqr NC=3 RW=32 tri=lds lds=72360 nchunk=8 merge=1" and got["F"].startswith("k_feature<0> ")
    assert lines(run(program, *args("f", 129, 30, 320, 0)))["Q"] == "tsqr NC=3 RW=32 tri=lds lds=67932 nchunk=1 merge=0"
    assert "Q" not in lines(run(program, *args("f", 2, 31, 1024, -1))) and "Q" not in lines(run(program, *args("d", 24, 32, 32, 3)))
