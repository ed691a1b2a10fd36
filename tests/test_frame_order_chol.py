"""The frame step's order 2 (routes::frame_order_chol, msckf_mono_amd/csrc/frame_order.h) as a stand-alone host program: which
frames of run_frames put propagate + augmentState into the Gram Cholesky's launch, without a device.  The program feeds the rule
from the same pure functions the frame step asks (frame_order, compress_route, small_route), over a grid of slices and handles."""
import os
import subprocess

import pytest

import helpers as H

SRC = os.path.join(H.ROOT, "tests", "cpp", "frame_order_chol_host.cpp")
CSRC = os.path.join(H.ROOT, "msckf_mono_amd", "csrc")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]}
DEFAULT = dict(setting=2, scalar="f", n_cap=30, small=84, route=-1, n_lit=0, first=0)
CHAIN_ONLY, SMALL_ONLY, SMALL_AND_CHAIN = 0, 1, 2


@pytest.fixture(scope="module", params=list(FLAGS))
def table(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_order_chol_" + request.param) / "frame_order_chol_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[request.param] + ["-o", exe, SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    rows = []
    for line in run.stdout.splitlines():
        left, right = line.split(" : ")
        tok = left.split()
        keys = {k: (v if k == "scalar" else int(v)) for k, v in (t.split("=") for t in tok[1:])}
        seen = {k: keys.pop(k) for k in ("blocks", "levels", "kind")}
        order1, decision = right.split()
        rows.append((tok[0], keys, seen, order1, decision))
    return rows


def row(table, name, **keys):
    want = dict(DEFAULT, **keys)
    got = [(s, o, d) for n, k, s, o, d in table if n == name and k == want]
    assert len(got) == 1, (name, keys, got)
    return got[0]


def test_the_three_joint_instances_and_the_two_level_factorization(table):
    """4, 8 and 12 column blocks take order 2 on a steady slice whose windows are the chain's; 40- and 60-camera handles
    factor in two levels and keep order 1"""
    for n_cap, small, blocks in ((30, 84, 12), (14, 60, 8), (14, 84, 8), (10, 0, 4)):
        seen, order1, decision = row(table, "steady", n_cap=n_cap, small=small)
        assert (seen["blocks"], seen["levels"], seen["kind"], order1, decision) == (blocks, 1, CHAIN_ONLY, "feature_first", "in_cholesky"), n_cap
    for n_cap in (40, 60):
        seen, order1, decision = row(table, "steady", n_cap=n_cap)
        assert (seen["levels"], order1, decision) == (2, "feature_first", "chol_levels"), n_cap


def test_the_window_fill_and_a_mixed_slice_keep_order_one(table):
    """up to 12 cameras (72 columns, what fits of the 84 asked for) the update is k_update_small's; 13 cameras are the chain's; a
    slice with windows on both sides launches both and keeps order 1; so does an all-small 10-camera handle; with the small update
    off the same mixed slice takes order 2"""
    assert row(table, "fill_small") == (dict(blocks=12, levels=1, kind=SMALL_ONLY), "feature_first", "small_update")
    assert row(table, "fill_edge") == (dict(blocks=12, levels=1, kind=SMALL_ONLY), "feature_first", "small_update")
    assert row(table, "fill_over") == (dict(blocks=12, levels=1, kind=CHAIN_ONLY), "feature_first", "in_cholesky")
    assert row(table, "mixed") == (dict(blocks=12, levels=1, kind=SMALL_AND_CHAIN), "feature_first", "small_update")
    assert row(table, "mixed", small=0) == (dict(blocks=12, levels=1, kind=CHAIN_ONLY), "feature_first", "in_cholesky")
    assert row(table, "steady", n_cap=10) == (dict(blocks=4, levels=1, kind=SMALL_ONLY), "feature_first", "small_update")
    # windows that are empty before the frame hold one camera state when the update runs: k_update_small's
    assert row(table, "empty")[1:] == ("feature_first", "small_update")


def test_a_frame_that_refuses_order_one_refuses_order_two(table):
    for name, why in (("newest_seen", "newest_seen"), ("skipped", "skipped"), ("full", "window_full")):
        assert row(table, name)[1:] == (why, "order1_refused"), name
    assert row(table, "steady", first=1)[1:] == ("first_frame", "order1_refused")
    assert row(table, "steady", scalar="d")[1:] == ("double", "order1_refused")
    seen, order1, decision = row(table, "steady", route=0)      # Householder TSQR: no selection launch of that kind, no Cholesky
    assert (seen["levels"], order1, decision) == (0, "route", "order1_refused")


def test_the_setting_and_the_literal_route(table):
    assert row(table, "steady", setting=1)[1:] == ("feature_first", "setting")
    assert row(table, "steady", setting=0)[1:] == ("setting", "setting")
    assert row(table, "steady", n_lit=1)[1:] == ("feature_first", "literal")
    assert row(table, "steady", n_lit=1, route=0)[1:] == ("feature_first", "literal")   # the literal route brings the information form back


def test_the_frame_step_asks_the_header(table):
    """enqueue_frame asks frame_order_chol once and hands launch_update the answer; the header stays free of device calls"""
    text = open(os.path.join(CSRC, "msckf_hip.hip")).read()
    body = text[text.rindex("void enqueue_frame("):]
    body = body[:body.index("\n  // records [r0, r0 + n)")]
    assert text.count("routes::frame_order_chol(") == 1 and body.count("routes::frame_order_chol(") == 1
    assert body.count("range_small_route(") == 1 and body.count("launch_update(") == 1
    header = open(os.path.join(CSRC, "frame_order.h")).read()
    assert "hip/" not in header and "hipStream" not in header
