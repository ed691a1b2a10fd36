"""The frame step's launch order (msckf_mono_amd/csrc/frame_order.h) as a stand-alone host program: which frames of run_frames
enqueue the per-track kernel first and the selection beside propagate + augmentState in one launch, without a device.
Batch<S>::enqueue_frame carries the answer out and decides nothing itself."""
import os
import re
import subprocess

import pytest

import helpers as H

SRC = os.path.join(H.ROOT, "tests", "cpp", "frame_order_host.cpp")
CSRC = os.path.join(H.ROOT, "msckf_mono_amd", "csrc")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]}
DEFAULT = dict(setting=1, overlap=0, scalar="f", select_diag=1, qroute=0, first=0, prof=0)


@pytest.fixture(scope="module", params=list(FLAGS))
def table(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_order_" + request.param) / "frame_order_host")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + FLAGS[request.param] + ["-o", exe, SRC], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    rows = []
    for line in run.stdout.splitlines():
        left, right = line.split(" : ")
        tok = left.split()
        keys = dict(t.split("=") for t in tok[1:])
        order, ahead = right.split()
        rows.append((tok[0], {k: (v if k == "scalar" else int(v)) for k, v in keys.items()}, order, ahead.split("=")[1]))
    return rows


def decision(table, name, **keys):
    want = dict(DEFAULT, **keys)
    got = [(o, a) for n, k, o, a in table if n == name and k == want]
    assert len(got) == 1, (name, keys, got)
    return got[0]


def test_slices_that_take_the_feature_first_order(table):
    """windows one below the capacity, windows still filling, empty windows, slices without tracks, mixed sizes, one trajectory"""
    for name in ("steady", "filling", "empty_window", "no_tracks", "mixed_sizes", "single", "zero_samples"):
        assert decision(table, name) == ("feature_first", "feature_first"), name


def test_every_window_reason_keeps_the_whole_slice_on_the_old_order(table):
    assert decision(table, "full") == ("window_full", "window_full")
    assert decision(table, "one_full") == ("window_full", "window_full")               # one trajectory decides for the slice
    assert decision(table, "newest_seen") == ("newest_seen", "newest_seen")
    assert decision(table, "newest_seen_filling") == ("newest_seen", "newest_seen")
    assert decision(table, "skipped") == ("skipped", "skipped")
    assert decision(table, "mixed_refusals") == ("window_full", "window_full")         # the first trajectory that refuses names the reason


def test_refusals_of_the_handle_and_the_call(table):
    """the setting, the side-stream overlap, a double handle, the TSQR route, a range with both Q_imu forms, the call's first
    frame, the stage profile; the side stream's own question (ahead) knows only the last two"""
    assert decision(table, "steady", setting=0) == ("setting", "feature_first")
    assert decision(table, "steady", overlap=1) == ("setting", "feature_first")
    assert decision(table, "steady", scalar="d") == ("double", "feature_first")
    assert decision(table, "steady", select_diag=0) == ("route", "feature_first")
    assert decision(table, "steady", qroute=1) == ("route", "feature_first")
    assert decision(table, "steady", qroute=2) == ("feature_first", "feature_first")
    assert decision(table, "steady", first=1) == ("first_frame", "first_frame")
    assert decision(table, "steady", prof=1) == ("profile", "profile")
    assert decision(table, "steady", first=1, prof=1) == ("first_frame", "first_frame")
    assert decision(table, "steady", setting=0, scalar="d", select_diag=0, qroute=1, first=1, prof=1) == ("setting", "first_frame")
    assert decision(table, "newest_seen", scalar="d") == ("double", "newest_seen")


def test_the_frame_step_asks_the_header_and_keeps_no_loop_of_its_own():
    """enqueue_frame calls frame_order and feature_ahead; the rule's words (maxslot, the skip mark) stand in the header only"""
    text = open(os.path.join(CSRC, "msckf_hip.hip")).read()
    body = text[text.index("void enqueue_frame("):]
    body = body[:body.index("\n  // records [r0, r0 + n)")]
    assert body.count("routes::frame_order(") == 1 and body.count("routes::feature_ahead(") == 1
    assert not re.search(r"maxslot\[[^\]]*\]\s*(<=|>|<|>=)", body), "the frame step compares maxslot itself"
    header = open(os.path.join(CSRC, "frame_order.h")).read()
    assert "hip/" not in header and "hipStream" not in header
