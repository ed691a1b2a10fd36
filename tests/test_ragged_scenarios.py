"""The scenarios of tests/test_gpu_ragged.py are worth comparing: on the CPU oracle alone, every updating trajectory of the ragged
handles has measurement rows on every full-window frame, the special trajectories are what their kind says, and the lockstep
batches beyond 64 update on the frames that are compared.  No GPU needed."""
import numpy as np
import pytest

import helpers as H
from msckf_mono_amd import scenario as sc


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def _run(po, rs, b):
    o = rs.oracle(po, po.F64, b)
    longest, rows = 0, {}
    for k in range(rs.nf):
        rs.oracle_frame(o, b, k)
        fr = rs.frames[b][k]
        if len(fr["M"]):
            longest = max(longest, int(fr["M"].max()))
            rows[k] = o.lastStats()
    assert np.all(np.isfinite(o.getCovariance()))
    return longest, rows


@pytest.mark.parametrize("handle", [1, 2])
def test_every_ragged_trajectory_updates_on_the_oracle(po, handle):
    rs = H.RaggedSet(handle)
    assert rs.n_cap == max(rs.N) == rs.m_cap and rs.B % 8 != 0
    assert any(len({rs.full(b, k) for b in range(rs.B)}) == 2 for k in range(rs.nf))      # mixed drop flags on one frame
    kinds = [s[2] for s in rs.specs]
    assert sorted(k for k in kinds if k) == ["dense", "gaps", "gated", "idle"]
    assert {14, 15} <= set(rs.N)
    for b in range(rs.B):
        longest, rows = _run(po, rs, b)
        kind = kinds[b]
        if kind == "idle":
            assert not rows
            continue
        for k in range(rs.nf):
            if kind == "gated" and k == H.GATED_FRAME:
                assert rows[k]["n_tracks"] > 0 and rows[k]["n_passed"] == 0 and rows[k]["m_rows"] == 0, (b, rows[k])
            elif kind == "gaps" and k % 3 == 1:
                assert k not in rows
            elif rs.full(b, k):
                assert rows[k]["m_rows"] > 0 and rows[k]["n_passed"] > 0, (b, k, rows[k])
        if kind == "dense":
            assert longest == rs.m_cap, (b, longest)      # a track of m_cap observations: every camera of the full window
        assert len(rs.frames[b][H.GATED_FRAME]["M"]) > 0 or kind != "gated"


def test_the_ragged_batch_of_96_updates_on_the_oracle(po):
    Ns = [s[0] for s in H.RAGGED[1]["specs"][:7]]
    rs = H.RaggedSet(0, seed0=900, n_cap=32, specs=[(Ns[b % 7], 10 + (7 * b) % 31, "") for b in range(96)])
    for b in list(range(7)) + [95]:
        _, rows = _run(po, rs, b)
        assert all(rows[k]["m_rows"] > 0 for k in range(rs.nf) if rs.full(b, k)), b


@pytest.mark.parametrize("config,seed0,N,F,nf,last", [(3, 0, 30, 40, 33, (64, 95, 126, 127, 128, 159)), (2, 700, 12, 24, 18, (64, 128, 129)), (2, 700, 20, 24, 26, (64, 128, 129))])
def test_the_lockstep_batches_update_on_their_compared_frame(po, config, seed0, N, F, nf, last):
    """the trajectories the GPU module samples at every batch size, and the last one of each batch size"""
    for b in (0, 7, 13, 21, 30, 42, 63) + last:
        tr = sc.Trajectory(config, seed0 + b, N, F, nf)
        o = po.Oracle(po.F64, po.LEAN)
        o.initialize(tr.cfg, tr.imu0)
        for k in range(nf):
            H.oracle_frame(o, tr, k, N)
        s = o.lastStats()
        assert s["m_rows"] > 0 and s["n_passed"] > 0, (b, s)
