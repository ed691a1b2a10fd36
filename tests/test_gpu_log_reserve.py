"""The head of run_frames / run_frames_streamed reserves the three device logs in the order frame, map, pruned, before
anything is enqueued: a call that the frame log refuses leaves the other two logs, their cursors and the filter as they
were, and the same call after frame_log_reset continues the map and pruned-state logs as if nothing had happened."""
import numpy as np
import pytest

from test_gpu_configs import _snapshot
from test_gpu_pruned_log import CAP, SMALL, _dtype, _small_drops, _staged, capi, small_trajs  # noqa: F401  (the pruned log's small fixture)

pytestmark = pytest.mark.gpu

CUT = 9                                             # the window is full from frame 7 on: both cuts drop states


def _all_on(capi, trajs, name, frame_cap):
    g = SMALL
    bt = _staged(capi, trajs, name, g, _small_drops(trajs), streams=2)
    bt.frame_log_enable(frame_cap); bt.map_log_enable(g["nf"] * g["F"]); bt.pruned_log_enable(CAP)
    return bt


def _log_state(bt):
    return (bt.frame_log_count(), bt.map_log_frames(), bt.pruned_log_frames(),
            [x.tolist() for x in bt.map_log_counts()], [x.tolist() for x in bt.pruned_log_counts()])


def _records(bt, B):
    return [(bt.map_log_read(b)[0], bt.pruned_log_read(b)[0], bt.pruned_log_read(b)[2]) for b in range(B)]


@pytest.mark.parametrize("dtype_name", ["f32", "f64"])
def test_a_call_the_frame_log_refuses_leaves_the_other_logs_and_the_filter_alone(capi, small_trajs, dtype_name):
    """All three logs on, the frame log one frame short of the two cuts [0, 9) and [9, 17).  The second cut is refused with
    -ENOSPC by run_frames and by run_frames_streamed: record counts, frame ordinals, cursors, IMU state, camera states,
    covariance and window sizes are what they were after the first cut, bit for bit.  After frame_log_reset it runs, and
    the map and pruned-state records of the two cuts are the bits of one handle that ran all frames in one call with a
    frame log large enough."""
    g = SMALL
    nf, B = g["nf"], g["B"]
    bt = _all_on(capi, small_trajs, dtype_name, nf - 1)
    bt.run_frames(0, CUT); bt.sync()
    logs, state, ncam = _log_state(bt), _snapshot(bt, B), [bt.num_cam_states(b) for b in range(B)]
    assert logs[:3] == (CUT, CUT, CUT) and all(n > 0 for n in logs[3][1]) and logs[4][1] == [CUT - 7] * B
    for run in (bt.run_frames, bt.run_frames_streamed):
        with pytest.raises(capi.HipError, match=r"\(-28\)"):
            run(CUT, nf)
        bt.sync()
        assert _log_state(bt) == logs, run.__name__
        assert [bt.num_cam_states(b) for b in range(B)] == ncam, run.__name__
        for b, (got, want) in enumerate(zip(_snapshot(bt, B), state)):
            for x, y in zip(got, want):
                assert np.array_equal(x, y), (run.__name__, b)
    bt.frame_log_reset()
    bt.run_frames(CUT, nf); bt.sync()
    assert _log_state(bt)[:3] == (nf - CUT, nf, nf)
    got, counts = _records(bt, B), _log_state(bt)[3:]
    bt.close()

    whole = _all_on(capi, small_trajs, dtype_name, nf)
    whole.run_frames(0, nf); whole.sync()
    assert _log_state(whole)[:3] == (nf, nf, nf) and _log_state(whole)[3:] == counts
    want = _records(whole, B)
    whole.close()
    for b in range(B):
        assert len(want[b][1]) == 12 and np.any(want[b][0][:, 4] >= CUT)      # both cuts left map and pruned records
        for x, y, what in zip(got[b], want[b], ("map records", "pruned records", "augment ordinals")):
            assert x.shape == y.shape and np.array_equal(x, y), (b, what)
