// slice_policy.h -- how many slices of the batch a frame loop runs side by side, stated once and free of device calls.
//
// run_frames / run_frames_streamed cut the batch into slices, each with a stream and an enqueue thread of its own
// (msckf_hip.hip, "the frame loop of a scenario").  The HIP runtime deals a process's streams onto at most GPU_MAX_HW_QUEUES
// hardware queues (4 unless the variable says otherwise), and a hardware queue runs its packets in order: two slices on one
// queue run one after the other, which is SLOWER than one slice (each slice's chain of launches is latency-bound and does not
// shrink with the slice: cfg3, 4 slices on 3 queues 123 k updates/s, 1 slice 188 k; profiles/hw_queue_slices.md).  So the
// count msckf_hip_set_streams asks for is an upper bound, and the handle runs as many slices as have queues of their own.
// BatchCore::n_slices() is a call of effective_slices() and nothing else decides the count.  No HIP header, no heap, no lock:
// a host compiler accepts this file on its own (tests/cpp/slice_policy_host.cpp).
#ifndef MSCKF_SLICE_POLICY_H
#define MSCKF_SLICE_POLICY_H

#include <cstdlib>

namespace msckf {
namespace slices {

constexpr int HW_QUEUES_DEFAULT = 4;    // the runtime's own default where GPU_MAX_HW_QUEUES is not set
constexpr int HW_QUEUES_MAX = 32;
constexpr int SLICES_MAX = 8;           // BatchCore::MAXS

// The text of GPU_MAX_HW_QUEUES: unset, empty or no number -> the runtime's default; a number is clamped to 1 .. 32
// ("0" -> 1, "99" -> 32).
inline int parse_hw_queue_budget(const char* text) {
  if (!text || !*text) return HW_QUEUES_DEFAULT;
  char* end = nullptr;
  const long v = strtol(text, &end, 10);   // (out of range: LONG_MIN / LONG_MAX, clamped like any number)
  if (end == text) return HW_QUEUES_DEFAULT;
  return v < 1 ? 1 : v > HW_QUEUES_MAX ? HW_QUEUES_MAX : (int)v;
}
// The library itself neither reads nor sets the variable (settings.h's table names every variable it reads): a handle starts
// with the runtime's default and its caller says what the process has (msckf_hip_set_hw_queues; capi.Batch passes the
// variable's text on when it creates a handle).

// One queue of the budget is not the handle's: the process's default stream (the host framework's work, the device set-up)
// holds it, and the runtime puts none of the handle's streams beside it while another queue has a single stream -- at a
// budget of 4 the fourth slice's stream lands on the third slice's queue, resident inputs or streamed
// (profiles/hw_queue_slices.md, "placement").  What is left is the budget effective_slices() is asked with.
constexpr int QUEUES_HELD_BY_PROCESS = 1;
inline int handle_queue_budget(int process_budget) { return process_budget - QUEUES_HELD_BY_PROCESS < 1 ? 1 : process_budget - QUEUES_HELD_BY_PROCESS; }

// Best slice count on `budget` queues where the requested count does not fit, cfg3 (64 trajectories) on MI355X, k updates/s
// (profiles/hw_queue_slices.md; the same at a budget of 4 and of 8 wherever no two slices share a queue):
//     slices           1       2       3       4
//     streamed     187.8   205.2   194.9   205.0
//     resident     192.4   211.1   201.7   209.5
// Two slices beat three, and four only equal two: with fewer than four queues the answer is 2 (1 on a single queue).  From four
// queues on it is 4 -- counts beyond 4 are not measured on this code and are only run where they fit (below).  Streamed and
// resident runs agree; the rows are kept apart because they are measured apart.  Index: queues, 0 unused.
constexpr int BEST_STREAMED[SLICES_MAX + 1] = {1, 1, 2, 2, 4, 4, 4, 4, 4};
constexpr int BEST_RESIDENT[SLICES_MAX + 1] = {1, 1, 2, 2, 4, 4, 4, 4, 4};

// The slices a frame loop really runs.  requested: msckf_hip_set_streams (an upper bound); B: trajectories; budget: queues the
// handle may fill; streamed: run_frames_streamed (its copy stream wants a queue too); exact: msckf_hip_set_slices_exact (the
// requested count whatever the budget, for A/B runs); profiling: the stage timers force a single stream.
// With budget >= requested + streamed the answer is min(requested, B), as it was before there was a policy.
inline int effective_slices(int requested, int B, int budget, bool streamed, bool exact = false, bool profiling = false) {
  if (profiling) return 1;
  const int fit = requested < B ? requested : B, base = fit < 1 ? 1 : fit;
  if (exact || budget >= requested + (streamed ? 1 : 0)) return base;
  const int q = budget < 1 ? 1 : budget > SLICES_MAX ? SLICES_MAX : budget;
  const int best = streamed ? BEST_STREAMED[q] : BEST_RESIDENT[q];
  return best < base ? best : base;
}

}  // namespace slices
}  // namespace msckf
#endif
