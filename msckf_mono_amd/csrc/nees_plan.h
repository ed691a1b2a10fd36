// nees_plan.h -- the host side of the full-state NEES log (msckf_hip_truth_set, msckf_hip_nees_log_*; kernels_log.hip:
// k_nees_log, k_nees_ensemble), free of device calls.
//
// Stated once here:
//   1. the strides    a truth row (the first 16 entries of the IMU state layout, doubles), a record (8 doubles whatever the
//                     handle's dtype), a row of the ensemble reduction (14 doubles), a walk row (6 doubles)
//   2. the columns    of a record and of an ensemble row, and the flag bits
//   3. the checks     of msckf_hip_truth_set's arguments, of the reserve at the head of a frame loop and of
//                     msckf_hip_nees_log_read / _ensemble, each refusal with its code and text
// No HIP header, no batch type: a host compiler accepts this file on its own (tests/cpp/nees_plan_host.cpp).
#ifndef MSCKF_NEES_PLAN_H
#define MSCKF_NEES_PLAN_H

#include <cerrno>
#include <cmath>
#include <cstddef>

#include "input_layouts.h"

namespace msckf_nees {

using msckf_inputs::Refusal;

// ---- 1. strides
constexpr int TRUTH_ROW = 16;   // q_IG(w x y z) b_g v b_a p: imu[0..15]
constexpr int REC = 8;          // one record per frame and trajectory
constexpr int ENS = 14;         // one row per (record, group)
constexpr int WALK_ROW = 6;     // a row of the replay's walk table: gyro, then accelerometer bias offset
constexpr int NX = 15;          // the IMU error state: theta b_g v b_a p, in P's own order
constexpr int NBLK = 5;         // its 3 x 3 diagonal blocks

// ---- 2. columns
// record: NEES of the whole 15-state, then of the blocks theta, b_g, v, b_a, p; the frame index; the flags
enum RecCol { REC_NEES = 0, REC_BLK = 1, REC_FRAME = 6, REC_FLAGS = 7 };
// flags: a diagonal entry or a pivot was not positive (columns 0..5 are 0) | the cell was skipped (columns 0..5 are 0) |
// STAT_ERR is set (the columns are computed all the same)
enum Flag { FLAG_NOT_PD = 1, FLAG_SKIPPED = 2, FLAG_STAT_ERR = 4 };
// ensemble row: members with flags == 0, members left out for a flag, the sums of columns 0..5 over the former, the sums of
// their squares
enum EnsCol { ENS_N = 0, ENS_FLAGGED = 1, ENS_SUM = 2, ENS_SUMSQ = 8 };
constexpr double QUAT_NORM_TOL = 1e-6;

inline size_t truth_at(int f, int row, int n_rows) { return ((size_t)f * n_rows + row) * TRUTH_ROW; }
inline size_t record_at(int r, int b, int B) { return ((size_t)r * B + b) * REC; }
inline size_t ensemble_at(int r, int g, int n_groups) { return ((size_t)r * n_groups + g) * ENS; }

// ---- 3. checks
// msckf_hip_truth_set (n_frames == 0 frees the table: nothing else is looked at).  model_q: a replay_assign_q assignment is in force
inline Refusal truth_refusal(int n_frames, int n_rows, const double* truth16, const int* row_of, int B, int add_walk, bool model_q) {
  if (n_frames < 0) return {-EINVAL, "truth table: negative frame count"};
  if (n_frames == 0) return {0, nullptr};
  if (n_rows <= 0 || !truth16 || !row_of) return {-EINVAL, "truth table: n_rows > 0, truth16 and row_of are needed"};
  if (add_walk != 0 && add_walk != 1) return {-EINVAL, "truth table: add_walk is 0 or 1"};
  if (add_walk && !model_q) return {-EINVAL, "truth table: add_walk needs an assignment through msckf_hip_replay_assign_q"};
  for (int b = 0; b < B; ++b) if (row_of[b] < 0 || row_of[b] >= n_rows) return {-EINVAL, "truth table: row_of names no row of the table"};
  const size_t n = (size_t)n_frames * n_rows;
  for (size_t i = 0; i < n * TRUTH_ROW; ++i) if (!std::isfinite(truth16[i])) return {-EINVAL, "truth table: entry not finite"};
  for (size_t i = 0; i < n; ++i) {
    const double* q = truth16 + i * TRUTH_ROW;
    const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (std::fabs(nrm - 1.0) > QUAT_NORM_TOL) return {-EINVAL, "truth table: quaternion norm off by more than 1e-6"};
  }
  return {0, nullptr};
}
// head of a frame loop over [f0, f1) while the log is on (fourth, after the frame, map and pruned-state logs): the truth table
// covers the range, its walk is only asked of the replay's loop, the records fit behind the `count` written
inline Refusal reserve_refusal(int f0, int f1, int truth_frames, int add_walk, bool replay_loop, bool model_q, int count, int cap) {
  if (truth_frames <= 0) return {-EINVAL, "NEES log on without a truth table (msckf_hip_truth_set); nothing was run"};
  if (f0 < 0 || f1 > truth_frames) return {-EINVAL, "NEES log: the truth table does not cover the call's frames; nothing was run"};
  if (add_walk && !replay_loop) return {-EINVAL, "NEES log: the truth table adds the replay's walk, only msckf_hip_run_frames_replay honours it; nothing was run"};
  if (add_walk && !model_q) return {-EINVAL, "NEES log: the truth table adds the replay's walk, but no msckf_hip_replay_assign_q assignment is in force; nothing was run"};
  if ((long)count + (f1 - f0) > cap) return {-ENOSPC, "NEES log full: the call's frames do not fit behind the records written (msckf_hip_nees_log_reset, or a larger msckf_hip_nees_log_enable); nothing was run"};
  return {0, nullptr};
}
inline Refusal read_refusal(int r0, int n, int count) {
  if (r0 < 0 || n < 0 || (long)r0 + n > count) return {-EINVAL, "record range beyond the records written (msckf_hip_nees_log_count)"};
  return {0, nullptr};
}
inline Refusal ensemble_refusal(int r0, int r1, int count, const int* group_of, int B, int n_groups) {
  if (r0 < 0 || r1 < r0 || r1 > count) return {-EINVAL, "record range beyond the records written (msckf_hip_nees_log_count)"};
  if (n_groups < 1) return {-EINVAL, "NEES ensemble: at least one group"};
  for (int b = 0; b < B; ++b) if (group_of[b] < -1 || group_of[b] >= n_groups) return {-EINVAL, "NEES ensemble: group_of outside [-1, n_groups)"};
  return {0, nullptr};
}

}  // namespace msckf_nees
#endif
