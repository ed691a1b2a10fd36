// nees_plan_host.cpp -- msckf_mono_amd/csrc/nees_plan.h on its own, with a host compiler (tests/test_nees_inputs.py builds and
// runs this, once more under the address and undefined-behaviour sanitizers): the strides and the column table, and every
// refusal of msckf_hip_truth_set, of the reserve at the head of a frame loop, of the read and of the ensemble reduction with its
// code, its text and its place in the order.  "--columns" prints the column table.  Exit code 0 and "nees plan ok" when
// everything holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../msckf_mono_amd/csrc/nees_plan.h"

using namespace msckf_nees;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool is(const Refusal& r, int code, const char* part) { return r.code == code && (code == 0 ? r.why == nullptr : (r.why && std::strstr(r.why, part))); }

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--columns")) {
    std::printf("record %d nees %d blocks %d frame %d flags %d\n", REC, REC_NEES, REC_BLK, REC_FRAME, REC_FLAGS);
    std::printf("flag not_pd %d skipped %d stat_err %d\n", FLAG_NOT_PD, FLAG_SKIPPED, FLAG_STAT_ERR);
    std::printf("ensemble %d n %d flagged %d sum %d sum_sq %d\n", ENS, ENS_N, ENS_FLAGGED, ENS_SUM, ENS_SUMSQ);
    std::printf("truth %d walk %d\n", TRUTH_ROW, WALK_ROW);
    return 0;
  }
  // strides: a record's six NEES columns are the whole state and its five blocks; an ensemble row is two counts and twice those six
  CHECK(NX == 3 * NBLK && REC_BLK + NBLK == REC_FRAME && REC_FLAGS == REC - 1);
  CHECK(ENS_SUM + REC_FRAME == ENS_SUMSQ && ENS_SUMSQ + REC_FRAME == ENS);
  CHECK(truth_at(0, 0, 3) == 0 && truth_at(2, 1, 3) == (size_t)(2 * 3 + 1) * 16);
  CHECK(record_at(3, 2, 5) == (size_t)(3 * 5 + 2) * 8 && ensemble_at(3, 1, 4) == (size_t)(3 * 4 + 1) * 14);

  // ---- msckf_hip_truth_set
  const int B = 3, frames = 2, rows = 2;
  std::vector<double> t((size_t)frames * rows * TRUTH_ROW, 0.25);
  for (int i = 0; i < frames * rows; ++i) { double* q = &t[(size_t)i * TRUTH_ROW]; q[0] = 0.5; q[1] = -0.5; q[2] = 0.5; q[3] = 0.5; }
  const int row_of[B] = {1, 0, 1};
  CHECK(is(truth_refusal(frames, rows, t.data(), row_of, B, 0, false), 0, ""));
  CHECK(is(truth_refusal(frames, rows, t.data(), row_of, B, 1, true), 0, ""));
  CHECK(is(truth_refusal(0, 0, nullptr, nullptr, B, 0, false), 0, ""));                  // frees the table: nothing else is looked at
  CHECK(is(truth_refusal(-1, rows, t.data(), row_of, B, 0, false), -EINVAL, "negative frame count"));
  CHECK(is(truth_refusal(frames, 0, t.data(), row_of, B, 0, false), -EINVAL, "n_rows > 0"));
  CHECK(is(truth_refusal(frames, rows, nullptr, row_of, B, 0, false), -EINVAL, "are needed"));
  CHECK(is(truth_refusal(frames, rows, t.data(), row_of, B, 2, true), -EINVAL, "add_walk is 0 or 1"));
  CHECK(is(truth_refusal(frames, rows, t.data(), row_of, B, 1, false), -EINVAL, "msckf_hip_replay_assign_q"));
  { const int bad[B] = {1, 2, 0}; CHECK(is(truth_refusal(frames, rows, t.data(), bad, B, 0, false), -EINVAL, "row_of names no row")); }
  { const int bad[B] = {-1, 0, 0}; CHECK(is(truth_refusal(frames, rows, t.data(), bad, B, 0, false), -EINVAL, "row_of names no row")); }
  {
    std::vector<double> u = t;
    u[truth_at(1, 1, rows) + 9] = std::numeric_limits<double>::quiet_NaN();
    CHECK(is(truth_refusal(frames, rows, u.data(), row_of, B, 0, false), -EINVAL, "entry not finite"));
    u[truth_at(1, 1, rows) + 9] = std::numeric_limits<double>::infinity();
    CHECK(is(truth_refusal(frames, rows, u.data(), row_of, B, 0, false), -EINVAL, "entry not finite"));
    const int bad[B] = {5, 0, 0};                                                          // the order: row_of before the entries
    CHECK(is(truth_refusal(frames, rows, u.data(), bad, B, 0, false), -EINVAL, "row_of names no row"));
  }
  {
    std::vector<double> u = t;
    u[truth_at(1, 0, rows)] = 0.5 + 3e-6;                                                   // norm off by 1.5e-6
    CHECK(is(truth_refusal(frames, rows, u.data(), row_of, B, 0, false), -EINVAL, "quaternion norm"));
    u[truth_at(1, 0, rows)] = 0.5 + 1e-6;                                                   // off by 5e-7: accepted
    CHECK(is(truth_refusal(frames, rows, u.data(), row_of, B, 0, false), 0, ""));
    u[truth_at(1, 0, rows)] = 0.5 + 3e-6; u[5] = std::numeric_limits<double>::infinity();   // the order: finite before the norm
    CHECK(is(truth_refusal(frames, rows, u.data(), row_of, B, 0, false), -EINVAL, "entry not finite"));
  }

  // ---- the reserve: no table, a table too short, the walk outside the replay's loop, the capacity -- in this order
  CHECK(is(reserve_refusal(0, 5, 5, 0, false, false, 0, 5), 0, ""));
  CHECK(is(reserve_refusal(0, 5, 5, 1, true, true, 0, 5), 0, ""));
  CHECK(is(reserve_refusal(3, 3, 5, 0, false, false, 5, 5), 0, ""));                        // an empty range needs no room
  CHECK(is(reserve_refusal(0, 5, 0, 0, false, false, 0, 1), -EINVAL, "without a truth table"));
  CHECK(is(reserve_refusal(0, 6, 5, 0, false, false, 0, 1), -EINVAL, "does not cover"));
  CHECK(is(reserve_refusal(0, 5, 5, 1, false, true, 0, 1), -EINVAL, "only msckf_hip_run_frames_replay"));
  CHECK(is(reserve_refusal(0, 5, 5, 1, true, false, 0, 1), -EINVAL, "no msckf_hip_replay_assign_q assignment"));
  CHECK(is(reserve_refusal(0, 5, 5, 0, false, false, 1, 5), -ENOSPC, "NEES log full"));
  CHECK(is(reserve_refusal(2, 5, 5, 0, false, false, 2, 5), 0, ""));
  CHECK(is(reserve_refusal(2, 5, 5, 0, false, false, 3, 5), -ENOSPC, "NEES log full"));
  CHECK(is(reserve_refusal(0, 2, 5, 0, false, false, 2147483647, 2147483647), -ENOSPC, "NEES log full"));   // no overflow of the sum

  // ---- read and ensemble
  CHECK(is(read_refusal(0, 4, 4), 0, "") && is(read_refusal(4, 0, 4), 0, ""));
  CHECK(is(read_refusal(-1, 1, 4), -EINVAL, "record range") && is(read_refusal(2, 3, 4), -EINVAL, "record range") && is(read_refusal(0, -1, 4), -EINVAL, "record range"));
  CHECK(is(read_refusal(2147483647, 2147483647, 4), -EINVAL, "record range"));
  const int groups[B] = {0, -1, 1};
  CHECK(is(ensemble_refusal(0, 4, 4, groups, B, 2), 0, "") && is(ensemble_refusal(2, 2, 4, groups, B, 3), 0, ""));
  CHECK(is(ensemble_refusal(0, 5, 4, groups, B, 2), -EINVAL, "record range") && is(ensemble_refusal(3, 2, 4, groups, B, 2), -EINVAL, "record range"));
  CHECK(is(ensemble_refusal(0, 4, 4, groups, B, 0), -EINVAL, "at least one group"));
  CHECK(is(ensemble_refusal(0, 4, 4, groups, B, 1), -EINVAL, "group_of outside"));
  { const int bad[B] = {0, -2, 1}; CHECK(is(ensemble_refusal(0, 4, 4, bad, B, 2), -EINVAL, "group_of outside")); }

  if (failures) return 1;
  std::printf("nees plan ok\n");
  return 0;
}
