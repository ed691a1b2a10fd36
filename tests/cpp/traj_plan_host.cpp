// traj_plan_host.cpp -- msckf_mono_amd/csrc/traj_plan.h on its own, with a host compiler (tests/test_traj_inputs.py builds and
// runs this, once more under the address and undefined-behaviour sanitizers).
//   (no argument)  the strides, and every refusal of the four calls with its code, its text and its place in the order; exit code
//                  0 and "traj plan ok" when everything holds
//   --columns      the column table
//   --close        the closing maths: reads lines "mode n pbar[3] gbar[3] S[9] pp gg pxy gxy" from standard input and prints for
//                  each "R[9] t[3] cond q[4]", 17 significant digits -- the text k_traj_align runs in registers
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../msckf_mono_amd/csrc/traj_plan.h"

using namespace msckf_traj;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool is(const Refusal& r, int code, const char* part) { return r.code == code && (code == 0 ? r.why == nullptr : (r.why && std::strstr(r.why, part))); }

static int close_lines() {
  for (;;) {
    int mode; double n, pbar[3], gbar[3]; Centred c;
    if (std::scanf("%d %lf", &mode, &n) != 2) return 0;
    for (double& x : pbar) if (std::scanf("%lf", &x) != 1) return 1;
    for (double& x : gbar) if (std::scanf("%lf", &x) != 1) return 1;
    for (double& x : c.S) if (std::scanf("%lf", &x) != 1) return 1;
    if (std::scanf("%lf %lf %lf %lf", &c.pp, &c.gg, &c.pxy, &c.gxy) != 4) return 1;
    Alignment a;
    close_alignment(mode, n, pbar, gbar, c, a);
    for (double x : a.R) std::printf("%.17g ", x);
    for (double x : a.t) std::printf("%.17g ", x);
    std::printf("%.17g", a.cond);
    for (double x : a.q) std::printf(" %.17g", x);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--columns")) {
    std::printf("align %d n %d R %d t %d cond %d sum_sq %d max %d last %d sum_sq_ang %d max_ang %d raw %d\n", ALIGN_ROW, AL_N, AL_R, AL_T, AL_COND,
                AL_SUM_SQ, AL_MAX, AL_LAST, AL_SUM_SQ_ANG, AL_MAX_ANG, AL_SUM_SQ_RAW);
    std::printf("rpe %d pairs %d sum_sq %d sum_sq_ang %d max %d max_lags %d\n", RPE_ROW, RPE_PAIRS, RPE_SUM_SQ, RPE_SUM_SQ_ANG, RPE_MAX, RPE_MAX_LAGS);
    std::printf("mode none %d yaw %d se3 %d pose %d\n", ALIGN_NONE, ALIGN_YAW, ALIGN_SE3, POSE);
    return 0;
  }
  if (argc > 1 && !std::strcmp(argv[1], "--close")) return close_lines();

  // strides
  CHECK(ALIGN_ROW == 20 && RPE_ROW == 4 && RPE_MAX_LAGS == 8 && POSE == 7);
  CHECK(AL_R + 9 == AL_T && AL_T + 3 == AL_COND && AL_SUM_SQ_RAW == ALIGN_ROW - 1 && RPE_MAX == RPE_ROW - 1);
  CHECK(pose_at(0, 0, 3) == 0 && pose_at(2, 1, 3) == (size_t)(2 * 3 + 1) * 7);

  // ---- the checks one by one
  const int nt = 3, r0 = 2, r1 = 6;
  std::vector<double> gt((size_t)(r1 - r0) * nt * POSE, 0.25);
  for (int i = 0; i < (r1 - r0) * nt; ++i) { double* q = &gt[(size_t)i * POSE]; q[0] = 0.5; q[1] = -0.5; q[2] = 0.5; q[3] = 0.5; }
  double out[1]; int dummy = 0;
  CHECK(is(pointer_refusal({&dummy, gt.data(), out}), 0, "") && is(pointer_refusal({&dummy, gt.data(), gt.data(), &dummy, out}), 0, ""));
  CHECK(is(pointer_refusal({nullptr, gt.data(), out}), -EINVAL, "null argument") && is(pointer_refusal({&dummy, nullptr, out}), -EINVAL, "null argument") &&
        is(pointer_refusal({&dummy, gt.data(), &dummy, nullptr}), -EINVAL, "null argument"));
  CHECK(is(mode_refusal(0), 0, "") && is(mode_refusal(1), 0, "") && is(mode_refusal(2), 0, ""));
  CHECK(is(mode_refusal(-1), -EINVAL, "mode is 0") && is(mode_refusal(3), -EINVAL, "mode is 0"));
  { const int ok[8] = {1, 2, 5, 64, 200, 1, 1, 2147483647}; CHECK(is(lags_refusal(ok, 8), 0, "") && is(lags_refusal(ok, 1), 0, ""));
    CHECK(is(lags_refusal(nullptr, 1), -EINVAL, "null argument"));
    CHECK(is(lags_refusal(ok, 0), -EINVAL, "between 1 and 8 lags") && is(lags_refusal(ok, 9), -EINVAL, "between 1 and 8 lags"));
    const int bad[3] = {1, 0, 2}; CHECK(is(lags_refusal(bad, 3), -EINVAL, "at least 1 record") && is(lags_refusal(bad, 1), 0, ""));
    const int neg[1] = {-4}; CHECK(is(lags_refusal(neg, 1), -EINVAL, "at least 1 record")); }
  const int a0[nt] = {2, 3, 6}, a1[nt] = {6, 3, 6};
  CHECK(is(ranges_refusal(r0, r1, nullptr, nullptr, nt), 0, "") && is(ranges_refusal(r0, r1, a0, a1, nt), 0, ""));
  CHECK(is(ranges_refusal(r0, r1, a0, nullptr, nt), -EINVAL, "both or neither") && is(ranges_refusal(r0, r1, nullptr, a1, nt), -EINVAL, "both or neither"));
  { const int b0[nt] = {1, 3, 6}; CHECK(is(ranges_refusal(r0, r1, b0, a1, nt), -EINVAL, "outside [r0, r1)")); }
  { const int b1[nt] = {6, 3, 7}; CHECK(is(ranges_refusal(r0, r1, a0, b1, nt), -EINVAL, "outside [r0, r1)")); }
  { const int b1[nt] = {6, 2, 6}; CHECK(is(ranges_refusal(r0, r1, a0, b1, nt), -EINVAL, "outside [r0, r1)")); }      // ends before it starts
  CHECK(is(gt_refusal(gt.data(), gt.size() / POSE), 0, "") && is(gt_refusal(nullptr, 0), 0, ""));
  CHECK(is(shape_refusal(0, 1), 0, "") && is(shape_refusal(-1, 1), -EINVAL, "pose arrays") && is(shape_refusal(4, 0), -EINVAL, "pose arrays"));

  // ---- the order: mode (or lags), the pair of ranges, the ranges, finite, the norm
  const int lags[2] = {1, 3}, bad_lags[2] = {1, 0}, out_of[nt] = {6, 3, 9};
  std::vector<double> nan_gt = gt, off_gt = gt;
  nan_gt[pose_at(1, 2, nt) + 5] = std::numeric_limits<double>::quiet_NaN();
  nan_gt[pose_at(3, 0, nt)] = 0.5 + 3e-6;                                                  // (and a norm that is off: finite comes first)
  off_gt[pose_at(3, 0, nt)] = 0.5 + 3e-6;                                                  // norm off by 1.5e-6
  CHECK(is(align_refusal(r0, r1, a0, a1, nt, gt.data(), ALIGN_SE3), 0, "") && is(rpe_refusal(r0, r1, a0, a1, nt, gt.data(), lags, 2), 0, ""));
  CHECK(is(align_refusal(r0, r1, a0, nullptr, nt, nan_gt.data(), 7), -EINVAL, "mode is 0"));
  CHECK(is(rpe_refusal(r0, r1, a0, nullptr, nt, nan_gt.data(), bad_lags, 2), -EINVAL, "at least 1 record"));
  CHECK(is(rpe_refusal(r0, r1, a0, nullptr, nt, nan_gt.data(), lags, 9), -EINVAL, "between 1 and 8 lags"));
  CHECK(is(align_refusal(r0, r1, a0, nullptr, nt, nan_gt.data(), ALIGN_YAW), -EINVAL, "both or neither"));
  CHECK(is(align_refusal(r0, r1, a0, out_of, nt, nan_gt.data(), ALIGN_YAW), -EINVAL, "outside [r0, r1)"));
  CHECK(is(rpe_refusal(r0, r1, a0, out_of, nt, nan_gt.data(), lags, 2), -EINVAL, "outside [r0, r1)"));
  CHECK(is(align_refusal(r0, r1, a0, a1, nt, nan_gt.data(), ALIGN_NONE), -EINVAL, "entry not finite"));
  CHECK(is(rpe_refusal(r0, r1, nullptr, nullptr, nt, nan_gt.data(), lags, 2), -EINVAL, "entry not finite"));
  nan_gt[pose_at(1, 2, nt) + 5] = std::numeric_limits<double>::infinity();
  CHECK(is(align_refusal(r0, r1, a0, a1, nt, nan_gt.data(), ALIGN_NONE), -EINVAL, "entry not finite"));
  CHECK(is(align_refusal(r0, r1, a0, a1, nt, off_gt.data(), ALIGN_SE3), -EINVAL, "quaternion norm") && is(rpe_refusal(r0, r1, a0, a1, nt, off_gt.data(), lags, 2), -EINVAL, "quaternion norm"));
  off_gt[pose_at(3, 0, nt)] = 0.5 + 1e-6;                                                  // off by 5e-7: accepted
  CHECK(is(align_refusal(r0, r1, a0, a1, nt, off_gt.data(), ALIGN_SE3), 0, ""));
  CHECK(is(align_refusal(4, 4, nullptr, nullptr, nt, nullptr, ALIGN_YAW), 0, ""));         // an empty record range looks at no pose

  // ---- the closing maths: what is flat, and that a rotation comes out whatever goes in
  const double zero3[3] = {0, 0, 0}, pb[3] = {1, 2, 3}, gb[3] = {-1, 0, 4};
  Centred c = {};
  Alignment a;
  for (int mode = 0; mode < 3; ++mode) {
    close_alignment(mode, 0.0, zero3, zero3, c, a);
    CHECK(a.R[0] == 1 && a.R[4] == 1 && a.R[8] == 1 && a.R[1] == 0 && a.cond == 0 && a.t[0] == 0 && a.t[2] == 0);
    close_alignment(mode, 1.0, pb, gb, c, a);                                                // one record: R = I, t = g - p
    CHECK(a.R[0] == 1 && a.R[5] == 0 && a.cond == 0 && a.t[0] == (mode ? -2.0 : 0.0) && a.t[2] == (mode ? 1.0 : 0.0));
  }
  c.S[8] = 2.0; c.pp = 2.0; c.gg = 2.0;                                                      // vertical extent only
  close_alignment(ALIGN_YAW, 5.0, pb, gb, c, a);
  CHECK(a.R[0] == 1 && a.R[1] == 0 && a.R[3] == 0 && a.R[4] == 1 && a.cond == 0 && a.q[0] == 1 && a.q[3] == 0);
  close_alignment(ALIGN_SE3, 5.0, pb, gb, c, a);                                             // collinear: a minimiser, cond 0
  CHECK(a.cond == 0 && std::fabs(a.R[8] - 1.0) < 1e-15);
  Centred m = {};
  m.S[0] = 3.0; m.S[4] = 2.0; m.S[8] = -1e-3; m.pp = m.gg = 5.0; m.pxy = m.gxy = 5.0;      // a mirrored z: still det = +1
  close_alignment(ALIGN_SE3, 9.0, zero3, zero3, m, a);
  const double det = a.R[0] * (a.R[4] * a.R[8] - a.R[5] * a.R[7]) - a.R[1] * (a.R[3] * a.R[8] - a.R[5] * a.R[6]) + a.R[2] * (a.R[3] * a.R[7] - a.R[4] * a.R[6]);
  CHECK(std::fabs(det - 1.0) < 1e-14 && a.cond > 0.1 && a.cond <= 1.0);

  if (failures) return 1;
  std::printf("traj plan ok\n");
  return 0;
}
