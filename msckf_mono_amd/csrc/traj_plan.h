// traj_plan.h -- the host side of the aligned trajectory error (msckf_hip_frame_log_align / _rpe, msckf_hip_traj_align / _rpe;
// kernels_traj.hip: k_traj_align, k_traj_rpe), free of device calls.
//
// Stated once here:
//   1. the modes      of the alignment: none, yaw about the global z axis plus translation (the gauge of a VIO; gravity is
//                     (0, 0, -9.81) throughout), SE(3).  Scale is left alone: the filter observes it
//   2. the rows       the strides and columns of an alignment row and of an RPE row, the most lags of one call
//   3. the checks     of the four calls' arguments, each refusal with its code and text, in the order they are applied
//   4. the closing    maths of one trajectory: from the centred sums of pass 2 to R, t and cond, as plain inline functions on
//                     doubles.  Under hipcc they are __host__ __device__, so that k_traj_align and a stand-alone host program
//                     (tests/cpp/traj_plan_host.cpp) run the same text
// Notation: p the estimate, g the ground truth, _c centred on its own mean; the alignment sought is g ~ R p + t.
// No HIP header, no batch type: a host compiler accepts this file on its own.
#ifndef MSCKF_TRAJ_PLAN_H
#define MSCKF_TRAJ_PLAN_H

#include <cerrno>
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "input_layouts.h"

#if defined(__HIPCC__)
#define MSCKF_TRAJ_HD __host__ __device__
#else
#define MSCKF_TRAJ_HD
#endif

namespace msckf_traj {

using msckf_inputs::Refusal;

// ---- 1. modes
enum Mode { ALIGN_NONE = 0, ALIGN_YAW = 1, ALIGN_SE3 = 2 };

// ---- 2. rows
constexpr int POSE = 7;           // a pose: q (w x y z) whose rotation matrix takes global vectors into the body frame, then p
constexpr int ALIGN_ROW = 20;     // one row per trajectory
constexpr int RPE_ROW = 4;        // one row per trajectory and lag
constexpr int RPE_MAX_LAGS = 8;
// alignment row: records, R row by row, t, cond, then over e = R p + t - g: sum |e|^2, max |e|, |e| at the last record; over the
// error angle e_th of the aligned attitude C(q) R^T against the truth: sum |e_th|^2, max |e_th|; sum |p - g|^2 before alignment
enum AlignCol { AL_N = 0, AL_R = 1, AL_T = 10, AL_COND = 13, AL_SUM_SQ = 14, AL_MAX = 15, AL_LAST = 16, AL_SUM_SQ_ANG = 17, AL_MAX_ANG = 18, AL_SUM_SQ_RAW = 19 };
// RPE row: pairs (r, r + lag) inside the range, sum |e_t|^2, sum |e_th|^2, max |e_t|
enum RpeCol { RPE_PAIRS = 0, RPE_SUM_SQ = 1, RPE_SUM_SQ_ANG = 2, RPE_MAX = 3 };
constexpr double QUAT_NORM_TOL = 1e-6;   // the bar of nees_plan.h
constexpr int JACOBI_SWEEPS = 16;        // the cap; a 4 x 4 symmetric matrix is down to rounding after 4 or 5

inline size_t pose_at(int r, int b, int n_traj) { return ((size_t)r * n_traj + b) * POSE; }

// ---- 3. checks, in the order the calls apply them: pointers, then the mode (align) or the lags (rpe), then the per-trajectory
// ranges, then the ground truth -- finite before the norm.  The record range [r0, r1) itself is checked by the caller against
// what it reduces (the frame log's records written, or the pose array's n_rec).
inline Refusal pointer_refusal(std::initializer_list<const void*> needed) {   // the handle, the poses, the lags, the rows
  for (const void* p : needed) if (!p) return {-EINVAL, "null argument"};
  return {0, nullptr};
}
inline Refusal mode_refusal(int mode) {
  if (mode < ALIGN_NONE || mode > ALIGN_SE3) return {-EINVAL, "trajectory alignment: mode is 0 (none), 1 (yaw and translation) or 2 (SE(3))"};
  return {0, nullptr};
}
inline Refusal lags_refusal(const int* lags, int n_lags) {
  if (!lags) return {-EINVAL, "null argument"};
  if (n_lags < 1 || n_lags > RPE_MAX_LAGS) return {-EINVAL, "relative pose error: between 1 and 8 lags"};
  for (int i = 0; i < n_lags; ++i) if (lags[i] < 1) return {-EINVAL, "relative pose error: a lag is at least 1 record"};
  return {0, nullptr};
}
// r0b / r1b: both or neither; each trajectory's range lies inside [r0, r1)
inline Refusal ranges_refusal(int r0, int r1, const int* r0b, const int* r1b, int n_traj) {
  if ((r0b == nullptr) != (r1b == nullptr)) return {-EINVAL, "trajectory ranges: r0b and r1b, both or neither"};
  if (!r0b) return {0, nullptr};
  for (int b = 0; b < n_traj; ++b)
    if (r0b[b] < r0 || r1b[b] < r0b[b] || r1b[b] > r1) return {-EINVAL, "trajectory ranges: a trajectory's range lies outside [r0, r1)"};
  return {0, nullptr};
}
inline Refusal gt_refusal(const double* gt7, size_t n_poses) {
  for (size_t i = 0; i < n_poses * POSE; ++i) if (!std::isfinite(gt7[i])) return {-EINVAL, "ground-truth poses: entry not finite"};
  for (size_t i = 0; i < n_poses; ++i) {
    const double* q = gt7 + i * POSE;
    const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (std::fabs(nrm - 1.0) > QUAT_NORM_TOL) return {-EINVAL, "ground-truth poses: quaternion norm off by more than 1e-6"};
  }
  return {0, nullptr};
}
// the pose-array calls: the array's own shape, before anything else
inline Refusal shape_refusal(int n_rec, int n_traj) {
  if (n_rec < 0 || n_traj < 1) return {-EINVAL, "pose arrays: n_rec >= 0 and n_traj >= 1 are needed"};
  return {0, nullptr};
}
// what follows the pointers and the record range in msckf_hip_frame_log_align / msckf_hip_traj_align ...
inline Refusal align_refusal(int r0, int r1, const int* r0b, const int* r1b, int n_traj, const double* gt7, int mode) {
  Refusal r = mode_refusal(mode);
  if (!r.code) r = ranges_refusal(r0, r1, r0b, r1b, n_traj);
  if (!r.code) r = gt_refusal(gt7, (size_t)(r1 - r0) * n_traj);
  return r;
}
// ... and in msckf_hip_frame_log_rpe / msckf_hip_traj_rpe
inline Refusal rpe_refusal(int r0, int r1, const int* r0b, const int* r1b, int n_traj, const double* gt7, const int* lags, int n_lags) {
  Refusal r = lags_refusal(lags, n_lags);
  if (!r.code) r = ranges_refusal(r0, r1, r0b, r1b, n_traj);
  if (!r.code) r = gt_refusal(gt7, (size_t)(r1 - r0) * n_traj);
  return r;
}

// ---- 4. the closing maths of one trajectory
// What pass 2 hands over: S = sum p_c g_c^T row by row (so that W = sum g_c p_c^T = S^T), sum |p_c|^2, sum |g_c|^2 and the
// horizontal (x, y) parts of both.
struct Centred { double S[9]; double pp, gg, pxy, gxy; };
// R row by row, its Hamilton quaternion (w x y z), t = gbar - R pbar, and cond in [0, 1]: how well the data fix R (0: not at all)
struct Alignment { double R[9]; double q[4]; double t[3]; double cond; };

MSCKF_TRAJ_HD inline void set_identity(Alignment& a) {
  for (int i = 0; i < 9; ++i) a.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  a.q[0] = 1.0; a.q[1] = a.q[2] = a.q[3] = 0.0;
  a.cond = 0.0;
}
// Eigen's toRotationMatrix of a unit quaternion, row by row
MSCKF_TRAJ_HD inline void quat_to_rows(const double* q, double* R) {
  const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
  const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
  const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
  const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// Yaw: the criterion sum |g_c - Rz(th) p_c|^2 is -2 (A cos th + B sin th) + const with A = W00 + W11, B = W10 - W01, so
// th = atan2(B, A); Rz(th) is formed from cos th = A / h, sin th = B / h, h = hypot(A, B), never from th itself (no branch of
// atan2 is crossed near +-pi), its quaternion from the half angle: (c2, 0, 0, s2) with c2 >= 0.
// cond = h / sqrt(sum |p_c,xy|^2 sum |g_c,xy|^2), by Cauchy-Schwarz in [0, 1].  Flat -- R = I, cond = 0 -- without horizontal extent.
MSCKF_TRAJ_HD inline void close_yaw(const Centred& c, Alignment& a) {
  set_identity(a);
  const double A = c.S[0] + c.S[4], B = c.S[1] - c.S[3];
  const double h = std::hypot(A, B), den = std::sqrt(c.pxy * c.gxy);
  if (!(c.pxy > 0.0) || !(c.gxy > 0.0) || !(h > 0.0) || !(den > 0.0)) return;
  const double cs = A / h, sn = B / h;
  a.R[0] = cs; a.R[1] = -sn; a.R[3] = sn; a.R[4] = cs;
  // half angle without cancellation: cs >= 0: c2 = sqrt((1 + cs) / 2), s2 = sn / (2 c2); else s2 = +-sqrt((1 - cs) / 2), c2 = sn / (2 s2)
  if (cs >= 0.0) { a.q[0] = std::sqrt(0.5 * (1.0 + cs)); a.q[3] = sn / (2.0 * a.q[0]); }
  else { const double s2 = std::sqrt(0.5 * (1.0 - cs)); a.q[3] = sn < 0.0 ? -s2 : s2; a.q[0] = std::fabs(sn) / (2.0 * s2); }
  const double cd = h / den;
  a.cond = cd > 1.0 ? 1.0 : cd;
}

// One Jacobi rotation of the symmetric 4 x 4 matrix A in the plane (P, Q), accumulated into V (A <- J^T A J, V <- V J)
template <int P, int Q>
MSCKF_TRAJ_HD inline void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double tau = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
  const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs;
  for (int k = 0; k < 4; ++k) { const double akp = A[k][P], akq = A[k][Q]; A[k][P] = cs * akp - sn * akq; A[k][Q] = sn * akp + cs * akq; }
  for (int k = 0; k < 4; ++k) { const double apk = A[P][k], aqk = A[Q][k]; A[P][k] = cs * apk - sn * aqk; A[Q][k] = sn * apk + cs * aqk; }
  for (int k = 0; k < 4; ++k) { const double vkp = V[k][P], vkq = V[k][Q]; V[k][P] = cs * vkp - sn * vkq; V[k][Q] = sn * vkp + cs * vkq; }
  A[P][Q] = A[Q][P] = 0.0;                                 // (what the rotation was chosen for)
}

// SE(3): Horn 1987's symmetric 4 x 4 matrix N of S; its eigenvector of largest eigenvalue is the Hamilton quaternion of R.
// Cyclic Jacobi, at most JACOBI_SWEEPS sweeps, stopping when the off-diagonal norm is <= 2^-52 |N|_F.  An eigenvector is a unit
// quaternion, so R is a proper rotation whatever S (no reflection fix-up).  cond = (l1 - l2) / l1 with l1 >= l2 the two largest
// eigenvalues: 0 where the minimiser is not unique (collinear points); N = 0 gives R = I, cond = 0.
MSCKF_TRAJ_HD inline void close_se3(const Centred& c, Alignment& a) {
  set_identity(a);
  if (!(c.pp > 0.0) || !(c.gg > 0.0)) return;
  const double* S = c.S;
  double A[4][4], V[4][4];
  A[0][0] = S[0] + S[4] + S[8]; A[0][1] = S[5] - S[7]; A[0][2] = S[6] - S[2]; A[0][3] = S[1] - S[3];
  A[1][1] = S[0] - S[4] - S[8]; A[1][2] = S[1] + S[3]; A[1][3] = S[6] + S[2];
  A[2][2] = -S[0] + S[4] - S[8]; A[2][3] = S[5] + S[7];
  A[3][3] = -S[0] - S[4] + S[8];
  double fro = 0.0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      if (j < i) A[i][j] = A[j][i];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) fro += A[i][j] * A[i][j];
  if (!(fro > 0.0)) return;
  const double stop = 0x1p-104 * fro;                      // (2^-52 |N|_F)^2
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    const double off = 2.0 * (A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3]);
    if (off <= stop) break;
    jacobi_rotate<0, 1>(A, V); jacobi_rotate<0, 2>(A, V); jacobi_rotate<0, 3>(A, V);
    jacobi_rotate<1, 2>(A, V); jacobi_rotate<1, 3>(A, V); jacobi_rotate<2, 3>(A, V);
  }
  // the largest diagonal entry and the next one; the first of equal ones
  double l1 = A[0][0];
  double q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > l1) { l1 = A[k][k]; q0 = V[0][k]; q1 = V[1][k]; q2 = V[2][k]; q3 = V[3][k]; }
  double l2 = 0.0; bool have = false, skipped = false;
  for (int k = 0; k < 4; ++k) {
    if (!skipped && A[k][k] == l1) { skipped = true; continue; }
    if (!have || A[k][k] > l2) { l2 = A[k][k]; have = true; }
  }
  if (!(l1 > 0.0)) return;
  const double nq = std::sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  const double sg = (q0 < 0.0 ? -1.0 : 1.0) / nq;
  a.q[0] = sg * q0; a.q[1] = sg * q1; a.q[2] = sg * q2; a.q[3] = sg * q3;
  quat_to_rows(a.q, a.R);
  const double cd = (l1 - l2) / l1;
  a.cond = cd < 0.0 ? 0.0 : (cd > 1.0 ? 1.0 : cd);
}

// From the record count, the two means and pass 2's sums to the alignment.  Flat -- R = I, cond = 0 -- when n <= 1 or all p_c or
// all g_c are zero; t = gbar - R pbar in both aligned modes, R = I and t = 0 without alignment.
MSCKF_TRAJ_HD inline void close_alignment(int mode, double n, const double* pbar, const double* gbar, const Centred& c, Alignment& a) {
  set_identity(a);
  a.t[0] = a.t[1] = a.t[2] = 0.0;
  if (mode == ALIGN_NONE || !(n > 0.0)) return;
  if (n > 1.0 && c.pp > 0.0 && c.gg > 0.0) {
    if (mode == ALIGN_YAW) close_yaw(c, a); else close_se3(c, a);
  }
  for (int i = 0; i < 3; ++i) a.t[i] = gbar[i] - (a.R[3 * i] * pbar[0] + a.R[3 * i + 1] * pbar[1] + a.R[3 * i + 2] * pbar[2]);
}

}  // namespace msckf_traj
#endif
