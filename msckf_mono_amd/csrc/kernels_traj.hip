// kernels_traj.hip -- the aligned trajectory error on the device: ATE after a yaw or an SE(3) alignment, and the relative pose
// error over a lag (Zhang & Scaramuzza's trajectory-evaluation tutorial), reduced per trajectory against ground-truth poses.
//
// k_traj_align makes three passes over a trajectory's records: the means; the centred cross matrix and extents (centred in a
// second pass, never expanded from raw moments: a trajectory a million metres from the origin keeps its digits); then, with R, t
// and cond from traj_plan.h's closing maths, the aligned position and attitude errors.  k_traj_rpe takes the pairs (r, r + lag)
// of up to 8 lags; it needs no alignment.
// One wavefront (one workgroup) per trajectory, as k_log_metrics; all arithmetic in f64; lane l takes the records r0 + l,
// r0 + l + 64, ... in ascending order and the lanes are combined by wave_sum / wave_max's fixed tree, so the same input gives the
// same bits on every call.  No atomics, no LDS.  The closing maths runs in every lane on the same numbers (nothing to hand
// round, no divergence).  The kernels only read their inputs and only write their rows.
// The estimate comes from the frame log (LogSrc: q at LOG_IMU + IQ, p at LOG_IMU + IP of a record, widened to double) or from a
// plain double pose array (PoseSrc: [r][n_traj][7] = q w x y z, p); everything after the load is shared.
#include "dev_common.h"
#include "traj_plan.h"

namespace msckf {

using namespace msckf_traj;

struct Pose { Q4<double> q; V3<double> p; };

// record r (of the log) of trajectory b
template <class S> struct LogSrc {
  const S* log; int B;
  __device__ __forceinline__ Pose load(int r, int b) const {
    const S* x = log + ((long)r * B + b) * LOG_STRIDE + LOG_IMU;
    Pose o;
    o.q.w = (double)x[IQ]; o.q.x = (double)x[IQ + 1]; o.q.y = (double)x[IQ + 2]; o.q.z = (double)x[IQ + 3];
    o.p = mk3((double)x[IP], (double)x[IP + 1], (double)x[IP + 2]);
    return o;
  }
};
struct PoseSrc {
  const double* pose; int n_traj;
  __device__ __forceinline__ Pose load(int r, int b) const {
    const double* x = pose + ((long)r * n_traj + b) * POSE;
    Pose o;
    o.q = ldq(x); o.p = ld3(x + 4);
    return o;
  }
};

// the three passes of one trajectory over [r0, r1); the ground truth's first record is rg.  Every lane returns with the row.
template <class Src>
__device__ __forceinline__ void align_trajectory(const Src& est, const PoseSrc& gt, int b, int lane, int rg, int r0, int r1, int mode, double* row) {
  // pass 1: n, sum p, sum g
  double n = 0, sp[3] = {0, 0, 0}, sg[3] = {0, 0, 0};
  for (int r = r0 + lane; r < r1; r += 64) {
    const V3<double> p = est.load(r, b).p, g = gt.load(r - rg, b).p;
    n += 1.0;
    sp[0] += p.x; sp[1] += p.y; sp[2] += p.z;
    sg[0] += g.x; sg[1] += g.y; sg[2] += g.z;
  }
  n = wave_sum(n);
  double pbar[3] = {0, 0, 0}, gbar[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < 3; ++c) { sp[c] = wave_sum(sp[c]); sg[c] = wave_sum(sg[c]); }
  if (mode != ALIGN_NONE && n > 0.0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { pbar[c] = sp[c] / n; gbar[c] = sg[c] / n; }
  }
  // pass 2: the centred cross matrix and extents
  Centred cs = {};
  if (mode != ALIGN_NONE) {
    for (int r = r0 + lane; r < r1; r += 64) {
      const V3<double> p = est.load(r, b).p, g = gt.load(r - rg, b).p;
      const double pc[3] = {p.x - pbar[0], p.y - pbar[1], p.z - pbar[2]}, gc[3] = {g.x - gbar[0], g.y - gbar[1], g.z - gbar[2]};
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) cs.S[3 * i + j] += pc[i] * gc[j];
      const double ph = pc[0] * pc[0] + pc[1] * pc[1], gh = gc[0] * gc[0] + gc[1] * gc[1];
      cs.pxy += ph; cs.gxy += gh;
      cs.pp += ph + pc[2] * pc[2]; cs.gg += gh + gc[2] * gc[2];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) cs.S[i] = wave_sum(cs.S[i]);
    cs.pp = wave_sum(cs.pp); cs.gg = wave_sum(cs.gg); cs.pxy = wave_sum(cs.pxy); cs.gxy = wave_sum(cs.gxy);
  }
  Alignment a;
  close_alignment(mode, n, pbar, gbar, cs, a);
  // pass 3: e = R p + t - g, formed as R (p - pbar) - (g - gbar) (t = gbar - R pbar; without alignment both means are zero here);
  // the aligned attitude C(q) R^T = C(q * q_R^-1) against the truth; and |p - g|^2 as it stands
  Q4<double> qr_inv; qr_inv.w = a.q[0]; qr_inv.x = -a.q[1]; qr_inv.y = -a.q[2]; qr_inv.z = -a.q[3];
  double s2 = 0, mx = 0, last = 0, sth = 0, mth = 0, raw = 0;
  for (int r = r0 + lane; r < r1; r += 64) {
    const Pose e = est.load(r, b), g = gt.load(r - rg, b);
    const double pc[3] = {e.p.x - pbar[0], e.p.y - pbar[1], e.p.z - pbar[2]}, gc[3] = {g.p.x - gbar[0], g.p.y - gbar[1], g.p.z - gbar[2]};
    const double e0 = a.R[0] * pc[0] + a.R[1] * pc[1] + a.R[2] * pc[2] - gc[0];
    const double e1 = a.R[3] * pc[0] + a.R[4] * pc[1] + a.R[5] * pc[2] - gc[1];
    const double e2 = a.R[6] * pc[0] + a.R[7] * pc[1] + a.R[8] * pc[2] - gc[2];
    const double d2 = e0 * e0 + e1 * e1 + e2 * e2, dist = sqrt(d2);
    const V3<double> th = error_angle(qmul(e.q, qr_inv), g.q);
    const double t2 = th.x * th.x + th.y * th.y + th.z * th.z, dth = sqrt(t2);
    const double u0 = e.p.x - g.p.x, u1 = e.p.y - g.p.y, u2 = e.p.z - g.p.z;
    s2 += d2; sth += t2; raw += u0 * u0 + u1 * u1 + u2 * u2;
    mx = dist > mx ? dist : mx; mth = dth > mth ? dth : mth;
    if (r == r1 - 1) last = dist;
  }
  s2 = wave_sum(s2); mx = wave_max(mx); last = wave_sum(last); sth = wave_sum(sth); mth = wave_max(mth); raw = wave_sum(raw);
  row[AL_N] = n;
#pragma unroll
  for (int i = 0; i < 9; ++i) row[AL_R + i] = a.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) row[AL_T + i] = a.t[i];
  row[AL_COND] = a.cond; row[AL_SUM_SQ] = s2; row[AL_MAX] = mx; row[AL_LAST] = last; row[AL_SUM_SQ_ANG] = sth; row[AL_MAX_ANG] = mth; row[AL_SUM_SQ_RAW] = raw;
}

// One workgroup (one wavefront) per trajectory over the records [r0, r1) of the estimate; gt [r1 - r0][n_traj][7] is indexed from
// r0.  r0b / r1b (both or neither): the trajectory's own range inside [r0, r1), as in k_log_metrics.  out [n_traj][ALIGN_ROW]
// (traj_plan.h: AlignCol).  Lanes 0 .. 19 store the row, one column each.
template <class Src>
__global__ __launch_bounds__(64) void k_traj_align(Src est, int n_traj, int r0, int r1, const int* r0b, const int* r1b, const double* gt, int mode, double* out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int rg = r0;
  if (r0b) { r0 = r0b[b]; r1 = r1b[b]; }
  PoseSrc g; g.pose = gt; g.n_traj = n_traj;
  double row[ALIGN_ROW];
  align_trajectory(est, g, b, lane, rg, r0, r1, mode, row);
  double v = 0.0;
#pragma unroll
  for (int c = 0; c < ALIGN_ROW; ++c) if (lane == c) v = row[c];
  if (lane < ALIGN_ROW) out[(long)b * ALIGN_ROW + lane] = v;
}

// The relative pose error of one trajectory and one lag over the pairs (r, r + lag), r in [r0, r1 - lag):
//   e_t  = C(q_r) (p_{r + lag} - p_r) - C(g_r) (g_{r + lag} - g_r), each displacement in its own body frame at r
//   e_th = the error angle of q_{r + lag} * q_r^-1 against the truth's
// Both are unchanged by a global rotation and translation of either trajectory.
template <class Src>
__device__ __forceinline__ void rpe_trajectory(const Src& est, const PoseSrc& gt, int b, int lane, int rg, int r0, int r1, int lag, double* row) {
  double cnt = 0, st = 0, sth = 0, mx = 0;
  for (long r = (long)r0 + lane; r + lag < r1; r += 64) {
    const Pose e0 = est.load((int)r, b), e1 = est.load((int)r + lag, b), g0 = gt.load((int)r - rg, b), g1 = gt.load((int)r + lag - rg, b);
    const V3<double> de = mulv(q2rot(e0.q), e1.p - e0.p), dg = mulv(q2rot(g0.q), g1.p - g0.p);
    const V3<double> et = de - dg;
    const V3<double> th = error_angle(qmul(e1.q, qinverse(e0.q)), qmul(g1.q, qinverse(g0.q)));
    const double d2 = dot3(et, et), dist = sqrt(d2);
    cnt += 1.0; st += d2; sth += dot3(th, th);
    mx = dist > mx ? dist : mx;
  }
  row[RPE_PAIRS] = wave_sum(cnt); row[RPE_SUM_SQ] = wave_sum(st); row[RPE_SUM_SQ_ANG] = wave_sum(sth); row[RPE_MAX] = wave_max(mx);
}

// One workgroup (one wavefront) per trajectory, the lags one after the other.  out [n_traj][n_lags][RPE_ROW] (traj_plan.h: RpeCol);
// a lag longer than the range has no pairs and gives zeros.
template <class Src>
__global__ __launch_bounds__(64) void k_traj_rpe(Src est, int n_traj, int r0, int r1, const int* r0b, const int* r1b, const double* gt, const int* lags, int n_lags, double* out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int rg = r0;
  if (r0b) { r0 = r0b[b]; r1 = r1b[b]; }
  PoseSrc g; g.pose = gt; g.n_traj = n_traj;
  for (int k = 0; k < n_lags; ++k) {
    double row[RPE_ROW];
    rpe_trajectory(est, g, b, lane, rg, r0, r1, lags[k], row);
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < RPE_ROW; ++c) if (lane == c) v = row[c];
    if (lane < RPE_ROW) out[((long)b * n_lags + k) * RPE_ROW + lane] = v;
  }
}

template <class S>
void launch_traj_align_log(const S* log, int B, int r0, int r1, const int* r0b, const int* r1b, const double* gt, int mode, double* out, hipStream_t st) {
  if (B <= 0) return;
  LogSrc<S> src; src.log = log; src.B = B;
  hipLaunchKernelGGL(k_traj_align<LogSrc<S>>, dim3(B), dim3(64), 0, st, src, B, r0, r1, r0b, r1b, gt, mode, out);
}
template <class S>
void launch_traj_rpe_log(const S* log, int B, int r0, int r1, const int* r0b, const int* r1b, const double* gt, const int* lags, int n_lags, double* out, hipStream_t st) {
  if (B <= 0) return;
  LogSrc<S> src; src.log = log; src.B = B;
  hipLaunchKernelGGL(k_traj_rpe<LogSrc<S>>, dim3(B), dim3(64), 0, st, src, B, r0, r1, r0b, r1b, gt, lags, n_lags, out);
}
void launch_traj_align_pose(const double* est, int n_traj, int n_rec, const int* r0b, const int* r1b, const double* gt, int mode, double* out, hipStream_t st) {
  if (n_traj <= 0) return;
  PoseSrc src; src.pose = est; src.n_traj = n_traj;
  hipLaunchKernelGGL(k_traj_align<PoseSrc>, dim3(n_traj), dim3(64), 0, st, src, n_traj, 0, n_rec, r0b, r1b, gt, mode, out);
}
void launch_traj_rpe_pose(const double* est, int n_traj, int n_rec, const int* r0b, const int* r1b, const double* gt, const int* lags, int n_lags, double* out, hipStream_t st) {
  if (n_traj <= 0) return;
  PoseSrc src; src.pose = est; src.n_traj = n_traj;
  hipLaunchKernelGGL(k_traj_rpe<PoseSrc>, dim3(n_traj), dim3(64), 0, st, src, n_traj, 0, n_rec, r0b, r1b, gt, lags, n_lags, out);
}

template void launch_traj_align_log<float>(const float*, int, int, int, const int*, const int*, const double*, int, double*, hipStream_t);
template void launch_traj_align_log<double>(const double*, int, int, int, const int*, const int*, const double*, int, double*, hipStream_t);
template void launch_traj_rpe_log<float>(const float*, int, int, int, const int*, const int*, const double*, const int*, int, double*, hipStream_t);
template void launch_traj_rpe_log<double>(const double*, int, int, int, const int*, const int*, const double*, const int*, int, double*, hipStream_t);

}  // namespace msckf
