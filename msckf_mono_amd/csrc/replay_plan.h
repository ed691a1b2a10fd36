// replay_plan.h -- the Monte-Carlo replay's host side, free of device calls: S noise-free SEQUENCES staged once, and B
// trajectories that each name a sequence, a 64-bit seed and a noise model: four white levels (sigma4), or the filter's own
// 12 x 12 Q_imu with its two bias random walks (MODEL below), and optionally a fault record: seeded missed observations and
// outliers (FAULTS below).  Before a frame the kernel k_replay_expand
// (kernels_replay.hip) turns the frame's S sequence cells into the ordinary per-trajectory frame block of input_layouts.h
// (FrameLayout(B, K, f_cap, esz), sections [rd | n | drop | k | M | off | slots | obs]) -- what an upload would have put there.
//
// Stated once here:
//   1. mix / U        the integer part of the random stream (value i of scenario.SplitMix64(seed) and the 53-bit uniform made of
//                     it), constexpr, shared by this file's host users, the kernel and -- bit for bit -- the numpy twin
//   2. the noise      which pair of which sub-seed a value takes (NOISE and MODEL below), and chol_psd, the factor of Q_imu
//                     and the faults on top of either model: missed observations and outliers (FAULTS below), the rule on a
//                     track stated serially (track_faults), the lane group of the faulted expansion
//                     and the camera's clock: time offset, jitter and rolling shutter (TIMING below), the image table of a
//                     sequence, the stencil of the shift and its preconditions
//                     and the sensors' calibration errors: IMU scale, misalignment, g-sensitivity, saturation and quantisation,
//                     the camera's residual intrinsics (CALIB below), as inline functions the kernels compile too
//   3. Plan           the sequence store (a ScenarioStore of S "trajectories" whose scalars are doubles), the assignment record
//                     of either model, per frame each trajectory's first entry in the expanded block and the block's size, the
//                     largest expanded frame, and every refusal with its code and text
// No HIP header, no batch type: a host compiler accepts this file on its own (tests/cpp/replay_plan_host.cpp).
#ifndef MSCKF_REPLAY_PLAN_H
#define MSCKF_REPLAY_PLAN_H

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "host_lists.h"
#include "input_layouts.h"

namespace msckf_replay {

// ---- 1. the integer part
constexpr uint64_t GAMMA = 0x9E3779B97F4A7C15ull;
// value i (0-based) of scenario.SplitMix64(seed): the finalizer of seed + (i + 1) gamma, all modulo 2^64
constexpr uint64_t mix(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * GAMMA;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the uniform in [0, 1) of its upper 53 bits: exact in a double
constexpr double U(uint64_t seed, uint64_t i) { return (double)(mix(seed, i) >> 11) * (1.0 / 9007199254740992.0); }

// ---- 2. NOISE: which draws a value takes
// pair(s, j) = (r cos(2 pi u2), r sin(2 pi u2)), u1 = 1 - U(s, 2 j), u2 = U(s, 2 j + 1), r = sqrt(-2 ln u1)      (Box-Muller)
// Trajectory b with seed s_b on frame f: s_imu = mix(s_b, 2 f), s_obs = mix(s_b, 2 f + 1).
//   IMU sample i < k of the cell: pairs 3 i, 3 i + 1, 3 i + 2 of s_imu = (g_x, g_y), (g_z, a_x), (a_y, a_z);
//                                 omega += sigma_g g, a += sigma_a a, dT unchanged, rows from k on zero
//   entry e of the cell:          pair e of s_obs = (n_u, n_v); obs += (sigma_u n_u, sigma_v n_v)
// Sequence values are doubles; value + sigma * noise is formed in double (product rounded, then the sum) and rounded once to
// the handle's scalar.
constexpr uint64_t imu_seed(uint64_t s, int f) { return mix(s, 2 * (uint64_t)f); }
constexpr uint64_t obs_seed(uint64_t s, int f) { return mix(s, 2 * (uint64_t)f + 1); }
enum Sigma { SIG_G, SIG_A, SIG_U, SIG_V, N_SIGMA };
constexpr int IMU_PAIRS = 3;   // pairs per IMU sample
// column c (0 .. 5) of an IMU sample is half (c & 1) of its pair c / 2 and scales with sigma[c < 3 ? SIG_G : SIG_A]

// ---- 2b. MODEL: noise drawn from Q_imu, with bias random walks (msckf_hip_replay_assign_q; normative, the header and DESIGN
// section 4.13 state the same)
// Trajectory b has Q[b] (12 x 12, column-major, noise order n_g n_wg n_a n_wa: the filter's own Q144, taken as its symmetric
// part 0.5 (Q + Q^T)), scale[b] >= 0 (scenario.Trajectory's imu_noise_scale) and (sigma_u, sigma_v)[b].
//   L = chol_psd(Q_sym), lower triangular, in double, in this order: for column c, d = Q_cc - s with s = sum_{j < c} L_cj^2
//     (terms added in ascending j, from 0); d < -1e-12 max_diag is refused; |d| <= 1e-12 max_diag makes the whole column zero (a
//     zero walk density is the common case); otherwise L_cc = sqrt(d), L_rc = (Q_rc - sum_{j < c} L_rj L_cj) / L_cc, the sum as s.
//   sample i < k of the cell takes pairs 6 i .. 6 i + 5 of s_imu as z[0 .. 11]: pair 6 i + p = (z[2 p], z[2 p + 1]);
//     w_r = sum_{c <= r} L_rc z_c, c ascending from 0.0, each product rounded, then added.
//   with dT_i > 0 (sq = sqrt(dT_i)): n_r = (scale w_r) / sq for the white rows r = 0 .. 2 (omega), 6 .. 8 (a);
//     delta_g = (scale w[3 .. 5]) sq, delta_a = (scale w[9 .. 11]) sq.  dT_i <= 0: no noise, no increment.
//   the walk, per component (0 .. 2 gyro, 3 .. 5 accelerometer), in double: P(f, 0) = 0, P(f, i + 1) = P(f, i) + delta(f, i);
//     Wstart(0) = 0, Wstart(f + 1) = Wstart(f) + P(f, k_f) (skipped cells and cells with k = 0 add nothing);
//     W(f, i) = Wstart(f) + P(f, i).  The bias starts at the sequence's constant bias, what the filter is initialised with.
//   sample i < k stores (value + W(f, i)) + n, rounded once to the handle's scalar (n absent when dT_i <= 0); rows from k on
//     are the sequence's (zero).  Observations as under NOISE: pair e of s_obs, obs += (sigma_u n_u, sigma_v n_v).
// Wstart has frames + 1 rows per trajectory: row f + 1 is the true bias offset at the time of frame f's log record.  A one-off
// scan (k_replay_walk_scan) tabulates it, so no state is carried between frames at run time.
constexpr int NQ = 12, L_SIZE = NQ * NQ;   // L is stored whole, column-major as Q: L_rc = L[c * NQ + r]
constexpr int MODEL_PAIRS = 6;             // pairs per IMU sample under the model
constexpr int WALK_ROW = 6;                // scalars of a walk row: gyro bias offset, accelerometer bias offset
constexpr double PSD_TOL = 1e-12;          // the project's symmetry tolerance, relative to the largest diagonal entry
enum Model { MODEL_SIGMA4, MODEL_Q };
// false: Q_sym has a negative pivot.  Q and L column-major [144]; L's upper triangle is zero.
inline bool chol_psd(const double* Q, double* L) {
  double A[L_SIZE], top = 0.0;
  for (int r = 0; r < NQ; ++r) for (int c = 0; c < NQ; ++c) A[c * NQ + r] = 0.5 * (Q[c * NQ + r] + Q[r * NQ + c]);
  for (int c = 0; c < NQ; ++c) top = std::max(top, A[c * NQ + c]);
  for (int i = 0; i < L_SIZE; ++i) L[i] = 0.0;
  for (int c = 0; c < NQ; ++c) {
    double s = 0.0;
    for (int j = 0; j < c; ++j) s += L[j * NQ + c] * L[j * NQ + c];
    const double d = A[c * NQ + c] - s;
    if (d < -PSD_TOL * top) return false;
    if (std::fabs(d) <= PSD_TOL * top) continue;
    const double p = std::sqrt(d);
    L[c * NQ + c] = p;
    for (int r = c + 1; r < NQ; ++r) {
      double t = 0.0;
      for (int j = 0; j < c; ++j) t += L[j * NQ + r] * L[j * NQ + c];
      L[c * NQ + r] = (A[c * NQ + r] - t) / p;
    }
  }
  return true;
}

// ---- 2c. FAULTS: seeded missed observations and outliers (msckf_hip_replay_set_faults; normative, the header, DESIGN section
// 4.13 and the twin state the same).  Independent of the noise model: it composes with NOISE and with MODEL.
// Trajectory b has fault4[b] = (p_miss, p_out, rho_u, rho_v): two probabilities in [0, 1], two radii in normalised image
// units, finite and >= 0.
//   sub-seed   s_flt(f) = mix(mix(s_b, 2^63 + 1), f).  Frames use mix(s_b, 2 f) and mix(s_b, 2 f + 1), replay_initial_error
//              uses mix(s_b, 2^63): no frame index reaches either.
//   draws      entry e (0-based among the SEQUENCE cell's entries, in sequence order) takes u_miss = U(s_flt, 3 e),
//              u_out = U(s_flt, 3 e + 1), u_ang = U(s_flt, 3 e + 2).
//   missed     raw_miss(e) = u_miss < p_miss.  A track that would keep fewer than two observations loses none: if
//              M - #raw_miss < 2 then miss = false on the whole track (the sequence's own tracks with M < 2 pass through
//              unchanged); otherwise miss = raw_miss.  A tracker hands the filter no track of one observation.
//   outliers   out(e) = !miss(e) && u_out < p_out.
//   values     obs = value + sigma noise exactly as without faults: pair e of s_obs, indexed by the sequence entry, so a
//              trajectory's Gaussian noise does not depend on its faults.  Where out(e): (x + rho_u cos a, y + rho_v sin a),
//              a the rounded product 6.283185307179586 u_ang, each product rounded, then added, all in double, rounded once to
//              the handle's scalar.
//   the block  off[t], the trajectory's base, the frame's entry count, n, drop, k and rd are unchanged: a track's range keeps
//              the sequence's length.  M[t] is the number of survivors; the range is a stable partition -- the survivors in
//              sequence order, then the missed entries in sequence order -- and every entry carries its slot and coordinates.
//              Nothing downstream reads beyond off[t] + M[t] (the kernels find a track through trk_off / trk_M alone).
// The host keeps the sequence's maxslot: an upper bound, which is all the frame step asks of it.  With no faults set, or
// every trajectory at p_miss = p_out = 0, the expansion launched is the unfaulted one.
constexpr uint64_t FAULT_STREAM = 0x8000000000000001ull;   // 2^63 + 1
constexpr uint64_t fault_seed(uint64_t s, int f) { return mix(mix(s, FAULT_STREAM), (uint64_t)f); }
enum Fault { FLT_P_MISS, FLT_P_OUT, FLT_RHO_U, FLT_RHO_V, N_FAULT };
enum FaultCode { FAULT_KEPT = 0, FAULT_OUTLIER = 1, FAULT_MISSED = 2 };   // msckf_hip_replay_expand_faults, per sequence entry
constexpr int FAULT_DRAWS = 3;             // uniforms per entry
// lanes per track of the faulted expansion: the smallest of 16, 32, 64 that holds a track of m_cap observations
constexpr int fault_group(int m_cap) { return m_cap <= 16 ? 16 : m_cap <= 32 ? 32 : 64; }
// the rule on one track, stated serially: its M entries start at entry e0 of the sequence cell; how many of them are missed
// and how many are outliers (what the expansion's lane groups decide by ballot, and what the two reductions recompute)
struct TrackFaults { int missed, outliers; };
constexpr TrackFaults track_faults(uint64_t s_flt, uint64_t e0, int M, double p_miss, double p_out) {
  int raw = 0;
  for (int l = 0; l < M; ++l) raw += U(s_flt, FAULT_DRAWS * (e0 + l)) < p_miss ? 1 : 0;
  const bool none = M - raw < 2;             // a track keeps two observations or loses none
  int out = 0;
  for (int l = 0; l < M; ++l) out += (none || !(U(s_flt, FAULT_DRAWS * (e0 + l)) < p_miss)) && U(s_flt, FAULT_DRAWS * (e0 + l) + 1) < p_out ? 1 : 0;
  return TrackFaults{none ? 0 : raw, out};
}
// columns of msckf_hip_replay_fault_counts and of msckf_hip_map_log_fault_metrics
enum FaultCount { FC_ENTRIES, FC_MISSED, FC_OUTLIERS, FC_TRACKS, FC_TRACKS_SHORTENED, FC_TRACKS_CONTAMINATED, N_FAULT_COUNT };
enum FaultMetric { FM_RECORDS, FM_CLEAN_PASS, FM_CLEAN_REJ, FM_CONT_PASS, FM_CONT_REJ, FM_SUM_GAMMA, FM_SUM_DOF, FM_UNMATCHED, N_FAULT_METRIC };

// ---- 2d. SUMS: a row of msckf_hip_replay_imu_sums, per trajectory over a frame range: the IMU samples the expansion hands the
// trajectory's propagate (rows below the cell's k of the cells that are not skipped), each scalar as the expansion stores it --
// rounded to the handle's scalar, widened to double -- summed in double: the count, omega, a, dT.  Sums and counts: ranges add.
enum ImuSum { IS_COUNT = 0, IS_OMEGA = 1, IS_A = 4, IS_DT = 7, IMU_SUM_ROW = 8 };

// ---- 2e. TIMING: camera time offset, per-image timestamp jitter and rolling-shutter readout (msckf_hip_replay_set_timing;
// normative, the header, DESIGN section 4.13 and the twin state the same).  Independent of the noise model and of the faults.
// Trajectory b has timing4[b] = (t_d, r_y, y_0, sigma_j): the offset [s], the readout slope [s per unit of normalised image y],
// the image row exposed at the image's stamp, the jitter [s]; all finite, sigma_j >= 0.  A record is non-zero when t_d, r_y or
// sigma_j is (y_0 alone moves nothing).
//   image table  of a sequence, built at commit from its cells alone.  Frames in order with T = 0 (double), ord = 0, W = 0: a
//                skipped cell changes nothing; any other cell adds its dT_i, i < k ascending, to T, sets ord += 1, W += 1,
//                records time[ord - 1] = T, frame_of[ord - 1] = f, base(f) = ord - W, then sets W -= n_drop(f).  Camera slot s
//                of frame f's cell is image base(f) + s: the window an empty start at frame 0 gives (a suffix of the images).
//   exposure     entry l of a track has the sequence value (x_l, y_l) and camera image i_l = base(f) + slot_l; it was exposed at
//                time[i_l] + delta_l, delta_l = (t_d + r_y (y_l - y_0)) + sigma_j g(frame_of[i_l]): the difference, the product,
//                the sum, the product sigma_j g, the sum, each rounded in double.  g(q) is the first component of
//                pair(mix(s_b, 2^63 + 2), q): one draw per image and seed, shared by every observation of that image in
//                whichever cell it surfaces (sigma_j == 0: no draw, the term is 0).
//   shift        along the entry's own track, nodes in sequence order: M = 1 unchanged; M = 2 both entries; M >= 3 the entries
//                l0, l0 + 1, l0 + 2 with l0 = min(max(l - 1, 0), M - 3).  d_j = time[i_j] - time[i_l];
//                w_j = prod_{m != j} (delta_l - d_m) / prod_{m != j} (d_j - d_m), m ascending, numerator and denominator each a
//                product (three nodes) or a single difference (two), then one division; the new value is sum_j w_j (x_j, y_j),
//                j ascending, the first product, then each further product added.  + - x / only, each rounded in double, no
//                contraction.  delta_l == 0 exactly: the value itself, no arithmetic.
//   then         the Gaussian pixel noise and the outlier ring are added to the shifted value exactly as without timing; a
//                missed observation still serves its neighbours as a node; draws stay indexed by the sequence entry.
//   refused      while some record is non-zero (set_timing on committed cells, commit under a non-zero record), with the
//                sequence, frame and track named: a cell that names a slot >= W(f); a track whose slots do not ascend
//                strictly; a track whose node times do not increase strictly.
// With no record, or every record zero, the expansion launched is the un-timed one.
constexpr uint64_t TIMING_STREAM = 0x8000000000000002ull;   // 2^63 + 2
constexpr uint64_t timing_seed(uint64_t s) { return mix(s, TIMING_STREAM); }
enum Timing { TIM_TD, TIM_RY, TIM_Y0, TIM_SIGMA_J, N_TIMING };
// the stencil of entry l of a track of M entries: its node count and its first node
constexpr int stencil_nodes(int M) { return M < 3 ? M : 3; }
constexpr int stencil_first(int l, int M) { return M < 3 ? 0 : (l - 1 < 0 ? 0 : l - 1 > M - 3 ? M - 3 : l - 1); }

// ---- 2f. CALIB: IMU and camera calibration errors (msckf_hip_replay_set_imu_calib, msckf_hip_replay_set_cam_calib; normative,
// the header, DESIGN section 4.13 and the twin state the same).  Independent of the noise model, the faults and the timing.
// The arithmetic is the inline functions below: the kernels and a host program compile this text.
//   IMU      trajectory b has imucal[b] = [31]: T_g (0 .. 8, 3 x 3 row-major), T_a (9 .. 17), G (18 .. 26, the gyro's response to
//            specific force [rad/s per m/s^2]), sat_g, sat_a (27, 28: saturation levels, 0: none), lsb_g, lsb_a (29, 30:
//            quantisation steps, 0: none); all finite, the last four >= 0.  The identity record is T_g = T_a = I, the rest 0; a
//            record is non-trivial when it differs from that.
//            The matrices act on the sequence's values, constant bias included: the cell holds omega + b_0 and a + b_0, and the
//            shift (T - I) b_0 is a bias the filter estimates anyway.
//   sample   i < k of a cell that is not skipped, v_g = cell[0:3], v_a = cell[3:6]:
//              c_a[r] = sum_c T_a[r][c] v_a[c], c_g[r] = sum_c T_g[r][c] v_g[c]: the first product, then each further product
//              added, c ascending; for the gyro then + G[r][0] v_a[0], + G[r][1] v_a[1], + G[r][2] v_a[2] in that order; every
//              product and every sum rounded in double (calib_imu).
//            c takes the place of the sequence value in the noise rule: c + sigma g under NOISE, (c + W(f, i)) + n under MODEL (no
//            n when dT_i <= 0).  The bias walk stays an output bias: Wstart and k_replay_walk_scan do not change.
//            then, per component with its sensor's sat and lsb (calib_out): where sat > 0, x = min(max(x, -sat), sat), and the
//            component is CLIPPED when its value before the clamp lies strictly outside [-sat, sat]; where lsb > 0,
//            x = lsb rint(x / lsb): the quotient rounded, rint to nearest even, then the product.  The result is rounded once to
//            the handle's scalar.  dT, rows from k on and skipped cells are untouched.
//   camera   trajectory b has camcal[b] = (e_u, e_v, d_u, d_v, k1, k2, p1, p2), all finite: the residual map, in normalised
//            coordinates, between the true camera and the calibration the front end undistorted with -- e the relative focal
//            length error, d the principal point error over the focal length, k and p the residual radial-tangential
//            coefficients.  The all-zero record is trivial.
//   entry    the map applies to an entry's value (x, y): the sequence value, or what the TIMING shift made of it (the timing
//            delta keeps using the sequence's y).  calib_cam:
//              xx = x x, yy = y y, xy = x y, r2 = xx + yy, rad = (1 + k1 r2) + k2 (r2 r2)
//              xd = (x rad + (2 p1) xy) + p2 (r2 + 2 xx),  yd = (y rad + p1 (r2 + 2 yy)) + (2 p2) xy
//              x' = (xd + e_u xd) + d_u,                   y' = (yd + e_v yd) + d_v
//            + - x only, each rounded in double, no contraction.  The Gaussian pixel noise and the outlier ring are then added to
//            (x', y') exactly as before; draws stay indexed by the sequence entry, so a seed's noise and faults do not depend on
//            its calibration.  Missed entries are mapped too: every entry carries its coordinates.
// With no record, or only trivial ones, the expansion launched is the one without calibration.
#if defined(__HIPCC__)
#define MSCKF_RP_HD __host__ __device__
#else
#define MSCKF_RP_HD
#endif
// a value that is rounded before anything else is done with it, whatever the translation unit's contraction mode: it passes
// through an empty asm the compiler cannot look into (a product that goes into a sum is never fused with it)
MSCKF_RP_HD inline double rnd(double p) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(p));
#elif defined(__x86_64__)
  asm volatile("" : "+x"(p));
#else
  volatile double q = p; p = q;
#endif
  return p;
}
constexpr int IMU_CAL = 31, CAM_CAL = 8;   // scalars of the two records
enum ImuCal { IC_TG = 0, IC_TA = 9, IC_G = 18, IC_SAT_G = 27, IC_SAT_A = 28, IC_LSB_G = 29, IC_LSB_A = 30 };
enum CamCal { CC_EU, CC_EV, CC_DU, CC_DV, CC_K1, CC_K2, CC_P1, CC_P2 };
// columns of msckf_hip_replay_calib_counts: samples, gyro x y z clipped, accelerometer x y z clipped, samples with any component clipped
enum CalibCount { CCNT_SAMPLES = 0, CCNT_CLIP = 1, CCNT_ANY = 7, N_CALIB_COUNT = 8 };
// c of column col (0 .. 2 gyro, 3 .. 5 accelerometer) of a sample with the sequence values v[6]
MSCKF_RP_HD inline double calib_imu(const double* ic, const double* v, int col) {
  const bool gyro = col < 3;
  const int r = gyro ? col : col - 3;
  const double* T = ic + (gyro ? IC_TG : IC_TA) + 3 * r;
  const double* x = v + (gyro ? 0 : 3);
  double a = rnd(T[0] * x[0]);
  a = rnd(a + rnd(T[1] * x[1]));
  a = rnd(a + rnd(T[2] * x[2]));
  if (gyro) {
    const double* G = ic + IC_G + 3 * r;
    a = rnd(a + rnd(G[0] * v[3]));
    a = rnd(a + rnd(G[1] * v[4]));
    a = rnd(a + rnd(G[2] * v[5]));
  }
  return a;
}
// saturation and quantisation of column col's value x (noise included); *clipped: x lay strictly outside [-sat, sat]
MSCKF_RP_HD inline double calib_out(const double* ic, int col, double x, bool* clipped) {
  const double sat = ic[col < 3 ? IC_SAT_G : IC_SAT_A], lsb = ic[col < 3 ? IC_LSB_G : IC_LSB_A];
  *clipped = sat > 0.0 && (x < -sat || x > sat);
  if (sat > 0.0) { x = x > -sat ? x : -sat; x = x < sat ? x : sat; }
  if (lsb > 0.0) x = lsb * std::rint(rnd(x / lsb));
  return x;
}
// the camera's residual map of (x, y) under cc[8], out[2] (out may be where x and y came from)
MSCKF_RP_HD inline void calib_cam(const double* cc, double x, double y, double* out) {
  const double xx = rnd(x * x), yy = rnd(y * y), xy = rnd(x * y), r2 = rnd(xx + yy);
  const double rad = rnd(rnd(1.0 + rnd(cc[CC_K1] * r2)) + rnd(cc[CC_K2] * rnd(r2 * r2)));
  const double xd = rnd(rnd(rnd(x * rad) + rnd(rnd(2.0 * cc[CC_P1]) * xy)) + rnd(cc[CC_P2] * rnd(r2 + rnd(2.0 * xx))));
  const double yd = rnd(rnd(rnd(y * rad) + rnd(cc[CC_P1] * rnd(r2 + rnd(2.0 * yy)))) + rnd(rnd(2.0 * cc[CC_P2]) * xy));
  out[0] = rnd(xd + rnd(cc[CC_EU] * xd)) + cc[CC_DU];
  out[1] = rnd(yd + rnd(cc[CC_EV] * yd)) + cc[CC_DV];
}
// the identity IMU record
inline void imu_calib_identity(double* ic) {
  for (int i = 0; i < IMU_CAL; ++i) ic[i] = 0.0;
  for (int r = 0; r < 3; ++r) ic[IC_TG + 4 * r] = ic[IC_TA + 4 * r] = 1.0;
}

// ---- 3. the plan
using msckf_inputs::FrameLayout;
using msckf_inputs::Refusal;
using msckf_inputs::ScenarioStore;

struct Plan {
  int S = 0, B = 0, f_cap = 0;
  ScenarioStore seq;                 // the sequences' cells: seq.lay.B == S, scalars double; seq.frames == 0: no replay allocated
  bool committed = false;            // the cells are indexed (and, for the caller, on the device) as they stand
  bool assigned = false;
  Model model = MODEL_SIGMA4;        // which of the two assignment records is in force
  std::vector<int> seq_of;           // [B]
  std::vector<uint64_t> seed;        // [B]
  std::vector<double> sigma;         // [B][N_SIGMA]                                    (MODEL_SIGMA4)
  std::vector<double> L, scale, sigma_uv;   // [B][L_SIZE], [B], [B][2]                 (MODEL_Q)
  // per frame and trajectory the first entry in the expanded block, [frames][B] (a prefix sum of entries(seq_of[b], f)), and the
  // frame's entries; filled by index_trajectories()
  std::vector<int> base; std::vector<size_t> nf;
  size_t largest = 0;                // entries of the largest expanded frame
  bool planned = false;              // base / nf / largest match the cells and the assignment
  bool walk_planned = false;         // the caller's walk table (MODEL_Q) matches the cells and the assignment: set by the caller
                                     // when it has tabulated it, cleared here by whatever the table depends on
  // the fault record (FAULTS above): [B][N_FAULT], empty: none set; faulted: some trajectory has a non-zero probability;
  // faults_uploaded: the caller's device copy is this record (set by the caller, cleared here)
  std::vector<double> fault; bool faulted = false, faults_uploaded = false;
  // the timing record (TIMING above): [B][N_TIMING], empty: none set; timed: some trajectory's record is non-zero;
  // timing_uploaded as faults_uploaded.  The image tables, built by commit(): per sequence img_n[s] images with
  // img_time / img_frame [S][frames] (row s, the first img_n[s] filled) and per cell img_base / img_W [frames][S]
  // (W: the window the cell's slots index, after the frame's own image joined it)
  std::vector<double> timing; bool timed = false, timing_uploaded = false;
  std::vector<double> img_time; std::vector<int> img_frame, img_base, img_W, img_n;
  std::string timing_why;            // the text of the last timing_precondition() refusal
  // the calibration records (CALIB above): [B][IMU_CAL] and [B][CAM_CAL], empty: none set; imu_calibrated / cam_calibrated:
  // some trajectory's record is non-trivial; calib_uploaded as faults_uploaded
  std::vector<double> imucal, camcal; bool imu_calibrated = false, cam_calibrated = false, calib_uploaded = false;
  bool calibrated() const { return imu_calibrated || cam_calibrated; }

  int frames() const { return seq.frames; }
  int K() const { return seq.lay.K; }
  size_t cell(int f, int s) const { return (size_t)f * S + s; }
  size_t entries(int s, int f) const { return seq.slots[cell(f, s)].size(); }
  // the ordinary frame block the kernel fills, for a handle whose scalars have esz bytes
  FrameLayout out_layout(size_t esz) const { return FrameLayout(B, K(), f_cap, esz); }
  size_t block_bytes(size_t esz) const { return out_layout(esz).bytes(largest); }

  // -- staging the sequences
  static Refusal alloc_refusal(int n_seq, int n_frames, int K) {
    if (n_seq <= 0 || n_frames <= 0 || K <= 0) return {-EINVAL, "bad replay size"};
    return {0, nullptr};
  }
  void alloc(int n_seq, int n_frames, int K, int B_, int f_cap_) {
    S = n_seq; B = B_; f_cap = f_cap_;
    seq.reset(n_frames, n_seq, K, f_cap_, sizeof(double));
    committed = assigned = planned = walk_planned = false; model = MODEL_SIGMA4;
    seq_of.clear(); seed.clear(); sigma.clear(); L.clear(); scale.clear(); sigma_uv.clear(); base.clear(); nf.clear(); largest = 0;
    fault.clear(); faulted = faults_uploaded = false;
    timing.clear(); timed = timing_uploaded = false;
    img_time.clear(); img_frame.clear(); img_base.clear(); img_W.clear(); img_n.clear();
    imucal.clear(); camcal.clear(); imu_calibrated = cam_calibrated = calib_uploaded = false;
  }
  // the rules of one sequence cell, in scenario_set_cell's order: its place, the work-list rules, the drop, the cell rule, the readings
  Refusal cell_refusal(int f, int s, const double* rd, int k, int F, const int* M, const int* slots, int n_drop, int flags, int m_cap, int n_cap) const {
    if (f < 0 || f >= seq.frames || s < 0 || s >= S) return {-EINVAL, "replay cell out of range"};
    const Refusal r = msckf_inputs::worklist_refusal(F, M, slots, f_cap, m_cap, n_cap);
    if (r.code) return r;
    if (n_drop < 0) return {-EINVAL, "negative n_drop"};
    if (const char* why = msckf_lists::cell_refusal(k, K(), F, n_drop, flags)) return {-EINVAL, why};
    if (k > 0 && !rd) return {-EINVAL, "null readings for a cell with samples"};
    return {0, nullptr};
  }
  void set_cell(int f, int s, const double* rd, int k, int F, const int* M, const int* slots, const double* obs, int n_drop, int flags) {
    seq.set_cell<double>(f, s, rd, k, (flags & msckf_lists::CELL_SKIP) != 0, F, M, slots, obs, n_drop);
    committed = planned = walk_planned = false;
  }
  Refusal commit_refusal() const {
    if (seq.frames <= 0) return {-EINVAL, "no replay allocated"};
    return {0, nullptr};
  }
  // every off and the frame index of the sequence store (ScenarioStore::index: a frame of S cells cannot pass 2^31 entries
  // unless an expanded one does, which index_trajectories refuses)
  Refusal commit() {
    if (!seq.index()) return {-E2BIG, "a frame's sequence work-lists exceed 2^31 observations"};
    build_image_table();
    if (timed) if (const Refusal r = timing_precondition(); r.code) return r;
    committed = true; planned = walk_planned = false;
    return {0, nullptr};
  }
  // the image table of every sequence (TIMING), a pure function of the cells
  void build_image_table() {
    using namespace msckf_inputs;
    const int F = seq.frames, K_ = K();
    img_time.assign((size_t)S * F, 0.0); img_frame.assign((size_t)S * F, 0); img_base.assign((size_t)F * S, 0); img_W.assign((size_t)F * S, 0); img_n.assign(S, 0);
    const double* rd = reinterpret_cast<const double*>(seq.fixed[SEC_RD].data());
    for (int s = 0; s < S; ++s) {
      double T = 0.0;
      int ord = 0, W = 0;
      for (int f = 0; f < F; ++f) {
        const size_t c = cell(f, s);
        const int k = seq.ints(SEC_K)[c];
        if (k != NO_IMAGE) {
          for (int i = 0; i < k; ++i) T += rd[(c * K_ + i) * RD_ROW + 6];
          ++ord; ++W;
          img_time[(size_t)s * F + ord - 1] = T; img_frame[(size_t)s * F + ord - 1] = f;
        }
        img_base[c] = ord - W; img_W[c] = k != NO_IMAGE ? W : 0;
        if (k != NO_IMAGE) W -= seq.ints(SEC_DROP)[c];
      }
      img_n[s] = ord;
    }
  }
  // what the shift asks of the committed cells (TIMING, refused), in this order per sequence, frame and track
  Refusal timing_precondition() {
    using namespace msckf_inputs;
    const int F = seq.frames;
    auto refuse = [&](const char* what, int s, int f, int t) {
      char buf[160];
      std::snprintf(buf, sizeof buf, "timing: sequence %d, frame %d, track %d: %s", s, f, t, what);
      timing_why = buf;
      return Refusal{-EINVAL, timing_why.c_str()};
    };
    for (int s = 0; s < S; ++s) for (int f = 0; f < F; ++f) {
      const size_t c = cell(f, s);
      const int n = seq.ints(SEC_N)[c], base_ = img_base[c], W = img_W[c];
      const int* sl = seq.slots[c].data();
      const double* tm = img_time.data() + (size_t)s * F;
      for (int t = 0, o = 0; t < n; ++t) {
        const int M = seq.ints(SEC_M)[c * f_cap + t];
        for (int l = 0; l < M; ++l) if (sl[o + l] < 0 || sl[o + l] >= W) return refuse("a camera slot beyond the window an empty start gives", s, f, t);
        for (int l = 1; l < M; ++l) if (sl[o + l] <= sl[o + l - 1]) return refuse("camera slots do not ascend strictly", s, f, t);
        for (int l = 1; l < M; ++l) if (!(tm[base_ + sl[o + l]] > tm[base_ + sl[o + l - 1]])) return refuse("node times do not increase strictly", s, f, t);
        o += M;
      }
    }
    return {0, nullptr};
  }

  // -- the assignment
  Refusal assign_refusal(const int* seq_of_, const double* sigma4) const {
    if (seq.frames <= 0) return {-EINVAL, "no replay allocated"};
    for (int b = 0; b < B; ++b) if (seq_of_[b] < 0 || seq_of_[b] >= S) return {-EINVAL, "seq_of names no sequence of the replay"};
    for (int i = 0; i < B * N_SIGMA; ++i) if (!(sigma4[i] >= 0.0) || !std::isfinite(sigma4[i])) return {-EINVAL, "sigma must be finite and not negative"};
    return {0, nullptr};
  }
  void assign(const int* seq_of_, const uint64_t* seed_, const double* sigma4) {
    seq_of.assign(seq_of_, seq_of_ + B); seed.assign(seed_, seed_ + B); sigma.assign(sigma4, sigma4 + (size_t)B * N_SIGMA);
    assigned = true; planned = walk_planned = false; model = MODEL_SIGMA4;
  }
  // the model's assignment, in this order: the sequence, every entry finite, nothing negative, Q positive semi-definite
  Refusal assign_q_refusal(const int* seq_of_, const double* Q144, const double* scale_, const double* sigma_uv_) const {
    if (seq.frames <= 0) return {-EINVAL, "no replay allocated"};
    for (int b = 0; b < B; ++b) if (seq_of_[b] < 0 || seq_of_[b] >= S) return {-EINVAL, "seq_of names no sequence of the replay"};
    for (size_t i = 0; i < (size_t)B * L_SIZE; ++i) if (!std::isfinite(Q144[i])) return {-EINVAL, "Q, scale and sigma must be finite"};
    for (int b = 0; b < B; ++b) if (!std::isfinite(scale_[b]) || !std::isfinite(sigma_uv_[2 * b]) || !std::isfinite(sigma_uv_[2 * b + 1])) return {-EINVAL, "Q, scale and sigma must be finite"};
    for (int b = 0; b < B; ++b) if (scale_[b] < 0.0 || sigma_uv_[2 * b] < 0.0 || sigma_uv_[2 * b + 1] < 0.0) return {-EINVAL, "scale and sigma must not be negative"};
    double Lb[L_SIZE];
    for (int b = 0; b < B; ++b) if (!chol_psd(Q144 + (size_t)b * L_SIZE, Lb)) return {-EINVAL, "Q is not positive semi-definite"};
    return {0, nullptr};
  }
  void assign_q(const int* seq_of_, const uint64_t* seed_, const double* Q144, const double* scale_, const double* sigma_uv_) {
    seq_of.assign(seq_of_, seq_of_ + B); seed.assign(seed_, seed_ + B); scale.assign(scale_, scale_ + B); sigma_uv.assign(sigma_uv_, sigma_uv_ + (size_t)2 * B);
    L.assign((size_t)B * L_SIZE, 0.0);
    for (int b = 0; b < B; ++b) (void)chol_psd(Q144 + (size_t)b * L_SIZE, L.data() + (size_t)b * L_SIZE);
    assigned = true; planned = walk_planned = false; model = MODEL_Q;
  }
  // the fault record (FAULTS), fault4 [B][N_FAULT] or null for none, in this order: the replay, the probabilities, the radii
  Refusal faults_refusal(const double* fault4) const {
    if (seq.frames <= 0) return {-EINVAL, "no replay allocated"};
    if (!fault4) return {0, nullptr};
    for (int b = 0; b < B; ++b) for (int c : {FLT_P_MISS, FLT_P_OUT}) if (!(fault4[b * N_FAULT + c] >= 0.0 && fault4[b * N_FAULT + c] <= 1.0)) return {-EINVAL, "fault probabilities must lie in [0, 1]"};
    for (int b = 0; b < B; ++b) for (int c : {FLT_RHO_U, FLT_RHO_V}) if (!(fault4[b * N_FAULT + c] >= 0.0) || !std::isfinite(fault4[b * N_FAULT + c])) return {-EINVAL, "fault radii must be finite and not negative"};
    return {0, nullptr};
  }
  // independent of the assignment and of the cells: it stays through assign, assign_q and commit, and alloc() clears it
  void set_faults(const double* fault4) {
    if (fault4) fault.assign(fault4, fault4 + (size_t)B * N_FAULT); else fault.clear();
    faulted = false;
    for (size_t b = 0; b * N_FAULT < fault.size(); ++b) faulted = faulted || fault[b * N_FAULT + FLT_P_MISS] > 0.0 || fault[b * N_FAULT + FLT_P_OUT] > 0.0;
    faults_uploaded = false;
  }
  // the timing record (TIMING), timing4 [B][N_TIMING] or null for none, in this order: the replay, every value finite, the
  // jitter, and -- on committed cells under a non-zero record -- the preconditions of the shift
  static bool nonzero_timing(const double* timing4, int B_) {
    for (int b = 0; timing4 && b < B_; ++b) if (timing4[b * N_TIMING + TIM_TD] != 0.0 || timing4[b * N_TIMING + TIM_RY] != 0.0 || timing4[b * N_TIMING + TIM_SIGMA_J] != 0.0) return true;
    return false;
  }
  Refusal timing_refusal(const double* timing4) {
    if (seq.frames <= 0) return {-EINVAL, "no replay allocated"};
    if (!timing4) return {0, nullptr};
    for (int i = 0; i < B * N_TIMING; ++i) if (!std::isfinite(timing4[i])) return {-EINVAL, "timing values must be finite"};
    for (int b = 0; b < B; ++b) if (timing4[b * N_TIMING + TIM_SIGMA_J] < 0.0) return {-EINVAL, "jitter must not be negative"};
    if (committed && nonzero_timing(timing4, B)) return timing_precondition();
    return {0, nullptr};
  }
  // independent of the assignment, the faults and the cells: it stays through assign, assign_q, set_faults and commit, and
  // alloc() clears it
  void set_timing(const double* timing4) {
    if (timing4) timing.assign(timing4, timing4 + (size_t)B * N_TIMING); else timing.clear();
    timed = nonzero_timing(timing.empty() ? nullptr : timing.data(), B);
    timing_uploaded = false;
  }
  // the calibration records (CALIB), imucal [B][IMU_CAL] / camcal [B][CAM_CAL] or null for none, in this order: the replay,
  // every value finite, and for the IMU record the saturation levels and quantisation steps
  Refusal imu_calib_refusal(const double* ic) const {
    if (seq.frames <= 0) return {-EINVAL, "no replay allocated"};
    if (!ic) return {0, nullptr};
    for (int i = 0; i < B * IMU_CAL; ++i) if (!std::isfinite(ic[i])) return {-EINVAL, "calibration values must be finite"};
    for (int b = 0; b < B; ++b) for (int c = IC_SAT_G; c < IMU_CAL; ++c) if (ic[b * IMU_CAL + c] < 0.0) return {-EINVAL, "saturation and quantisation must not be negative"};
    return {0, nullptr};
  }
  Refusal cam_calib_refusal(const double* cc) const {
    if (seq.frames <= 0) return {-EINVAL, "no replay allocated"};
    if (!cc) return {0, nullptr};
    for (int i = 0; i < B * CAM_CAL; ++i) if (!std::isfinite(cc[i])) return {-EINVAL, "calibration values must be finite"};
    return {0, nullptr};
  }
  static bool nontrivial_imu_calib(const double* ic, int B_) {
    double id[IMU_CAL];
    imu_calib_identity(id);
    for (int b = 0; ic && b < B_; ++b) for (int i = 0; i < IMU_CAL; ++i) if (ic[b * IMU_CAL + i] != id[i]) return true;
    return false;
  }
  static bool nontrivial_cam_calib(const double* cc, int B_) {
    for (int i = 0; cc && i < B_ * CAM_CAL; ++i) if (cc[i] != 0.0) return true;
    return false;
  }
  // independent of the assignment, the faults, the timing and the cells: they stay through assign, assign_q, set_faults,
  // set_timing and commit, and alloc() clears them
  void set_imu_calib(const double* ic) {
    if (ic) imucal.assign(ic, ic + (size_t)B * IMU_CAL); else imucal.clear();
    imu_calibrated = nontrivial_imu_calib(imucal.empty() ? nullptr : imucal.data(), B);
    calib_uploaded = false;
  }
  void set_cam_calib(const double* cc) {
    if (cc) camcal.assign(cc, cc + (size_t)B * CAM_CAL); else camcal.clear();
    cam_calibrated = nontrivial_cam_calib(camcal.empty() ? nullptr : camcal.data(), B);
    calib_uploaded = false;
  }

  // -- a run
  // in run_frames' order: the range, then what has to have happened before
  Refusal run_refusal(int f0, int f1) const {
    if (f0 < 0 || f1 > seq.frames || f0 > f1) return {-EINVAL, "frame range out of bounds"};
    if (!committed) return {-EINVAL, "replay not committed"};
    if (!assigned) return {-EINVAL, "replay not assigned"};
    return {0, nullptr};
  }
  // msckf_hip_replay_imu_sums reads what a run over [f0, f1) would expand: a run's refusals, in a run's order
  Refusal sums_refusal(int f0, int f1) const { return run_refusal(f0, f1); }
  Refusal expand_refusal(int f, int b) const {
    if (const Refusal r = run_refusal(0, seq.frames); r.code) return r;
    if (f < 0 || f >= seq.frames || b < 0 || b >= B) return {-EINVAL, "replay cell out of range"};
    return {0, nullptr};
  }
  // rows [f0, f1) of the walk table (frames + 1 rows) for the trajectories [b0, b0 + nb): the ranges, then what has to have happened
  Refusal walk_refusal(int f0, int f1, int b0, int nb) const {
    if (seq.frames <= 0) return {-EINVAL, "no replay allocated"};
    if (f0 < 0 || f1 > seq.frames + 1 || f0 > f1 || b0 < 0 || nb < 0 || b0 + nb > B) return {-EINVAL, "walk range out of bounds"};
    if (!committed) return {-EINVAL, "replay not committed"};
    if (!assigned || model != MODEL_Q) return {-EINVAL, "replay not assigned through msckf_hip_replay_assign_q"};
    return {0, nullptr};
  }
  // base, nf and largest from the committed cells and the assignment
  Refusal index_trajectories() {
    if (planned) return {0, nullptr};
    base.assign((size_t)seq.frames * B, 0); nf.assign(seq.frames, 0); largest = 0;
    for (int f = 0; f < seq.frames; ++f) {
      size_t o = 0;
      for (int b = 0; b < B; ++b) { base[(size_t)f * B + b] = (int)o; o += entries(seq_of[b], f); if (o > 0x7fffffffu) return {-E2BIG, "an expanded frame's work-lists exceed 2^31 observations"}; }
      nf[f] = o;
      largest = std::max(largest, o);
    }
    planned = true;
    return {0, nullptr};
  }
  // what the frame step reads on the host of trajectory b's cell: its sequence's
  size_t cell_of(int f, int b) const { return cell(f, seq_of[b]); }
};

}  // namespace msckf_replay

#endif  // MSCKF_REPLAY_PLAN_H
