// kernels_log.hip -- the per-frame device log of run_frames / run_frames_streamed and its reduction against ground truth.
//
// k_frame_log copies what a caller would read with the getters after a frame -- the first 16 scalars of the IMU state, the
// diagonal of P_II, the position block of P, the window size, three statistics and the pose of camera slot 0 -- into one
// record of LOG_STRIDE scalars per trajectory.  It runs on the slice's stream after the frame's update and prune, only
// reads the filter's arrays and only writes the log: the filter cannot see whether it ran.
// k_log_metrics reduces a range of records against ground-truth positions: the sums behind ATE and NEES, per trajectory.
// k_map_log is the per-track counterpart: the frame's triangulated landmarks with their gate statistics, compacted inside
// the wavefront behind a per-trajectory cursor; k_map_metrics reduces them against ground-truth landmarks.
// k_pruned_log records the camera states a frame is about to prune, between the frame's update and its prune launch: the
// posterior pose with its 6 x 6 covariance block, the fixed-lag smoothed trajectory; k_pruned_metrics reduces them against
// ground-truth poses.
// k_nees_log is the consistency counterpart of k_frame_log: the 15-state NEES of the IMU state against a resident truth table,
// whole and per 3 x 3 block, one record of 8 doubles per frame and trajectory; k_nees_ensemble reduces those records over groups
// of trajectories (the seeds of a sequence) at each frame: the sums behind the ANEES curves.
#include "dev_common.h"
#include "nees_plan.h"
#include "replay_plan.h"

namespace msckf {

// four scalars with the alignment of one 16-byte (float) / two 16-byte (double) vector accesses
template <class S> struct alignas(4 * sizeof(S)) Vec4 { S x[4]; };

// The log kernels of the frame path run one wavefront per trajectory, four per workgroup: the lane, and the trajectory's index
// i within the slice's nb.  False: the wavefront has no trajectory and leaves as a whole.
__device__ __forceinline__ bool log_wave(int nb, int& lane, int& i) {
  lane = threadIdx.x & 63; i = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  return i < nb;
}
// The cursor of a cursor log, found[b]: records found so far, stored or not.  The trajectory belongs to one slice and its
// frames are ordered on that slice's stream: lane 0 reads the cursor (every lane gets it) and stores it back, no atomics.  A
// record whose destination is >= cap is counted but not stored, so the stored ones are the first cap in order.
__device__ __forceinline__ long cursor_read(const int* found, int b, int lane) {
  int cur = 0;
  if (lane == 0) cur = found[b];
  return wave_bcast(cur, 0);
}
__device__ __forceinline__ void cursor_store(int* found, int b, int lane, long end) { if (lane == 0) found[b] = (int)min(end, (long)INT32_MAX); }
// What the metrics kernels of a cursor log walk: the records stored, and of those the ones stamped with an ordinal in [q0, q1)
__device__ __forceinline__ int cursor_stored(const int* found, int b, int cap) { return min(max(found[b], 0), cap); }
__device__ __forceinline__ bool ordinal_in(int fr, int q0, int q1) { return fr >= q0 && fr < q1; }

// One wavefront per trajectory, four per workgroup.  Record index (include/msckf_hip.h, "frame log record"):
//   0..15 imu[0..15] | 16..30 diag P_II | 31..36 P_pp xx xy xz yy yz zz | 37 window size | 38..40 STAT_NTRACKS, _PASSED, _ERR |
//   41..47 cam slot 0 (zeros when the window is empty)
// Lanes 0..3 move the IMU part as aligned 4-vectors; lanes 16..47 load one scalar each (value = record index of the lane),
// lanes 4..11 collect four of them over the LDS crossbar; the twelve lanes 0..11 store the record as 4-vectors.
// P: the covariance buffer that is current after the frame; pending: the frame's prune rode on the downdate, the window
// size waits in ncam_upd (as size + 1) and ncam is still the size before the prune.
template <class S>
__global__ __launch_bounds__(256) void k_frame_log(Dev<S> d, int b0, int nb, const S* P, int pending, S* rec) {
  int lane, i;
  if (!log_wave(nb, lane, i)) return;
  const int b = b0 + i;
  const int n = pending ? d.ncam_upd[b] - 1 : d.ncam[b];
  const S* Pb = P + (long)b * d.ld * d.ld;
  S v = S(0);
  if (lane >= LOG_PII && lane < LOG_PPP) { const int k = lane - LOG_PII; v = Pb[(long)k * d.ld + k]; }
  else if (lane >= LOG_PPP && lane < LOG_NCAM) {
    const int k = lane - LOG_PPP;                                    // xx xy xz yy yz zz: element (r, c), r <= c
    const int r = k < 3 ? 0 : (k < 5 ? 1 : 2), c = k < 3 ? k : (k < 5 ? k - 2 : 2);
    v = Pb[(long)(12 + c) * d.ld + 12 + r];
  }
  else if (lane == LOG_NCAM) v = (S)n;
  else if (lane > LOG_NCAM && lane < LOG_CAM0) {
    const int k = lane - LOG_STATS;
    v = (S)d.stats[(long)b * STAT_STRIDE + (k == 0 ? STAT_NTRACKS : (k == 1 ? STAT_PASSED : STAT_ERR))];
  }
  else if (lane >= LOG_CAM0 && lane < LOG_STRIDE && n > 0) v = d.cam[(long)b * d.n_cap * CAM_STRIDE + (lane - LOG_CAM0)];
  Vec4<S> o = {};
  if (lane < 4) o = *reinterpret_cast<const Vec4<S>*>(d.imu + (long)b * IMU_STRIDE + 4 * lane);
#pragma unroll
  for (int k = 0; k < 4; ++k) {   // (every lane takes part in the exchange)
    const S g = lane_gather(v, ((4 * lane + k) & 63) << 2);
    if (lane >= 4) o.x[k] = g;
  }
  if (lane < LOG_STRIDE / 4) *reinterpret_cast<Vec4<S>*>(rec + (long)b * LOG_STRIDE + 4 * lane) = o;
}

// One workgroup (one wavefront) per trajectory over the records [r0, r1) of the log ([.][B][LOG_STRIDE]), ground truth
// gt[r1 - r0][B][3].  out[b][6] = n, sum |e|^2, max |e|, |e| at r1 - 1, sum e^T P_pp^-1 e, records with STAT_ERR != 0;
// e = p - p_gt, no alignment.  All in f64; lane l takes the records r0 + l, r0 + l + 64, ... in ascending order and the
// lanes are combined by wave_sum's fixed tree, so the same log gives the same bits on every call.  P_pp = L L^T by
// Cholesky, e^T P_pp^-1 e = |L^-1 e|^2 (a P_pp that is not positive definite gives NaN there).
// r0b / r1b (both or neither): the trajectory's own range [r0b[b], r1b[b]) inside [r0, r1) -- sequences of unequal length
// leave their skipped tail out; the ground truth is still indexed from r0.  Null: [r0, r1) for every trajectory.
template <class S>
__global__ __launch_bounds__(64) void k_log_metrics(const S* log, int B, int r0, int r1, const int* r0b, const int* r1b, const double* gt, double* out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int rg = r0;                       // the ground truth's first record
  if (r0b) { r0 = r0b[b]; r1 = r1b[b]; }
  double s2 = 0, mx = 0, last = 0, nees = 0, nerr = 0, cnt = 0;
  for (int r = r0 + lane; r < r1; r += 64) {
    const S* q = log + ((long)r * B + b) * LOG_STRIDE;
    const double* g = gt + ((long)(r - rg) * B + b) * 3;
    const double e0 = (double)q[IP] - g[0], e1 = (double)q[IP + 1] - g[1], e2 = (double)q[IP + 2] - g[2];
    const double d2 = e0 * e0 + e1 * e1 + e2 * e2, dist = sqrt(d2);
    const double pxx = (double)q[LOG_PPP], pxy = (double)q[LOG_PPP + 1], pxz = (double)q[LOG_PPP + 2];
    const double pyy = (double)q[LOG_PPP + 3], pyz = (double)q[LOG_PPP + 4], pzz = (double)q[LOG_PPP + 5];
    const double l00 = sqrt(pxx), l10 = pxy / l00, l20 = pxz / l00;
    const double l11 = sqrt(pyy - l10 * l10), l21 = (pyz - l20 * l10) / l11;
    const double l22 = sqrt(pzz - l20 * l20 - l21 * l21);
    const double y0 = e0 / l00, y1 = (e1 - l10 * y0) / l11, y2 = (e2 - l20 * y0 - l21 * y1) / l22;
    s2 += d2; nees += y0 * y0 + y1 * y1 + y2 * y2; cnt += 1.0;
    mx = dist > mx ? dist : mx;
    if (r == r1 - 1) last = dist;
    if (q[LOG_STATS + 2] != S(0)) nerr += 1.0;
  }
  cnt = wave_sum(cnt); s2 = wave_sum(s2); mx = wave_max(mx); last = wave_sum(last); nees = wave_sum(nees); nerr = wave_sum(nerr);
  if (lane == 0) {
    double* o = out + (long)b * 6;
    o[0] = cnt; o[1] = s2; o[2] = mx; o[3] = last; o[4] = nees; o[5] = nerr;
  }
}

// The map log: the frame's triangulated landmarks and gate statistics, one record of MAP_STRIDE scalars per track that
// append_map (host_lists.h) would take -- motion check passed or skipped, triangulation valid -- compacted in track order
// behind the trajectory's cursor found[b].  One wavefront per trajectory, four per workgroup, launched for the slice
// [b0, b0 + nb) after the frame's update; n / M: the work-list counts the update read (already offset to b0).  A skipped cell
// has n == 0, so nothing of the stale per-track arrays is logged.  Record index (include/msckf_hip.h, "map log record"):
//   0..2 p_f_G | 3 gamma | 4 frame ordinal | 5 track index | 6 flags (1 gate passed, 2 included, 4 gamma is the early-accept
//   bound) | 7 M
// The wavefront walks the tracks in chunks of 64: ballot of the keep flag, rank = kept lanes below, destination = cursor +
// kept of the earlier chunks + rank (cursor_read: the records stored are the first cap in (frame, track) order).
template <class S>
__global__ __launch_bounds__(256) void k_map_log(Dev<S> d, int b0, int nb, const int* n, const int* M, int ordinal, int cap, S* rec, int* found) {
  int lane, i;
  if (!log_wave(nb, lane, i)) return;
  const int b = b0 + i;
  const int F = min(max(n[i], 0), d.f_cap);
  if (F == 0) return;
  long base = cursor_read(found, b, lane);
  const long first = (long)b * cap;
  for (int t0 = 0; t0 < F; t0 += 64) {
    const int t = t0 + lane;
    const long tb = (long)b * d.f_cap + t;
    const int st = t < F ? d.trk_status[tb] : 0;
    const bool keep = (st & (ST_MOTION_OK | ST_MOTION_SKIPPED)) && (st & ST_TRI_VALID);
    const unsigned long long mask = __ballot(keep ? 1 : 0);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    const long dst = base + rank;
    if (keep && dst < cap) {
      Vec4<S> a = *reinterpret_cast<const Vec4<S>*>(d.trk_pf + tb * 4), c;
      a.x[3] = d.trk_gamma[tb];
      c.x[0] = (S)ordinal; c.x[1] = (S)t;
      c.x[2] = (S)(((st & ST_GATE_PASS) ? MAP_FLAG_PASS : 0) | ((st & ST_INCLUDED) ? MAP_FLAG_INCLUDED : 0) | ((st & ST_GATE_BOUND) ? MAP_FLAG_BOUND : 0));
      c.x[3] = (S)M[(long)i * d.f_cap + t];
      Vec4<S>* o = reinterpret_cast<Vec4<S>*>(rec + (first + dst) * MAP_STRIDE);
      o[0] = a; o[1] = c;
    }
    base += __popcll(mask);
  }
  cursor_store(found, b, lane, base);
}

// One workgroup (one wavefront) per trajectory over the stored records of the map log whose frame ordinal lies in [q0, q1).
// Ground truth (gt and off both null: none): off is CSR over the cells (frame - q0) * B + b, the landmark of a record is
// gt[off[cell] + track]; a record whose track index is >= its cell's length is unmatched.
// out[b][8] = records in range, matched, sum |e|^2, max |e|, gate-passed records whose gamma is not the early-accept bound,
// sum of gamma and sum of 2 M - 3 over those, unmatched.  All in f64; lane l takes the records l, l + 64, ... in ascending
// order and the lanes are combined by wave_sum's fixed tree: the same log gives the same bits on every call.
template <class S>
__global__ __launch_bounds__(64) void k_map_metrics(const S* rec, const int* found, int cap, int B, int q0, int q1, const double* gt, const int* off, double* out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = cursor_stored(found, b, cap);
  double cnt = 0, nm = 0, s2 = 0, mx = 0, ng = 0, sg = 0, sd = 0, un = 0;
  for (int r = lane; r < n; r += 64) {
    const Vec4<S>* q = reinterpret_cast<const Vec4<S>*>(rec + ((long)b * cap + r) * MAP_STRIDE);
    const Vec4<S> a = q[0], c = q[1];
    const int fr = (int)c.x[0], trk = (int)c.x[1], flags = (int)c.x[2];
    if (!ordinal_in(fr, q0, q1)) continue;
    cnt += 1.0;
    if (gt) {
      const long cell = (long)(fr - q0) * B + b;
      const int o0 = off[cell], len = off[cell + 1] - o0;
      if (trk >= len) un += 1.0;
      else {
        const double* g = gt + ((long)o0 + trk) * 3;
        const double e0 = (double)a.x[0] - g[0], e1 = (double)a.x[1] - g[1], e2 = (double)a.x[2] - g[2];
        const double d2 = e0 * e0 + e1 * e1 + e2 * e2, dist = sqrt(d2);
        nm += 1.0; s2 += d2;
        mx = dist > mx ? dist : mx;
      }
    }
    if ((flags & MAP_FLAG_PASS) && !(flags & MAP_FLAG_BOUND)) { ng += 1.0; sg += (double)a.x[3]; sd += 2.0 * (double)c.x[3] - 3.0; }
  }
  cnt = wave_sum(cnt); nm = wave_sum(nm); s2 = wave_sum(s2); mx = wave_max(mx); ng = wave_sum(ng); sg = wave_sum(sg); sd = wave_sum(sd); un = wave_sum(un);
  if (lane == 0) {
    double* o = out + (long)b * 8;
    o[0] = cnt; o[1] = nm; o[2] = s2; o[3] = mx; o[4] = ng; o[5] = sg; o[6] = sd; o[7] = un;
  }
}

// The gate's confusion table under the replay's faults (msckf_hip_map_log_fault_metrics; replay_plan.h, FAULTS): one workgroup
// (one wavefront) per trajectory over the stored records with frame ordinal in [q0, q1); the record with ordinal q belongs to
// replay frame f0 + (q - q0).  Whether its track carries an outlier is recomputed from (seed, frame, the sequence cell's
// off / M, fault4) with rp::track_faults; fault == null: nothing does.  n / M / off: the sequence store's sections from frame 0.
// out[b][8] = records in range, clean and passed, clean and rejected, contaminated and passed, contaminated and rejected,
// sum gamma and sum 2 M - 3 (M: the record's, the survivors) over the clean passed records whose gamma is not the early-accept
// bound, records whose track index is >= the cell's n (unmatched, counted in column 0 only).  All in f64, records l, l + 64, ...
// in ascending order per lane, the lanes combined by wave_sum's fixed tree: the same log gives the same bits on every call.
template <class S>
__global__ __launch_bounds__(64) void k_map_fault_metrics(const S* rec, const int* found, int cap, int q0, int q1, int f0, const int* n, const int* M, const int* off,
                                                          const int* seq_of, const uint64_t* seed, const double* fault, int n_seq, int f_cap, double* out) {
  namespace rp = msckf_replay;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int stored = cursor_stored(found, b, cap);
  const int s = seq_of[b];
  const uint64_t sd = seed[b];
  const double p_miss = fault ? fault[(long)b * rp::N_FAULT + rp::FLT_P_MISS] : 0.0, p_out = fault ? fault[(long)b * rp::N_FAULT + rp::FLT_P_OUT] : 0.0;
  double c[rp::N_FAULT_METRIC] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = lane; r < stored; r += 64) {
    const Vec4<S>* q = reinterpret_cast<const Vec4<S>*>(rec + ((long)b * cap + r) * MAP_STRIDE);
    const Vec4<S> a = q[0], w = q[1];
    const int fr = (int)w.x[0], trk = (int)w.x[1], flags = (int)w.x[2];
    if (!ordinal_in(fr, q0, q1)) continue;
    c[rp::FM_RECORDS] += 1.0;
    const int f = f0 + (fr - q0);
    const long cell = (long)f * n_seq + s;
    if (trk < 0 || trk >= n[cell]) { c[rp::FM_UNMATCHED] += 1.0; continue; }
    const int e0 = off[cell * f_cap + trk] - off[cell * f_cap];
    const bool dirty = p_out > 0.0 && rp::track_faults(rp::fault_seed(sd, f), (uint64_t)e0, M[cell * f_cap + trk], p_miss, p_out).outliers > 0;
    const bool pass = (flags & MAP_FLAG_PASS) != 0;
    c[rp::FM_CLEAN_PASS] += !dirty && pass ? 1.0 : 0.0; c[rp::FM_CLEAN_REJ] += !dirty && !pass ? 1.0 : 0.0;
    c[rp::FM_CONT_PASS] += dirty && pass ? 1.0 : 0.0; c[rp::FM_CONT_REJ] += dirty && !pass ? 1.0 : 0.0;
    if (!dirty && pass && !(flags & MAP_FLAG_BOUND)) { c[rp::FM_SUM_GAMMA] += (double)a.x[3]; c[rp::FM_SUM_DOF] += 2.0 * (double)w.x[3] - 3.0; }
  }
#pragma unroll
  for (int i = 0; i < rp::N_FAULT_METRIC; ++i) {
    const double v = wave_sum(c[i]);
    if (lane == 0) out[(long)b * rp::N_FAULT_METRIC + i] = v;
  }
}

// The pruned-state log: the camera states that the frame's prune drops, as the frame's update left them -- one record of
// PRN_STRIDE scalars per dropped state, in (frame, slot) order behind the trajectory's cursor found[b].  One wavefront per
// trajectory, four per workgroup, launched for the slice [b0, b0 + nb) between the frame's update and its k_prune_inplace
// launch: d.P is the posterior covariance in place, d.cam the corrected camera states, d.ncam the window size before the prune.
// drop (already offset to b0): the cell's n_drop, clamped to 0 .. window size as k_prune_inplace / k_make_keep clamp it; the
// dropped states are the slots 0 .. nd - 1.  A skipped cell has n_drop == 0 (cell_refusal): it and a cell that drops nothing
// write nothing, not even the cursor.  Record index (include/msckf_hip.h, "pruned-state log record"):
//   0..3 q_CG | 4..6 p_C_G | 7 prune frame ordinal | 8..28 upper triangle of P[15 + 6 k .. 15 + 6 k + 5]^2 row by row |
//   29 window size before the prune | 30 k, the dropped slot | 31 zero
// Two records per step: lane = 32 * (record of the pair) + record index loads one scalar, the sixteen lanes 0..15 collect four
// each over the LDS crossbar (lane l: scalars 4 l .. 4 l + 3 of the pair) and store them as aligned 4-vectors, behind the
// cursor (cursor_read).
template <class S>
__global__ __launch_bounds__(256) void k_pruned_log(Dev<S> d, int b0, int nb, const int* drop, int ordinal, int cap, S* rec, int* found) {
  int lane, i;
  if (!log_wave(nb, lane, i)) return;
  const int b = b0 + i;
  const int n = min(d.ncam[b], d.n_cap);
  int nd = drop[i];
  nd = nd < 0 ? 0 : (nd > n ? n : nd);
  if (nd == 0) return;
  const long base = cursor_read(found, b, lane);
  const int half = lane >> 5, j = lane & 31;
  const int t = j - PRN_COV;                                         // triangle entry t = (r, c), r <= c: row r starts at r (13 - r) / 2
  const int r = t < 6 ? 0 : (t < 11 ? 1 : (t < 15 ? 2 : (t < 18 ? 3 : (t < 20 ? 4 : 5))));
  const int c = t - r * (13 - r) / 2 + r;
  const S* Pb = d.P + (long)b * d.ld * d.ld;
  const S* cam = d.cam + (long)b * d.n_cap * CAM_STRIDE;
  for (int k0 = 0; k0 < nd; k0 += 2) {
    const int k = k0 + half;
    S v = S(0);
    if (k < nd) {
      if (j < PRN_FRAME) v = cam[(long)k * CAM_STRIDE + j];
      else if (j == PRN_FRAME) v = (S)ordinal;
      else if (j < PRN_NCAM) { const int o = 15 + 6 * k; v = Pb[(long)(o + c) * d.ld + o + r]; }
      else if (j == PRN_NCAM) v = (S)n;
      else if (j == PRN_K) v = (S)k;
    }
    Vec4<S> o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o.x[e] = lane_gather(v, ((4 * lane + e) & 63) << 2);   // (every lane takes part in the exchange)
    const int ks = k0 + (lane >> 3);                                 // lanes 0..15: the record whose vector lane & 7 this lane stores
    const long dst = base + ks;
    if (lane < 16 && ks < nd && dst < cap) *reinterpret_cast<Vec4<S>*>(rec + ((long)b * cap + dst) * PRN_STRIDE + 4 * (lane & 7)) = o;
  }
  cursor_store(found, b, lane, base + nd);
}

// One workgroup (one wavefront) per trajectory over the stored records of the pruned-state log whose prune ordinal lies in
// [q0, q1).  aug[B][cap]: per stored record the ordinal of the frame that augmented its camera state, or -1; a record with
// 0 <= ordinal < n_ord is matched to the ground-truth pose gt[ordinal][B][7] (q_CG p_C_G), any other is unmatched.
// Pose error e = [e_th ; e_p]: e_p = p - p_gt, e_th the error-state angle of q_CG against the ground truth (error_angle).
// out[b][10] = records in range, matched, sum |e_p|^2, max |e_p|, sum |e_th|^2, max |e_th|, sum e^T P6^-1 e over the matched
// records whose logged block factors (6 x 6 Cholesky in registers, P6 = L L^T, |L^-1 e|^2), their number, the matched records
// with a non-positive pivot (left out of that sum), unmatched.  All in f64; lane l takes the records l, l + 64, ... in
// ascending order and the lanes are combined by wave_sum's fixed tree: the same log gives the same bits on every call.
template <class S>
__global__ __launch_bounds__(64) void k_pruned_metrics(const S* rec, const int* found, int cap, int B, int q0, int q1, const int* aug, const double* gt, int n_ord, double* out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = cursor_stored(found, b, cap);
  double cnt = 0, nm = 0, sp = 0, mp = 0, sth = 0, mth = 0, nees = 0, nn = 0, bad = 0, un = 0;
  for (int rr = lane; rr < n; rr += 64) {
    const Vec4<S>* q = reinterpret_cast<const Vec4<S>*>(rec + ((long)b * cap + rr) * PRN_STRIDE);
    double x[PRN_STRIDE];
#pragma unroll
    for (int v = 0; v < PRN_STRIDE / 4; ++v) {
      const Vec4<S> a = q[v];
#pragma unroll
      for (int e = 0; e < 4; ++e) x[4 * v + e] = (double)a.x[e];
    }
    const int fr = (int)x[PRN_FRAME];
    if (!ordinal_in(fr, q0, q1)) continue;
    cnt += 1.0;
    const int ord = aug[(long)b * cap + rr];
    if (ord < 0 || ord >= n_ord) { un += 1.0; continue; }
    const double* g = gt + ((long)ord * B + b) * 7;
    const V3<double> th = error_angle(ldq(x + PRN_Q), ldq(g));
    double e[6] = {th.x, th.y, th.z, x[PRN_P] - g[4], x[PRN_P + 1] - g[5], x[PRN_P + 2] - g[6]};
    const double t2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], p2 = e[3] * e[3] + e[4] * e[4] + e[5] * e[5];
    const double dt = sqrt(t2), dp = sqrt(p2);
    nm += 1.0; sp += p2; sth += t2;
    mp = dp > mp ? dp : mp; mth = dt > mth ? dt : mth;
    double L[6][6];
    bool ok = true;
    double y2 = 0;
#pragma unroll
    for (int jc = 0; jc < 6; ++jc) {                                   // column jc of L, then row jc of the forward solve
      double s = x[PRN_COV + jc * (13 - jc) / 2];
#pragma unroll
      for (int k = 0; k < jc; ++k) s -= L[jc][k] * L[jc][k];
      ok = ok && (s > 0);
      const double piv = sqrt(s);
      L[jc][jc] = piv;
#pragma unroll
      for (int ir = jc + 1; ir < 6; ++ir) {
        double a = x[PRN_COV + jc * (13 - jc) / 2 + (ir - jc)];
#pragma unroll
        for (int k = 0; k < jc; ++k) a -= L[ir][k] * L[jc][k];
        L[ir][jc] = a / piv;
      }
      double y = e[jc];
#pragma unroll
      for (int k = 0; k < jc; ++k) y -= L[jc][k] * e[k];
      e[jc] = y / piv;                                                 // (e is overwritten by L^-1 e from the top)
      y2 += e[jc] * e[jc];
    }
    if (ok) { nees += y2; nn += 1.0; } else bad += 1.0;
  }
  cnt = wave_sum(cnt); nm = wave_sum(nm); sp = wave_sum(sp); mp = wave_max(mp); sth = wave_sum(sth); mth = wave_max(mth);
  nees = wave_sum(nees); nn = wave_sum(nn); bad = wave_sum(bad); un = wave_sum(un);
  if (lane == 0) {
    double* o = out + (long)b * 10;
    o[0] = cnt; o[1] = nm; o[2] = sp; o[3] = mp; o[4] = sth; o[5] = mth; o[6] = nees; o[7] = nn; o[8] = bad; o[9] = un;
  }
}

// The NEES log: the normalised estimation error squared of the IMU state after a frame against the resident truth table, one
// record of msckf_nees::REC doubles per trajectory whatever the handle's dtype (include/msckf_hip.h, "NEES log record"):
//   0 NEES of the 15-state | 1..5 NEES of the blocks theta, b_g, v, b_a, p | 6 frame index | 7 flags
// One wavefront per trajectory, four per workgroup, after the frame log's launch.  P: the covariance buffer that is current
// after the frame (P_II sits at the same place whatever the window, so a pending window size does not matter here).
// k (offset to b0): the cell's sample count, IMU_SKIP for a skipped cell.  truth: the frame's rows [n_rows][16] of the truth
// table, trajectory b's is row_of[b]; walk: row frame + 1 of the replay's walk table, [B][6], added to the true b_g and b_a,
// or null.  imu[0..15], P_II's upper triangle, the truth row and the walk row are widened to double once; all arithmetic is f64.
//   e = [e_th ; b_g - b_g* ; v - v* ; b_a - b_a* ; p - p*], P's own order; e_th = error_angle(q_IG, q_IG*)
//   D = diag P_II, C = D^-1/2 P_II D^-1/2 (diagonal exactly 1), z = D^-1/2 e; NEES = |L^-1 z|^2 with C = L L^T
// Lane r < 15 owns row r of C, lane 15 the riding row z: the left-looking factorisation of [C ; z^T] leaves L^-1 z in lane 15's
// row (column j: s_r = A_rj - sum_{k < j} L_rk L_jk with L_jk handed over from lane j by wave_bcast, pivot s_j, L_rj = s_r /
// sqrt(s_j)).  15 pivot steps, no LDS, no atomics.  Lane g < 5 factors the 3 x 3 block g of P_II itself as k_log_metrics does
// P_pp.  Flags: FLAG_NOT_PD a diagonal entry or a pivot (of either factorisation) is not positive, FLAG_SKIPPED the cell was
// skipped -- either zeroes columns 0..5 --, FLAG_STAT_ERR the trajectory's STAT_ERR is set.
template <class S>
__global__ __launch_bounds__(256) void k_nees_log(Dev<S> d, int b0, int nb, const S* P, const int* k, const double* truth, const int* row_of, const double* walk, int frame, double* rec) {
  using namespace msckf_nees;
  int lane, i;
  if (!log_wave(nb, lane, i)) return;
  const int b = b0 + i;
  const S* Pb = P + (long)b * d.ld * d.ld;
  const S* xs = d.imu + (long)b * IMU_STRIDE;
  const double* tr = truth + (long)row_of[b] * TRUTH_ROW;
  double x[TRUTH_ROW], g[TRUTH_ROW], e[NX];
#pragma unroll
  for (int c = 0; c < TRUTH_ROW; ++c) { x[c] = (double)xs[c]; g[c] = tr[c]; }
  if (walk) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { g[IBG + c] += walk[(long)b * WALK_ROW + c]; g[IBA + c] += walk[(long)b * WALK_ROW + 3 + c]; }
  }
  const V3<double> th = error_angle(ldq(x + IQ), ldq(g + IQ));
  e[0] = th.x; e[1] = th.y; e[2] = th.z;
#pragma unroll
  for (int c = 3; c < NX; ++c) e[c] = x[c + 1] - g[c + 1];            // b_g v b_a p follow q in the state as in the error state
  // row min(lane, 14) of P_II's upper triangle mirrored: entry c <= r is element (c, r)
  const int r = lane < NX ? lane : NX - 1;
  double row[NX], er = 0.0;
#pragma unroll
  for (int c = 0; c < NX; ++c) { row[c] = (double)Pb[(long)r * d.ld + c]; if (lane == c) er = e[c]; }
  const double dg = (double)Pb[(long)r * d.ld + r];
  bool bad = !(dg > 0.0);
  const double dinv = 1.0 / sqrt(dg), zr = er * dinv;
#pragma unroll
  for (int c = 0; c < NX; ++c) {
    const double dc = wave_bcast(dinv, c), zc = wave_bcast(zr, c);
    row[c] = lane < NX ? (lane == c ? 1.0 : row[c] * dinv * dc) : zc;
  }
  double L[NX];
#pragma unroll
  for (int j = 0; j < NX; ++j) {
    double s = row[j];
#pragma unroll
    for (int c = 0; c < j; ++c) s -= L[c] * wave_bcast(L[c], j);
    const double piv = wave_bcast(s, j);
    bad = bad || !(piv > 0.0);
    L[j] = s / sqrt(piv);
  }
  double nees = 0.0;
#pragma unroll
  for (int j = 0; j < NX; ++j) nees += L[j] * L[j];
  nees = wave_bcast(nees, NX);                                         // lane 15's row is L^-1 z
  // block min(lane, 4) of P_II, upper triangle xx xy xz yy yz zz, and its part of e
  const int o = 3 * (lane < NBLK ? lane : NBLK - 1);
  double e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll
  for (int c = 0; c < NBLK; ++c) if (o == 3 * c) { e0 = e[3 * c]; e1 = e[3 * c + 1]; e2 = e[3 * c + 2]; }
  const double pxx = (double)Pb[(long)o * d.ld + o], pxy = (double)Pb[(long)(o + 1) * d.ld + o], pxz = (double)Pb[(long)(o + 2) * d.ld + o];
  const double pyy = (double)Pb[(long)(o + 1) * d.ld + o + 1], pyz = (double)Pb[(long)(o + 2) * d.ld + o + 1], pzz = (double)Pb[(long)(o + 2) * d.ld + o + 2];
  const double l00 = sqrt(pxx), l10 = pxy / l00, l20 = pxz / l00;
  const double d11 = pyy - l10 * l10, l11 = sqrt(d11), l21 = (pyz - l20 * l10) / l11;
  const double d22 = pzz - l20 * l20 - l21 * l21, l22 = sqrt(d22);
  const double y0 = e0 / l00, y1 = (e1 - l10 * y0) / l11, y2 = (e2 - l20 * y0 - l21 * y1) / l22;
  const double blk = y0 * y0 + y1 * y1 + y2 * y2;
  bad = bad || !(pxx > 0.0) || !(d11 > 0.0) || !(d22 > 0.0);
  const bool not_pd = __ballot(bad ? 1 : 0) != 0ull;
  const bool skipped = k[i] == IMU_SKIP;
  const int flags = (not_pd ? FLAG_NOT_PD : 0) | (skipped ? FLAG_SKIPPED : 0) | (d.stats[(long)b * STAT_STRIDE + STAT_ERR] != 0 ? FLAG_STAT_ERR : 0);
  // lanes 0..7 store the record: lane l in 1..5 takes block l - 1 from lane l - 1 (every lane takes part in the exchange)
  const double from_below = lane_gather(blk, ((lane - 1) & 63) << 2);
  double v = lane == REC_NEES ? nees : (lane < REC_FRAME ? from_below : (lane == REC_FRAME ? (double)frame : (double)flags));
  if ((not_pd || skipped) && lane < REC_FRAME) v = 0.0;
  if (lane < REC) rec[(long)b * REC + lane] = v;
}

// One wavefront (one workgroup) per (record, group) over the records [r0, r0 + gridDim.x / n_groups) of the NEES log
// ([.][B][8] doubles): group_of[b] in [-1, n_groups) names trajectory b's group, -1 none.  out[record - r0][group][14] =
// members with flags == 0, members left out for a flag, the sums of columns 0..5 over the former, the sums of their squares.
// Lane l takes the trajectories l, l + 64, ... in ascending order and the lanes are combined by wave_sum's fixed tree: the same
// log gives the same bits on every call.  An empty group gives zeros.
__global__ __launch_bounds__(64) void k_nees_ensemble(const double* rec, int B, int r0, int n_groups, const int* group_of, double* out) {
  using namespace msckf_nees;
  const int lane = threadIdx.x, r = r0 + (int)blockIdx.x / n_groups, g = (int)blockIdx.x % n_groups;
  double n_ok = 0, n_out = 0, s[REC_FRAME] = {0}, q[REC_FRAME] = {0};
  for (int b = lane; b < B; b += 64) {
    if (group_of[b] != g) continue;
    const double* x = rec + ((long)r * B + b) * REC;
    if (x[REC_FLAGS] != 0.0) { n_out += 1.0; continue; }
    n_ok += 1.0;
#pragma unroll
    for (int c = 0; c < REC_FRAME; ++c) { s[c] += x[c]; q[c] += x[c] * x[c]; }
  }
  n_ok = wave_sum(n_ok); n_out = wave_sum(n_out);
#pragma unroll
  for (int c = 0; c < REC_FRAME; ++c) { s[c] = wave_sum(s[c]); q[c] = wave_sum(q[c]); }
  if (lane == 0) {
    double* o = out + (long)blockIdx.x * ENS;
    o[ENS_N] = n_ok; o[ENS_FLAGGED] = n_out;
#pragma unroll
    for (int c = 0; c < REC_FRAME; ++c) { o[ENS_SUM + c] = s[c]; o[ENS_SUMSQ + c] = q[c]; }
  }
}

template <class S>
void launch_nees_log(const Dev<S>& d, int b0, int nb, hipStream_t st, const S* P, const int* k, const double* truth, const int* row_of, const double* walk, int frame, double* rec) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_nees_log<S>, dim3((nb + 3) / 4), dim3(256), 0, st, d, b0, nb, P, k, truth, row_of, walk, frame, rec);
}
void launch_nees_ensemble(const double* rec, int B, int r0, int r1, int n_groups, const int* group_of, double* out, hipStream_t st) {
  if (r1 <= r0 || n_groups <= 0) return;
  hipLaunchKernelGGL(k_nees_ensemble, dim3((unsigned)(r1 - r0) * n_groups), dim3(64), 0, st, rec, B, r0, n_groups, group_of, out);
}

template <class S>
void launch_pruned_log(const Dev<S>& d, int b0, int nb, hipStream_t st, const int* drop, int ordinal, int cap, S* rec, int* found) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_pruned_log<S>, dim3((nb + 3) / 4), dim3(256), 0, st, d, b0, nb, drop, ordinal, cap, rec, found);
}
template <class S>
void launch_pruned_metrics(const S* rec, const int* found, int cap, int B, int q0, int q1, const int* aug, const double* gt, int n_ord, double* out, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_pruned_metrics<S>, dim3(B), dim3(64), 0, st, rec, found, cap, B, q0, q1, aug, gt, n_ord, out);
}

template <class S>
void launch_map_log(const Dev<S>& d, int b0, int nb, hipStream_t st, const int* n, const int* M, int ordinal, int cap, S* rec, int* found) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_map_log<S>, dim3((nb + 3) / 4), dim3(256), 0, st, d, b0, nb, n, M, ordinal, cap, rec, found);
}
template <class S>
void launch_map_metrics(const S* rec, const int* found, int cap, int B, int q0, int q1, const double* gt, const int* off, double* out, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_map_metrics<S>, dim3(B), dim3(64), 0, st, rec, found, cap, B, q0, q1, gt, off, out);
}

template <class S>
void launch_map_fault_metrics(const S* rec, const int* found, int cap, int B, int q0, int q1, int f0, const int* n, const int* M, const int* off, const ReplayTrajIn& t, int n_seq, int f_cap, double* out, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_map_fault_metrics<S>, dim3(B), dim3(64), 0, st, rec, found, cap, q0, q1, f0, n, M, off, t.seq_of, t.seed, t.fault, n_seq, f_cap, out);
}

template <class S>
void launch_frame_log(const Dev<S>& d, int b0, int nb, hipStream_t st, const S* P, bool pending, S* rec) {
  if (nb <= 0) return;
  hipLaunchKernelGGL(k_frame_log<S>, dim3((nb + 3) / 4), dim3(256), 0, st, d, b0, nb, P, pending ? 1 : 0, rec);
}
template <class S>
void launch_log_metrics(const S* log, int B, int r0, int r1, const int* r0b, const int* r1b, const double* gt, double* out, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_log_metrics<S>, dim3(B), dim3(64), 0, st, log, B, r0, r1, r0b, r1b, gt, out);
}

#define MSCKF_LOG_LAUNCHERS(S)                                                                                        \
  template void launch_frame_log<S>(const Dev<S>&, int, int, hipStream_t, const S*, bool, S*);                         \
  template void launch_log_metrics<S>(const S*, int, int, int, const int*, const int*, const double*, double*, hipStream_t); \
  template void launch_map_log<S>(const Dev<S>&, int, int, hipStream_t, const int*, const int*, int, int, S*, int*);   \
  template void launch_map_metrics<S>(const S*, const int*, int, int, int, int, const double*, const int*, double*, hipStream_t); \
  template void launch_map_fault_metrics<S>(const S*, const int*, int, int, int, int, int, const int*, const int*, const int*, const ReplayTrajIn&, int, int, double*, hipStream_t); \
  template void launch_pruned_log<S>(const Dev<S>&, int, int, hipStream_t, const int*, int, int, S*, int*);            \
  template void launch_pruned_metrics<S>(const S*, const int*, int, int, int, int, const int*, const double*, int, double*, hipStream_t); \
  template void launch_nees_log<S>(const Dev<S>&, int, int, hipStream_t, const S*, const int*, const double*, const int*, const double*, int, double*);
MSCKF_LOG_LAUNCHERS(float)
MSCKF_LOG_LAUNCHERS(double)

}  // namespace msckf
