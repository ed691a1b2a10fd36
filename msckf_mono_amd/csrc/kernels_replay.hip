// kernels_replay.hip -- the Monte-Carlo replay's expansion: the frame's S noise-free sequence cells become the ordinary frame
// block of the B trajectories that replay them, each with its own seeded noise (replay_plan.h states the random stream, which
// draw a value takes and the layouts on both sides).
//
// k_replay_expand runs on the slice's stream ahead of the frame's propagate and writes only its slice's trajectories: their
// rows of the fixed sections and their entries [base[b], base[b] + entries) of slots / obs.  It reads the sequence store and the
// assignment, never the filter: the frame step cannot tell the block from an uploaded one.
//
// Work of one trajectory, as items; a workgroup takes REPLAY_CHUNK consecutive items, one lane each:
//   [0, E)                    entry e of the cell: its slot, and its coordinate pair + one Box-Muller pair, stored as one 2-vector
//   [E, E + 3 K)              pair j of the IMU noise: columns 2 (j % 3), 2 (j % 3) + 1 of sample j / 3 (noise only below the cell's k)
//   [E + 3 K, E + 4 K)        dT of sample i, as it is
//   [E + 4 K, .. + f_cap)     M[t], and off[t] rebased from the sequence's first entry to the trajectory's
//   the last                  n, drop, k
// All arithmetic is double whatever the handle's scalar; a value is rounded once when it is stored.  A reading's row has seven
// scalars, so only the coordinate pairs have an alignment to store vectors by (16 bytes in double, 8 in float); they are all but
// 7 K of a trajectory's scalars.  No LDS, no exchange between lanes.
//
// Under the Q_imu model (replay_plan.h, MODEL; the kernel's second instantiation) the IMU noise is no item: a sample's reading
// needs the walk's prefix over the samples before it, so a trajectory's first workgroup forms all of them together ahead of its
// items (model_imu: one lane per pair, per row of w = L z, per walk component, per stored scalar, handed over through LDS).
// k_replay_walk_scan tabulates the walk at every frame's start once per assignment.
//
// With a fault record (replay_plan.h, FAULTS) k_replay_expand_faults runs in its place: the same fixed items, and track items
// instead of entry items -- a group of lanes per track drops the missed observations behind the survivors and displaces the
// outliers.  k_replay_fault_counts counts a frame range's faults without expanding anything, and k_replay_imu_sums sums the IMU
// samples a frame range would expand, per trajectory, from the same device functions (the stand-still initialisation's means).
//
// With a non-zero timing record (replay_plan.h, TIMING) k_replay_expand_timed runs in place of either: the faulted form's lane
// groups, where each lane first moves its entry along the track to the time the pixel was exposed -- the stencil's neighbours come
// from the lanes of its group -- and then goes through the same entry_obs.  The two forms above are not touched by it.
//
// With a non-trivial calibration record (replay_plan.h, CALIB) k_replay_expand_calib runs in place of all three: the timed form's
// lane groups with the camera's residual map between the shift and entry_obs, the IMU pair items under the calibration rule
// (model_imu's CAL instantiation under the Q_imu model), with or without faults and timing.  k_replay_imu_sums has a CAL
// instantiation that sums the calibrated rows, and k_replay_calib_counts counts the clipped components of a frame range from
// the same device function (sample_stored).  The arithmetic of the records is replay_plan.h's inline functions.
#include <type_traits>

#include "dev_common.h"
#include "replay_plan.h"

namespace msckf {

namespace rp = msckf_replay;

struct Pair { double c, s; };
// pair j of sub-seed sd (replay_plan.h, NOISE).  The argument of sin / cos is the rounded product 2 pi u2, as the twin forms it.
__device__ __forceinline__ Pair box_muller(uint64_t sd, uint64_t j) {
  const double u1 = 1.0 - rp::U(sd, 2 * j), u2 = rp::U(sd, 2 * j + 1);
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  return Pair{r * cs, r * sn};
}
// value + sigma * noise: the product rounded, then the sum -- the twin's two operations, not one fused one
__device__ __forceinline__ double noisy(double v, double sigma, double g) {
#pragma clang fp contract(off)
  const double p = sigma * g;
  return v + p;
}
template <class S> struct alignas(2 * sizeof(S)) Vec2 { S x, y; };

// ---- the Q_imu model (replay_plan.h, MODEL): a cell's samples one after the other, by one lane (the scan's)
// w = L z of sample i: z from the pairs 6 i .. 6 i + 5 of s_imu, w_r = sum_{c <= r} L_rc z_c with c ascending, product rounded, then added
__device__ __forceinline__ void model_w(uint64_t s_imu, int i, const double* L, double* w) {
#pragma clang fp contract(off)
  double z[rp::NQ];
#pragma unroll
  for (int p = 0; p < rp::MODEL_PAIRS; ++p) {
    const Pair g = box_muller(s_imu, (uint64_t)(rp::MODEL_PAIRS * i + p));
    z[2 * p] = g.c; z[2 * p + 1] = g.s;
  }
#pragma unroll
  for (int r = 0; r < rp::NQ; ++r) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c <= r; ++c) { const double p = L[c * rp::NQ + r] * z[c]; a = a + p; }
    w[r] = a;
  }
}
// one walk component's increment over a sample with dT > 0, and the scalar a sample stores: (value + W(f, i)) + n, n absent when
// dT <= 0 -- w: the component's row of w = L z (n_wg 3 .. 5, n_wa 9 .. 11 for the increment; n_g 0 .. 2, n_a 6 .. 8 for the noise).
// Stated once for the scan, the expansion and the sums.
__device__ __forceinline__ double model_delta(double scale, double w, double dT) {
#pragma clang fp contract(off)
  const double sq = sqrt(dT);
  return (scale * w) * sq;
}
__device__ __forceinline__ double model_stored(double v, double W, double scale, double w, double dT) {
#pragma clang fp contract(off)
  v = v + W;
  if (dT > 0.0) { const double nz = (scale * w) / sqrt(dT); v = v + nz; }
  return v;
}
// P(f, n) of a cell: the sequential sum of the first n samples' increments, per component; rd: the cell's readings [K][7]
__device__ __forceinline__ void model_prefix(const double* rd, uint64_t s_imu, const double* L, double scale, int n, double* P) {
#pragma clang fp contract(off)
  for (int c = 0; c < rp::WALK_ROW; ++c) P[c] = 0.0;
  for (int i = 0; i < n; ++i) {
    const double dT = rd[i * RD_STRIDE + 6];
    if (!(dT > 0.0)) continue;
    double w[rp::NQ];
    model_w(s_imu, i, L, w);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double dg = model_delta(scale, w[3 + c], dT), da = model_delta(scale, w[9 + c], dT);
      P[c] = P[c] + dg; P[3 + c] = P[3 + c] + da;
    }
  }
}

// The IMU readings of one trajectory under the model, by the whole workgroup, MODEL_TILE samples at a time:
//   1. lane j draws pair j of the tile (sample j / 6, z[2 (j % 6)], z[2 (j % 6) + 1])
//   2. lane j forms row j % 12 of sample j / 12: w_r = sum_{c <= r} L_rc z_c, c ascending
//   3. six lanes, one per walk component, go through the samples in order: W(f, i) = Wstart(f) + P, then P = P + delta(f, i)
//      (P is carried from tile to tile in LDS)
//   4. lane j stores scalar j % 6 of sample j / 6: (value + W(f, i)) + noise; rows from k on are the sequence's
// Every sum is the normative one (replay_plan.h): who forms it changes, its order does not.
constexpr int MODEL_TILE = 32;
// CAL (replay_plan.h, CALIB; the calibrated expansion's instantiation): step 4's lane forms its own component of the calibrated
// row from the sample's six values, puts it in the value's place and passes the sum through saturation and quantisation;
// rd_cal / clip (or null): the read-back's noise-free calibrated values and clipped components, [K][6] each.
template <class S, bool CAL = false>
__device__ __forceinline__ void model_imu(const double* cell, S* out, const double* L, double scale, const double* wstart, uint64_t s_imu, int K, int k, const double* ic = nullptr, double* rd_cal = nullptr, int* clip = nullptr) {
#pragma clang fp contract(off)
  __shared__ double z[MODEL_TILE][rp::NQ], w[MODEL_TILE][rp::NQ], W[MODEL_TILE][rp::WALK_ROW], P[rp::WALK_ROW];
  const int lane = (int)threadIdx.x;
  if (lane < rp::WALK_ROW) P[lane] = 0.0;
  for (int i0 = 0; i0 < K; i0 += MODEL_TILE) {
    const int rows = K - i0 < MODEL_TILE ? K - i0 : MODEL_TILE;         // samples of the tile, of which n carry noise
    const int n = k - i0 < 0 ? 0 : k - i0 < rows ? k - i0 : rows;
    for (int j = lane; j < rp::MODEL_PAIRS * n; j += REPLAY_CHUNK) {
      const Pair g = box_muller(s_imu, (uint64_t)(rp::MODEL_PAIRS * i0 + j));
      z[j / rp::MODEL_PAIRS][2 * (j % rp::MODEL_PAIRS)] = g.c; z[j / rp::MODEL_PAIRS][2 * (j % rp::MODEL_PAIRS) + 1] = g.s;
    }
    __syncthreads();
    for (int j = lane; j < rp::NQ * n; j += REPLAY_CHUNK) {
      const int i = j / rp::NQ, r = j % rp::NQ;
      double a = 0.0;
      for (int c = 0; c <= r; ++c) { const double p = L[c * rp::NQ + r] * z[i][c]; a = a + p; }
      w[i][r] = a;
    }
    __syncthreads();
    if (lane < rp::WALK_ROW) {
      const int r = lane < 3 ? 3 + lane : 6 + lane;                     // n_wg: rows 3 .. 5, n_wa: rows 9 .. 11
      const double start = wstart[lane];
      double run = P[lane];
      for (int i = 0; i < n; ++i) {
        W[i][lane] = start + run;
        const double dT = cell[(i0 + i) * RD_STRIDE + 6];
        if (dT > 0.0) { const double d = model_delta(scale, w[i][r], dT); run = run + d; }
      }
      P[lane] = run;
    }
    __syncthreads();
    for (int j = lane; j < rp::WALK_ROW * rows; j += REPLAY_CHUNK) {
      const int i = j / rp::WALK_ROW, c = j % rp::WALK_ROW;
      const double* rd = cell + (i0 + i) * RD_STRIDE;
      double v = rd[c];
      if constexpr (CAL) {
        bool cl = false;
        if (i < n) {
          v = rp::calib_imu(ic, rd, c);
          const double cv = v;
          v = rp::calib_out(ic, c, model_stored(v, W[i][c], scale, w[i][c < 3 ? c : 3 + c], rd[6]), &cl);
          if (rd_cal) rd_cal[(i0 + i) * 6 + c] = cv;
        } else if (rd_cal) rd_cal[(i0 + i) * 6 + c] = v;
        if (clip) clip[(i0 + i) * 6 + c] = cl ? 1 : 0;
      } else if (i < n) v = model_stored(v, W[i][c], scale, w[i][c < 3 ? c : 3 + c], rd[6]);   // n_g: rows 0 .. 2, n_a: rows 6 .. 8
      out[(i0 + i) * RD_STRIDE + c] = (S)v;
    }
    __syncthreads();                                                   // the next tile overwrites z, w and W
  }
}

// One entry's coordinate pair, stated once for both forms of the expansion: value + sigma * noise with pair e of s_obs (e: the
// entry's index in the SEQUENCE cell), and for an outlier (replay_plan.h, FAULTS) the ring term on top of it -- a = the rounded
// product 2 pi u_ang, each product rounded, then added -- all in double, rounded once.  out == false: flt and u_ang are not read.
template <class S, bool MODEL>
__device__ __forceinline__ Vec2<S> entry_obs(const double* z, const double* sg, uint64_t s_obs, uint64_t e, bool out, double u_ang, const double* flt) {
  const Pair g = box_muller(s_obs, e);
  double x = noisy(z[0], sg[MODEL ? 0 : rp::SIG_U], g.c), y = noisy(z[1], sg[MODEL ? 1 : rp::SIG_V], g.s);
  if (out) {
    double sn, cs;
    sincos(6.283185307179586 * u_ang, &sn, &cs);
    x = noisy(x, flt[rp::FLT_RHO_U], cs); y = noisy(y, flt[rp::FLT_RHO_V], sn);
  }
  Vec2<S> w;
  w.x = (S)x; w.y = (S)y;
  return w;
}

// The sigma4 model's pair p (0 .. 2) of IMU sample i: columns 2 p, 2 p + 1 of its row r with pair 3 i + p of s_imu (replay_plan.h, NOISE)
__device__ __forceinline__ void sigma4_pair(const double* r, const double* sg, uint64_t s_imu, int i, int p, double& v0, double& v1) {
  const int cc = 2 * p;
  const Pair g = box_muller(s_imu, (uint64_t)(rp::IMU_PAIRS * i + p));
  v0 = noisy(r[cc], sg[cc < 3 ? rp::SIG_G : rp::SIG_A], g.c); v1 = noisy(r[cc + 1], sg[cc + 1 < 3 ? rp::SIG_G : rp::SIG_A], g.s);
}

// The fixed items of a trajectory, j counted from the first of them (the list at the top of the file without the entries):
// IMU noise pairs (sigma4 model only), dT, M[t] / off[t], and n / drop / k.  with_M == false: M[t] is somebody else's (the
// faulted form's track items store the survivors).
struct ReplayCell { int s, b, kc, first, base; uint64_t seed; const double* sg; const int* Ms; const int* offs; };
template <class S, bool MODEL>
__device__ __forceinline__ void fixed_item(const ReplaySeqIn& q, const ReplayOut<S>& o, const ReplayCell& c, int j, int f, int K, int f_cap, bool with_M) {
  const int dt0 = (MODEL ? 0 : rp::IMU_PAIRS) * K, m0 = dt0 + K, last = m0 + f_cap;
  const int s = c.s, b = c.b;
  if (j < dt0) {
    const int i = j / rp::IMU_PAIRS, cc = 2 * (j % rp::IMU_PAIRS);
    const double* r = q.rd + ((long)s * K + i) * RD_STRIDE;
    S* w = o.rd + ((long)b * K + i) * RD_STRIDE;
    double v0 = r[cc], v1 = r[cc + 1];
    if (i < c.kc) sigma4_pair(r, c.sg, rp::imu_seed(c.seed, f), i, j % rp::IMU_PAIRS, v0, v1);   // (a skipped cell's k is IMU_SKIP: no noise; rows from k on stay zero)
    w[cc] = (S)v0; w[cc + 1] = (S)v1;
  } else if (j < m0) {
    const int i = j - dt0;
    o.rd[((long)b * K + i) * RD_STRIDE + 6] = (S)q.rd[((long)s * K + i) * RD_STRIDE + 6];
  } else if (j < last) {
    const int tr = j - m0;
    if (with_M) o.M[(long)b * f_cap + tr] = c.Ms[tr];
    o.off[(long)b * f_cap + tr] = c.offs[tr] - c.first + c.base;
  } else {
    o.n[b] = q.n[s]; o.drop[b] = q.drop[s]; o.k[b] = c.kc;
  }
}
// fixed items of a trajectory: IMU pairs (sigma4 model only), dT, tracks, the last
constexpr int fixed_items(bool model, int K, int f_cap) { return ((model ? 0 : rp::IMU_PAIRS) + 1) * K + f_cap + 1; }

// MODEL: false the sigma4 noise (the items above), true the Q_imu model (no IMU items: model_imu; t.sigma is sigma_uv[B][2])
template <class S, bool MODEL>
__global__ __launch_bounds__(REPLAY_CHUNK) void k_replay_expand(ReplaySeqIn q, ReplayTrajIn t, ReplayModelIn m, ReplayOut<S> o, int f, int b0, int K, int f_cap) {
  const int b = b0 + (int)blockIdx.y;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double* sg = t.sigma + (long)b * (MODEL ? 2 : rp::N_SIGMA);
  const int* Ms = q.M + (long)s * f_cap;
  const int* offs = q.off + (long)s * f_cap;
  const int first = offs[0];                                           // the sequence cell's first entry among the frame's sequence entries
  const int E = offs[f_cap - 1] + Ms[f_cap - 1] - first;
  const int base = t.base[b];                                          // the trajectory's first entry in the expanded block
  const int kc = q.k[s];
  if constexpr (MODEL) {                                               // (a skipped cell's k is IMU_SKIP: no noise)
    if (blockIdx.x == 0)
      model_imu<S>(q.rd + (long)s * K * RD_STRIDE, o.rd + (long)b * K * RD_STRIDE, m.L + (long)b * rp::L_SIZE, m.scale[b], m.wstart + (long)b * rp::WALK_ROW, rp::imu_seed(seed, f), K, kc < K ? kc : K);
  }
  const ReplayCell c{s, b, kc, first, base, seed, sg, Ms, offs};
  const int last = E + fixed_items(MODEL, K, f_cap) - 1;
  for (int it = (int)blockIdx.x * REPLAY_CHUNK + (int)threadIdx.x; it <= last; it += (int)gridDim.x * REPLAY_CHUNK) {
    if (it < E) {
      o.slots[(long)base + it] = q.slots[(long)first + it];
      *reinterpret_cast<Vec2<S>*>(o.obs + 2 * ((long)base + it)) = entry_obs<S, MODEL>(q.obs + 2 * (long)(first + it), sg, rp::obs_seed(seed, f), (uint64_t)it, false, 0.0, nullptr);
    } else fixed_item<S, MODEL>(q, o, c, it - E, f, K, f_cap, true);
  }
}

// The faulted form (replay_plan.h, FAULTS; t.fault is fault4[B][4]): the fixed items stay, the entry items become TRACK items --
// a group of G lanes takes one track, one lane per entry (G = 16, 32 or 64 >= m_cap, chosen at launch, so that short-track
// handles do not idle three quarters of a wavefront).  The lane draws its three uniforms and its noise pair; the group cuts its
// part out of the wavefront's ballot of raw_miss, applies the "fewer than two" rule on the popcount, and each lane ranks itself
// with mbcnt among the survivors or among the missed entries (as k_map_log ranks its records): slot and coordinate pair go to
// base + off[t] - first + rank (+ survivors for a missed entry), the group's first lane stores M[t] = survivors.  The track items
// [0, f_cap G) are padded to whole wavefronts, so a wavefront is either all track items or all fixed items.  code (null in the
// frame loop): per entry of the block, at base + the entry's SEQUENCE index, 0 kept, 1 outlier, 2 missed.
// No LDS, no atomics, no exchange between wavefronts.
template <class S, bool MODEL, int G>
__global__ __launch_bounds__(REPLAY_CHUNK) void k_replay_expand_faults(ReplaySeqIn q, ReplayTrajIn t, ReplayModelIn m, ReplayOut<S> o, int* code, int f, int b0, int K, int f_cap) {
  const int b = b0 + (int)blockIdx.y;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double* sg = t.sigma + (long)b * (MODEL ? 2 : rp::N_SIGMA);
  const double* flt = t.fault + (long)b * rp::N_FAULT;
  const int* Ms = q.M + (long)s * f_cap;
  const int* offs = q.off + (long)s * f_cap;
  const int first = offs[0];
  const int base = t.base[b];
  const int kc = q.k[s];
  if constexpr (MODEL) {
    if (blockIdx.x == 0)
      model_imu<S>(q.rd + (long)s * K * RD_STRIDE, o.rd + (long)b * K * RD_STRIDE, m.L + (long)b * rp::L_SIZE, m.scale[b], m.wstart + (long)b * rp::WALK_ROW, rp::imu_seed(seed, f), K, kc < K ? kc : K);
  }
  const ReplayCell c{s, b, kc, first, base, seed, sg, Ms, offs};
  const double p_miss = flt[rp::FLT_P_MISS], p_out = flt[rp::FLT_P_OUT];
  const uint64_t s_flt = rp::fault_seed(seed, f), s_obs = rp::obs_seed(seed, f);
  const int lane = (int)threadIdx.x & 63;
  const int T = (f_cap * G + 63) & ~63;                                // REPLAY_CHUNK is a multiple of 64: `it < T` is the same for a whole wavefront
  const int end = T + fixed_items(MODEL, K, f_cap);
  for (int it = (int)blockIdx.x * REPLAY_CHUNK + (int)threadIdx.x; it < end; it += (int)gridDim.x * REPLAY_CHUNK) {
    if (it < T) {
      const int tr = it / G, l = it % G;
      const int M = tr < f_cap ? Ms[tr] : 0;                           // (M <= m_cap <= G)
      const bool have = l < M;
      const int e = have ? offs[tr] - first + l : 0;                   // the entry's index in the sequence cell
      const bool raw = have && rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e) < p_miss;
      unsigned long long gm = __ballot(raw ? 1 : 0);
      if constexpr (G < 64) gm &= ((1ull << G) - 1) << (lane & ~(G - 1));
      if (M - __popcll(gm) < 2) gm = 0;                                // a track keeps two observations or loses none
      const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(gm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)gm, 0u));   // missed entries of the track before this one
      const int surv = M - __popcll(gm);
      if (have) {
        const bool miss = (gm >> lane) & 1;
        const bool out = !miss && rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e + 1) < p_out;
        const long dst = (long)base + (offs[tr] - first) + (miss ? surv + below : l - below);
        o.slots[dst] = q.slots[(long)first + e];
        *reinterpret_cast<Vec2<S>*>(o.obs + 2 * dst) = entry_obs<S, MODEL>(q.obs + 2 * (long)(first + e), sg, s_obs, (uint64_t)e, out, rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e + 2), flt);
        if (code) code[(long)base + e] = miss ? rp::FAULT_MISSED : out ? rp::FAULT_OUTLIER : rp::FAULT_KEPT;
      }
      if (l == 0 && tr < f_cap) o.M[(long)b * f_cap + tr] = surv;
    } else fixed_item<S, MODEL>(q, o, c, it - T, f, K, f_cap, false);
  }
}

// A product that is rounded before anything is added to it, whatever the file's contraction mode (-ffp-contract=fast fuses
// across statements and disregards the pragma): the value passes through an empty asm the compiler cannot look into.
__device__ __forceinline__ double rounded(double p) {
  asm volatile("" : "+v"(p));
  return p;
}
// The shift of one entry along its track (replay_plan.h, TIMING): n nodes (2 or 3) with values (x[j], y[j]) and times d[j]
// relative to the entry's own, the entry exposed dl after its image's time.  w_j = prod_{m != j} (dl - d_m) / prod_{m != j}
// (d_j - d_m), the value sum_j w_j (x_j, y_j) with j ascending: + - x / only, each rounded in double (every product that an
// addition takes goes through rounded()).
__device__ __forceinline__ void timing_shift(int n, const double* d, const double* x, const double* y, double dl, double* z) {
#pragma clang fp contract(off)
  double w[3] = {0.0, 0.0, 0.0};
  if (n == 2) {
    w[0] = (dl - d[1]) / (d[0] - d[1]);
    w[1] = (dl - d[0]) / (d[1] - d[0]);
  } else {
    w[0] = ((dl - d[1]) * (dl - d[2])) / ((d[0] - d[1]) * (d[0] - d[2]));
    w[1] = ((dl - d[0]) * (dl - d[2])) / ((d[1] - d[0]) * (d[1] - d[2]));
    w[2] = ((dl - d[0]) * (dl - d[1])) / ((d[2] - d[0]) * (d[2] - d[1]));
  }
  double ax = rounded(w[0] * x[0]), ay = rounded(w[0] * y[0]);
  { const double px = rounded(w[1] * x[1]), py = rounded(w[1] * y[1]); ax = ax + px; ay = ay + py; }
  if (n == 3) { const double px = rounded(w[2] * x[2]), py = rounded(w[2] * y[2]); ax = ax + px; ay = ay + py; }
  z[0] = ax; z[1] = ay;
}
// delta_l of an entry with sequence value y on image q of the sequence (replay_plan.h, TIMING): tm4 the trajectory's record,
// s_tim = timing_seed(s_b); sigma_j == 0: no draw
__device__ __forceinline__ double timing_delta(const double* tm4, uint64_t s_tim, double y, int frame_of) {
#pragma clang fp contract(off)
  const double a = y - tm4[rp::TIM_Y0];
  const double p = rounded(tm4[rp::TIM_RY] * a);
  const double s = tm4[rp::TIM_TD] + p;
  const double sj = tm4[rp::TIM_SIGMA_J];
  const double g = sj != 0.0 ? box_muller(s_tim, (uint64_t)frame_of).c : 0.0;
  const double j = rounded(sj * g);
  return s + j;
}

// The timed form (replay_plan.h, TIMING): k_replay_expand_faults' items and lane groups -- one lane per entry of a track -- with
// the entry's value moved along its track before it goes through entry_obs.  A lane loads its entry's value, its slot and the
// time and frame of image base(f) + slot, forms its delta, and fetches the values and times of its stencil's nodes from the
// lanes l0 .. l0 + 2 of its group (__shfl: ds_bpermute; every lane of a track wavefront is active, the lanes beyond M hold
// zeros nobody asks for).  Missed entries serve as nodes like any other.  With p_miss = p_out = 0 it is timing alone: all
// survive, in sequence order.  delta (null in the frame loop): per entry, at base + the entry's SEQUENCE index.
// No LDS, no atomics, no exchange between wavefronts.
template <class S, bool MODEL, int G>
__global__ __launch_bounds__(REPLAY_CHUNK) void k_replay_expand_timed(ReplaySeqIn q, ReplayTrajIn t, ReplayModelIn m, ReplayTimingIn tm, ReplayOut<S> o, int* code, double* delta, int f, int b0, int K, int f_cap) {
  const int b = b0 + (int)blockIdx.y;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double* sg = t.sigma + (long)b * (MODEL ? 2 : rp::N_SIGMA);
  const double* flt = t.fault + (long)b * rp::N_FAULT;
  const double* tm4 = tm.timing + (long)b * rp::N_TIMING;
  const double* times = tm.time + (long)s * tm.stride;
  const int* frames_of = tm.frame_of + (long)s * tm.stride;
  const int img0 = tm.base[s];                                         // camera slot 0 of the cell is this image of the sequence
  const int* Ms = q.M + (long)s * f_cap;
  const int* offs = q.off + (long)s * f_cap;
  const int first = offs[0];
  const int base = t.base[b];
  const int kc = q.k[s];
  if constexpr (MODEL) {
    if (blockIdx.x == 0)
      model_imu<S>(q.rd + (long)s * K * RD_STRIDE, o.rd + (long)b * K * RD_STRIDE, m.L + (long)b * rp::L_SIZE, m.scale[b], m.wstart + (long)b * rp::WALK_ROW, rp::imu_seed(seed, f), K, kc < K ? kc : K);
  }
  const ReplayCell c{s, b, kc, first, base, seed, sg, Ms, offs};
  const double p_miss = flt[rp::FLT_P_MISS], p_out = flt[rp::FLT_P_OUT];
  const uint64_t s_flt = rp::fault_seed(seed, f), s_obs = rp::obs_seed(seed, f), s_tim = rp::timing_seed(seed);
  const int lane = (int)threadIdx.x & 63;
  const int T = (f_cap * G + 63) & ~63;                                // as in k_replay_expand_faults: `it < T` is the same for a whole wavefront
  const int end = T + fixed_items(MODEL, K, f_cap);
  for (int it = (int)blockIdx.x * REPLAY_CHUNK + (int)threadIdx.x; it < end; it += (int)gridDim.x * REPLAY_CHUNK) {
    if (it < T) {
      const int tr = it / G, l = it % G;
      const int M = tr < f_cap ? Ms[tr] : 0;                           // (M <= m_cap <= G)
      const bool have = l < M;
      const int e = have ? offs[tr] - first + l : 0;
      // the entry's own value, slot and image; the host has checked slot < W(f): base(f) + slot names an image of the table
      const int slot = have ? q.slots[(long)first + e] : 0;
      const double vx = have ? q.obs[2 * (long)(first + e)] : 0.0, vy = have ? q.obs[2 * (long)(first + e) + 1] : 0.0;
      const double tl = have ? times[img0 + slot] : 0.0;
      const double dl = have ? timing_delta(tm4, s_tim, vy, frames_of[img0 + slot]) : 0.0;
      // the stencil's nodes from the lanes of the group (every lane of the wavefront takes part)
      const int n = rp::stencil_nodes(M), g0 = (lane & ~(G - 1)) + (have ? rp::stencil_first(l, M) : 0);
      double nx[3], ny[3], nd[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int src = j < n ? g0 + j : lane;
        nx[j] = __shfl(vx, src, 64); ny[j] = __shfl(vy, src, 64); nd[j] = __shfl(tl, src, 64) - tl;
      }
      double z[2] = {vx, vy};
      if (have && n >= 2 && dl != 0.0) timing_shift(n, nd, nx, ny, dl, z);
      // from here on k_replay_expand_faults, on the shifted value
      const bool raw = have && p_miss > 0.0 && rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e) < p_miss;
      unsigned long long gm = __ballot(raw ? 1 : 0);
      if constexpr (G < 64) gm &= ((1ull << G) - 1) << (lane & ~(G - 1));
      if (M - __popcll(gm) < 2) gm = 0;                                // a track keeps two observations or loses none
      const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(gm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)gm, 0u));
      const int surv = M - __popcll(gm);
      if (have) {
        const bool miss = (gm >> lane) & 1;
        const bool out = !miss && p_out > 0.0 && rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e + 1) < p_out;
        const long dst = (long)base + (offs[tr] - first) + (miss ? surv + below : l - below);
        o.slots[dst] = slot;
        *reinterpret_cast<Vec2<S>*>(o.obs + 2 * dst) = entry_obs<S, MODEL>(z, sg, s_obs, (uint64_t)e, out, out ? rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e + 2) : 0.0, flt);
        if (code) code[(long)base + e] = miss ? rp::FAULT_MISSED : out ? rp::FAULT_OUTLIER : rp::FAULT_KEPT;
        if (delta) delta[(long)base + e] = dl;
      }
      if (l == 0 && tr < f_cap) o.M[(long)b * f_cap + tr] = surv;
    } else fixed_item<S, MODEL>(q, o, c, it - T, f, K, f_cap, false);
  }
}

template <class S, bool MODEL, int G>
static void launch_timed(const dim3& grid, hipStream_t st, const ReplaySeqIn& q, const ReplayTrajIn& t, const ReplayModelIn& m, const ReplayTimingIn& tm, const ReplayOut<S>& o, int* code, double* delta, int f, int b0, int K, int f_cap) {
  hipLaunchKernelGGL((k_replay_expand_timed<S, MODEL, G>), grid, dim3(REPLAY_CHUNK), 0, st, q, t, m, tm, o, code, delta, f, b0, K, f_cap);
}
// the faulted form's grid: f_cap tracks of G lanes, G from m_cap
template <class S>
void launch_replay_expand_timed(const ReplaySeqIn& q, const ReplayTrajIn& t, const ReplayModelIn& m, const ReplayTimingIn& tm, const ReplayOut<S>& o, int f, int b0, int nb, int K, int f_cap, hipStream_t st, int m_cap, int* code, double* delta) {
  if (nb <= 0) return;
  const bool model = m.L != nullptr;
  const int G = rp::fault_group(m_cap);
  const long items = (long)((f_cap * G + 63) & ~63) + fixed_items(model, K, f_cap);
  const dim3 grid((unsigned)((items + REPLAY_CHUNK - 1) / REPLAY_CHUNK), (unsigned)nb);
  auto go = [&](auto mdl) {
    constexpr bool MD = decltype(mdl)::value;
    if (G == 16) launch_timed<S, MD, 16>(grid, st, q, t, m, tm, o, code, delta, f, b0, K, f_cap);
    else if (G == 32) launch_timed<S, MD, 32>(grid, st, q, t, m, tm, o, code, delta, f, b0, K, f_cap);
    else launch_timed<S, MD, 64>(grid, st, q, t, m, tm, o, code, delta, f, b0, K, f_cap);
  };
  if (model) go(std::true_type{}); else go(std::false_type{});
}
template void launch_replay_expand_timed<float>(const ReplaySeqIn&, const ReplayTrajIn&, const ReplayModelIn&, const ReplayTimingIn&, const ReplayOut<float>&, int, int, int, int, int, hipStream_t, int, int*, double*);
template void launch_replay_expand_timed<double>(const ReplaySeqIn&, const ReplayTrajIn&, const ReplayModelIn&, const ReplayTimingIn&, const ReplayOut<double>&, int, int, int, int, int, hipStream_t, int, int*, double*);

// The calibrated form (replay_plan.h, CALIB): k_replay_expand_timed's items and lane groups, with the camera's residual map
// (rp::calib_cam) between the shift and entry_obs, and the IMU items under the calibration rule -- in the sigma4 form an item
// still owns one pair of columns of one sample and reads the sample's six values (rp::calib_imu for its two components, the
// noise of its pair, rp::calib_out); under the Q_imu model model_imu's CAL instantiation.  It runs whenever some trajectory's
// calibration record is non-trivial, with or without faults and timing: zero fault records mean all survive in sequence order,
// and with c.timed false no image table is consulted and every delta is 0 exactly -- the value itself.
// c.rd_cal / c.clip / c.obs_cal (null in the frame loop): the read-back's, for a launch of one trajectory.
// No LDS in the track items, no atomics, no exchange between wavefronts.
template <class S, bool MODEL, int G>
__global__ __launch_bounds__(REPLAY_CHUNK) void k_replay_expand_calib(ReplaySeqIn q, ReplayTrajIn t, ReplayModelIn m, ReplayTimingIn tm, ReplayCalibIn cal, ReplayOut<S> o, int* code, double* delta, int f, int b0, int K, int f_cap) {
  const int b = b0 + (int)blockIdx.y;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double* sg = t.sigma + (long)b * (MODEL ? 2 : rp::N_SIGMA);
  const double* flt = t.fault + (long)b * rp::N_FAULT;
  const double* ic = cal.imu + (long)b * rp::IMU_CAL;
  const double* cc = cal.cam + (long)b * rp::CAM_CAL;
  const bool timed = cal.timed;
  const double* tm4 = timed ? tm.timing + (long)b * rp::N_TIMING : nullptr;
  const double* times = timed ? tm.time + (long)s * tm.stride : nullptr;
  const int* frames_of = timed ? tm.frame_of + (long)s * tm.stride : nullptr;
  const int img0 = timed ? tm.base[s] : 0;
  const int* Ms = q.M + (long)s * f_cap;
  const int* offs = q.off + (long)s * f_cap;
  const int first = offs[0];
  const int base = t.base[b];
  const int kc = q.k[s];
  if constexpr (MODEL) {
    if (blockIdx.x == 0)
      model_imu<S, true>(q.rd + (long)s * K * RD_STRIDE, o.rd + (long)b * K * RD_STRIDE, m.L + (long)b * rp::L_SIZE, m.scale[b], m.wstart + (long)b * rp::WALK_ROW, rp::imu_seed(seed, f), K, kc < K ? kc : K,
                         ic, cal.rd_cal, cal.clip);
  }
  const ReplayCell c{s, b, kc, first, base, seed, sg, Ms, offs};
  const double p_miss = flt[rp::FLT_P_MISS], p_out = flt[rp::FLT_P_OUT];
  const uint64_t s_flt = rp::fault_seed(seed, f), s_obs = rp::obs_seed(seed, f), s_tim = rp::timing_seed(seed);
  const int lane = (int)threadIdx.x & 63;
  const int T = (f_cap * G + 63) & ~63;                                // as in k_replay_expand_faults: `it < T` is the same for a whole wavefront
  const int dt0 = (MODEL ? 0 : rp::IMU_PAIRS) * K;                     // the IMU pair items of the sigma4 form
  const int end = T + fixed_items(MODEL, K, f_cap);
  for (int it = (int)blockIdx.x * REPLAY_CHUNK + (int)threadIdx.x; it < end; it += (int)gridDim.x * REPLAY_CHUNK) {
    if (it < T) {
      const int tr = it / G, l = it % G;
      const int M = tr < f_cap ? Ms[tr] : 0;                           // (M <= m_cap <= G)
      const bool have = l < M;
      const int e = have ? offs[tr] - first + l : 0;
      const int slot = have ? q.slots[(long)first + e] : 0;
      const double vx = have ? q.obs[2 * (long)(first + e)] : 0.0, vy = have ? q.obs[2 * (long)(first + e) + 1] : 0.0;
      double z[2] = {vx, vy};
      double dl = 0.0;
      if (timed) {                                                     // (uniform over the launch: every lane of the wavefront takes part in the exchange)
        const double tl = have ? times[img0 + slot] : 0.0;
        dl = have ? timing_delta(tm4, s_tim, vy, frames_of[img0 + slot]) : 0.0;
        const int n = rp::stencil_nodes(M), g0 = (lane & ~(G - 1)) + (have ? rp::stencil_first(l, M) : 0);
        double nx[3], ny[3], nd[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int src = j < n ? g0 + j : lane;
          nx[j] = __shfl(vx, src, 64); ny[j] = __shfl(vy, src, 64); nd[j] = __shfl(tl, src, 64) - tl;
        }
        if (have && n >= 2 && dl != 0.0) timing_shift(n, nd, nx, ny, dl, z);
      }
      if (have) rp::calib_cam(cc, z[0], z[1], z);                      // the camera's residual map of the (shifted) value
      // from here on k_replay_expand_faults, on the mapped value
      const bool raw = have && p_miss > 0.0 && rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e) < p_miss;
      unsigned long long gm = __ballot(raw ? 1 : 0);
      if constexpr (G < 64) gm &= ((1ull << G) - 1) << (lane & ~(G - 1));
      if (M - __popcll(gm) < 2) gm = 0;                                // a track keeps two observations or loses none
      const int below = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(gm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)gm, 0u));
      const int surv = M - __popcll(gm);
      if (have) {
        const bool miss = (gm >> lane) & 1;
        const bool out = !miss && p_out > 0.0 && rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e + 1) < p_out;
        const long dst = (long)base + (offs[tr] - first) + (miss ? surv + below : l - below);
        o.slots[dst] = slot;
        *reinterpret_cast<Vec2<S>*>(o.obs + 2 * dst) = entry_obs<S, MODEL>(z, sg, s_obs, (uint64_t)e, out, out ? rp::U(s_flt, rp::FAULT_DRAWS * (uint64_t)e + 2) : 0.0, flt);
        if (code) code[(long)base + e] = miss ? rp::FAULT_MISSED : out ? rp::FAULT_OUTLIER : rp::FAULT_KEPT;
        if (delta) delta[(long)base + e] = dl;
        if (cal.obs_cal) { cal.obs_cal[2 * ((long)base + e)] = z[0]; cal.obs_cal[2 * ((long)base + e) + 1] = z[1]; }
      }
      if (l == 0 && tr < f_cap) o.M[(long)b * f_cap + tr] = surv;
    } else if (!MODEL && it - T < dt0) {
      // pair p of sample i under the calibration rule: the row's six values, the two components of the pair
      const int j = it - T, i = j / rp::IMU_PAIRS, p = j % rp::IMU_PAIRS, c0 = 2 * p;
      const double* r = q.rd + ((long)s * K + i) * RD_STRIDE;
      S* w = o.rd + ((long)b * K + i) * RD_STRIDE;
      double v[2] = {r[c0], r[c0 + 1]}, cv[2] = {r[c0], r[c0 + 1]};
      bool cl[2] = {false, false};
      if (i < kc) {
        double row[6];
#pragma unroll
        for (int x = 0; x < 6; ++x) row[x] = r[x];
        cv[0] = rp::calib_imu(ic, row, c0); cv[1] = rp::calib_imu(ic, row, c0 + 1);
        const Pair g = box_muller(rp::imu_seed(seed, f), (uint64_t)(rp::IMU_PAIRS * i + p));
        v[0] = rp::calib_out(ic, c0, noisy(cv[0], sg[c0 < 3 ? rp::SIG_G : rp::SIG_A], g.c), &cl[0]);
        v[1] = rp::calib_out(ic, c0 + 1, noisy(cv[1], sg[c0 + 1 < 3 ? rp::SIG_G : rp::SIG_A], g.s), &cl[1]);
      }
      w[c0] = (S)v[0]; w[c0 + 1] = (S)v[1];
      if (cal.rd_cal) { cal.rd_cal[i * 6 + c0] = cv[0]; cal.rd_cal[i * 6 + c0 + 1] = cv[1]; }
      if (cal.clip) { cal.clip[i * 6 + c0] = cl[0] ? 1 : 0; cal.clip[i * 6 + c0 + 1] = cl[1] ? 1 : 0; }
    } else fixed_item<S, MODEL>(q, o, c, it - T, f, K, f_cap, false);
  }
}

template <class S, bool MODEL, int G>
static void launch_calib(const dim3& grid, hipStream_t st, const ReplaySeqIn& q, const ReplayTrajIn& t, const ReplayModelIn& m, const ReplayTimingIn& tm, const ReplayCalibIn& c, const ReplayOut<S>& o, int* code, double* delta, int f, int b0, int K, int f_cap) {
  hipLaunchKernelGGL((k_replay_expand_calib<S, MODEL, G>), grid, dim3(REPLAY_CHUNK), 0, st, q, t, m, tm, c, o, code, delta, f, b0, K, f_cap);
}
// the faulted form's grid: f_cap tracks of G lanes, G from m_cap
template <class S>
void launch_replay_expand_calib(const ReplaySeqIn& q, const ReplayTrajIn& t, const ReplayModelIn& m, const ReplayTimingIn& tm, const ReplayCalibIn& c, const ReplayOut<S>& o, int f, int b0, int nb, int K, int f_cap, hipStream_t st, int m_cap, int* code, double* delta) {
  if (nb <= 0) return;
  const bool model = m.L != nullptr;
  const int G = rp::fault_group(m_cap);
  const long items = (long)((f_cap * G + 63) & ~63) + fixed_items(model, K, f_cap);
  const dim3 grid((unsigned)((items + REPLAY_CHUNK - 1) / REPLAY_CHUNK), (unsigned)nb);
  auto go = [&](auto mdl) {
    constexpr bool MD = decltype(mdl)::value;
    if (G == 16) launch_calib<S, MD, 16>(grid, st, q, t, m, tm, c, o, code, delta, f, b0, K, f_cap);
    else if (G == 32) launch_calib<S, MD, 32>(grid, st, q, t, m, tm, c, o, code, delta, f, b0, K, f_cap);
    else launch_calib<S, MD, 64>(grid, st, q, t, m, tm, c, o, code, delta, f, b0, K, f_cap);
  };
  if (model) go(std::true_type{}); else go(std::false_type{});
}
template void launch_replay_expand_calib<float>(const ReplaySeqIn&, const ReplayTrajIn&, const ReplayModelIn&, const ReplayTimingIn&, const ReplayCalibIn&, const ReplayOut<float>&, int, int, int, int, int, hipStream_t, int, int*, double*);
template void launch_replay_expand_calib<double>(const ReplaySeqIn&, const ReplayTrajIn&, const ReplayModelIn&, const ReplayTimingIn&, const ReplayCalibIn&, const ReplayOut<double>&, int, int, int, int, int, hipStream_t, int, int*, double*);

// max_entries: the entries of the frame's largest sequence cell (the unfaulted grid's width; a trajectory with fewer leaves its
// lanes idle).  t.fault != nullptr: the faulted form, its grid sized from f_cap tracks of G lanes, G from m_cap.
template <class S, bool MODEL, int G>
static void launch_faulted(const dim3& grid, hipStream_t st, const ReplaySeqIn& q, const ReplayTrajIn& t, const ReplayModelIn& m, const ReplayOut<S>& o, int* code, int f, int b0, int K, int f_cap) {
  hipLaunchKernelGGL((k_replay_expand_faults<S, MODEL, G>), grid, dim3(REPLAY_CHUNK), 0, st, q, t, m, o, code, f, b0, K, f_cap);
}
template <class S>
void launch_replay_expand(const ReplaySeqIn& q, const ReplayTrajIn& t, const ReplayModelIn& m, const ReplayOut<S>& o, int f, int b0, int nb, int K, int f_cap, int max_entries, hipStream_t st, int m_cap, int* code) {
  if (nb <= 0) return;
  const bool model = m.L != nullptr;
  if (t.fault) {
    const int G = rp::fault_group(m_cap);
    const long items = (long)((f_cap * G + 63) & ~63) + fixed_items(model, K, f_cap);
    const dim3 grid((unsigned)((items + REPLAY_CHUNK - 1) / REPLAY_CHUNK), (unsigned)nb);
    auto go = [&](auto mdl) {
      constexpr bool MD = decltype(mdl)::value;
      if (G == 16) launch_faulted<S, MD, 16>(grid, st, q, t, m, o, code, f, b0, K, f_cap);
      else if (G == 32) launch_faulted<S, MD, 32>(grid, st, q, t, m, o, code, f, b0, K, f_cap);
      else launch_faulted<S, MD, 64>(grid, st, q, t, m, o, code, f, b0, K, f_cap);
    };
    if (model) go(std::true_type{}); else go(std::false_type{});
    return;
  }
  const long items = (long)max_entries + fixed_items(model, K, f_cap);
  const dim3 grid((unsigned)((items + REPLAY_CHUNK - 1) / REPLAY_CHUNK), (unsigned)nb);
  if (model) hipLaunchKernelGGL((k_replay_expand<S, true>), grid, dim3(REPLAY_CHUNK), 0, st, q, t, m, o, f, b0, K, f_cap);
  else hipLaunchKernelGGL((k_replay_expand<S, false>), grid, dim3(REPLAY_CHUNK), 0, st, q, t, m, o, f, b0, K, f_cap);
}
template void launch_replay_expand<float>(const ReplaySeqIn&, const ReplayTrajIn&, const ReplayModelIn&, const ReplayOut<float>&, int, int, int, int, int, int, hipStream_t, int, int*);
template void launch_replay_expand<double>(const ReplaySeqIn&, const ReplayTrajIn&, const ReplayModelIn&, const ReplayOut<double>&, int, int, int, int, int, int, hipStream_t, int, int*);

// msckf_hip_replay_fault_counts: the faults of the frames [f0, f1) counted without expanding anything -- one workgroup (one
// wavefront) per trajectory, lane l takes the (frame, track) pairs l, l + 64, ... and goes through a track's entries with
// rp::track_faults (the rule stated serially); the lanes are combined by wave_sum.  Integers below 2^53 in doubles: exact.
// n / M / off: the sequence store's sections from frame 0 ([frames][S], [frames][S][f_cap]); out [B][6] (replay_plan.h, FaultCount).
__global__ __launch_bounds__(64) void k_replay_fault_counts(const int* n, const int* M, const int* off, ReplayTrajIn t, int f0, int f1, int S, int f_cap, long long* out) {
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double p_miss = t.fault[(long)b * rp::N_FAULT + rp::FLT_P_MISS], p_out = t.fault[(long)b * rp::N_FAULT + rp::FLT_P_OUT];
  double c[rp::N_FAULT_COUNT] = {0, 0, 0, 0, 0, 0};
  const long items = (long)(f1 - f0) * f_cap;
  for (long it = lane; it < items; it += 64) {
    const int f = f0 + (int)(it / f_cap), tr = (int)(it % f_cap);
    const long cell = (long)f * S + s;
    if (tr >= n[cell]) continue;
    const int Mt = M[cell * f_cap + tr], e0 = off[cell * f_cap + tr] - off[cell * f_cap];
    const rp::TrackFaults tf = rp::track_faults(rp::fault_seed(seed, f), (uint64_t)e0, Mt, p_miss, p_out);
    c[rp::FC_ENTRIES] += Mt; c[rp::FC_MISSED] += tf.missed; c[rp::FC_OUTLIERS] += tf.outliers;
    c[rp::FC_TRACKS] += 1.0; c[rp::FC_TRACKS_SHORTENED] += tf.missed > 0; c[rp::FC_TRACKS_CONTAMINATED] += tf.outliers > 0;
  }
#pragma unroll
  for (int i = 0; i < rp::N_FAULT_COUNT; ++i) {
    const double v = wave_sum(c[i]);
    if (lane == 0) out[(long)b * rp::N_FAULT_COUNT + i] = (long long)v;
  }
}
void launch_replay_fault_counts(const int* n, const int* M, const int* off, const ReplayTrajIn& t, int f0, int f1, int S, int f_cap, int B, long long* out, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_replay_fault_counts, dim3((unsigned)B), dim3(64), 0, st, n, M, off, t, f0, f1, S, f_cap, out);
}

// One sample as the expansion stores it, before the rounding to the handle's scalar: v[6] of sample i with the readings r[7] --
// sigma4_pair's values, or model_stored's on the walk W(f, i) = start + P with P advanced past the sample as model_imu advances
// it.  CAL (replay_plan.h, CALIB): rp::calib_imu's row in the values' place and rp::calib_out on the sums; returns the mask of
// clipped components (0 without CAL).  Stated once for the sums and the counts.
template <bool MODEL, bool CAL>
__device__ __forceinline__ int sample_stored(const double* r, int i, uint64_t s_imu, const double* sg, const double* L, const double* start, double scale, const double* ic, double* P, double* v) {
#pragma clang fp contract(off)
  double cv[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) cv[c] = CAL ? rp::calib_imu(ic, r, c) : r[c];
  if constexpr (MODEL) {
    const double dT = r[6];
    double w[rp::NQ];
    if (dT > 0.0) model_w(s_imu, i, L, w);
    else for (int q = 0; q < rp::NQ; ++q) w[q] = 0.0;              // (not read: a sample with dT <= 0 gets no noise and no increment)
#pragma unroll
    for (int c = 0; c < rp::WALK_ROW; ++c) {
      const double W = start[c] + P[c];
      v[c] = model_stored(cv[c], W, scale, w[c < 3 ? c : 3 + c], dT);
      if (dT > 0.0) { const double d = model_delta(scale, w[c < 3 ? 3 + c : 6 + c], dT); P[c] = P[c] + d; }
    }
  } else {
#pragma unroll
    for (int p = 0; p < rp::IMU_PAIRS; ++p) sigma4_pair(cv, sg, s_imu, i, p, v[2 * p], v[2 * p + 1]);
  }
  int mask = 0;
  if constexpr (CAL) {
#pragma unroll
    for (int c = 0; c < 6; ++c) { bool cl; v[c] = rp::calib_out(ic, c, v[c], &cl); mask |= cl ? 1 << c : 0; }
  }
  return mask;
}
// msckf_hip_replay_imu_sums: what the expansion would hand each trajectory's propagate over the frames [f0, f1), summed --
// one workgroup (one wavefront) per trajectory; lane l takes the frames f0 + l, f0 + l + 64, ... in ascending order and a frame's
// samples i < k in ascending order, adds the count, the six scalars and dT of each sample as the expansion stores them (the
// value of sigma4_pair, or of model_stored on the walk W(f, i) = Wstart(f) + P(f, i) built as model_imu builds it; rounded to
// the handle's scalar S, widened to double) onto its own eight doubles; the lanes are combined by wave_sum.  The order of every
// addition is fixed: the same inputs give the same bits.  Skipped cells add nothing.  No LDS, no atomics.
// rd / kcell: the sequence store's readings [frames][S][K][7] and counts [frames][S] from frame 0; m.wstart: the walk table from
// row 0; out [B][8] (replay_plan.h, ImuSum).  CAL: imucal is the IMU calibration record [B][31] and the calibrated rows are
// summed (replay_plan.h, CALIB); without it imucal is not read.
template <class S, bool MODEL, bool CAL>
__global__ __launch_bounds__(64) void k_replay_imu_sums(const double* rd, const int* kcell, ReplayTrajIn t, ReplayModelIn m, const double* imucal, int f0, int f1, int n_seq, int K, int B, double* out) {
#pragma clang fp contract(off)
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double* ic = CAL ? imucal + (long)b * rp::IMU_CAL : nullptr;
  double acc[rp::IMU_SUM_ROW] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int f = f0 + lane; f < f1; f += 64) {
    const long cell = (long)f * n_seq + s;
    const int kc = kcell[cell];                                        // (a skipped cell's k is IMU_SKIP: nothing)
    const int k = kc < K ? kc : K;
    const double* cr = rd + cell * K * RD_STRIDE;
    const uint64_t s_imu = rp::imu_seed(seed, f);
    double P[rp::WALK_ROW] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < k; ++i) {
      const double* r = cr + i * RD_STRIDE;
      double v[6];
      if constexpr (MODEL) sample_stored<true, CAL>(r, i, s_imu, nullptr, m.L + (long)b * rp::L_SIZE, m.wstart + ((long)f * B + b) * rp::WALK_ROW, m.scale[b], ic, P, v);
      else sample_stored<false, CAL>(r, i, s_imu, t.sigma + (long)b * rp::N_SIGMA, nullptr, nullptr, 0.0, ic, P, v);
      acc[rp::IS_COUNT] += 1.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[rp::IS_OMEGA + c] += (double)(S)v[c];
      acc[rp::IS_DT] += (double)(S)r[6];
    }
  }
#pragma unroll
  for (int i = 0; i < rp::IMU_SUM_ROW; ++i) {
    const double v = wave_sum(acc[i]);
    if (lane == 0) out[(long)b * rp::IMU_SUM_ROW + i] = v;
  }
}
void launch_replay_imu_sums(const double* rd, const int* k, const ReplayTrajIn& t, const ReplayModelIn& m, int f0, int f1, int S, int K, int B, bool scalar_is_float, double* out, hipStream_t st, const double* imucal) {
  if (B <= 0) return;
  const bool model = m.L != nullptr;
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(64), 0, st, rd, k, t, m, imucal, f0, f1, S, K, B, out); };
  auto pick = [&](auto cal) {
    constexpr bool CAL = decltype(cal)::value;
    if (scalar_is_float) { if (model) go(k_replay_imu_sums<float, true, CAL>); else go(k_replay_imu_sums<float, false, CAL>); }
    else { if (model) go(k_replay_imu_sums<double, true, CAL>); else go(k_replay_imu_sums<double, false, CAL>); }
  };
  if (imucal) pick(std::true_type{}); else pick(std::false_type{});
}

// msckf_hip_replay_calib_counts: the samples of the frames [f0, f1) and the components the saturation clips, counted without
// expanding anything -- one workgroup (one wavefront) per trajectory, lane l takes the frames f0 + l, f0 + l + 64, ... in ascending
// order and a frame's samples i < k in ascending order, recomputes each stored value with sample_stored (what the expansion and
// the sums use) and counts; the lanes are combined by wave_sum, a fixed tree.  Integers below 2^53 in doubles: exact.
// out [B][8] (replay_plan.h, CalibCount).  No LDS, no atomics.
template <bool MODEL>
__global__ __launch_bounds__(64) void k_replay_calib_counts(const double* rd, const int* kcell, ReplayTrajIn t, ReplayModelIn m, const double* imucal, int f0, int f1, int n_seq, int K, int B, long long* out) {
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double* ic = imucal + (long)b * rp::IMU_CAL;
  double cnt[rp::N_CALIB_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int f = f0 + lane; f < f1; f += 64) {
    const long cell = (long)f * n_seq + s;
    const int kc = kcell[cell];                                        // (a skipped cell's k is IMU_SKIP: nothing)
    const int k = kc < K ? kc : K;
    const double* cr = rd + cell * K * RD_STRIDE;
    const uint64_t s_imu = rp::imu_seed(seed, f);
    double P[rp::WALK_ROW] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < k; ++i) {
      double v[6];
      int mask;
      if constexpr (MODEL) mask = sample_stored<true, true>(cr + i * RD_STRIDE, i, s_imu, nullptr, m.L + (long)b * rp::L_SIZE, m.wstart + ((long)f * B + b) * rp::WALK_ROW, m.scale[b], ic, P, v);
      else mask = sample_stored<false, true>(cr + i * RD_STRIDE, i, s_imu, t.sigma + (long)b * rp::N_SIGMA, nullptr, nullptr, 0.0, ic, P, v);
      cnt[rp::CCNT_SAMPLES] += 1.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) cnt[rp::CCNT_CLIP + c] += (mask >> c) & 1;
      cnt[rp::CCNT_ANY] += mask != 0;
    }
  }
#pragma unroll
  for (int i = 0; i < rp::N_CALIB_COUNT; ++i) {
    const double v = wave_sum(cnt[i]);
    if (lane == 0) out[(long)b * rp::N_CALIB_COUNT + i] = (long long)v;
  }
}
void launch_replay_calib_counts(const double* rd, const int* k, const ReplayTrajIn& t, const ReplayModelIn& m, const double* imucal, int f0, int f1, int S, int K, int B, long long* out, hipStream_t st) {
  if (B <= 0) return;
  if (m.L != nullptr) hipLaunchKernelGGL(k_replay_calib_counts<true>, dim3((unsigned)B), dim3(64), 0, st, rd, k, t, m, imucal, f0, f1, S, K, B, out);
  else hipLaunchKernelGGL(k_replay_calib_counts<false>, dim3((unsigned)B), dim3(64), 0, st, rd, k, t, m, imucal, f0, f1, S, K, B, out);
}

// The walk table of the model, wstart[frames + 1][B][6], once per assignment: workgroup b takes trajectory b.  Per chunk of
// REPLAY_SCAN_CHUNK frames lane j forms P(f, k_f) of frame f = chunk + j serially over the cell's samples into LDS; then six
// lanes, one per component, add the chunk's increments in frame order onto their running sum and store the rows.  The order of
// the additions is the normative one (no tree), the sum is carried in a register from chunk to chunk.
__global__ __launch_bounds__(REPLAY_SCAN_CHUNK) void k_replay_walk_scan(const double* rd, const int* kcell, ReplayTrajIn t, ReplayModelIn m, double* wstart, int frames, int S, int K, int B) {
#pragma clang fp contract(off)
  __shared__ double inc[REPLAY_SCAN_CHUNK][rp::WALK_ROW];
  const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double* L = m.L + (long)b * rp::L_SIZE;
  const double scale = m.scale[b];
  double run = 0.0;
  if (lane < rp::WALK_ROW) wstart[(long)b * rp::WALK_ROW + lane] = 0.0;
  for (int c0 = 0; c0 < frames; c0 += REPLAY_SCAN_CHUNK) {
    const int f = c0 + lane;
    if (f < frames) {
      const long cell = (long)f * S + s;
      const int k = kcell[cell];                                       // (a skipped cell's k is IMU_SKIP: nothing)
      double P[rp::WALK_ROW];
      model_prefix(rd + cell * K * RD_STRIDE, rp::imu_seed(seed, f), L, scale, k < K ? k : K, P);
      for (int c = 0; c < rp::WALK_ROW; ++c) inc[lane][c] = P[c];
    }
    __syncthreads();
    if (lane < rp::WALK_ROW) {
      const int n = frames - c0 < REPLAY_SCAN_CHUNK ? frames - c0 : REPLAY_SCAN_CHUNK;
      for (int j = 0; j < n; ++j) {
        run = run + inc[j][lane];
        wstart[((long)(c0 + j + 1) * B + b) * rp::WALK_ROW + lane] = run;
      }
    }
    __syncthreads();
  }
}

void launch_replay_walk_scan(const double* rd, const int* k, const ReplayTrajIn& t, const ReplayModelIn& m, double* wstart, int frames, int S, int K, int B, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(k_replay_walk_scan, dim3((unsigned)B), dim3(REPLAY_SCAN_CHUNK), 0, st, rd, k, t, m, wstart, frames, S, K, B);
}

}  // namespace msckf
