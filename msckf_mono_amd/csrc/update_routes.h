// update_routes.h -- which launches a measurement update turns into, stated once and free of device calls.
//
// A handle's geometry (what Batch<S>::alloc derives from B, n_cap, f_cap, m_cap and the scalar) and the route of each stage of
// the update -- feature kernels, the one-launch update of short windows, compression, Kalman stage -- as pure functions that
// return small PODs.  The launchers of kernels_feature / _qr / _gram / _chol / _kalman.hip and the head of launch_update
// (msckf_hip.hip) ask here and carry the answer out; none of them decides.  No HIP header, no heap, no lock (the functions
// run on the enqueue threads and on the single-filter path): a host compiler accepts this file on its own, and
// tests/cpp/update_routes_host.cpp prints the routes of a grid of handles for tests/test_update_routes.py.
// Every numeric bound of a route is a named constant below, stated once.
#ifndef MSCKF_UPDATE_ROUTES_H
#define MSCKF_UPDATE_ROUTES_H

#include <cstddef>

#if defined(__HIPCC__)
#define MSCKF_ROUTES_HD __host__ __device__
#else
#define MSCKF_ROUTES_HD
#endif

namespace msckf {
namespace routes {

// ---------------------------------------------------------------- the bounds
constexpr int N_CAP_MAX = 63;               // 6 n_cap + 1 <= 384 columns: six 64-column panels of the compression kernels
constexpr int M_REG = 30;                   // 2 * 30 + 4 = 64: the register-resident gate factorization of the feature kernels
constexpr int M_STAGED = 62;                // float: longest track whose gate matrix goes through LDS sixteen columns at a time
constexpr int LONG_BIN_SPLIT = 16;          // long tracks without the staged kernel: two bins once the range beyond M_REG spans this many lengths
constexpr int PAIR_F_CAP = 512;             // k_feature_pair: track capacity (its NC = 8 status words per lane)
constexpr int PAIR_SINGLE_TRACKS = 1024;    // k_feature_pair: a launch of at most this many tracks takes one track per wavefront
constexpr int PAIR_WAVES_PER_SIMD = 4;      // k_feature_pair: wavefronts per SIMD its register budget is held to (the kernel's attribute reads this)
constexpr int INFO_F_CAP = 1024;            // information-form compression: track capacity
constexpr int BLOCKS_ONE_LEVEL = 12;        // blocked matrix-core Cholesky: 16-column blocks in one level (192 columns)
constexpr int BLOCKS_TWO_LEVELS = 24;       // ... in two levels (384 columns)
constexpr int BLOCKS_REG_F64 = 8;           // register-resident k_gain / k_gain_w in double (float: BLOCKS_ONE_LEVEL)
constexpr int GRAM_PARTS = 3;               // split-K SYRK: copies of Lam^ that the one-level Cholesky adds up while loading
constexpr size_t CHOL_INV_LDS = 150 * 1024; // k_chol_inv keeps S in LDS up to here, in global memory beyond
constexpr int GAIN_TWO_PARTS_B = 96;        // blocked gain at 9 .. 12 blocks: two parts per trajectory from this batch size on, else four
constexpr int GAIN_W_8_NB = 64, GAIN_W_4_NB = 128;   // k_gain_w: 8 parts per trajectory up to 64 trajectories in the launch, 4 up to 128, else 2
constexpr size_t FEATURE_LDS = 160 * 1024;  // dynamic LDS granted to the feature kernels
constexpr size_t SMALL_LDS = 156 * 1024;    // ... that k_update_small may ask for
constexpr int ALL_LO = -0x7fffffff, ALL_HI = 0x7fffffff;   // a feature launch that takes every track length

// ---------------------------------------------------------------- LDS of the feature kernels
inline size_t feature_lds_bytes(int m_cap, size_t scalar, bool staged = false) {
  const size_t r2 = 2 * (size_t)m_cap + 4;
  const size_t x = (size_t)m_cap * 12 > 16 ? (size_t)m_cap * 12 : 16;
  return ((staged ? r2 * 17 : r2 * (r2 + 1) / 2) + x) * scalar + (size_t)m_cap * sizeof(int) + 16;
}
inline size_t feature_pair_lds_bytes(int lm, int& s_cap) {
  const int r2 = 2 * lm + 4;
  s_cap = r2 * (r2 + 1) / 2 + 12 * 13 / 2;            // the longest track + a 4-observation partner
  if (s_cap < 64) s_cap = 64;                          // the prologue's histogram lives there
  return ((size_t)s_cap + 16) * sizeof(float) + 2 * (size_t)lm * sizeof(int) + 16;
}
// Slots of k_feature_pair: its workgroups are single wavefronts, so a compute unit holds waves_per_simd of them on each of its
// four SIMDs as far as its LDS holds that many.  PAIR_WAVES_PER_SIMD is four because a slice of 32 trajectories x 200 tracks
// is 3 200 pair-wavefronts: three per SIMD are 3 072 slots on 256 compute units, one residency does not take the launch even on
// an empty chip; four are 4 096 (tests/test_feature_residency.py).
constexpr int SIMDS_PER_CU = 4;
struct PairResidency {
  int s_cap; size_t lds_bytes;   // what the launch asks for (feature_pair_lds_bytes)
  bool lds_fits;                 // SIMDS_PER_CU x waves_per_simd wavefronts' LDS fits FEATURE_LDS: the registers bound the residency
  int waves_per_cu;              // the smaller of the two bounds
  long slots(int cus) const { return (long)cus * waves_per_cu; }
  bool one_residency(long wavefronts, int cus) const { return wavefronts <= slots(cus); }
};
inline PairResidency feature_pair_residency(int lm, int waves_per_simd = PAIR_WAVES_PER_SIMD) {
  PairResidency r{};
  r.lds_bytes = feature_pair_lds_bytes(lm, r.s_cap);
  const size_t by_regs = (size_t)SIMDS_PER_CU * waves_per_simd, by_lds = FEATURE_LDS / r.lds_bytes;
  r.lds_fits = by_regs <= by_lds;
  r.waves_per_cu = (int)(r.lds_fits ? by_regs : by_lds);
  return r;
}

// ---------------------------------------------------------------- geometry of a handle
enum GeometryRefusal { GEO_OK = 0, GEO_N_CAP, GEO_M_CAP };   // alloc words the message
struct Geometry {
  GeometryRefusal refusal;
  int n6cap;       // 6 n_cap
  int ld;          // leading dimension of P and the D x * work matrices (multiple of 16)
  int ldR;         // row stride of the compression work matrices: 64-column panels >= 6 n_cap + 1
  int nchunk;      // TSQR chunks per trajectory: chunks x trajectories ~ one workgroup per CU
  int compress;    // 0 Householder TSQR, 3 information form (k_gram + blocked Cholesky)
  bool has_Mp;     // level A's per-panel M of the two-level Gram factorization
  bool has_Mp2;    // per-panel M of the two-level factorization of S
  bool lam_parts;  // Lam^ has room for the split-K copies (lam_part > 0)
};
inline Geometry geometry(int B, int n_cap, int f_cap, int m_cap, size_t scalar) {
  Geometry g{};
  g.n6cap = 6 * n_cap;
  g.ld = ((15 + 6 * n_cap + 15) / 16) * 16;
  g.ldR = ((6 * n_cap + 1 + 63) / 64) * 64;
  g.refusal = g.ldR / 16 > BLOCKS_TWO_LEVELS ? GEO_N_CAP : feature_lds_bytes(m_cap, scalar) > FEATURE_LDS ? GEO_M_CAP : GEO_OK;
  g.nchunk = 1;
  while (g.nchunk < 8 && (long)B * g.nchunk * 2 <= 256) g.nchunk *= 2;
  g.compress = (g.ldR <= 16 * BLOCKS_TWO_LEVELS && f_cap <= INFO_F_CAP) ? 3 : 0;
  g.has_Mp2 = g.n6cap > 16 * BLOCKS_ONE_LEVEL;
  g.has_Mp = g.compress && g.ldR > 16 * BLOCKS_ONE_LEVEL;
  g.lam_parts = g.compress && g.ldR <= 16 * BLOCKS_ONE_LEVEL;   // windows up to 31 cameras
  return g;
}
inline int column_blocks(int n6cap) { return (n6cap + 15) / 16; }   // 16-column blocks of S

// Compression route of an update's launches (k_feature publishes B^ only for the information form): the handle's geometry,
// or the handle's override where the information form's buffers exist; a batch with a trajectory on the literal anisotropic
// route always takes the information form (that route hands over an information matrix: Cholesky tail).
inline int effective_compress(int geometry_compress, int override_route, int n_lit) {
  int cmp = geometry_compress;
  if (override_route >= 0) cmp = (override_route && geometry_compress) ? 3 : 0;
  if (n_lit > 0 && !cmp) cmp = geometry_compress;
  return cmp;
}

// ---------------------------------------------------------------- feature route
// pair: k_feature_pair (float, information form), else k_feature<S, long_form>; the launch takes the tracks of m_lo < M <= m_hi
struct FeatureLaunch { bool pair, long_form; int lm, m_lo, m_hi, staged, single, items; };
struct FeatureRoute { int n; FeatureLaunch l[3]; };
inline FeatureRoute feature_route(size_t scalar, int f_cap, int m_cap, int nb, int feat_pair, int compress) {
  FeatureRoute r{};
  auto plain = [&](bool long_form, int lm, int m_lo, int m_hi, int staged) { r.l[r.n++] = FeatureLaunch{false, long_form, lm, m_lo, m_hi, staged, 0, 0}; };
  const bool reg = m_cap <= M_REG;
  // float filters on the information-form route: tracks of up to M_REG observations two per wavefront.  A small launch takes
  // ONE track per wavefront (feat_pair 2 forces pairs, 3 the single form)
  const bool pair = scalar == 4 && feat_pair && compress && f_cap <= PAIR_F_CAP;
  if (pair) {
    const int single = (feat_pair == 3 || (feat_pair == 1 && (long)nb * f_cap <= PAIR_SINGLE_TRACKS)) ? 1 : 0;
    r.l[r.n++] = FeatureLaunch{true, false, reg ? m_cap : M_REG, ALL_LO, reg ? ALL_HI : M_REG, 0, single, single ? f_cap : (f_cap + 1) / 2};
  }
  if (reg) { if (!pair) plain(false, m_cap, ALL_LO, ALL_HI, 0); return r; }
  // long windows: tracks binned by length, one launch per bin over the same grid
  if (!pair) plain(false, M_REG, ALL_LO, M_REG, 0);
  if (scalar == 4 && m_cap <= M_STAGED && feat_pair) { plain(true, m_cap, M_REG, ALL_HI, 1); return r; }   // ONE launch takes every long track
  if (m_cap - M_REG >= LONG_BIN_SPLIT) {
    const int mid = (M_REG + m_cap + 1) / 2;
    plain(true, mid, M_REG, mid, 0);
    plain(true, m_cap, mid, ALL_HI, 0);
  } else plain(true, m_cap, M_REG, ALL_HI, 0);
  return r;
}

// ---------------------------------------------------------------- k_update_small: the whole update of a short window in one launch
constexpr int US_UMAX = 2;     // tasks per wavefront of the factorizations
constexpr int US_SEG_E = 12;   // columns per task of chol(S) with its D + 1 riding rows (10 cameras: 3 row chunks x 5 segments = 15 tasks); chol(Lam^): SEGB = 4 (61 rows: one chunk, 15 tasks) or 8
// scalars of the PHt / W block [15 + n_max][n_max | 1]: it also stages 24 rows of B^ (doubles, 16 ceil((n_max + 1) / 16) + 1 columns) in
// phase A, the larger need for the first few frames of a window; and of the P staging block [n_max][(15 + n_max) | 1], later S [n_max][n_max | 1]
MSCKF_ROUTES_HD inline size_t update_small_ph_elems(int n_max, size_t scalar) {
  const size_t w = (size_t)(15 + n_max) * (n_max | 1), nb1 = 16 * (((size_t)n_max + 1 + 15) / 16) + 1, stg = (24 * nb1 * sizeof(double) + scalar - 1) / scalar;
  return ((w > stg ? w : stg) + 3) & ~(size_t)3;
}
// (phase A keeps two ints per included track there: f_cap of them at most)
MSCKF_ROUTES_HD inline size_t update_small_pt_elems(int n_max, int f_cap, size_t scalar) {
  const size_t a = (size_t)n_max * ((15 + n_max) | 1), b = (size_t)n_max * (n_max | 1), c = ((size_t)f_cap * 2 * sizeof(int) + scalar - 1) / scalar;
  const size_t m = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return (m + 3) & ~(size_t)3;
}
inline size_t update_small_lds_bytes(int n_max, int f_cap, size_t scalar) {
  const size_t n1 = (size_t)n_max + 1, LL = n1 | 1, Dm = 15 + (size_t)n_max, cstride = 2 * (size_t)n_max + 20;
  return (n1 * LL + n1 + 1 + 2 * cstride) * sizeof(double) + (update_small_pt_elems(n_max, f_cap, scalar) + update_small_ph_elems(n_max, scalar) + n_max + 2 + Dm + 1) * scalar + 64;
}
// column-segment width of chol(Lam^) for a launch sized by n_max columns: ceil(n / SEG) x ceil((n + 1) / 64) tasks on 16 wavefronts
// (4 up to 63 columns, 8 beyond); 0: neither fits
inline int update_small_segb(int n_max) {
  const int nrcb = (n_max + 1 + 63) / 64;
  if (((n_max + 3) / 4) * nrcb <= 16 * US_UMAX) return 4;
  if (((n_max + 7) / 8) * nrcb <= 16 * US_UMAX) return 8;
  return 0;
}
// does a window of n_max camera columns fit k_update_small (its LDS, the tasks of its factorizations)?  Monotone in n_max.
// granted: the device granted the kernel its dynamic LDS (kalman_device_setup)
inline bool update_small_fits(int n_max, int f_cap, size_t scalar, bool granted) {
  // tasks of chol(S): ceil(n / 12) x ceil((2 n + 16) / 64) <= 32; tiles of Lam^: <= 15 of the 16 wavefronts
  const int ncs = (n_max + US_SEG_E - 1) / US_SEG_E, nrc = (2 * n_max + 16 + 63) / 64, nt1 = (n_max + 1 + 15) / 16;
  return granted && update_small_lds_bytes(n_max, f_cap, scalar) <= SMALL_LDS && ncs * nrc <= 16 * US_UMAX && update_small_segb(n_max) != 0 &&
         nt1 * (nt1 + 1) / 2 <= 16 && (15 + n_max) * n_max <= 1024 * 7;
}
// settings.small_update as far as it fits at this handle's dtype and f_cap: the per-trajectory limit (columns) the update routes by
inline int small_limit(int small_update, int f_cap, size_t scalar, bool granted) {
  for (int n = small_update / 6 * 6; n >= 6; n -= 6) if (update_small_fits(n, f_cap, scalar, granted)) return n;
  return 0;
}
// camera columns of a trajectory's window when its update runs: run_frames enqueues the update before its host mirror has the
// frame's augmentState (ahead = 1), and a skipped cell has no augmentState ahead
inline int window_cols(int ncam, int ahead, bool skipped, int n_cap) {
  const int n = ncam + (skipped ? 0 : ahead);
  return 6 * (n < n_cap ? n : n_cap);
}
// Which route a TRAJECTORY takes depends on its own window size only.  A range whose windows all lie on one side of limit
// launches that side's sequence alone; a range with windows on both sides launches both (Dev::small_split = small_split), and
// k_update_small is sized by the largest short window, nsmall.  An empty window has no update: it makes no range mixed, and in
// a mixed one it is k_update_small's.
enum SmallKind { CHAIN_ONLY = 0, SMALL_ONLY, SMALL_AND_CHAIN };
struct SmallRoute { SmallKind kind; int small_split, nsmall, segb; };
// cols(i): window_cols of the range's i-th trajectory
template <class Cols>
inline SmallRoute small_route(int nb, Cols&& cols, int limit, int compress, int n_lit, int joseph, int f_cap, size_t scalar, bool granted) {
  SmallRoute r{CHAIN_ONLY, 0, 0, 0};
  if (!limit || !compress || n_lit != 0 || joseph != 0) return r;
  int nmax = 0, nsmall = 0;                    // largest window of the range, largest one within the limit
  for (int i = 0; i < nb; ++i) { const int n = cols(i); if (n > nmax) nmax = n; if (n > 0 && n <= limit && n > nsmall) nsmall = n; }
  const bool mixed = nsmall > 0 && nmax > limit;
  if (!((nmax > 0 && nmax <= limit) || mixed)) return r;
  if (!update_small_fits(nsmall, f_cap, scalar, granted)) return r;   // (not reached: limit fits, and the rule is monotone) the chain takes everybody
  r.kind = mixed ? SMALL_AND_CHAIN : SMALL_ONLY;
  r.small_split = mixed ? limit : 0;
  r.nsmall = nsmall;
  r.segb = update_small_segb(nsmall);
  return r;
}

// ---------------------------------------------------------------- compression route
// TSQR (launch_compress) or information form: k_select with the block-diagonal sums, k_gram with gram_parts split-K copies,
// then [T | r_n] = chol(Lam^) in one level (k_chol_mfma<.., nb_a, .., CH_GRAM>) or two (CH_GRAM_A<nb_a>, TR_GRAM over
// trsm_items, CH_GRAM_B<nb_b>).  chol_levels == 0 on the information form: no Cholesky takes this width.
struct CompressRoute { bool info, select_diag; int gram_parts, chol_levels, nb_a, nb_b, trsm_items; };
inline CompressRoute compress_route(int compress, int ldR, bool has_Mp, bool lam_parts, int gram_parts_setting) {
  CompressRoute r{};
  r.info = r.select_diag = compress != 0;
  r.gram_parts = 1;
  if (!r.info) return r;
  const int nblk = ldR / 16;
  if (nblk == 4 || nblk == 8 || nblk == BLOCKS_ONE_LEVEL) { r.chol_levels = 1; r.nb_a = nblk; }
  else if (has_Mp && (nblk == 16 || nblk == 20 || nblk == BLOCKS_TWO_LEVELS)) {
    r.chol_levels = 2; r.nb_a = BLOCKS_ONE_LEVEL; r.nb_b = nblk - BLOCKS_ONE_LEVEL; r.trsm_items = (nblk - BLOCKS_ONE_LEVEL + 3) / 4;
  }
  // split-K partial sums only where the consumer adds them up: the one-level Cholesky
  if (r.chol_levels == 1 && lam_parts) r.gram_parts = gram_parts_setting >= GRAM_PARTS ? gram_parts_setting : GRAM_PARTS;
  return r;
}

// ---------------------------------------------------------------- Householder TSQR route (kernels_qr.hip)
// k_qr_update<S, NC, RW, RLDS>: NC 64-column panels of [R | Q^T r] per lane, blocks of RW stacked rows per wavefront, the packed
// work triangle in LDS (RLDS) or ldR-strided in global memory.  Stage 1 runs nchunk workgroups per trajectory, stage 2 merges
// their triangles into chunk 0 (merge: it runs only where there is more than one chunk).
constexpr int QR_PIPELINE = 12;             // wavefronts per workgroup = depth of the software pipeline over R's rows
constexpr int QR_RING = 512;                // progress words per workgroup: block q of a chunk lives in slot q % QR_RING (a power of two)
constexpr size_t QR_TRI_LDS = 150 * 1024;   // the progress ring + the packed triangle stay in LDS up to here, the triangle in global memory beyond
constexpr int QR_RW_WIDE = 32, QR_RW = 16;  // rows per block: 32 where the registers hold them (float, up to QR_RW_WIDE_NC panels), else 16
constexpr int QR_RW_WIDE_NC = 3;
constexpr int QR_NC_MAX = 6;                // 384 columns (N_CAP_MAX)
constexpr int qr_rows_per_block(size_t scalar, int nc) { return (scalar == 4 && nc <= QR_RW_WIDE_NC) ? QR_RW_WIDE : QR_RW; }
struct TsqrRoute { int nc, rw; bool tri_lds; size_t lds_bytes; int nchunk; bool merge; };
inline TsqrRoute tsqr_route(size_t scalar, int n6cap, int ldR, int nchunk) {
  TsqrRoute r{};
  r.nc = ldR / 64 < QR_NC_MAX ? ldR / 64 : QR_NC_MAX;
  r.rw = qr_rows_per_block(scalar, r.nc);
  const size_t ring = sizeof(int) * (size_t)QR_RING, tri = scalar * (size_t)(n6cap + 1) * (n6cap + 2) / 2;
  r.tri_lds = ring + tri <= QR_TRI_LDS;
  r.lds_bytes = r.tri_lds ? ring + tri : ring;
  r.nchunk = nchunk;
  r.merge = nchunk > 1;
  return r;
}

// ---------------------------------------------------------------- Kalman route
// the float blocked gain solve k_chol_mfma<float, float, NB, NA, CH_GAIN, NPART>: NPART parts x NA blocks of 16 rows cover the
// D + 1 appended rows (rows per part = 16 NA - 1; D = 15 + 6 n_cap <= NPART (16 NA - 1))
struct BlockedGain { int nb, na, npart; };
constexpr BlockedGain BLOCKED_GAIN[4] = {{4, 2, 3},     // D <= 79 <= 3 * 31
                                         {8, 3, 3},     // D <= 143 <= 3 * 47
                                         {12, 4, 4},    // D <= 207 <= 4 * 63
                                         {12, 7, 2}};   // D <= 207 <= 2 * 111
constexpr bool has_blocked_gain(size_t scalar) { return scalar == 4; }
constexpr int reg_blocks_max(size_t scalar) { return scalar == 4 ? BLOCKS_ONE_LEVEL : BLOCKS_REG_F64; }
enum GainSolve {
  GAIN_NONE = 0,
  GAIN_BLOCKED,    // BLOCKED_GAIN[blocked]: factors S with [PHt ; r_n^T] appended; forms S itself where fused_s says so
  GAIN_W,          // k_gain_w<S, nbn, npart>
  GAIN_LARGE,      // CH_S_A<nb_a>, TR_S21 over items_s21, CH_S_B<nb_b>, TR_W<nb_w> over items_w, k_dx_wz
  GAIN_CHOL_INV,   // k_chol_inv (LDS or global), OP_W, k_dx_w
  GAIN_K,          // Joseph form: k_gain<S, nbn>, k_inject<S, true>
  GAIN_K_CHOL_INV  // Joseph form: k_chol_inv (LDS or global), OP_W, OP_K, k_inject<S, false>
};
struct KalmanRoute {
  GainSolve solve;
  bool s_fused;                  // PHt is written only row-major and no S GEMM runs: the gain solve forms S
  int blocked;                   // GAIN_BLOCKED
  int nbn, npart;                // GAIN_W, GAIN_K
  int nb_a, items_s21, nb_b, nb_w, items_w;   // GAIN_LARGE
  bool chol_inv_lds; size_t chol_inv_bytes;   // GAIN_CHOL_INV, GAIN_K_CHOL_INV
};
// form: 0 square-root gain form, 1 the reference's Joseph sequence, 2 square-root gain form with the register-resident solve.
// B: the whole batch (its slices run these launches side by side); nb: the launch's trajectories
inline KalmanRoute kalman_route(size_t scalar, int n_cap, int B, int nb, int form, int fused_s, int gain_parts, bool has_Mp2) {
  KalmanRoute r{};
  const int n = 6 * n_cap, nbn = column_blocks(n), reg_max = reg_blocks_max(scalar);
  const int nbn_reg = nbn <= 4 ? 4 : nbn <= 8 ? 8 : reg_max;   // the register-resident instantiation that holds nbn blocks
  auto chol_inv = [&](GainSolve s) {
    r.solve = s;
    r.chol_inv_bytes = (size_t)n * (n + 1) * scalar;
    r.chol_inv_lds = r.chol_inv_bytes <= CHOL_INV_LDS;
    if (!r.chol_inv_lds) r.chol_inv_bytes = 0;
  };
  if (form == 1) {
    if (nbn <= reg_max) { r.solve = GAIN_K; r.nbn = nbn_reg; }
    else chol_inv(GAIN_K_CHOL_INV);
  } else if (form == 0 && has_blocked_gain(scalar) && nbn <= BLOCKS_ONE_LEVEL) {
    r.solve = GAIN_BLOCKED;
    if (nbn <= 4) r.blocked = 0;
    else if (nbn <= 8) r.blocked = 1;
    else {
      // four parts per trajectory fill the chip at 64 trajectories; from a batch of GAIN_TWO_PARTS_B on, two parts (each redoes the
      // factorization: half the workgroups, one round of them instead of two).  Same bits either way; gain_parts 2 | 4 forces one
      const bool two = gain_parts ? gain_parts == 2 : B >= GAIN_TWO_PARTS_B;
      r.blocked = (two && 15 + n <= BLOCKED_GAIN[3].npart * (16 * BLOCKED_GAIN[3].na - 1)) ? 3 : 2;
    }
  } else if (nbn <= reg_max) {
    r.solve = GAIN_W; r.nbn = nbn_reg;
    r.npart = nb <= GAIN_W_8_NB ? 8 : nb <= GAIN_W_4_NB ? 4 : 2;   // more workgroups per trajectory while the batch leaves CUs idle
  } else if (form == 0 && nbn > BLOCKS_ONE_LEVEL && nbn <= BLOCKS_TWO_LEVELS && has_Mp2) {
    r.solve = GAIN_LARGE;
    const int nb2 = nbn <= 16 ? 4 : nbn <= 20 ? 8 : 12, rblk = (15 + n + 1 + 15) / 16;   // rblk: 16-row blocks of [P T_H^T ; r_n^T]
    r.nb_a = BLOCKS_ONE_LEVEL; r.items_s21 = (nbn - BLOCKS_ONE_LEVEL + 3) / 4; r.nb_b = nb2; r.nb_w = BLOCKS_ONE_LEVEL + nb2; r.items_w = (rblk + 3) / 4;
  } else chol_inv(GAIN_CHOL_INV);
  r.s_fused = r.solve == GAIN_BLOCKED && fused_s != 0;
  return r;
}

}  // namespace routes
}  // namespace msckf
#endif
