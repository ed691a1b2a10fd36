// kernels_chol.hip -- blocked right-looking Cholesky on the matrix cores, one workgroup (16 wavefronts) per matrix.
//
// Two uses, one kernel template:
//   GRAM (T = double): [T_H | r_n] = chol(Lam^), Lam^ = [H_o | r_o]^T [H_o | r_o] accumulated by k_gram -- the
//        compression of the stacked Jacobian (HouseholderQR + Q_1^T r_o of measurementUpdate, msckf.h:1338-1366) in
//        information form; semi-definite pivot skipping (a direction the stack says nothing about gives
//        a zero row of T_H).
//   GAIN (T = float):  S = L L^T for S = T_H P T_H^T + R_n (msckf.h:1369) with the rows [P T_H^T ; r_n^T] appended, which
//        the factorization turns into W = P T_H^T L^-T and z^T = (L^-1 r_n)^T; dx = K r_n = W z (msckf.h:1370-1373 without
//        the explicit inverse).  NPART workgroups per trajectory share the appended rows (each redoes the factorization).
//
// The trailing matrix lives in MFMA accumulators: 16 x 16 blocks, 4 x 4 block-cyclic over the sixteen wavefronts.  Per panel
// of 16 columns:
//   (1) the owners drop the panel's blocks into LDS;
//   (2) ONE wavefront factors the 16 x 16 diagonal block with lane = row, pivots and multipliers broadcast by v_readlane,
//       and runs the SAME eliminations on the rows of the identity: that yields M with  y = x M  for the forward
//       substitution of any row x against the block (zero columns for skipped pivots included);
//   (3) all wavefronts form the panel below the diagonal as L21 = A21 M on the matrix cores (the per-row substitution of
//       round 2's kernel -- 136 dependent FMAs fed by LDS reads per thread -- is gone);
//   (4) finished rows of T_H / columns of W go to global memory, dx accumulates;
//   (5) rank-16 update of the trailing blocks, operands straight from the LDS panel.
// 12 panels x 4 barriers instead of 180 steps x (LDS exchange + barrier); the O(n^3) part runs at MFMA rate.
// The body is chol_mfma_body (chol_mfma.h): k_chol_mfma runs it, and so do the CHOL instances of k_propagate
// (kernels_state.hip), which put the one-level Gram Cholesky and propagate + augmentState into one launch.
#include <utility>

#include "dev_common.h"
#define MSCKF_CHOL_TIMERS 1   // the -DMSCKF_ABLATE phase timers of the body count in this file's kernels
#include "chol_mfma.h"

namespace msckf {

template <class T, class SO, int NB, int NA, int MODE, int NPART>
__global__ __launch_bounds__(1024) void k_chol_mfma(Dev<SO> d, int b0, int nb) {
  chol_mfma_body<T, SO, NB, NA, MODE, NPART>(d, b0, nb, (int)blockIdx.x);
}

// Y = X L^-T for 16-row blocks X that do not take part in the factorization itself, one block per wavefront, independent
// of every other block.  Per 16-column panel p of L: Y_p = X_p M_p on the matrix cores (M_p from the factorization:
// y = x M solves y L_pp^T = x), then X_q -= Y_p L(q, p)^T for the panels right of it.
//   TR_GRAM  X = rows CH_SPLIT .. n of Lam^ (the row n = H_o^T r_o included), columns < CH_SPLIT: L21 of the two-level
//            Gram factorization; Y goes back to Lam (f64, read by level B) and, transposed, into T_H's columns CH_SPLIT..
//   TR_S21   the same for S (rows CH_SPLIT .. n-1 of Smat), in place
//   TR_W     X = [P T_H^T ; r_n^T] (D + 1 rows, all n columns): W = P T_H^T L^-T (msckf.h:1370 without the inverse) and
//            z = L^-1 r_n, left in W and Linv[0..n)
enum { TR_GRAM = 0, TR_S21 = 1, TR_W = 2 };
template <class T, class SO, int NP, int TMODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 4))) void k_trsm_rows(Dev<SO> d, int b0, int nb, int nwg) {
  typedef typename Mfma16<T>::V V;
  constexpr int LP = 17;
  // the row blocks of a trajectory all read its factor L: on one XCD (xcd_item), whose private L2 then fetches it once
  int bi_, wg_;
  if (!xcd_item(nb, nwg, bi_, wg_)) return;
  const int b = b0 + bi_, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int* st = d.stats + (long)b * STAT_STRIDE;
  if (st[STAT_MROWS] == 0 || other_route(d, d.ncam[b], false)) return;
  const int i = 4 * wg_ + w;                             // 16-row block
  const int nfull = 6 * d.ncam[b], D = 15 + nfull;
  const int ncols = TMODE == TR_W ? nfull : min(nfull, CH_SPLIT);      // columns of L that exist
  const int R0 = TMODE == TR_W ? 16 * i : CH_SPLIT + 16 * i;           // first row of the block (TR_W: row of [PHt ; r_n^T])
  const int row_end = TMODE == TR_GRAM ? nfull + 1 : (TMODE == TR_S21 ? nfull : D + 1);   // rows that exist
  // (a wavefront without a block keeps taking part in the staging of L and its barriers: `active` instead of a return)
  bool active = TMODE == TR_GRAM ? R0 < d.ldR : R0 < row_end;
  double* Lam = TMODE == TR_GRAM ? d.Lam + (long)b * d.ldR * d.ldR : nullptr;
  SO* Sm = TMODE != TR_GRAM ? d.Smat + (long)b * d.n6cap * d.n6cap : nullptr;
  SO* Rt = d.Rbuf + ((long)b * d.nchunk) * (long)d.n6cap * d.ldR;
  __shared__ T sT[4][16][LP];
  // round 6: the block column L(q, p), q > p, of the panel in LDS, fetched once per WORKGROUP with whole 64-byte rows; every
  // wavefront of the four takes its MFMA operands from there.  (Before: every wavefront fetched every operand itself, a 4-byte
  // load per lane scattered over sixteen rows, one per MFMA: the W solve of a 60-camera window ran at 9 % of the f32 MFMA rate.)
  __shared__ T sLc[(NP - 1) * 16][LP];
  if (TMODE == TR_GRAM && active && R0 >= row_end) {     // nothing below the split in this block: zero columns of T_H
    for (int e = lane; e < 16 * CH_SPLIT; e += 64) { const int k = e >> 4, c = e & 15; if (k < nfull) Rt[(long)k * d.ldR + R0 + c] = SO(0); }
    active = false;
  }
  auto xin = [&](int row, int col) -> T {                // X(row, col), row = absolute row of this mode's operand
    if (TMODE == TR_GRAM) return (T)lam_hat(Lam, nullptr, d.ldR, nfull, d.n_cap, row, col);
    if (col >= ncols) return T(0);
    if (TMODE == TR_S21) return row < nfull ? (T)Sm[(long)row * d.n6cap + col] : T(0);
    if (row < D) return (T)d.K[(long)b * d.ld * d.n6cap + (long)row * d.n6cap + col];   // row-major copy of P T_H^T left by OP_PHT
    return row == D ? (T)Rt[(long)col * d.ldR + nfull] : T(0);                           // r_n[col]
  };
  auto lblk = [&](int q, int p, int r, int c) -> T {     // L(16 q + r, 16 p + c)
    if (TMODE == TR_GRAM) return (T)Lam[(long)(16 * q + r) * d.ldR + 16 * p + c];
    return (T)Sm[(long)(16 * q + r) * d.n6cap + 16 * p + c];
  };
  const int lrow_max = (TMODE == TR_GRAM ? d.ldR : d.n6cap) - 1;   // last row of L's storage (rows past the matrix multiply columns that are never stored)
  V acc[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[q][r] = active ? xin(R0 + Mfma16<T>::row(lane, r), 16 * q + (lane & 15)) : T(0);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if (16 * p >= ncols) continue;
    // the panel's block column into LDS: rows 16 (p + 1) .. of the columns 16 p .. 16 p + 15 (sixteen threads per 64-byte row)
    if (p + 1 < NP) {
      __syncthreads();                                   // the previous panel's operands have been read
      const int NRW = (NP - 1 - p) * 16;
      for (int e0 = 0; e0 < NRW * 16; e0 += 256) {
        const int e = e0 + tid, r = e >> 4, c = e & 15;
        if (e < NRW * 16 && 16 * (p + 1) + (r & ~15) < ncols) sLc[r][c] = lblk(p + 1, p, min(r, lrow_max - 16 * (p + 1)), c);
      }
      __syncthreads();
    }
    if (!active) continue;
    // Y = X_p M_p
#pragma unroll
    for (int r = 0; r < 4; ++r) sT[w][Mfma16<T>::row(lane, r)][lane & 15] = acc[p][r];
    wave_lds_sync();
    V y = V{0, 0, 0, 0};
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const T a = sT[w][lane & 15][(lane >> 4) + 4 * s4];
      const int mi = ((lane >> 4) + 4 * s4) * 16 + (lane & 15);
      const T bq = TMODE == TR_GRAM ? (T)d.Mp[((long)b * (CH_SPLIT / 16) + p) * 256 + mi] : (T)d.Mp2[((long)b * 24 + p) * 256 + mi];
      y = Mfma16<T>::mma(a, bq, y);
    }
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = Mfma16<T>::row(lane, r), col = lane & 15;
      sT[w][row][col] = y[r];
      if (TMODE == TR_GRAM) { if (R0 + row <= nfull) Lam[(long)(R0 + row) * d.ldR + 16 * p + col] = (double)y[r]; }
      if (TMODE == TR_S21) { if (R0 + row < nfull && 16 * p + col < ncols) Sm[(long)(R0 + row) * d.n6cap + 16 * p + col] = (SO)y[r]; }
    }
    wave_lds_sync();
    // transposed outputs, lanes along the rows of the block
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 16 * p + (lane >> 4) + 4 * r, c = lane & 15;
      const T yv = sT[w][c][(lane >> 4) + 4 * r];
      if (TMODE == TR_GRAM) { if (k < nfull) Rt[(long)k * d.ldR + R0 + c] = (R0 + c <= nfull) ? (SO)yv : SO(0); }
      if (TMODE == TR_W && k < nfull) {
        if (R0 + c < D) d.W[(long)b * d.ld * d.n6cap + (long)k * d.ld + R0 + c] = (SO)yv;
        else if (R0 + c == D) d.Linv[(long)b * d.n6cap * d.n6cap + k] = (SO)yv;       // z_k
      }
    }
    // X_q -= Y L(q, p)^T, q > p
    T a[4];
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) a[s4] = -sT[w][lane & 15][4 * s4 + (lane >> 4)];
#pragma unroll
    for (int q = p + 1; q < NP; ++q) {
      if (16 * q >= ncols) continue;
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) acc[q] = Mfma16<T>::mma(a[s4], sLc[(q - p - 1) * 16 + (lane & 15)][4 * s4 + (lane >> 4)], acc[q]);
    }
    wave_lds_sync();
    __builtin_amdgcn_sched_barrier(0);   // keep the next panels' loads of L out of this one (the scheduler otherwise hoists them all: spills)
  }
}

// dx = W z (z = L^-1 r_n left in Linv[0..n) by k_trsm_rows<TR_W>); one workgroup per trajectory
template <class SO>
__global__ __launch_bounds__(256) void k_dx_wz(Dev<SO> d, int b0) {
  const int b = b0 + blockIdx.x, tid = threadIdx.x;
  if (d.stats[(long)b * STAT_STRIDE + STAT_MROWS] == 0 || other_route(d, d.ncam[b], false)) return;
  const int n = 6 * d.ncam[b], D = 15 + n;
  __shared__ SO sz[384];
  for (int j = tid; j < n; j += 256) sz[j] = d.Linv[(long)b * d.n6cap * d.n6cap + j];
  __syncthreads();
  const SO* W = d.W + (long)b * d.ld * d.n6cap;
  for (int i = tid; i < D; i += 256) {
    SO s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    int j = 0;
    for (; j + 3 < n; j += 4) { s0 += W[(long)j * d.ld + i] * sz[j]; s1 += W[(long)(j + 1) * d.ld + i] * sz[j + 1]; s2 += W[(long)(j + 2) * d.ld + i] * sz[j + 2]; s3 += W[(long)(j + 3) * d.ld + i] * sz[j + 3]; }
    for (; j < n; ++j) s0 += W[(long)j * d.ld + i] * sz[j];
    d.dx[(long)b * d.ld + i] = (s0 + s1) + (s2 + s3);
  }
}

// S = L L^T in two levels, W = P T_H^T L^-T, z = L^-1 r_n, dx = W z for windows with n > 192 (6 n_cap in {256, 320, 384} padded)
template <class S>
void launch_chol_gain_large(const Dev<S>& d, int b0, int nb, hipStream_t st, const routes::KalmanRoute& r) {
  if (nb <= 0) return;
  hipLaunchKernelGGL((k_chol_mfma<S, S, 12, 0, CH_S_A, 1>), dim3(nb), dim3(1024), 0, st, d, b0, nb);
  hipLaunchKernelGGL((k_trsm_rows<S, S, 12, TR_S21>), dim3(xcd_grid(nb, r.items_s21)), dim3(256), 0, st, d, b0, nb, r.items_s21);
  dispatch_int<4, 8, 12>(r.nb_b, [&](auto NB) { hipLaunchKernelGGL((k_chol_mfma<S, S, NB(), 0, CH_S_B, 1>), dim3(nb), dim3(1024), 0, st, d, b0, nb); });
  dispatch_int<16, 20, 24>(r.nb_w, [&](auto NB) { hipLaunchKernelGGL((k_trsm_rows<S, S, NB(), TR_W>), dim3(xcd_grid(nb, r.items_w)), dim3(256), 0, st, d, b0, nb, r.items_w); });
  hipLaunchKernelGGL((k_dx_wz<S>), dim3(nb), dim3(256), 0, st, d, b0);
}

// (Measured and rejected, round 4: the factorizations padded with unused dynamic LDS so that they have their compute unit to
// themselves -- the gain factorization leaves 128 registers per SIMD free, room for one k_feature wavefront of another slice
// each, sharing the LDS pipe its pivot chain runs on: 200.9 k / 199.4 k -> 202.3 k updates/s in four slices, inside the noise.)
template <class S>
void launch_chol_gram(const Dev<S>& d, int b0, int nb, hipStream_t st, const routes::CompressRoute& r) {
  if (nb <= 0) return;
  if (r.chol_levels == 1) {
    dispatch_int<4, 8, 12>(r.nb_a, [&](auto NB) { hipLaunchKernelGGL((k_chol_mfma<double, S, NB(), 0, CH_GRAM, 1>), dim3(nb), dim3(1024), 0, st, d, b0, nb); });
  } else if (r.chol_levels == 2) {
    // two levels: columns [0, 192), L21, Schur complement
    hipLaunchKernelGGL((k_chol_mfma<double, S, 12, 0, CH_GRAM_A, 1>), dim3(nb), dim3(1024), 0, st, d, b0, nb);
    hipLaunchKernelGGL((k_trsm_rows<double, S, 12, TR_GRAM>), dim3(xcd_grid(nb, r.trsm_items)), dim3(256), 0, st, d, b0, nb, r.trsm_items);
    dispatch_int<4, 8, 12>(r.nb_b, [&](auto NB) { hipLaunchKernelGGL((k_chol_mfma<double, S, NB(), 0, CH_GRAM_B, 1>), dim3(nb), dim3(1024), 0, st, d, b0, nb); });
  }
}

// GAIN: routes::BLOCKED_GAIN states the four forms <NB, NA, NPART> and which window takes which
void launch_chol_gain(const Dev<float>& d, int b0, int nb, hipStream_t st, const routes::KalmanRoute& r) {
  if (nb <= 0) return;
  dispatch_int<0, 1, 2, 3>(r.blocked, [&](auto I) {
    constexpr routes::BlockedGain g = routes::BLOCKED_GAIN[I()];
    hipLaunchKernelGGL((k_chol_mfma<float, float, g.nb, g.na, CH_GAIN, g.npart>), dim3(xcd_grid(nb, g.npart)), dim3(1024), 0, st, d, b0, nb);
  });
}

#ifdef MSCKF_ABLATE
void chol_debug_set(int v) { (void)hipMemcpyToSymbol(HIP_SYMBOL(g_chol_dbg), &v, sizeof(int)); }
void chol_sub_read(unsigned long long* out32, int reset) {
  (void)hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_chol_sub), sizeof(unsigned long long) * 32);
  if (reset) { unsigned long long z[32] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_chol_sub), z, sizeof(z)); }
}
void chol_cycles_read(unsigned long long* out16, int reset) {
  (void)hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_chol_cycles), sizeof(unsigned long long) * 16);
  if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_chol_cycles), z, sizeof(z)); }
}
#endif

template void launch_chol_gram<float>(const Dev<float>&, int, int, hipStream_t, const routes::CompressRoute&);
template void launch_chol_gain_large<float>(const Dev<float>&, int, int, hipStream_t, const routes::KalmanRoute&);
template void launch_chol_gain_large<double>(const Dev<double>&, int, int, hipStream_t, const routes::KalmanRoute&);
template void launch_chol_gram<double>(const Dev<double>&, int, int, hipStream_t, const routes::CompressRoute&);

}  // namespace msckf
