// select_diag.h -- the track selection and the block-diagonal sums of the information form as workgroup bodies: k_select and
// k_select_diag (kernels_feature.hip) and k_propagate's HEAD instance (kernels_state.hip) run them.
#ifndef MSCKF_SELECT_DIAG_H
#define MSCKF_SELECT_DIAG_H

#include "dev_common.h"

namespace msckf {

// (update_ncam, the window size as the launches of an update see it: dev_common.h)

// One wavefront per trajectory: resolves the order-dependent part of marginalize (:352-399) -- checkMotion is
// skipped while fewer than 4 tracks have ever been residualized (Q4, msckf.h:354) -- and lays the gated-in
// tracks' rows out for the compression stage: tracks are counting-sorted by their first camera slot (stable,
// deterministic), so that consecutive row blocks of the TSQR share their leading zero columns and can start
// their elimination late.  order[p] = track id of sorted position p, row_start[p] = first stacked row.
// Once more than 3 tracks have been residualized the decisions are independent per track and run
// lane-parallel; the first few frames of a run take the serial path.
template <class S>
__device__ __forceinline__ void select_body(const Dev<S>& d, const int b0, const int nb, const int i, const int lane) {
  if (i >= nb) return;
  const int b = b0 + i;
  const int F = d.trk_n[(long)i * d.wl_stride_n];
  long long nres = d.n_resid[b];
  int* st = d.stats + (long)b * STAT_STRIDE;
  int mrej = 0, trej = 0, grej = 0, pass = 0;
  int* rs = d.row_start + (long)b * (d.f_cap + 1);
  int* order = d.trk_order + (long)b * d.f_cap;
  __shared__ int sCnt[64], sBase[64], sRows[64];
  sCnt[lane] = 0; sRows[lane] = 0;
  __syncthreads();
  // ---- fast path (steady state, F <= 256): every per-track word is loaded ONCE, four tracks per lane, all loads in
  // flight together; decisions, stable counting sort by first camera slot and the row prefix then run from registers
  // and LDS.  (The generic path below re-reads per pass: ~12 dependent global round trips for a 64-thread kernel.)
  if (!(nres <= 3 && d.mode == 0) && F <= 256) {
    __shared__ short sMrow[256];
    __shared__ short sOrd[256];
    int sv[4], Mv[4], fv[4];
    bool inc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int t = 64 * c + lane, tc = min(t, max(F - 1, 0));
      const long tb = (long)b * d.f_cap + tc;
      sv[c] = d.trk_status[tb]; Mv[c] = d.trk_M[(long)i * d.wl_stride_f + tc]; fv[c] = d.trk_first[tb] & 63;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int t = 64 * c + lane;
      const bool in = t < F;
      int sx = in ? sv[c] : 0;
      const int M = in ? Mv[c] : 0;
      bool m_rej = false, t_rej = false, g_rej = false, valid = false, incl = false;
      if (in) {
        if (M < 2 || !(sx & ST_MOTION_OK)) { m_rej = true; sx = (M < 2) ? 0 : (sx & ~(ST_TRI_VALID | ST_GATE_PASS)); }
        else if (sx & ST_TRI_VALID) valid = true;
        else { t_rej = true; sx &= ~ST_GATE_PASS; }
        if (valid) { if (sx & ST_GATE_PASS) { incl = true; sx |= ST_INCLUDED; } else g_rej = true; }
        d.trk_status[(long)b * d.f_cap + t] = sx;
        sMrow[t] = (short)(2 * M - 3);
      }
      inc[c] = incl;
      if (incl) { atomicAdd(&sCnt[fv[c]], 1); atomicAdd(&sRows[fv[c]], 2 * M - 3); }
      mrej += __popcll(__ballot(m_rej)); trej += __popcll(__ballot(t_rej)); grej += __popcll(__ballot(g_rej));
      pass += __popcll(__ballot(incl)); if (d.mode == 0) nres += __popcll(__ballot(valid));
    }
    __syncthreads();
    {
      const int c0 = sCnt[lane];
      int scan = c0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(scan, o, 64); if (lane >= o) scan += up; }
      sBase[lane] = scan - c0;
    }
    __syncthreads();
    const int nbin = min(d.n_cap, 64);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int bin = inc[c] ? fv[c] : -1;
      int rank = 0, cnt = 0;
      for (int sbin = 0; sbin < nbin; ++sbin) {
        const unsigned long long m = __ballot(bin == sbin);
        if (bin == sbin) { rank = __popcll(m & ((1ull << lane) - 1ull)); cnt = __popcll(m); }
      }
      int pos = 0;
      if (inc[c]) { pos = sBase[bin] + rank; sOrd[pos] = (short)(64 * c + lane); order[pos] = 64 * c + lane; }
      __syncthreads();
      if (inc[c] && rank == 0) sBase[bin] += cnt;     // one writer per bin
      __syncthreads();
    }
    int rows = 0;
    for (int p0 = 0; p0 < pass; p0 += 64) {
      const int p = p0 + lane;
      const int r = p < pass ? (int)sMrow[sOrd[p]] : 0;
      int scan = r;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(scan, o, 64); if (lane >= o) scan += up; }
      if (p < pass) rs[p] = rows + scan - r;
      rows += __shfl(scan, 63, 64);
    }
    if (lane == 0) {
      rs[pass] = rows;
      d.n_resid[b] = nres;
      st[STAT_NTRACKS] = F; st[STAT_MOTION_REJ] = mrej; st[STAT_TRI_REJ] = trej; st[STAT_GATE_REJ] = grej;
      st[STAT_PASSED] = pass; st[STAT_MROWS] = rows; st[STAT_RROWS] = rows > 0 ? 6 * update_ncam(d, b) : 0;
    }
    return;
  }
  // ---- pass 1: decisions (status bits), per-bin counts
  if (nres <= 3 && d.mode == 0) {
    if (lane == 0) {
      for (int t = 0; t < F; ++t) {
        const long tb = (long)b * d.f_cap + t;
        int s = d.trk_status[tb];
        const int M = d.trk_M[(long)i * d.wl_stride_f + t];
        bool valid = false;
        if (M < 2) { if (nres > 3) mrej++; else trej++; s = 0; }
        else if (nres > 3 && !(s & ST_MOTION_OK)) { mrej++; s &= ~(ST_TRI_VALID | ST_GATE_PASS); }
        else {
          if (nres <= 3) s |= ST_MOTION_SKIPPED;
          if (s & ST_TRI_VALID) { valid = true; nres++; } else { trej++; s &= ~ST_GATE_PASS; }
        }
        if (valid) {
          if (s & ST_GATE_PASS) { s |= ST_INCLUDED; pass++; const int f0 = d.trk_first[tb] & 63; sCnt[f0]++; sRows[f0] += 2 * M - 3; }
          else grej++;
        }
        d.trk_status[tb] = s;
      }
    }
    mrej = __shfl(mrej, 0, 64); trej = __shfl(trej, 0, 64); grej = __shfl(grej, 0, 64); pass = __shfl(pass, 0, 64);
    nres = __shfl((int)nres, 0, 64);
  } else {
    for (int t0 = 0; t0 < F; t0 += 64) {
      const int t = t0 + lane;
      const bool in = t < F;
      const long tb = (long)b * d.f_cap + t;
      int s = in ? d.trk_status[tb] : 0;
      const int M = in ? d.trk_M[(long)i * d.wl_stride_f + t] : 0;
      bool m_rej = false, t_rej = false, g_rej = false, valid = false, incl = false;
      if (in) {
        if (M < 2 || !(s & ST_MOTION_OK)) { m_rej = true; s = (M < 2) ? 0 : (s & ~(ST_TRI_VALID | ST_GATE_PASS)); }
        else if (s & ST_TRI_VALID) valid = true;
        else { t_rej = true; s &= ~ST_GATE_PASS; }
        if (valid) { if (s & ST_GATE_PASS) { incl = true; s |= ST_INCLUDED; } else g_rej = true; }
        d.trk_status[tb] = s;
      }
      if (incl) { const int f0 = d.trk_first[tb] & 63; atomicAdd(&sCnt[f0], 1); atomicAdd(&sRows[f0], 2 * M - 3); }
      mrej += __popcll(__ballot(m_rej)); trej += __popcll(__ballot(t_rej)); grej += __popcll(__ballot(g_rej));
      pass += __popcll(__ballot(incl)); if (d.mode == 0) nres += __popcll(__ballot(valid));
    }
  }
  __syncthreads();
  // ---- exclusive prefix of the per-bin track counts (bins = first camera slot, ascending)
  {
    const int c = sCnt[lane];
    int scan = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(scan, o, 64); if (lane >= o) scan += up; }
    sBase[lane] = scan - c;
  }
  __syncthreads();
  // ---- pass 2: stable placement (track index order inside a bin), then row prefix over sorted positions
  for (int t0 = 0; t0 < F; t0 += 64) {
    const int t = t0 + lane;
    const long tb = (long)b * d.f_cap + t;
    const bool incl = (t < F) && (d.trk_status[tb] & ST_INCLUDED);
    const int bin = incl ? (d.trk_first[tb] & 63) : -1;
    int pos = -1;
    for (int sbin = 0; sbin < d.n_cap && sbin < 64; ++sbin) {
      const unsigned long long m = __ballot(bin == sbin);
      if (bin == sbin) pos = sBase[sbin] + __popcll(m & ((1ull << lane) - 1ull));
      __syncthreads();
      if (lane == 0) sBase[sbin] += __popcll(m);
      __syncthreads();
    }
    if (incl) order[pos] = t;
  }
  __syncthreads();
  int rows = 0;
  for (int p0 = 0; p0 < pass; p0 += 64) {
    const int p = p0 + lane;
    int r = 0;
    if (p < pass) { const int t = order[p]; r = 2 * d.trk_M[(long)i * d.wl_stride_f + t] - 3; }
    int scan = r;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(scan, o, 64); if (lane >= o) scan += up; }
    if (p < pass) rs[p] = rows + scan - r;
    rows += __shfl(scan, 63, 64);
  }
  if (lane == 0) {
    rs[pass] = rows;
    d.n_resid[b] = nres;
    st[STAT_NTRACKS] = F; st[STAT_MOTION_REJ] = mrej; st[STAT_TRI_REJ] = trej; st[STAT_GATE_REJ] = grej;
    st[STAT_PASSED] = pass; st[STAT_MROWS] = rows; st[STAT_RROWS] = rows > 0 ? 6 * update_ncam(d, b) : 0;
  }
}

// k_select and the block-diagonal part of Lam^ (sum h^T h per camera slot, sum h^T r; information-form route) in ONE launch:
// both only read what k_feature left behind, both are latency-bound (one wavefront per trajectory: 11 us; one per camera
// slot: 16 us), and as two launches they ran one after the other.  Workgroup ndiag of a trajectory is k_select (its first
// wavefront); workgroups 0 .. ndiag - 1 reduce four camera slots each, one wavefront per slot, lanes over ALL tracks of the
// update with the inclusion decision re-derived from the raw status bits (k_select's rule, msckf.h:352-399):
//   steady state: M >= 2, motion ok, triangulation valid, gate passed;
//   while fewer than 4 tracks have ever been residualized (Q4, msckf.h:354) the motion check is skipped up to and including
//   the track that brings the count to 4 -- found by scanning the tracks in order from the count k_feature recorded at the
//   start of the update (nres_upd: n_resid itself is being updated by the k_select workgroup of this very launch).
// Two dependent load levels (status | slot map -> Jacobian block) instead of three (sorted order -> slot map -> block).
// Measured and rejected (round 3): the two load levels batched over four rounds of 64 tracks (clamped addresses, masked
// afterwards, no `continue`): 16.5 -> 22.0 us -- 190 registers, and the Jacobian blocks of the ~45 % of (track, slot) pairs
// that do not exist are fetched too.
// Also rejected: one workgroup per slot with its four wavefronts splitting the rounds (16.5 -> 23.0 us: the 27 f64 butterfly
// reductions, ~1 600 instructions per wavefront, are then done four times over), and the 27 sums through an LDS transpose
// instead of butterflies (~160 instructions, but 58 KB of LDS per workgroup: 18.6 us, and the changed summation order moves
// the float TSQR-vs-information-form comparison at the 60-camera geometry past its tolerance).
// The launch's workgroup (x, i): x < ndiag the camera slots 4 x .. 4 x + 3 of its i-th trajectory, x == ndiag its selection.
template <class S>
__device__ __forceinline__ void select_diag_body(const Dev<S>& d, const int b0, const int nb, const int ndiag, const int x, const int i) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (x == ndiag) { if (tid < 64) select_body<S>(d, b0, nb, i, tid); return; }
  const int b = b0 + i;
  const int N = update_ncam(d, b), F = d.trk_n[(long)i * d.wl_stride_n];
  const int s = 4 * x + w;
  if (s >= N) return;
  const int f_cap = d.f_cap, m_cap = d.m_cap;
  const int* stt = d.trk_status + (long)b * f_cap;
  const int* Mv = d.trk_M + (long)i * d.wl_stride_f;
  constexpr int ALL = ST_MOTION_OK | ST_TRI_VALID | ST_GATE_PASS;
  int tcut = 0;                                      // tracks below tcut skip the motion check (Q4)
  if (d.mode == 0 && F > 0) {
    int need = 4 - d.nres_upd[b];                    // valid tracks still to come before the motion check applies
    if (need > 0) {
      tcut = F;
      for (int t0 = 0; t0 < F && need > 0; t0 += 64) {
        const int t = t0 + lane;
        const bool v = t < F && Mv[t] >= 2 && (stt[t] & ST_TRI_VALID);
        unsigned long long m = __ballot(v);
        const int c = __popcll(m);
        if (c < need) { need -= c; continue; }
        int pos = 0;
        for (int k = 0; k < need; ++k) { pos = __builtin_ctzll(m); m &= m - 1; }
        tcut = t0 + pos + 1; need = 0;
      }
    }
  }
  double acc[27];
#pragma unroll
  for (int e = 0; e < 27; ++e) acc[e] = 0.0;
  for (int t = lane; t < F; t += 64) {
    const long tb = (long)b * f_cap + t;
    const int sx = stt[t], M = Mv[t];
    const int oi = d.trk_inv[tb * d.n_cap + s];      // issued with the status loads; meaningful only for residualized tracks
    const int need_bits = t < tcut ? (ST_TRI_VALID | ST_GATE_PASS) : ALL;
    if (M < 2 || (sx & need_bits) != need_bits || oi < 0) continue;
    const long h0i = (tb * m_cap + oi) * 12;
    const S* rw = d.trk_rw + tb * 2 * m_cap + 2 * oi;
    double h0[6], h1[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { h0[k] = (double)ld_hx(d, h0i + k); h1[k] = (double)ld_hx(d, h0i + 6 + k); }
    const double r0 = (double)rw[0], r1 = (double)rw[1];
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) acc[e++] += h0[a] * h0[c] + h1[a] * h1[c];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] += h0[a] * r0 + h1[a] * r1;
  }
  double* out = d.Dg + ((long)b * d.n_cap + s) * DG_STRIDE;
#pragma unroll
  for (int e = 0; e < 27; ++e) {
    const double v = wave_sum(acc[e]);
    if (lane == 0) out[e] = v;
  }
}

template <class S>
__global__ __launch_bounds__(256) void k_select_diag(Dev<S> d, int b0, int nb, int ndiag) {
  select_diag_body<S>(d, b0, nb, ndiag, (int)blockIdx.x, (int)blockIdx.y);
}

}  // namespace msckf
#endif
