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

template <class S>
__global__ __launch_bounds__(REPLAY_CHUNK) void k_replay_expand(ReplaySeqIn q, ReplayTrajIn t, ReplayOut<S> o, int f, int b0, int K, int f_cap) {
  const int b = b0 + (int)blockIdx.y;
  const int s = t.seq_of[b];
  const uint64_t seed = t.seed[b];
  const double* sg = t.sigma + (long)b * rp::N_SIGMA;
  const int* Ms = q.M + (long)s * f_cap;
  const int* offs = q.off + (long)s * f_cap;
  const int first = offs[0];                                           // the sequence cell's first entry among the frame's sequence entries
  const int E = offs[f_cap - 1] + Ms[f_cap - 1] - first;
  const int base = t.base[b];                                          // the trajectory's first entry in the expanded block
  const int kc = q.k[s];
  const int imu0 = E, dt0 = E + rp::IMU_PAIRS * K, m0 = dt0 + K, last = m0 + f_cap;
  for (int it = (int)blockIdx.x * REPLAY_CHUNK + (int)threadIdx.x; it <= last; it += (int)gridDim.x * REPLAY_CHUNK) {
    if (it < imu0) {
      const Pair g = box_muller(rp::obs_seed(seed, f), (uint64_t)it);
      const double* z = q.obs + 2 * (long)(first + it);
      o.slots[(long)base + it] = q.slots[(long)first + it];
      Vec2<S> w;
      w.x = (S)noisy(z[0], sg[rp::SIG_U], g.c); w.y = (S)noisy(z[1], sg[rp::SIG_V], g.s);
      *reinterpret_cast<Vec2<S>*>(o.obs + 2 * ((long)base + it)) = w;
    } else if (it < dt0) {
      const int j = it - imu0, i = j / rp::IMU_PAIRS, c = 2 * (j % rp::IMU_PAIRS);
      const double* r = q.rd + ((long)s * K + i) * RD_STRIDE;
      S* w = o.rd + ((long)b * K + i) * RD_STRIDE;
      double v0 = r[c], v1 = r[c + 1];
      if (i < kc) {                                                    // (a skipped cell's k is IMU_SKIP: no noise; rows from k on stay zero)
        const Pair g = box_muller(rp::imu_seed(seed, f), (uint64_t)j);
        v0 = noisy(v0, sg[c < 3 ? rp::SIG_G : rp::SIG_A], g.c); v1 = noisy(v1, sg[c + 1 < 3 ? rp::SIG_G : rp::SIG_A], g.s);
      }
      w[c] = (S)v0; w[c + 1] = (S)v1;
    } else if (it < m0) {
      const int i = it - dt0;
      o.rd[((long)b * K + i) * RD_STRIDE + 6] = (S)q.rd[((long)s * K + i) * RD_STRIDE + 6];
    } else if (it < last) {
      const int tr = it - m0;
      o.M[(long)b * f_cap + tr] = Ms[tr];
      o.off[(long)b * f_cap + tr] = offs[tr] - first + base;
    } else {
      o.n[b] = q.n[s]; o.drop[b] = q.drop[s]; o.k[b] = kc;
    }
  }
}

// max_entries: the entries of the frame's largest sequence cell (the grid's width; a trajectory with fewer leaves its lanes idle)
template <class S>
void launch_replay_expand(const ReplaySeqIn& q, const ReplayTrajIn& t, const ReplayOut<S>& o, int f, int b0, int nb, int K, int f_cap, int max_entries, hipStream_t st) {
  if (nb <= 0) return;
  const long items = (long)max_entries + (long)(rp::IMU_PAIRS + 1) * K + f_cap + 1;
  const dim3 grid((unsigned)((items + REPLAY_CHUNK - 1) / REPLAY_CHUNK), (unsigned)nb);
  hipLaunchKernelGGL(k_replay_expand<S>, grid, dim3(REPLAY_CHUNK), 0, st, q, t, o, f, b0, K, f_cap);
}
template void launch_replay_expand<float>(const ReplaySeqIn&, const ReplayTrajIn&, const ReplayOut<float>&, int, int, int, int, int, int, hipStream_t);
template void launch_replay_expand<double>(const ReplaySeqIn&, const ReplayTrajIn&, const ReplayOut<double>&, int, int, int, int, int, int, hipStream_t);

}  // namespace msckf
