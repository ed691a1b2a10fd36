// The Monte-Carlo replay's host side (msckf_mono_amd/csrc/replay_plan.h) on its own: no HIP header, a host compiler only.
//   replay_plan_host                 the integer part at literal values, a small plan with its bases and block sizes, every refusal
//   replay_plan_host mix             prints "mix <seed> <index> <value> <uniform>" for a table of seeds and indices (hex / hexfloat)
//   replay_plan_host plan <file>     reads cells "frame seq F M[F] slots[sum M]" (one per line, after a head line
//                                    "S frames K B f_cap m_cap n_cap" and a line "seq_of[B]"), prints per frame
//                                    "frame <f> <entries> <bytes f32> <bytes f64> base[B]" and "largest <entries>"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../msckf_mono_amd/csrc/replay_plan.h"

using namespace msckf_replay;
using msckf_inputs::SEC_OBS;
using msckf_inputs::SEC_SLOTS;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)
using VI = std::vector<int>;

// ---- the integer part: compile-time values (scenario.SplitMix64 printed them)
static_assert(mix(0, 0) == 0xe220a8397b1dcdafull, "value 0 of seed 0");
static_assert(mix(0xC0FFEE00ull, 0) == 0xab8231f0d3ccdbd9ull && mix(0xC0FFEE00ull, 5) == 0x4291475aff2b0638ull, "seed of the common shape");
static_assert(mix(0xFFFFFFFFFFFFFFFFull, 3) == 0x6d1db36ccba982d2ull, "seed + (i + 1) gamma wraps past 2^64");
static_assert(U(0, 0) == 0x1.c4415072f63b9p-1 && U(0xFFFFFFFFFFFFFFFFull, 3) == 0x1.b476cdb32ea60p-2, "the uniform of the upper 53 bits");
static_assert(imu_seed(7, 3) == mix(7, 6) && obs_seed(7, 3) == mix(7, 7), "frame sub-seeds");

static const uint64_t SEEDS[] = {0ull, 1ull, 0xC0FFEE00ull, 0xC0FFEE04ull, 0x5EED0000ull, 0x8000000000000000ull, 0xFFFFFFFFFFFFFFFFull, 0x61C8864680B583EBull /* = -gamma: seed + gamma wraps to 0 */};
static const uint64_t INDICES[] = {0ull, 1ull, 2ull, 31ull, 799ull, 0xFFFFFFFFull, 0x100000000ull, 0x3FFFFFFFFFFFFFFFull};

static int print_mix() {
  for (uint64_t s : SEEDS) for (uint64_t i : INDICES) std::printf("mix %" PRIx64 " %" PRIx64 " %" PRIx64 " %a\n", s, i, mix(s, i), U(s, i));
  return 0;
}

static bool is(const Refusal& r, int code, const char* why) {
  if (r.code != code) return false;
  if (!why) return r.why == nullptr;
  return r.why && std::strcmp(r.why, why) == 0;
}

// one cell of F tracks, each of m observations of the slots 0 .. m - 1
static void put(Plan& p, int f, int s, int F, int m, int k = 2, int flags = 0) {
  VI M(F, m), sl; std::vector<double> ob, rd((size_t)std::max(k, 1) * 7, 0.5);
  for (int t = 0; t < F; ++t) for (int j = 0; j < m; ++j) { sl.push_back(j); ob.push_back(0.01 * t); ob.push_back(-0.01 * j); }
  CHECK(is(p.cell_refusal(f, s, rd.data(), k, F, M.data(), sl.data(), 0, flags, 4, 4), 0, nullptr));
  p.set_cell(f, s, rd.data(), k, F, M.data(), sl.data(), ob.data(), 0, flags);
}

// ---- a small plan: S = 2, B = 5, f_cap = 3, m_cap = n_cap = 4, K = 2, 4 frames
//   frame 0: no entry anywhere        frame 1: sequence 0 has F == f_cap tracks of 4 (12 entries), sequence 1 none
//   frame 2: 0 -> 2 x 3 = 6, 1 -> 1 x 2 = 2        frame 3: sequence 1 skipped, 0 -> 1 x 4
static void small_plan() {
  Plan p;
  CHECK(is(Plan::alloc_refusal(0, 4, 2), -EINVAL, "bad replay size") && is(Plan::alloc_refusal(2, 0, 2), -EINVAL, "bad replay size") && is(Plan::alloc_refusal(2, 4, 0), -EINVAL, "bad replay size"));
  CHECK(is(Plan::alloc_refusal(2, 4, 2), 0, nullptr));
  // nothing allocated: every later step says so
  const int q0[5] = {1, 0, 1, 1, 0}; const uint64_t sd[5] = {1, 2, 3, 4, 5};
  std::vector<double> sg(20, 0.25);
  CHECK(is(p.commit_refusal(), -EINVAL, "no replay allocated") && is(p.assign_refusal(q0, sg.data()), -EINVAL, "no replay allocated"));
  CHECK(is(p.run_refusal(0, 0), -EINVAL, "replay not committed") && is(p.run_refusal(0, 1), -EINVAL, "frame range out of bounds"));
  p.alloc(2, 4, 2, 5, 3);
  CHECK(p.frames() == 4 && p.K() == 2 && p.S == 2 && p.B == 5);
  put(p, 1, 0, 3, 4); put(p, 2, 0, 2, 3); put(p, 2, 1, 1, 2); put(p, 3, 0, 1, 4); put(p, 3, 1, 0, 0, 0, msckf_lists::CELL_SKIP);
  // the order of a run's refusals: the range, the commit, the assignment
  CHECK(is(p.run_refusal(-1, 2), -EINVAL, "frame range out of bounds") && is(p.run_refusal(0, 5), -EINVAL, "frame range out of bounds") && is(p.run_refusal(3, 2), -EINVAL, "frame range out of bounds"));
  CHECK(is(p.run_refusal(0, 4), -EINVAL, "replay not committed"));
  CHECK(is(p.commit_refusal(), 0, nullptr) && is(p.commit(), 0, nullptr));
  CHECK(is(p.run_refusal(0, 4), -EINVAL, "replay not assigned") && is(p.expand_refusal(0, 0), -EINVAL, "replay not assigned"));
  // the assignment's rules: the sequence first, then sigma; a refused assignment leaves none behind
  { int bad[5] = {1, 0, 2, 1, 0}; CHECK(is(p.assign_refusal(bad, sg.data()), -EINVAL, "seq_of names no sequence of the replay")); bad[2] = -1; CHECK(is(p.assign_refusal(bad, sg.data()), -EINVAL, "seq_of names no sequence of the replay")); }
  for (double v : {-1e-300, -1.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
    std::vector<double> b2(sg); b2[19] = v;
    CHECK(is(p.assign_refusal(q0, b2.data()), -EINVAL, "sigma must be finite and not negative"));
    int bad[5] = {1, 0, 1, 1, 7};
    CHECK(is(p.assign_refusal(bad, b2.data()), -EINVAL, "seq_of names no sequence of the replay"));
  }
  { std::vector<double> z(20, 0.0); CHECK(is(p.assign_refusal(q0, z.data()), 0, nullptr)); }
  CHECK(!p.assigned && is(p.assign_refusal(q0, sg.data()), 0, nullptr));
  p.assign(q0, sd, sg.data());
  CHECK(is(p.run_refusal(0, 4), 0, nullptr) && is(p.run_refusal(2, 2), 0, nullptr));
  CHECK(is(p.expand_refusal(4, 0), -EINVAL, "replay cell out of range") && is(p.expand_refusal(0, 5), -EINVAL, "replay cell out of range") && is(p.expand_refusal(3, 4), 0, nullptr));
  // bases: seq_of = 1 0 1 1 0
  CHECK(is(p.index_trajectories(), 0, nullptr) && p.planned);
  const VI want = {0, 0, 0, 0, 0,   0, 0, 12, 12, 12,   0, 2, 8, 10, 12,   0, 0, 4, 4, 4};
  CHECK(p.base == want);
  CHECK((p.nf == std::vector<size_t>{0, 24, 18, 8}) && p.largest == 24);
  // the block is the ordinary one: FrameLayout(B, K, f_cap, esz) with the expanded frame's entries
  for (size_t esz : {sizeof(float), sizeof(double)}) {
    const FrameLayout L = p.out_layout(esz);
    CHECK(L.B == 5 && L.K == 2 && L.f_cap == 3 && L.esz == esz);
    CHECK(p.block_bytes(esz) == L.bytes(24) && L.bytes(24) == msckf_inputs::align_up(L.off_obs(24) + 48 * esz, 256));
    CHECK(L.off_obs(24) == msckf_inputs::align_up(L.at[SEC_SLOTS] + 96, 256) && L.block_at(SEC_OBS, 0) == L.at[SEC_SLOTS]);
  }
  // the sequence store: off counted from the frame's first sequence entry, a skipped cell's count, the host's per-cell values
  const int* off = p.seq.ints(msckf_inputs::SEC_OFF);
  CHECK(off[p.cell(2, 0) * 3] == 0 && off[p.cell(2, 0) * 3 + 1] == 3 && off[p.cell(2, 1) * 3] == 6 && off[p.cell(2, 1) * 3 + 1] == 8);
  CHECK(p.seq.ints(msckf_inputs::SEC_K)[p.cell(3, 1)] == msckf_inputs::NO_IMAGE && p.seq.ints(msckf_inputs::SEC_K)[p.cell(3, 0)] == 2);
  CHECK(p.cell_of(2, 0) == p.cell(2, 1) && p.cell_of(2, 1) == p.cell(2, 0) && p.seq.maxslot[p.cell_of(2, 1)] == 2 && p.seq.maxslot[p.cell_of(0, 0)] == -1);
  // a new assignment moves the bases; a patched cell un-commits
  const int q1[5] = {0, 0, 0, 0, 0};
  p.assign(q1, sd, sg.data());
  CHECK(!p.planned && is(p.index_trajectories(), 0, nullptr) && p.base[5 + 4] == 48 && p.largest == 60 && p.nf[0] == 0);
  put(p, 0, 1, 1, 2);
  CHECK(!p.committed && !p.planned && is(p.run_refusal(0, 4), -EINVAL, "replay not committed"));
  CHECK(is(p.commit(), 0, nullptr) && is(p.run_refusal(0, 4), 0, nullptr));
}

// ---- a cell's rules, in scenario_set_cell's order: place, work-list (worklist_refusal), drop, cell rule, readings
static void cell_rules() {
  Plan p;
  p.alloc(2, 3, 4, 5, 3);
  const int M[3] = {2, 2, 2}, sl[6] = {0, 1, 1, 2, 2, 3}; const double rd[28] = {0};
  auto R = [&](int f, int s, const double* r, int k, int F, const int* Mp, const int* sp, int nd, int fl) { return p.cell_refusal(f, s, r, k, F, Mp, sp, nd, fl, 4, 4); };
  CHECK(is(R(0, 0, rd, 4, 3, M, sl, 1, 0), 0, nullptr));
  CHECK(is(R(3, 0, rd, 4, 3, M, sl, 1, 0), -EINVAL, "replay cell out of range") && is(R(0, 2, rd, 4, 3, M, sl, 1, 0), -EINVAL, "replay cell out of range") && is(R(-1, 0, rd, 4, 3, M, sl, 1, 0), -EINVAL, "replay cell out of range"));
  CHECK(is(R(3, 0, rd, 4, 4, M, sl, 1, 0), -EINVAL, "replay cell out of range"));                 // the place before the work-list
  CHECK(is(R(0, 0, rd, 4, 4, M, sl, -1, 0), -E2BIG, "more tracks than f_cap"));                    // the work-list before the drop
  { const int Ml[3] = {2, 5, 2}; CHECK(is(R(0, 0, rd, 4, 3, Ml, sl, 1, 0), -E2BIG, "track longer than m_cap")); }
  { const int so[6] = {0, 1, 1, 4, 2, 3}; CHECK(is(R(0, 0, rd, 4, 3, M, so, 1, 0), -EINVAL, "camera slot out of range")); }
  { const int sr[6] = {0, 1, 2, 2, 2, 3}; CHECK(is(R(0, 0, rd, 4, 3, M, sr, 1, 0), -EINVAL, "camera slot repeated within a track")); }
  CHECK(is(R(0, 0, rd, 5, 3, M, sl, -1, 0), -EINVAL, "negative n_drop"));                         // the drop before the cell rule
  CHECK(is(R(0, 0, rd, 5, 3, M, sl, 0, 0), -EINVAL, "IMU sample count k exceeds the scenario's K (msckf_hip_scenario_alloc)"));
  CHECK(is(R(0, 0, rd, -1, 3, M, sl, 0, 0), -EINVAL, "negative IMU sample count k") && is(R(0, 0, rd, 4, 3, M, sl, 0, 2), -EINVAL, "unknown cell flag bit"));
  CHECK(is(R(0, 0, rd, 0, 3, M, sl, 0, msckf_lists::CELL_SKIP), -EINVAL, "a skipped cell carries no IMU samples, no tracks and no drop"));
  CHECK(is(R(0, 0, nullptr, 1, 3, M, sl, 0, 0), -EINVAL, "null readings for a cell with samples") && is(R(0, 0, nullptr, 0, 3, M, sl, 0, 0), 0, nullptr));
  CHECK(is(R(0, 1, nullptr, 0, 0, nullptr, nullptr, 0, msckf_lists::CELL_SKIP), 0, nullptr));
}

static int print_plan(const char* path) {
  std::FILE* fp = std::fopen(path, "r");
  if (!fp) { std::printf("cannot open %s\n", path); return 2; }
  int S, frames, K, B, f_cap, m_cap, n_cap;
  if (std::fscanf(fp, "%d %d %d %d %d %d %d", &S, &frames, &K, &B, &f_cap, &m_cap, &n_cap) != 7) return 2;
  VI seq_of(B);
  for (int& v : seq_of) if (std::fscanf(fp, "%d", &v) != 1) return 2;
  Plan p;
  p.alloc(S, frames, K, B, f_cap);
  int f, s, F;
  while (std::fscanf(fp, "%d %d %d", &f, &s, &F) == 3) {
    VI M(F), sl; size_t tot = 0;
    for (int& v : M) { if (std::fscanf(fp, "%d", &v) != 1) return 2; tot += v; }
    sl.resize(tot);
    for (int& v : sl) if (std::fscanf(fp, "%d", &v) != 1) return 2;
    std::vector<double> rd((size_t)K * 7, 0.0), ob(2 * tot, 0.0);
    const Refusal r = p.cell_refusal(f, s, rd.data(), K, F, M.data(), sl.data(), 0, 0, m_cap, n_cap);
    if (r.code) { std::printf("cell %d %d refused: %s\n", f, s, r.why); return 2; }
    p.set_cell(f, s, rd.data(), K, F, M.data(), sl.data(), ob.data(), 0, 0);
  }
  std::fclose(fp);
  std::vector<uint64_t> seed(B, 1); std::vector<double> sg((size_t)B * N_SIGMA, 0.0);
  if (p.commit().code || p.assign_refusal(seq_of.data(), sg.data()).code) return 2;
  p.assign(seq_of.data(), seed.data(), sg.data());
  if (p.index_trajectories().code) return 2;
  for (f = 0; f < frames; ++f) {
    std::printf("frame %d %zu %zu %zu", f, p.nf[f], p.out_layout(4).bytes(p.nf[f]), p.out_layout(8).bytes(p.nf[f]));
    for (int b = 0; b < B; ++b) std::printf(" %d", p.base[(size_t)f * B + b]);
    std::printf("\n");
  }
  std::printf("largest %zu %zu %zu\n", p.largest, p.block_bytes(4), p.block_bytes(8));
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "mix") == 0) return print_mix();
  if (argc >= 3 && std::strcmp(argv[1], "plan") == 0) return print_plan(argv[2]);
  // run-time values of the integer part, against the compile-time ones and the wrap
  volatile uint64_t s0 = 0xC0FFEE00ull;
  CHECK(mix(s0, 5) == 0x4291475aff2b0638ull && U(s0, 0) == 0x1.570463e1a799bp-1 && U(s0, 5) == 0x1.0a451d6bfcac0p-2);
  CHECK(mix(0x61C8864680B583EBull, 0) == 0 && U(0x61C8864680B583EBull, 0) == 0.0);   // seed + gamma == 2^64: the finalizer of 0
  for (uint64_t s : SEEDS) for (uint64_t i : INDICES) CHECK(U(s, i) >= 0.0 && U(s, i) < 1.0);
  small_plan();
  cell_rules();
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("replay plan ok\n");
  return 0;
}
