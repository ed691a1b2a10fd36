// The host side of the Monte-Carlo replay's fault model (msckf_mono_amd/csrc/replay_plan.h, FAULTS) on its own: no HIP header, a
// host compiler only.
//   replay_faults_host                   every refusal of set_faults with its code, text and order; a refused call leaves the
//                                        previous record in force; the record stays through both assigns and a commit and alloc
//                                        clears it; fault_seed at three literal values; the rule on a track (track_faults); the
//                                        lane group of a window size
//   replay_faults_host seed S F ...      prints "seed <S> <F> <fault_seed(S, F)>" (hex) for every pair (S, F) given
//   replay_faults_host track S F E0 M PM PO   prints "track <missed> <outliers>" of one track by track_faults
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../msckf_mono_amd/csrc/replay_plan.h"

using namespace msckf_replay;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

static bool is(const Refusal& r, int code, const char* why) {
  if (r.code != code) return false;
  if (!why) return r.why == nullptr;
  return r.why && std::strcmp(r.why, why) == 0;
}

// the three values tests/test_replay_faults_plan.py also takes from the twin (scenario.replay_fault_seed)
static_assert(fault_seed(0x0ull, 0) == 0xb39eedfc2740d498ull, "fault_seed(0, 0)");
static_assert(fault_seed(0xC0FFEE00ull, 7) == 0xf41882913a46030bull, "fault_seed(0xC0FFEE00, 7)");
static_assert(fault_seed(0xFFFFFFFFFFFFFFFFull, 199) == 0xdbf3bb1f8a55d8dbull, "fault_seed(2^64 - 1, 199)");
static_assert(FAULT_STREAM == (1ull << 63) + 1, "the fault stream's index");
static_assert(fault_group(1) == 16 && fault_group(16) == 16 && fault_group(17) == 32 && fault_group(32) == 32 && fault_group(33) == 64 && fault_group(64) == 64, "lane groups");

static const char* NO_REPLAY = "no replay allocated";
static const char* BAD_P = "fault probabilities must lie in [0, 1]";
static const char* BAD_RHO = "fault radii must be finite and not negative";

static void check_plan() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  constexpr int B = 3, K = 4, F_CAP = 2;
  const std::vector<double> good = {0.15, 0.10, 0.01, 0.02, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 5.0};
  const std::vector<double> zeros((size_t)B * N_FAULT, 0.0);
  Plan p;
  // nothing allocated: refused before anything is looked at, with and without a record
  CHECK(is(p.faults_refusal(good.data()), -EINVAL, NO_REPLAY));
  CHECK(is(p.faults_refusal(nullptr), -EINVAL, NO_REPLAY));
  p.alloc(2, 3, K, B, F_CAP);
  CHECK(p.fault.empty() && !p.faulted && !p.faults_uploaded);
  CHECK(is(p.faults_refusal(nullptr), 0, nullptr));
  CHECK(is(p.faults_refusal(good.data()), 0, nullptr));
  CHECK(is(p.faults_refusal(zeros.data()), 0, nullptr));
  // the probabilities, every place and every kind of bad value
  for (int b = 0; b < B; ++b) for (int c : {FLT_P_MISS, FLT_P_OUT}) for (double bad : {-1e-9, 1.0 + 1e-9, inf, -inf, nan}) {
    std::vector<double> v = good;
    v[(size_t)b * N_FAULT + c] = bad;
    CHECK(is(p.faults_refusal(v.data()), -EINVAL, BAD_P));
  }
  // the radii
  for (int b = 0; b < B; ++b) for (int c : {FLT_RHO_U, FLT_RHO_V}) for (double bad : {-1e-9, inf, -inf, nan}) {
    std::vector<double> v = good;
    v[(size_t)b * N_FAULT + c] = bad;
    CHECK(is(p.faults_refusal(v.data()), -EINVAL, BAD_RHO));
  }
  // the order: a bad probability of the last trajectory is named before a bad radius of the first
  {
    std::vector<double> v = good;
    v[FLT_RHO_U] = -1.0; v[(size_t)(B - 1) * N_FAULT + FLT_P_OUT] = 2.0;
    CHECK(is(p.faults_refusal(v.data()), -EINVAL, BAD_P));
  }
  // a radius above 1 and a probability of exactly 0 or 1 are fine
  {
    std::vector<double> v = good;
    v[FLT_RHO_V] = 1e3; v[FLT_P_MISS] = 1.0; v[FLT_P_OUT] = 0.0;
    CHECK(is(p.faults_refusal(v.data()), 0, nullptr));
  }
  // set, and what a refused call leaves behind (the caller asks faults_refusal first and does not call set_faults)
  p.set_faults(good.data());
  CHECK(p.fault == good && p.faulted && !p.faults_uploaded);
  p.faults_uploaded = true;                          // the caller has uploaded it
  {
    std::vector<double> v = good;
    v[FLT_P_MISS] = 1.5;
    if (p.faults_refusal(v.data()).code == 0) p.set_faults(v.data());
    CHECK(p.fault == good && p.faulted && p.faults_uploaded);
  }
  // the record stays through both assigns and a commit, and they leave the device copy's validity alone
  const int seq_of[B] = {1, 0, 1};
  const uint64_t seed[B] = {1, 2, 3};
  const std::vector<double> sigma((size_t)B * N_SIGMA, 0.01);
  p.assign(seq_of, seed, sigma.data());
  CHECK(p.fault == good && p.faulted && p.faults_uploaded);
  std::vector<double> Q((size_t)B * L_SIZE, 0.0);
  for (int b = 0; b < B; ++b) for (int i = 0; i < NQ; ++i) Q[(size_t)b * L_SIZE + i * NQ + i] = 1e-4;
  const double scale[B] = {1.0, 0.5, 0.0}, uv[2 * B] = {1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3};
  CHECK(is(p.assign_q_refusal(seq_of, Q.data(), scale, uv), 0, nullptr));
  p.assign_q(seq_of, seed, Q.data(), scale, uv);
  CHECK(p.fault == good && p.faulted && p.faults_uploaded && p.model == MODEL_Q);
  const int M[2] = {2, 3}, slots[5] = {0, 1, 0, 1, 2};
  const double obs[10] = {0}, rd[K * 7] = {0};
  CHECK(is(p.cell_refusal(1, 0, rd, K, 2, M, slots, 0, 0, 3, 3), 0, nullptr));
  p.set_cell(1, 0, rd, K, 2, M, slots, obs, 0, 0);
  CHECK(is(p.commit(), 0, nullptr));
  CHECK(p.fault == good && p.faulted && p.faults_uploaded && p.committed);
  p.assign(seq_of, seed, sigma.data());
  CHECK(p.fault == good && p.faulted && p.model == MODEL_SIGMA4);
  // all zeros: a record, but nothing is faulted; null: no record; both invalidate the device copy only
  p.set_faults(zeros.data());
  CHECK(p.fault == zeros && !p.faulted && !p.faults_uploaded && p.committed && p.assigned);
  p.set_faults(good.data());
  p.faults_uploaded = true;
  p.set_faults(nullptr);
  CHECK(p.fault.empty() && !p.faulted && !p.faults_uploaded && p.committed && p.assigned);
  // radii alone fault nothing; one probability of one trajectory does
  {
    std::vector<double> v = zeros;
    v[FLT_RHO_U] = 0.1;
    p.set_faults(v.data());
    CHECK(!p.faulted);
    v[(size_t)(B - 1) * N_FAULT + FLT_P_OUT] = 1e-9;
    p.set_faults(v.data());
    CHECK(p.faulted);
  }
  // alloc clears it
  p.alloc(2, 3, K, B, F_CAP);
  CHECK(p.fault.empty() && !p.faulted && !p.faults_uploaded);
}

// the rule on a track, against the definition written out with U alone
static void check_tracks() {
  const uint64_t s = fault_seed(0xC0FFEE00ull, 7);
  int shielded = 0, shortened = 0;
  for (int M = 0; M <= 9; ++M) for (uint64_t e0 : {0ull, 5ull, 1000ull}) for (double pm : {0.0, 0.3, 0.9, 1.0}) for (double po : {0.0, 0.5, 1.0}) {
    int raw = 0;
    for (int l = 0; l < M; ++l) raw += U(s, 3 * (e0 + l)) < pm;
    const bool none = M - raw < 2;
    int out = 0;
    for (int l = 0; l < M; ++l) { const bool miss = !none && U(s, 3 * (e0 + l)) < pm; out += !miss && U(s, 3 * (e0 + l) + 1) < po; }
    const TrackFaults t = track_faults(s, e0, M, pm, po);
    CHECK(t.missed == (none ? 0 : raw) && t.outliers == out);
    CHECK(M - t.missed >= (M < 2 ? M : 2));
    if (pm == 1.0) CHECK(t.missed == 0);           // every entry raw-missed: the track loses none
    if (po == 1.0) CHECK(t.outliers == M - t.missed);
    if (pm == 0.0) CHECK(t.missed == 0);
    shielded += none && raw > 0; shortened += t.missed > 0;
  }
  CHECK(shielded > 0 && shortened > 0);
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "seed") == 0) {
    for (int i = 2; i + 1 < argc; i += 2) {
      const uint64_t s = std::strtoull(argv[i], nullptr, 16);
      const int f = std::atoi(argv[i + 1]);
      std::printf("seed %llx %d %llx\n", (unsigned long long)s, f, (unsigned long long)fault_seed(s, f));
    }
    return 0;
  }
  if (argc == 8 && std::strcmp(argv[1], "track") == 0) {
    const TrackFaults t = track_faults(fault_seed(std::strtoull(argv[2], nullptr, 16), std::atoi(argv[3])), std::strtoull(argv[4], nullptr, 10), std::atoi(argv[5]),
                                       std::strtod(argv[6], nullptr), std::strtod(argv[7], nullptr));
    std::printf("track %d %d\n", t.missed, t.outliers);
    return 0;
  }
  check_plan();
  check_tracks();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("replay faults ok\n");
  return 0;
}
