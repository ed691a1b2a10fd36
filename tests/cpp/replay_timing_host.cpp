// The host side of the Monte-Carlo replay's timing model (msckf_mono_amd/csrc/replay_plan.h, TIMING) on its own: no HIP header,
// a host compiler only.
//   replay_timing_host                   every refusal of set_timing with its code, text and order; a refused call leaves the
//                                        previous record in force; the record stays through both assigns, set_faults and a commit
//                                        and alloc clears it; the sub-seed at three literal values; the stencil rule; the image
//                                        table of a hand-traced sequence (a skipped cell, an image without samples, drops); the
//                                        three preconditions of the shift, each with the sequence, frame and track it names
//   replay_timing_host table             prints the hand-traced sequence's table: "image <i> <time %.17g> <frame_of>" per image and
//                                        "base <f> <base(f)>" per frame
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

// the three values tests/test_replay_timing_plan.py also takes from the twin (scenario.replay_mix(s, REPLAY_TIMING_STREAM))
static_assert(TIMING_STREAM == (1ull << 63) + 2 && TIMING_STREAM != FAULT_STREAM, "the timing stream's index");
static_assert(timing_seed(0x0ull) == 0x61a685ffc80a8140ull, "timing_seed(0)");
static_assert(timing_seed(0xC0FFEE00ull) == 0x398ed654c613a63full, "timing_seed(0xC0FFEE00)");
static_assert(timing_seed(0xFFFFFFFFFFFFFFFFull) == 0xec159351af424190ull, "timing_seed(2^64 - 1)");
// the stencil: the whole track below three entries, else three nodes around the entry, pulled inside at both ends
static_assert(stencil_nodes(0) == 0 && stencil_nodes(1) == 1 && stencil_nodes(2) == 2 && stencil_nodes(3) == 3 && stencil_nodes(64) == 3, "node count");
static_assert(stencil_first(0, 1) == 0 && stencil_first(0, 2) == 0 && stencil_first(1, 2) == 0, "short tracks start at their first entry");
static_assert(stencil_first(0, 3) == 0 && stencil_first(1, 3) == 0 && stencil_first(2, 3) == 0, "three entries: all of them");
static_assert(stencil_first(0, 6) == 0 && stencil_first(1, 6) == 0 && stencil_first(2, 6) == 1 && stencil_first(4, 6) == 3 && stencil_first(5, 6) == 3, "interior and both ends");

static const char* NO_REPLAY = "no replay allocated";
static const char* NOT_FINITE = "timing values must be finite";
static const char* NEG_JITTER = "jitter must not be negative";

constexpr int B = 3, K = 3, F_CAP = 2, FRAMES = 7, N_CAP = 3, M_CAP = 3;

// The hand-traced sequence (sequence 0 of one):
//   frame  cell                                     T      ord  W (slots index)  base  W after the drop
//   0      k = 2, dT 0.01 0.02                      0.03   1    1                0     1
//   1      skipped                                  .      .    .                0     .
//   2      k = 0 (an image without samples)         0.03   2    2                0     2
//   3      k = 3, dT 0.01 x 3, track {0, 2}, drop 2 0.06   3    3                0     1
//   4      k = 1, dT 0.04                           0.10   4    2                2     2
//   5      k = 2, dT 0.02 0.03, track {0, 1, 2}, drop 1  0.15  5  3              2     2
//   6      k = 1, dT 0.05                           0.20   6    3                3     3
struct Cell { int k; double dT[K]; int F; int M[F_CAP]; int slots[M_CAP]; int drop; int flags; };
static const Cell GOOD[FRAMES] = {
  {2, {0.01, 0.02, 0}, 0, {0, 0}, {0, 0, 0}, 0, 0},
  {0, {0, 0, 0}, 0, {0, 0}, {0, 0, 0}, 0, msckf_lists::CELL_SKIP},
  {0, {0, 0, 0}, 0, {0, 0}, {0, 0, 0}, 0, 0},
  {3, {0.01, 0.01, 0.01}, 1, {2, 0}, {0, 2, 0}, 2, 0},
  {1, {0.04, 0, 0}, 0, {0, 0}, {0, 0, 0}, 0, 0},
  {2, {0.02, 0.03, 0}, 1, {3, 0}, {0, 1, 2}, 1, 0},
  {1, {0.05, 0, 0}, 0, {0, 0}, {0, 0, 0}, 0, 0},
};

static void put(Plan& p, int f, const Cell& c) {
  double rd[K * 7] = {0};
  for (int i = 0; i < c.k; ++i) { rd[i * 7] = 0.1 * (i + 1); rd[i * 7 + 6] = c.dT[i]; }
  const double obs[2 * M_CAP] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6};
  CHECK(is(p.cell_refusal(f, 0, rd, c.k, c.F, c.M, c.slots, c.drop, c.flags, M_CAP, N_CAP), 0, nullptr));
  p.set_cell(f, 0, rd, c.k, c.F, c.M, c.slots, obs, c.drop, c.flags);
}
static void stage(Plan& p) {
  p.alloc(1, FRAMES, K, B, F_CAP);
  for (int f = 0; f < FRAMES; ++f) put(p, f, GOOD[f]);
}

static void check_table() {
  Plan p;
  stage(p);
  CHECK(is(p.commit(), 0, nullptr));
  CHECK(p.img_n.size() == 1 && p.img_n[0] == 6);
  const int frame_of[6] = {0, 2, 3, 4, 5, 6}, base[FRAMES] = {0, 0, 0, 0, 2, 2, 3}, W[FRAMES] = {1, 0, 2, 3, 2, 3, 3};
  double T = 0.0, time[6];
  T += 0.01; T += 0.02; time[0] = T; time[1] = T;               // the sums the table forms, in its order
  T += 0.01; T += 0.01; T += 0.01; time[2] = T;
  T += 0.04; time[3] = T;
  T += 0.02; T += 0.03; time[4] = T;
  T += 0.05; time[5] = T;
  for (int i = 0; i < 6; ++i) CHECK(p.img_time[i] == time[i] && p.img_frame[i] == frame_of[i]);
  for (int f = 0; f < FRAMES; ++f) CHECK(p.img_base[p.cell(f, 0)] == base[f] && p.img_W[p.cell(f, 0)] == W[f]);
  // a pure function of the cells: a second commit gives the same, and a patched cell another
  const std::vector<double> before = p.img_time;
  CHECK(is(p.commit(), 0, nullptr) && p.img_time == before);
  Cell longer = GOOD[4];
  longer.dT[0] = 0.07;
  put(p, 4, longer);
  CHECK(!p.committed && is(p.commit(), 0, nullptr) && p.img_time[3] != before[3] && p.img_time[2] == before[2]);
}

static void check_record() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> good = {2e-3, 0.0, 0.0, 0.0, 0.0, 0.03, -0.1, 0.0, -5e-3, 0.02, 0.2, 1e-3};
  const std::vector<double> zeros((size_t)B * N_TIMING, 0.0);
  Plan p;
  CHECK(is(p.timing_refusal(good.data()), -EINVAL, NO_REPLAY));
  CHECK(is(p.timing_refusal(nullptr), -EINVAL, NO_REPLAY));
  stage(p);
  CHECK(p.timing.empty() && !p.timed && !p.timing_uploaded);
  CHECK(is(p.timing_refusal(nullptr), 0, nullptr) && is(p.timing_refusal(good.data()), 0, nullptr) && is(p.timing_refusal(zeros.data()), 0, nullptr));
  // every place and every kind of value that is not finite
  for (int i = 0; i < B * N_TIMING; ++i) for (double bad : {inf, -inf, nan}) {
    std::vector<double> v = good;
    v[i] = bad;
    CHECK(is(p.timing_refusal(v.data()), -EINVAL, NOT_FINITE));
  }
  for (int b = 0; b < B; ++b) {
    std::vector<double> v = good;
    v[(size_t)b * N_TIMING + TIM_SIGMA_J] = -1e-12;
    CHECK(is(p.timing_refusal(v.data()), -EINVAL, NEG_JITTER));
  }
  // the order: a value of the last trajectory that is not finite is named before a negative jitter of the first
  {
    std::vector<double> v = good;
    v[TIM_SIGMA_J] = -1.0; v[(size_t)(B - 1) * N_TIMING + TIM_Y0] = nan;
    CHECK(is(p.timing_refusal(v.data()), -EINVAL, NOT_FINITE));
  }
  // negative offsets and slopes are fine
  {
    std::vector<double> v = good;
    v[TIM_TD] = -0.01; v[TIM_RY] = -0.03;
    CHECK(is(p.timing_refusal(v.data()), 0, nullptr));
  }
  p.set_timing(good.data());
  CHECK(p.timing == good && p.timed && !p.timing_uploaded);
  p.timing_uploaded = true;
  {
    std::vector<double> v = good;
    v[TIM_SIGMA_J] = -1.0;
    if (p.timing_refusal(v.data()).code == 0) p.set_timing(v.data());
    CHECK(p.timing == good && p.timed && p.timing_uploaded);
  }
  // the record stays through both assigns, a fault record and a commit, and they leave the device copy's validity alone
  const int seq_of[B] = {0, 0, 0};
  const uint64_t seed[B] = {1, 2, 3};
  const std::vector<double> sigma((size_t)B * N_SIGMA, 0.01);
  p.assign(seq_of, seed, sigma.data());
  CHECK(p.timing == good && p.timed && p.timing_uploaded);
  std::vector<double> Q((size_t)B * L_SIZE, 0.0);
  for (int b = 0; b < B; ++b) for (int i = 0; i < NQ; ++i) Q[(size_t)b * L_SIZE + i * NQ + i] = 1e-4;
  const double scale[B] = {1.0, 0.5, 0.0}, uv[2 * B] = {1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3};
  p.assign_q(seq_of, seed, Q.data(), scale, uv);
  CHECK(p.timing == good && p.timed && p.timing_uploaded && p.model == MODEL_Q);
  const std::vector<double> fault = {0.1, 0.1, 0.01, 0.01, 0, 0, 0, 0, 0, 0, 0, 0};
  p.set_faults(fault.data());
  CHECK(p.timing == good && p.timed && p.timing_uploaded && p.faulted);
  CHECK(is(p.commit(), 0, nullptr));
  CHECK(p.timing == good && p.timed && p.timing_uploaded && p.committed && p.fault == fault);
  // all zeros and a record with y_0 alone: a record, but nothing is timed; null: no record
  p.set_timing(zeros.data());
  CHECK(p.timing == zeros && !p.timed && !p.timing_uploaded && p.committed && p.assigned);
  {
    std::vector<double> v = zeros;
    for (int b = 0; b < B; ++b) v[(size_t)b * N_TIMING + TIM_Y0] = 0.3;
    p.set_timing(v.data());
    CHECK(!p.timed);
    v[(size_t)(B - 1) * N_TIMING + TIM_SIGMA_J] = 1e-9;
    p.set_timing(v.data());
    CHECK(p.timed);
  }
  p.timing_uploaded = true;
  p.set_timing(nullptr);
  CHECK(p.timing.empty() && !p.timed && !p.timing_uploaded && p.faulted);
  p.set_timing(good.data());
  p.alloc(1, FRAMES, K, B, F_CAP);
  CHECK(p.timing.empty() && !p.timed && !p.timing_uploaded && p.img_time.empty());
}

// the three preconditions, checked only under a non-zero record: at set_timing on committed cells, and at commit
static void check_preconditions() {
  const std::vector<double> rec = {2e-3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, zeros((size_t)B * N_TIMING, 0.0);
  struct Bad { int f; Cell c; const char* why; };
  Cell beyond = GOOD[4]; beyond.F = 1; beyond.M[0] = 2; beyond.slots[0] = 0; beyond.slots[1] = 2;            // W(4) = 2
  Cell descend = GOOD[5]; descend.slots[0] = 1; descend.slots[1] = 0;
  Cell equal_times = GOOD[3]; equal_times.slots[1] = 1;                                                        // images 0 and 1: both at 0.03
  const Bad bad[3] = {
    {4, beyond, "timing: sequence 0, frame 4, track 0: a camera slot beyond the window an empty start gives"},
    {5, descend, "timing: sequence 0, frame 5, track 0: camera slots do not ascend strictly"},
    {3, equal_times, "timing: sequence 0, frame 3, track 0: node times do not increase strictly"},
  };
  for (const Bad& x : bad) {
    Plan p;
    stage(p);
    put(p, x.f, x.c);
    // no record, a zero record: the cells are committed as they are
    CHECK(is(p.commit(), 0, nullptr));
    p.set_timing(zeros.data());
    CHECK(is(p.commit(), 0, nullptr) && is(p.timing_refusal(zeros.data()), 0, nullptr));
    // a non-zero record on them is refused, and the zero record stays
    CHECK(is(p.timing_refusal(rec.data()), -EINVAL, x.why));
    CHECK(p.timing == zeros && !p.timed);
    // the cell mended: accepted; broken again under the record: the commit is refused
    put(p, x.f, GOOD[x.f]);
    CHECK(is(p.timing_refusal(rec.data()), 0, nullptr));       // (not committed: nothing to check yet)
    p.set_timing(rec.data());
    CHECK(is(p.commit(), 0, nullptr) && p.committed);
    put(p, x.f, x.c);
    CHECK(is(p.commit(), -EINVAL, x.why) && !p.committed && p.timing == rec);
  }
  // the value refusals come before the preconditions
  {
    Plan p;
    stage(p);
    put(p, bad[0].f, bad[0].c);
    CHECK(is(p.commit(), 0, nullptr));
    std::vector<double> v = rec;
    v[TIM_SIGMA_J] = -1.0;
    CHECK(is(p.timing_refusal(v.data()), -EINVAL, NEG_JITTER));
  }
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "table") == 0) {
    Plan p;
    stage(p);
    if (p.commit().code) return 1;
    for (int i = 0; i < p.img_n[0]; ++i) std::printf("image %d %.17g %d\n", i, p.img_time[i], p.img_frame[i]);
    for (int f = 0; f < FRAMES; ++f) std::printf("base %d %d\n", f, p.img_base[p.cell(f, 0)]);
    return failures ? 1 : 0;
  }
  check_table();
  check_record();
  check_preconditions();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("replay timing ok\n");
  return 0;
}
