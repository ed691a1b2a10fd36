// The host side of the Monte-Carlo replay's calibration model (msckf_mono_amd/csrc/replay_plan.h, CALIB) on its own: no HIP header,
// a host compiler only.
//   replay_calib_host                    every refusal of set_imu_calib / set_cam_calib with its code, text and order; a refused
//                                        call leaves the previous record in force; the records stay through both assigns,
//                                        set_faults, set_timing and a commit and alloc clears them; which records are trivial;
//                                        the identity and zero records return the values' bits; clamp and rint at exact
//                                        thresholds and ties
//   replay_calib_host imu                N_ROWS rows drawn from the integer stream the twin shares, under three records drawn
//                                        the same way, through calib_imu and calib_out: "imu <n> <c x 6> <out x 6> <mask>" in
//                                        hex doubles
//   replay_calib_host cam                N_ROWS entries through calib_cam: "cam <n> <x'> <y'>" in hex doubles
// tests/test_replay_calib_plan.py draws the same inputs and compares the bits with the numpy twin's.
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

static const char* NO_REPLAY = "no replay allocated";
static const char* NOT_FINITE = "calibration values must be finite";
static const char* NEGATIVE = "saturation and quantisation must not be negative";

constexpr int B = 3, K = 2, F_CAP = 2, FRAMES = 2;
constexpr int N_ROWS = 300, N_REC = 3;
constexpr uint64_t SEED_ROW = 1234, SEED_NOISE = 555, SEED_IMU_REC = 99, SEED_OBS = 4321, SEED_CAM_REC = 98;

static_assert(IMU_CAL == 31 && CAM_CAL == 8 && IC_TG == 0 && IC_TA == 9 && IC_G == 18 && IC_SAT_G == 27 && IC_SAT_A == 28 && IC_LSB_G == 29 && IC_LSB_A == 30, "the IMU record's layout");
static_assert(CC_EU == 0 && CC_EV == 1 && CC_DU == 2 && CC_DV == 3 && CC_K1 == 4 && CC_K2 == 5 && CC_P1 == 6 && CC_P2 == 7, "the camera record's layout");
static_assert(N_CALIB_COUNT == 8 && CCNT_SAMPLES == 0 && CCNT_CLIP == 1 && CCNT_ANY == 7, "the counts' columns");

static double centred(uint64_t seed, uint64_t i, double scale) { return (U(seed, i) - 0.5) * scale; }

// record j of the bit-for-bit comparison: matrices near the identity; j >= 1 saturates, j == 2 quantises as well
static void imu_record(int j, double* ic) {
  for (int i = 0; i < 27; ++i) {
    const bool diag = i < 18 && (i % 9) % 4 == 0;
    ic[i] = (diag ? 1.0 : 0.0) + centred(SEED_IMU_REC, (uint64_t)(IMU_CAL * j + i), i < 18 ? 0.02 : 2e-3);
  }
  ic[IC_SAT_G] = j >= 1 ? 0.5 + U(SEED_IMU_REC, (uint64_t)(IMU_CAL * j + 27)) * 0.3 : 0.0;
  ic[IC_SAT_A] = j >= 1 ? 8.0 + U(SEED_IMU_REC, (uint64_t)(IMU_CAL * j + 28)) * 4.0 : 0.0;
  ic[IC_LSB_G] = j == 2 ? 1e-4 * (1.0 + U(SEED_IMU_REC, (uint64_t)(IMU_CAL * j + 29))) : 0.0;
  ic[IC_LSB_A] = j == 2 ? 1e-2 * (1.0 + U(SEED_IMU_REC, (uint64_t)(IMU_CAL * j + 30))) : 0.0;
}
static void cam_record(int j, double* cc) {
  const double scale[CAM_CAL] = {0.01, 0.01, 0.01, 0.01, 0.2, 0.05, 2e-3, 2e-3};
  for (int i = 0; i < CAM_CAL; ++i) cc[i] = centred(SEED_CAM_REC, (uint64_t)(CAM_CAL * j + i), scale[i]);
}

static void print_imu() {
  for (int n = 0; n < N_ROWS; ++n) {
    double ic[IMU_CAL], v[6];
    imu_record(n % N_REC, ic);
    for (int c = 0; c < 6; ++c) v[c] = centred(SEED_ROW, (uint64_t)(6 * n + c), c < 3 ? 2.0 : 30.0);
    std::printf("imu %d", n);
    double cv[6];
    for (int c = 0; c < 6; ++c) { cv[c] = calib_imu(ic, v, c); std::printf(" %a", cv[c]); }
    int mask = 0;
    for (int c = 0; c < 6; ++c) {
      bool cl;
      const double x = cv[c] + centred(SEED_NOISE, (uint64_t)(6 * n + c), 0.1);
      std::printf(" %a", calib_out(ic, c, x, &cl));
      mask |= cl ? 1 << c : 0;
    }
    std::printf(" %d\n", mask);
  }
}
static void print_cam() {
  for (int n = 0; n < N_ROWS; ++n) {
    double cc[CAM_CAL], z[2];
    cam_record(n % N_REC, cc);
    calib_cam(cc, centred(SEED_OBS, (uint64_t)(2 * n), 1.2), centred(SEED_OBS, (uint64_t)(2 * n + 1), 1.2), z);
    std::printf("cam %d %a %a\n", n, z[0], z[1]);
  }
}

static void stage(Plan& p) {
  p.alloc(1, FRAMES, K, B, F_CAP);
  const double rd[K * 7] = {0.1, 0.2, 0.3, 9.8, 0.1, 0.2, 0.005, 0.1, 0.2, 0.3, 9.8, 0.1, 0.2, 0.005};
  const int M[F_CAP] = {2, 0}, slots[2] = {0, 1};
  const double obs[4] = {0.1, 0.2, 0.3, 0.4};
  for (int f = 0; f < FRAMES; ++f) p.set_cell(f, 0, rd, K, f ? 1 : 0, M, slots, obs, 0, 0);
}

static void check_records() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> id((size_t)B * IMU_CAL), good, zeros((size_t)B * CAM_CAL, 0.0), cam((size_t)B * CAM_CAL, 0.0);
  for (int b = 0; b < B; ++b) imu_calib_identity(id.data() + (size_t)b * IMU_CAL);
  good = id;
  good[IMU_CAL + IC_TG + 1] = 1e-3; good[2 * IMU_CAL + IC_SAT_A] = 9.0; good[2 * IMU_CAL + IC_LSB_G] = 1e-4;
  cam[CAM_CAL + CC_K1] = -0.01; cam[2 * CAM_CAL + CC_DU] = 1e-3;
  Plan p;
  CHECK(is(p.imu_calib_refusal(good.data()), -EINVAL, NO_REPLAY) && is(p.imu_calib_refusal(nullptr), -EINVAL, NO_REPLAY));
  CHECK(is(p.cam_calib_refusal(cam.data()), -EINVAL, NO_REPLAY) && is(p.cam_calib_refusal(nullptr), -EINVAL, NO_REPLAY));
  stage(p);
  CHECK(p.imucal.empty() && p.camcal.empty() && !p.calibrated() && !p.calib_uploaded);
  CHECK(is(p.imu_calib_refusal(nullptr), 0, nullptr) && is(p.imu_calib_refusal(good.data()), 0, nullptr) && is(p.imu_calib_refusal(id.data()), 0, nullptr));
  CHECK(is(p.cam_calib_refusal(nullptr), 0, nullptr) && is(p.cam_calib_refusal(cam.data()), 0, nullptr) && is(p.cam_calib_refusal(zeros.data()), 0, nullptr));
  // every place and every kind of value that is not finite
  for (int i = 0; i < B * IMU_CAL; ++i) for (double bad : {inf, -inf, nan}) {
    std::vector<double> v = good;
    v[i] = bad;
    CHECK(is(p.imu_calib_refusal(v.data()), -EINVAL, NOT_FINITE));
  }
  for (int i = 0; i < B * CAM_CAL; ++i) for (double bad : {inf, -inf, nan}) {
    std::vector<double> v = cam;
    v[i] = bad;
    CHECK(is(p.cam_calib_refusal(v.data()), -EINVAL, NOT_FINITE));
  }
  for (int b = 0; b < B; ++b) for (int c = IC_SAT_G; c < IMU_CAL; ++c) {
    std::vector<double> v = good;
    v[(size_t)b * IMU_CAL + c] = -1e-12;
    CHECK(is(p.imu_calib_refusal(v.data()), -EINVAL, NEGATIVE));
  }
  // the order: a value of the last trajectory that is not finite is named before a negative level of the first
  {
    std::vector<double> v = good;
    v[IC_SAT_G] = -1.0; v[(size_t)(B - 1) * IMU_CAL + IC_G] = nan;
    CHECK(is(p.imu_calib_refusal(v.data()), -EINVAL, NOT_FINITE));
  }
  // negative matrix entries and camera fields are fine
  {
    std::vector<double> v = good, w = cam;
    v[IC_TG] = -1.0; v[IC_G + 4] = -1e-3; w[CC_EU] = -0.01; w[CC_P2] = -1e-4;
    CHECK(is(p.imu_calib_refusal(v.data()), 0, nullptr) && is(p.cam_calib_refusal(w.data()), 0, nullptr));
  }
  p.set_imu_calib(good.data());
  p.set_cam_calib(cam.data());
  CHECK(p.imucal == good && p.camcal == cam && p.imu_calibrated && p.cam_calibrated && p.calibrated() && !p.calib_uploaded);
  p.calib_uploaded = true;
  // a refused call leaves the previous record in force
  {
    std::vector<double> v = good, w = cam;
    v[IC_LSB_A] = -1.0; w[3] = nan;
    if (p.imu_calib_refusal(v.data()).code == 0) p.set_imu_calib(v.data());
    if (p.cam_calib_refusal(w.data()).code == 0) p.set_cam_calib(w.data());
    CHECK(p.imucal == good && p.camcal == cam && p.calibrated() && p.calib_uploaded);
  }
  // the records stay through both assigns, a fault record, a timing record and a commit, and these leave the device copy's validity alone
  const int seq_of[B] = {0, 0, 0};
  const uint64_t seed[B] = {1, 2, 3};
  const std::vector<double> sigma((size_t)B * N_SIGMA, 0.01);
  p.assign(seq_of, seed, sigma.data());
  CHECK(p.imucal == good && p.camcal == cam && p.calibrated() && p.calib_uploaded);
  std::vector<double> Q((size_t)B * L_SIZE, 0.0);
  for (int b = 0; b < B; ++b) for (int i = 0; i < NQ; ++i) Q[(size_t)b * L_SIZE + i * NQ + i] = 1e-4;
  const double scale[B] = {1.0, 0.5, 0.0}, uv[2 * B] = {1e-3, 1e-3, 1e-3, 1e-3, 1e-3, 1e-3};
  p.assign_q(seq_of, seed, Q.data(), scale, uv);
  CHECK(p.imucal == good && p.camcal == cam && p.calibrated() && p.calib_uploaded && p.model == MODEL_Q);
  const std::vector<double> fault = {0.1, 0.1, 0.01, 0.01, 0, 0, 0, 0, 0, 0, 0, 0};
  p.set_faults(fault.data());
  const std::vector<double> timing = {1e-3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  CHECK(is(p.timing_refusal(timing.data()), 0, nullptr));
  p.set_timing(timing.data());
  CHECK(p.imucal == good && p.camcal == cam && p.calibrated() && p.calib_uploaded && p.faulted && p.timed);
  CHECK(is(p.commit(), 0, nullptr));
  CHECK(p.imucal == good && p.camcal == cam && p.calibrated() && p.calib_uploaded && p.committed && p.fault == fault && p.timing == timing);
  // which records are trivial: the identity and zeros are records, but nothing is calibrated; null: no record
  p.set_imu_calib(id.data());
  CHECK(p.imucal == id && !p.imu_calibrated && p.cam_calibrated && p.calibrated() && !p.calib_uploaded && p.committed && p.assigned);
  p.set_cam_calib(zeros.data());
  CHECK(p.camcal == zeros && !p.cam_calibrated && !p.calibrated());
  for (int i = 0; i < IMU_CAL; ++i) {                            // any single field of the last trajectory makes it non-trivial
    std::vector<double> v = id;
    v[(size_t)(B - 1) * IMU_CAL + i] += 1e-9;
    p.set_imu_calib(v.data());
    CHECK(p.imu_calibrated);
  }
  for (int i = 0; i < CAM_CAL; ++i) {
    std::vector<double> v = zeros;
    v[(size_t)(B - 1) * CAM_CAL + i] = -1e-12;
    p.set_cam_calib(v.data());
    CHECK(p.cam_calibrated);
  }
  p.calib_uploaded = true;
  p.set_imu_calib(nullptr);
  CHECK(p.imucal.empty() && !p.imu_calibrated && !p.calib_uploaded && p.cam_calibrated && p.faulted && p.timed);
  p.set_cam_calib(nullptr);
  CHECK(p.camcal.empty() && !p.calibrated());
  p.set_imu_calib(good.data());
  p.set_cam_calib(cam.data());
  p.alloc(1, FRAMES, K, B, F_CAP);
  CHECK(p.imucal.empty() && p.camcal.empty() && !p.calibrated() && !p.calib_uploaded);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static void check_arithmetic() {
  double id[IMU_CAL], zero[CAM_CAL] = {0};
  imu_calib_identity(id);
  // the identity and the zero record return the values' bits
  for (int n = 0; n < 50; ++n) {
    double v[6], z[2];
    for (int c = 0; c < 6; ++c) v[c] = centred(SEED_ROW, (uint64_t)(6 * n + c), c < 3 ? 2.0 : 30.0);
    for (int c = 0; c < 6; ++c) { bool cl = true; CHECK(same_bits(calib_imu(id, v, c), v[c]) && same_bits(calib_out(id, c, v[c], &cl), v[c]) && !cl); }
    calib_cam(zero, v[0], v[1], z);
    CHECK(same_bits(z[0], v[0]) && same_bits(z[1], v[1]));
  }
  // the clamp at the exact thresholds: +-sat is not clipped, the next double beyond is
  double ic[IMU_CAL];
  imu_calib_identity(ic);
  ic[IC_SAT_G] = 0.25; ic[IC_SAT_A] = 9.0;
  bool cl;
  CHECK(calib_out(ic, 0, 0.25, &cl) == 0.25 && !cl);
  CHECK(calib_out(ic, 1, -0.25, &cl) == -0.25 && !cl);
  CHECK(calib_out(ic, 2, std::nextafter(0.25, 1.0), &cl) == 0.25 && cl);
  CHECK(calib_out(ic, 0, std::nextafter(-0.25, -1.0), &cl) == -0.25 && cl);
  CHECK(calib_out(ic, 3, 0.3, &cl) == 0.3 && !cl);              // the accelerometer's level, not the gyro's
  CHECK(calib_out(ic, 5, -12.0, &cl) == -9.0 && cl);
  // rint at exact ties goes to the even multiple; the step is a power of two, so quotient and product are exact
  imu_calib_identity(ic);
  ic[IC_LSB_G] = 0.25; ic[IC_LSB_A] = 0.5;
  CHECK(calib_out(ic, 0, 0.125, &cl) == 0.0 && !cl);            // 0.5 steps -> 0
  CHECK(calib_out(ic, 0, 0.375, &cl) == 0.5);                   // 1.5 -> 2
  CHECK(calib_out(ic, 1, 0.625, &cl) == 0.5);                   // 2.5 -> 2
  CHECK(calib_out(ic, 2, -0.375, &cl) == -0.5);                 // -1.5 -> -2
  CHECK(calib_out(ic, 2, -0.125, &cl) == 0.0);                  // -0.5 -> -0
  CHECK(calib_out(ic, 4, 0.75, &cl) == 1.0 && calib_out(ic, 4, 1.25, &cl) == 1.0 && calib_out(ic, 4, 1.2500000000000002, &cl) == 1.5);
  // saturation first, then quantisation: the clamped value lands on the grid nearest to the level
  ic[IC_SAT_G] = 0.3;
  CHECK(calib_out(ic, 0, 1.0, &cl) == 0.25 && cl);              // 0.3 / 0.25 = 1.2 -> 1
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "imu") == 0) { print_imu(); return 0; }
  if (argc == 2 && std::strcmp(argv[1], "cam") == 0) { print_cam(); return 0; }
  check_records();
  check_arithmetic();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("replay calib ok\n");
  return 0;
}
