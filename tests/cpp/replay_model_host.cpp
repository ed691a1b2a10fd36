// The host side of the Monte-Carlo replay's Q_imu model (msckf_mono_amd/csrc/replay_plan.h, MODEL) on its own: no HIP header, a
// host compiler only.
//   replay_model_host            chol_psd at literal matrices, every refusal of the model's assignment with its code, text and
//                                order, the walk_planned flag and the model tag
//   replay_model_host factor     prints, per literal matrix, "Q <name> <144 hexfloats>" and "L <name> <144 hexfloats>" (both
//                                column-major) or "L <name> refused"
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../msckf_mono_amd/csrc/replay_plan.h"

using namespace msckf_replay;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)
using Mat = std::vector<double>;   // 12 x 12, column-major

static bool is(const Refusal& r, int code, const char* why) {
  if (r.code != code) return false;
  if (!why) return r.why == nullptr;
  return r.why && std::strcmp(r.why, why) == 0;
}
static double& at(Mat& m, int r, int c) { return m[(size_t)c * NQ + r]; }
static double at(const Mat& m, int r, int c) { return m[(size_t)c * NQ + r]; }

// ---- the literal matrices
static Mat diagonal() {   // the filter's default Q_imu
  Mat q(L_SIZE, 0.0);
  const double d[4] = {1e-4, 3.6733e-5, 1e-2, 7e-2};
  for (int i = 0; i < NQ; ++i) at(q, i, i) = d[i / 3];
  return q;
}
static Mat dense_spd() {   // A A^T + 0.01 I with A_rc = ((7 r + 3 c) mod 5 - 2) / 100
  Mat q(L_SIZE, 0.0);
  for (int r = 0; r < NQ; ++r) for (int c = 0; c < NQ; ++c) {
    double s = r == c ? 0.01 : 0.0;
    for (int j = 0; j < NQ; ++j) s += (((7 * r + 3 * j) % 5 - 2) * 0.01) * (((7 * c + 3 * j) % 5 - 2) * 0.01);
    at(q, r, c) = s;
  }
  return q;
}
static Mat zero_walk() {   // white noise with one cross term, both walk blocks zero
  Mat q = diagonal();
  for (int i = 0; i < 3; ++i) { at(q, 3 + i, 3 + i) = 0.0; at(q, 9 + i, 9 + i) = 0.0; }
  at(q, 0, 6) = at(q, 6, 0) = 5e-4;
  return q;
}
static Mat rank_deficient() {   // the gyro walk block is 4 (1 1 1)^T (1 1 1): rank one; the rest diagonal
  Mat q = diagonal();
  for (int r = 3; r < 6; ++r) for (int c = 3; c < 6; ++c) at(q, r, c) = 4.0;
  return q;
}
static Mat small_exact() {   // [[4, 2], [2, 5]] in the corner, given asymmetrically (1 | 3): L = [[2, 0], [1, 2]]
  Mat q(L_SIZE, 0.0);
  at(q, 0, 0) = 4.0; at(q, 1, 1) = 5.0; at(q, 0, 1) = 1.0; at(q, 1, 0) = 3.0;
  return q;
}
static Mat negative_pivot() {   // [[1, 2], [2, 1]]: d = 1 - 4
  Mat q = diagonal();
  at(q, 0, 0) = 1.0; at(q, 1, 1) = 1.0; at(q, 0, 1) = at(q, 1, 0) = 2.0;
  return q;
}
struct Named { const char* name; Mat (*make)(); };
static const Named MATRICES[] = {{"diagonal", diagonal}, {"dense_spd", dense_spd}, {"zero_walk", zero_walk}, {"rank_deficient", rank_deficient},
                                 {"small_exact", small_exact}, {"negative_pivot", negative_pivot}};

static int print_factors() {
  for (const Named& m : MATRICES) {
    const Mat q = m.make();
    Mat L(L_SIZE, -1.0);
    std::printf("Q %s", m.name);
    for (double v : q) std::printf(" %a", v);
    std::printf("\n");
    if (!chol_psd(q.data(), L.data())) { std::printf("L %s refused\n", m.name); continue; }
    std::printf("L %s", m.name);
    for (double v : L) std::printf(" %a", v);
    std::printf("\n");
  }
  return 0;
}

static void factor_checks() {
  Mat L(L_SIZE, -1.0);
  // diagonal: the square roots, nothing else
  CHECK(chol_psd(diagonal().data(), L.data()));
  for (int r = 0; r < NQ; ++r) for (int c = 0; c < NQ; ++c) CHECK(at(L, r, c) == (r == c ? std::sqrt(at(diagonal(), r, r)) : 0.0));
  // the symmetric part, and exact values
  CHECK(chol_psd(small_exact().data(), L.data()));
  CHECK(at(L, 0, 0) == 2.0 && at(L, 1, 0) == 1.0 && at(L, 0, 1) == 0.0 && at(L, 1, 1) == 2.0 && at(L, 2, 2) == 0.0);
  // dense: lower triangular, L L^T = Q to rounding
  const Mat q = dense_spd();
  CHECK(chol_psd(q.data(), L.data()));
  for (int r = 0; r < NQ; ++r) for (int c = 0; c < NQ; ++c) {
    if (c > r) CHECK(at(L, r, c) == 0.0);
    double s = 0.0;
    for (int j = 0; j < NQ; ++j) s += at(L, r, j) * at(L, c, j);
    CHECK(std::fabs(s - at(q, r, c)) <= 1e-15);
  }
  for (int c = 0; c < NQ; ++c) CHECK(at(L, c, c) > 0.0);
  // zero walk blocks: six zero columns, the cross term in its place
  CHECK(chol_psd(zero_walk().data(), L.data()));
  for (int c : {3, 4, 5, 9, 10, 11}) for (int r = 0; r < NQ; ++r) CHECK(at(L, r, c) == 0.0);
  CHECK(at(L, 0, 0) == std::sqrt(1e-4) && at(L, 6, 0) == 5e-4 / std::sqrt(1e-4) && at(L, 6, 6) == std::sqrt(1e-2 - at(L, 6, 0) * at(L, 6, 0)));
  // a rank-one block: one column, then zero pivots -- whole columns zero, no division
  CHECK(chol_psd(rank_deficient().data(), L.data()));
  CHECK(at(L, 3, 3) == 2.0 && at(L, 4, 3) == 2.0 && at(L, 5, 3) == 2.0);
  for (int c : {4, 5}) for (int r = 0; r < NQ; ++r) CHECK(at(L, r, c) == 0.0);
  CHECK(at(L, 6, 6) == std::sqrt(1e-2));
  // a negative pivot is refused; one within the tolerance of zero is not
  CHECK(!chol_psd(negative_pivot().data(), L.data()));
  { Mat z(L_SIZE, 0.0); CHECK(chol_psd(z.data(), L.data())); for (double v : L) CHECK(v == 0.0); }
  { Mat t = diagonal(); at(t, 4, 4) = -1e-15; CHECK(chol_psd(t.data(), L.data()) && at(L, 4, 4) == 0.0); at(t, 4, 4) = -1e-12; CHECK(!chol_psd(t.data(), L.data())); }
}

// one cell of k samples and no track
static void put(Plan& p, int f, int s, int k) {
  std::vector<double> rd((size_t)std::max(k, 1) * 7, 0.005);
  const int none[1] = {0}; const double no_obs[2] = {0.0, 0.0};
  CHECK(is(p.cell_refusal(f, s, rd.data(), k, 0, none, none, 0, 0, 4, 4), 0, nullptr));
  p.set_cell(f, s, rd.data(), k, 0, none, none, no_obs, 0, 0);
}

// ---- the model's assignment: S = 2, B = 3, K = 2, 3 frames
static void assignment() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  Plan p;
  const int q0[3] = {1, 0, 1}; const uint64_t sd[3] = {1, 2, 3};
  std::vector<double> Q;
  for (int b = 0; b < 3; ++b) { const Mat m = b == 1 ? zero_walk() : dense_spd(); Q.insert(Q.end(), m.begin(), m.end()); }
  const std::vector<double> scale(3, 0.05), uv(6, 1e-3), sg(12, 0.25);
  CHECK(is(p.assign_q_refusal(q0, Q.data(), scale.data(), uv.data()), -EINVAL, "no replay allocated"));
  CHECK(is(p.walk_refusal(0, 0, 0, 0), -EINVAL, "no replay allocated") && is(p.walk_refusal(0, 2, 0, 3), -EINVAL, "no replay allocated"));
  p.alloc(2, 3, 2, 3, 3);
  CHECK(p.model == MODEL_SIGMA4 && !p.walk_planned);
  CHECK(is(p.walk_refusal(0, 0, 0, 0), -EINVAL, "replay not committed") && is(p.walk_refusal(0, 5, 0, 0), -EINVAL, "walk range out of bounds"));
  put(p, 0, 0, 2); put(p, 1, 0, 1); put(p, 0, 1, 2); put(p, 2, 1, 2);
  CHECK(is(p.commit(), 0, nullptr));
  // the rules in order: the sequence, finite, not negative, positive semi-definite -- each with everything after it wrong too
  std::vector<double> Qneg(Q); { const Mat m = negative_pivot(); std::copy(m.begin(), m.end(), Qneg.begin() + 2 * L_SIZE); }
  std::vector<double> s_neg(scale), uv_neg(uv); s_neg[1] = -1e-300; uv_neg[5] = -1.0;
  { int bad[3] = {1, 2, 1}; CHECK(is(p.assign_q_refusal(bad, Qneg.data(), s_neg.data(), uv.data()), -EINVAL, "seq_of names no sequence of the replay")); bad[1] = -1; CHECK(is(p.assign_q_refusal(bad, Q.data(), scale.data(), uv.data()), -EINVAL, "seq_of names no sequence of the replay")); }
  for (double v : {inf, -inf, nan}) {
    std::vector<double> Qb(Qneg), sb(s_neg), ub(uv_neg);
    Qb[L_SIZE + 17] = v;
    CHECK(is(p.assign_q_refusal(q0, Qb.data(), s_neg.data(), uv_neg.data()), -EINVAL, "Q, scale and sigma must be finite"));
    sb[2] = v;
    CHECK(is(p.assign_q_refusal(q0, Qneg.data(), sb.data(), uv_neg.data()), -EINVAL, "Q, scale and sigma must be finite"));
    ub[0] = v;
    CHECK(is(p.assign_q_refusal(q0, Qneg.data(), s_neg.data(), ub.data()), -EINVAL, "Q, scale and sigma must be finite"));
  }
  CHECK(is(p.assign_q_refusal(q0, Qneg.data(), s_neg.data(), uv.data()), -EINVAL, "scale and sigma must not be negative"));
  CHECK(is(p.assign_q_refusal(q0, Qneg.data(), scale.data(), uv_neg.data()), -EINVAL, "scale and sigma must not be negative"));
  CHECK(is(p.assign_q_refusal(q0, Qneg.data(), scale.data(), uv.data()), -EINVAL, "Q is not positive semi-definite"));
  { const std::vector<double> z(3, 0.0), zu(6, 0.0); CHECK(is(p.assign_q_refusal(q0, Q.data(), z.data(), zu.data()), 0, nullptr)); }
  // a refusal leaves the assignment made before: here none, then the sigma4 one
  CHECK(!p.assigned && is(p.run_refusal(0, 3), -EINVAL, "replay not assigned"));
  p.assign(q0, sd, sg.data());
  CHECK(p.assigned && p.model == MODEL_SIGMA4 && is(p.walk_refusal(0, 4, 0, 3), -EINVAL, "replay not assigned through msckf_hip_replay_assign_q"));
  CHECK(is(p.assign_q_refusal(q0, Qneg.data(), scale.data(), uv.data()), -EINVAL, "Q is not positive semi-definite") && p.model == MODEL_SIGMA4 && p.sigma == sg && p.L.empty());
  // the model's record
  CHECK(is(p.assign_q_refusal(q0, Q.data(), scale.data(), uv.data()), 0, nullptr));
  p.assign_q(q0, sd, Q.data(), scale.data(), uv.data());
  CHECK(p.model == MODEL_Q && p.assigned && !p.planned && !p.walk_planned);
  CHECK(p.L.size() == (size_t)3 * L_SIZE && p.scale == scale && p.sigma_uv == uv && p.seq_of == std::vector<int>(q0, q0 + 3) && p.seed == std::vector<uint64_t>(sd, sd + 3));
  { Mat L(L_SIZE); CHECK(chol_psd(zero_walk().data(), L.data()) && std::equal(L.begin(), L.end(), p.L.begin() + L_SIZE)); CHECK(chol_psd(dense_spd().data(), L.data()) && std::equal(L.begin(), L.end(), p.L.begin() + 2 * L_SIZE)); }
  // the walk's ranges: frames + 1 rows, then what has to have happened
  CHECK(is(p.walk_refusal(0, 4, 0, 3), 0, nullptr) && is(p.walk_refusal(4, 4, 3, 0), 0, nullptr) && is(p.walk_refusal(2, 2, 1, 1), 0, nullptr));
  CHECK(is(p.walk_refusal(0, 5, 0, 3), -EINVAL, "walk range out of bounds") && is(p.walk_refusal(-1, 2, 0, 3), -EINVAL, "walk range out of bounds") && is(p.walk_refusal(3, 2, 0, 3), -EINVAL, "walk range out of bounds"));
  CHECK(is(p.walk_refusal(0, 4, 1, 3), -EINVAL, "walk range out of bounds") && is(p.walk_refusal(0, 4, -1, 2), -EINVAL, "walk range out of bounds") && is(p.walk_refusal(0, 4, 0, -1), -EINVAL, "walk range out of bounds"));
  CHECK(is(p.run_refusal(0, 3), 0, nullptr) && is(p.expand_refusal(2, 2), 0, nullptr) && is(p.index_trajectories(), 0, nullptr) && p.planned);
  // walk_planned (set by the caller that has tabulated the walk) falls on each of the four events
  p.walk_planned = true; put(p, 1, 1, 1);
  CHECK(!p.walk_planned && !p.committed && is(p.walk_refusal(0, 4, 0, 3), -EINVAL, "replay not committed"));
  p.walk_planned = true; CHECK(is(p.commit(), 0, nullptr) && !p.walk_planned && is(p.walk_refusal(0, 4, 0, 3), 0, nullptr));
  p.walk_planned = true; p.assign_q(q0, sd, Q.data(), scale.data(), uv.data());
  CHECK(!p.walk_planned && p.model == MODEL_Q);
  p.walk_planned = true; p.assign(q0, sd, sg.data());
  // a sigma4 assignment after the model's switches the tag back, and the model's again forth
  CHECK(!p.walk_planned && p.model == MODEL_SIGMA4 && p.sigma == sg && is(p.walk_refusal(0, 4, 0, 3), -EINVAL, "replay not assigned through msckf_hip_replay_assign_q"));
  CHECK(is(p.run_refusal(0, 3), 0, nullptr));
  p.assign_q(q0, sd, Q.data(), scale.data(), uv.data());
  CHECK(p.model == MODEL_Q && is(p.walk_refusal(0, 4, 0, 3), 0, nullptr));
  // a new replay starts from the sigma4 tag
  p.walk_planned = true; p.alloc(2, 3, 2, 3, 3);
  CHECK(p.model == MODEL_SIGMA4 && !p.walk_planned && !p.assigned && p.L.empty());
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "factor") == 0) return print_factors();
  factor_checks();
  assignment();
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("replay model ok\n");
  return 0;
}
