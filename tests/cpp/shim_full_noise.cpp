// tests/cpp/shim_full_noise.cpp -- the drop-in shim (include/msckf_mono/msckf.h, Eigen-free build) with a whole, correlated
// Q_imu and initial_imu_covar given through the full-matrix members of noiseParams (pod_types.h): the call sequence of
// datasets/asl_msckf.cpp:227-294 on numbers read from stdin; prints the state for the pytest wrapper to compare with the numpy
// twin.  A copy of the filter taken half-way (MSCKF is copyable, msckf.h:31-67) finishes the run too and must print the same.
//   input : cam12 uv2 Q_imu(12 x 12, row by row) initial_imu_covar(15 x 15, row by row) params8 imu29,
//           then frames: "F K" K*7 readings, n_cur (x y id)*, n_new (x y id)*
//   output: imu16 | ncam | D*D covariance (column-major) | 1 if the copy ended bit-identical, else 0
#include <cstdio>
#include <iostream>
#include <vector>

#include "msckf_mono/msckf.h"

using namespace msckf_mono;
typedef double S;

static bool same(const std::vector<double>& a, const std::vector<double>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) if (a[i] != b[i]) return false;
  return true;
}

int main() {
  double cam[12], uv[2], prm[8], imu[29];
  for (double& v : cam) std::cin >> v;
  for (double& v : uv) std::cin >> v;
  noiseParams<S> np;
  np.u_var_prime = uv[0]; np.v_var_prime = uv[1];
  for (int i = 0; i < 12; ++i) for (int j = 0; j < 12; ++j) std::cin >> np.Q_imu[i][j];
  for (int i = 0; i < 15; ++i) for (int j = 0; j < 15; ++j) std::cin >> np.initial_imu_covar[i][j];
  for (double& v : prm) std::cin >> v;
  for (double& v : imu) std::cin >> v;
  Camera<S> camera;
  camera.c_u = cam[0]; camera.c_v = cam[1]; camera.f_u = cam[2]; camera.f_v = cam[3]; camera.b = cam[4];
  camera.q_CI = Quaternion<S>(cam[5], cam[6], cam[7], cam[8]);
  for (int i = 0; i < 3; ++i) camera.p_C_I(i) = cam[9 + i];
  MSCKFParams<S> mp;
  mp.max_gn_cost_norm = prm[0]; mp.min_rcond = prm[1]; mp.translation_threshold = prm[2];
  mp.redundancy_angle_thresh = prm[3]; mp.redundancy_distance_thresh = prm[4];
  mp.min_track_length = (int)prm[5]; mp.max_track_length = (int)prm[6]; mp.max_cam_states = (int)prm[7];
  imuState<S> st;
  st.q_IG = Quaternion<S>(imu[0], imu[1], imu[2], imu[3]);
  for (int i = 0; i < 3; ++i) { st.b_g(i) = imu[4 + i]; st.v_I_G(i) = imu[7 + i]; st.b_a(i) = imu[10 + i]; st.p_I_G(i) = imu[13 + i]; st.g(i) = imu[16 + i]; }

  MSCKF<S> msckf;
  msckf.initialize(camera, np, mp, st);
  if (msckf.lastError()) return 2;
  int nframes;
  std::cin >> nframes;
  int state_k = 0;
  MSCKF<S> twin;
  bool have_twin = false;
  for (int f = 0; f < nframes; ++f) {
    if (f == nframes / 2) { twin = msckf; have_twin = true; if (twin.lastError()) return 4; }
    int K; std::cin >> K;
    for (int k = 0; k < K; ++k) {
      imuReading<S> rd;
      for (int i = 0; i < 3; ++i) std::cin >> rd.omega(i);
      for (int i = 0; i < 3; ++i) std::cin >> rd.a(i);
      std::cin >> rd.dT;
      state_k++;
      msckf.propagate(rd);
      if (have_twin) twin.propagate(rd);
    }
    MSCKF<S>::Vec2List cur, fresh; std::vector<size_t> cur_ids, new_ids;
    int n; std::cin >> n;
    for (int i = 0; i < n; ++i) { Vector2<S> z; size_t id; std::cin >> z(0) >> z(1) >> id; cur.push_back(z); cur_ids.push_back(id); }
    std::cin >> n;
    for (int i = 0; i < n; ++i) { Vector2<S> z; size_t id; std::cin >> z(0) >> z(1) >> id; fresh.push_back(z); new_ids.push_back(id); }
    msckf.augmentState(state_k, (S)f);
    msckf.update(cur, cur_ids);
    msckf.addFeatures(fresh, new_ids);
    msckf.marginalize();
    msckf.pruneEmptyStates();
    if (msckf.lastError()) return 3;
    if (have_twin) {
      twin.augmentState(state_k, (S)f); twin.update(cur, cur_ids); twin.addFeatures(fresh, new_ids); twin.marginalize(); twin.pruneEmptyStates();
      if (twin.lastError()) return 5;
    }
  }
  imuState<S> s = msckf.getImuState();
  std::printf("%.17g %.17g %.17g %.17g", s.q_IG.w(), s.q_IG.x(), s.q_IG.y(), s.q_IG.z());
  for (int i = 0; i < 3; ++i) std::printf(" %.17g", s.b_g(i));
  for (int i = 0; i < 3; ++i) std::printf(" %.17g", s.v_I_G(i));
  for (int i = 0; i < 3; ++i) std::printf(" %.17g", s.b_a(i));
  for (int i = 0; i < 3; ++i) std::printf(" %.17g", s.p_I_G(i));
  std::printf("\n%d\n", (int)msckf.getNumCamStates());
  const std::vector<double> P = msckf.getCovariance();
  for (size_t i = 0; i < P.size(); ++i) std::printf(i ? " %.17g" : "%.17g", P[i]);
  imuState<S> t = twin.getImuState();
  const bool copy_same = have_twin && same(P, twin.getCovariance()) && t.q_IG.w() == s.q_IG.w() && t.q_IG.x() == s.q_IG.x() &&
                         t.q_IG.y() == s.q_IG.y() && t.q_IG.z() == s.q_IG.z() && t.p_I_G(0) == s.p_I_G(0) && t.p_I_G(1) == s.p_I_G(1) &&
                         t.p_I_G(2) == s.p_I_G(2) && t.v_I_G(0) == s.v_I_G(0) && t.b_g(0) == s.b_g(0) && t.b_a(0) == s.b_a(0);
  std::printf("\n%d\n", copy_same ? 1 : 0);
  return 0;
}
