// settings.h -- every tunable of a batch handle in one record, and the one table that says where each comes from.
//
// A handle (BatchCore in msckf_hip.hip) keeps a Settings.  SETTINGS_TABLE has one row per field: the environment variable that
// sets it when the handle is created (settings_from_env; null: only a setter of the C interface changes it), the values the
// variable may take where that is checked, and whether a copy of the handle (msckf_hip_copy_state -> Settings::take_over) takes
// the field over -- everything that decides numerics or which kernels run -- or leaves it with its own handle (plumbing; the host
// affinity of the enqueue threads, a list, stays with its handle too).  The three process-wide variables, which belong to no
// handle and are read where they are used, close the table, so that it names every variable the library reads.
// INTEGRATION.md, "Settings", is the same table in prose.  No HIP header: a host compiler accepts this file on its own.
#ifndef MSCKF_SETTINGS_H
#define MSCKF_SETTINGS_H

#include <cstdlib>
#include <string>

namespace msckf_settings {

struct Settings {
  int nstreams = 1;          // slices of the batch that run_frames enqueues concurrently (msckf_hip_set_streams)
  int fuse_prune = 1;        // run_frames: prune rides on the downdate (0: separate k_prune_inplace launch)
  int overlap_feature = 0;   // measured on MI355X at cfg3: 100 k -> 82 k updates/s with the overlap on (k_feature floods the CUs the
                             // latency-bound propagate/augment workgroups need); kept selectable, off by default
  int compress_route = -1;   // -1 default, 0 Householder TSQR, != 0 information form + blocked matrix-core Cholesky
  int small_update = 84;     // windows of at most this many camera columns (6 x cameras) take the one-launch update k_update_small; 0 switches it off
  int gain_parts = 0;        // workgroups per trajectory of the float blocked gain solve (2 | 4), 0: by the batch size (Dev::gain_parts)
  int fused_s = 2;           // Dev::gain_fused_s; 0: the S GEMM as a launch of its own (A/B runs)
  int feat_pair = 1;         // k_feature_pair (0: k_feature)
  int cov_update = 0;        // 0 square-root gain (P - W W^T), 1 Joseph, 2 square-root gain with the register-resident solve
  int gate_early = 0;
  // anisotropic pixel noise (u_var' != v_var'): 0 = the reference's construction R_o_j = A_j^T R_j A_j, R_n = Q_1^T R_o Q_1 on
  // the device (kernels_literal.hip; default), 1 = rows pre-whitened by 1/sigma (generalized least squares, unit noise)
  int aniso_mode = 0;
  double lit_tol = -1;       // zero-tail tolerance of the literal route; < 0: 1e-10 (double) / 8e-4 (float: H_x is float-rounded)
  int lit_route = 0;         // 0 the compact route; 1 the sweep over the dense stack (tests, A/B)
  int lit_serial = 0;        // 1: k_lit_pre's per-track part on one lane with literal_core.h's serial reference (A/B runs)
  int lit_timers = 0;        // phase stamps of k_literal, printed by msckf_hip_literal_info (profiling runs)
  int ring = 6, up_mode = 0; // run_frames_streamed's staging sets; up_mode 0: the host threads hand frames over, 1: hipStreamWaitEvent
  int test_fail_upload = -1; // test hook: run_frames_streamed pretends that this frame's copy failed
  inline void take_over(const Settings& o);
};

enum { KEPT = 0, COPIED = 1 };      // what a copy of the handle does with the field
enum { NUMBER = 0, FLAG = 1 };      // how the variable's text is read: atoi, or atoi != 0
struct SettingRow {
  const char* env;                  // null: no variable
  int Settings::* field = nullptr;  // field and dfield both null: process-wide, not a handle's
  double Settings::* dfield = nullptr;
  int copied = KEPT, flag = NUMBER;
  const int* allowed = nullptr; int n_allowed = 0; const char* refusal = nullptr;   // the check of the variable's value, where there is one
};
inline constexpr int GAIN_PARTS_ALLOWED[] = {0, 2, 4};
inline constexpr SettingRow SETTINGS_TABLE[] = {
    {nullptr, &Settings::nstreams, nullptr, COPIED},
    {"MSCKF_HIP_FUSE_PRUNE", &Settings::fuse_prune, nullptr, COPIED, FLAG},
    {nullptr, &Settings::overlap_feature, nullptr, COPIED},
    {nullptr, &Settings::compress_route, nullptr, COPIED},
    {"MSCKF_HIP_SMALL_UPDATE", &Settings::small_update, nullptr, COPIED},
    {"MSCKF_HIP_GAIN_PARTS", &Settings::gain_parts, nullptr, COPIED, NUMBER, GAIN_PARTS_ALLOWED, 3, "MSCKF_HIP_GAIN_PARTS must be 0, 2 or 4"},
    {"MSCKF_HIP_FUSED_S", &Settings::fused_s, nullptr, COPIED},
    {"MSCKF_HIP_FEATURE_PAIR", &Settings::feat_pair, nullptr, COPIED},
    {nullptr, &Settings::cov_update, nullptr, COPIED},
    {nullptr, &Settings::gate_early, nullptr, COPIED},
    {nullptr, &Settings::aniso_mode, nullptr, COPIED},
    {nullptr, nullptr, &Settings::lit_tol, COPIED},
    {"MSCKF_HIP_LITERAL_ROUTE", &Settings::lit_route, nullptr, COPIED},
    {"MSCKF_HIP_LITERAL_SERIAL", &Settings::lit_serial, nullptr, COPIED},
    {"MSCKF_HIP_LITERAL_TIMERS", &Settings::lit_timers, nullptr, KEPT, FLAG},
    {nullptr, &Settings::ring, nullptr, KEPT},
    {nullptr, &Settings::up_mode, nullptr, KEPT},
    {"MSCKF_HIP_TEST_FAIL_UPLOAD", &Settings::test_fail_upload, nullptr, KEPT},
    {"MSCKF_HIP_ROCTX"},          // read on first use (Roctx)
    {"MSCKF_HIP_HOST_THREADS"},   // read by every parallel_for
    {"MSCKF_HIP_CYCLE_TIMERS"},   // read once (host_image_cycle)
};

inline void Settings::take_over(const Settings& o) {
  for (const SettingRow& r : SETTINGS_TABLE) {
    if (r.copied != COPIED) continue;
    if (r.field) this->*r.field = o.*r.field;
    if (r.dfield) this->*r.dfield = o.*r.dfield;
  }
}

// The order of a frame's first launches in run_frames (msckf_hip_set_frame_order; routes::frame_order in frame_order.h reads
// it).  A record of its own beside Settings, whose fields, size and table tests/cpp/settings_host.cpp holds as they are: no
// environment variable, only the setter changes it, and a copy of the handle takes it over like every setting that decides
// which kernels run (same bits either way).
struct FrameSettings {
  int order = 1;   // 1: k_feature first, then selection and propagate + augmentState in one launch, on the frames that allow it; 0: propagate first on every frame
  // msckf_hip_set_frame_order_chol, under order 1: on the frames that allow it (routes::frame_order_chol) the selection keeps its
  // own launch and propagate + augmentState run inside the Gram Cholesky's launch -- "order 2"; 0: order 1 as it was
  int in_cholesky = 1;
  int effective() const { return order ? (in_cholesky ? 2 : 1) : 0; }   // the order routes::frame_order_chol is asked with
  void take_over(const FrameSettings& o) { order = o.order; in_cholesky = o.in_cholesky; }
};

// the environment's say on a new handle's settings; false: a value was refused, err says which
inline bool settings_from_env(Settings& s, std::string& err) {
  for (const SettingRow& r : SETTINGS_TABLE) {
    const char* e = (r.env && r.field) ? getenv(r.env) : nullptr;
    if (!e) continue;
    const int v = r.flag == FLAG ? atoi(e) != 0 : atoi(e);
    bool ok = r.n_allowed == 0;
    for (int i = 0; i < r.n_allowed; ++i) ok = ok || v == r.allowed[i];
    if (!ok) { err = r.refusal; return false; }
    s.*r.field = v;
  }
  return true;
}

}   // namespace msckf_settings
#endif
