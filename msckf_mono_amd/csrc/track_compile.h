// track_compile.h -- a recorded feature-id stream compiled into the positional cells the frame loops take, free of device calls.
//
// The frame loops (run_frames / _streamed / _replay) take per image a work-list (M, slots, obs) and a drop count.  A recording
// arrives as ids: the tracked and the new features of every image (the reference's front-end output).  Without
// pruneRedundantStates, what turns one into the other -- update(), addFeatures(), marginalize()'s work-list, pruneEmptyStates()
// (msckf.h:215-332, 336-371, 685-717) -- reads ids and three integers and nothing of the filter's estimate, so it runs here once,
// offline, on one HostTraj that never meets a device.  No rule is restated: every step is host_lists.h's, called in
// host_image_cycle's order with flags = 2 (pruneEmptyStates, no pruneRedundantStates):
//   begin_image -> update_lists -> add_features_lists -> build_worklist -> plan_prune_empty -> retire_plan_leading / retire_commit
// pruneRedundantStates cannot be compiled: find_redundant reads the estimated camera poses (msckf.h:1049-1098).
// No HIP header, no batch type: a host compiler accepts this file on its own (tests/cpp/track_compile_host.cpp).
#ifndef MSCKF_TRACK_COMPILE_H
#define MSCKF_TRACK_COMPILE_H

#include <cstdint>
#include <vector>

#include "host_lists.h"

namespace msckf_compile {

struct Refusal { int code; const char* why; };
// what one image left: its work-list's tracks and entries, the leading camera states pruneEmptyStates removes, the window after
// the augment (before that drop), the tracks still live (msckf_hip_compile_image's out5, in this order)
struct ImageSummary { int F, entries, n_drop, window, live; };

struct Compiler {
  msckf_lists::HostTraj t;
  msckf_lists::WorkList wl;          // the last image's work-list, in feature_tracks_to_residualize_ order
  std::vector<uint64_t> ids;         // its tracks' feature ids
  bool broken = false;               // a refused addFeatures left the lists half-changed
  int next_state_id = 0;             // the compiler's own camera ids: ascending, never reused

  static Refusal create_refusal(int max_cam_states, int min_track_length, int max_track_length) {
    if (max_cam_states <= 0 || min_track_length <= 0 || max_track_length <= 0) return {-EINVAL, "max_cam_states, min_track_length and max_track_length must be positive"};
    return {0, nullptr};
  }
  Compiler(int max_cam_states, int min_track_length, int max_track_length) {
    t.initialized = true;
    t.max_cam_states = max_cam_states; t.min_track_length = min_track_length; t.max_track_length = max_track_length;
  }
  // in this order: the compiler's state, the counts, the pointers
  Refusal image_refusal(const double* upd_meas, const uint64_t* upd_ids, int upd_n, const double* new_meas, const uint64_t* new_ids, int new_n) const {
    if (broken) return {-EIO, "the compiler is unusable after a refused image"};
    if (upd_n < 0 || new_n < 0) return {-EINVAL, "negative feature count"};
    if ((upd_n > 0 && (!upd_meas || !upd_ids)) || (new_n > 0 && (!new_meas || !new_ids))) return {-EINVAL, "null feature list with a positive count"};
    return {0, nullptr};
  }
  // one image: augmentState's host half, update, addFeatures, marginalize's work-list, pruneEmptyStates
  Refusal image(const double* upd_meas, const uint64_t* upd_ids, int upd_n, const double* new_meas, const uint64_t* new_ids, int new_n, ImageSummary& out) {
    using namespace msckf_lists;
    if (const Refusal r = image_refusal(upd_meas, upd_ids, upd_n, new_meas, new_ids, new_n); r.code) return r;
    begin_image(t, next_state_id++, 0.0);
    update_lists(t, upd_meas, upd_ids, upd_n);
    if (add_features_lists(t, new_meas, new_ids, new_n)) { broken = true; return {-EEXIST, "added new feature that was already being tracked"}; }
    build_worklist(t.to_resid, wl);
    ids.clear();
    for (const TrackToResid& r : t.to_resid) ids.push_back(r.id);
    out.F = (int)wl.M.size(); out.entries = (int)wl.slots.size(); out.window = (int)t.cams.size();
    const int last_to_remove = plan_prune_empty(t);
    out.n_drop = last_to_remove + 1;
    if (last_to_remove >= 0) {
      // (pruned_states_ keeps the pose of a state that goes; a compiler has none and keeps no record)
      const std::vector<double> no_poses((size_t)7 * t.cams.size(), 0.0);
      Retirement ret;
      retire_plan_leading(t, no_poses.data(), last_to_remove, ret);
      retire_commit(t, ret);
      t.pruned.clear();
    }
    out.live = (int)t.tracks.size();
    return {0, nullptr};
  }
  // the last image's work-list into the caller's arrays; the capacities first
  Refusal cell_refusal(int cap_tracks, int cap_entries) const {
    if (broken) return {-EIO, "the compiler is unusable after a refused image"};
    if (cap_tracks < 0 || cap_entries < 0) return {-EINVAL, "negative capacity"};
    if ((size_t)cap_tracks < wl.M.size() || (size_t)cap_entries < wl.slots.size()) return {-E2BIG, "the work-list exceeds the caller's capacities"};
    return {0, nullptr};
  }
};

}  // namespace msckf_compile

#endif  // MSCKF_TRACK_COMPILE_H
