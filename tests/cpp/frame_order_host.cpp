// The frame step's launch order (msckf_mono_amd/csrc/frame_order.h) on its own: no HIP header, a host compiler only.
// Prints one line per case, "name key=value ... : decision", over a grid of slices: every reason to keep the propagate-first
// order, windows that are still filling, full windows, and slices whose trajectories differ.  tests/test_frame_order.py reads it.
#include <cstdio>
#include <vector>

#include "../../msckf_mono_amd/csrc/frame_order.h"

using namespace msckf::routes;

static const int SKIP = -1, N_CAP = 6;

struct Slice { const char* name; std::vector<int> ncam, maxslot, k; };

static void print(const Slice& s, int setting, int overlap, size_t scalar, bool select_diag, int qroute, bool first, bool prof) {
  const int nb = (int)s.ncam.size();
  const FrameOrderRefusal r = frame_order(setting, overlap, scalar, select_diag, qroute, nb, s.ncam.data(), s.maxslot.data(), s.k.data(), SKIP, N_CAP, first, prof);
  const FrameOrderRefusal a = feature_ahead(nb, s.ncam.data(), s.maxslot.data(), s.k.data(), SKIP, N_CAP, first, prof);
  std::printf("%s setting=%d overlap=%d scalar=%c select_diag=%d qroute=%d first=%d prof=%d : %s ahead=%s\n", s.name, setting, overlap, scalar == 4 ? 'f' : 'd',
              select_diag ? 1 : 0, qroute, first ? 1 : 0, prof ? 1 : 0, frame_order_text(r), frame_order_text(a));
}

int main() {
  // window sizes are those BEFORE the frame's augmentState; a track on slot ncam is on the camera state the frame adds
  const Slice slices[] = {
      {"steady", {5, 5, 5}, {4, 4, 3}, {10, 10, 10}},              // windows one below the capacity, newest slot unseen
      {"filling", {2, 3, 1}, {1, 2, 0}, {10, 9, 11}},              // windows that still grow
      {"empty_window", {0, 0}, {-1, -1}, {10, 10}},                // nothing to observe yet
      {"no_tracks", {4, 5}, {-1, -1}, {10, 10}},
      {"full", {6, 6, 6}, {4, 4, 4}, {10, 10, 10}},                // no room for the frame's camera state
      {"one_full", {5, 6, 5}, {4, 4, 4}, {10, 10, 10}},
      {"newest_seen", {5, 5, 5}, {4, 5, 4}, {10, 10, 10}},         // a track of trajectory 1 observes the new camera state
      {"newest_seen_filling", {2, 3}, {2, 2}, {10, 10}},
      {"skipped", {5, 5, 5}, {4, 4, -1}, {10, 10, SKIP}},          // trajectory 2 has no image on this frame
      {"zero_samples", {5, 5}, {4, 4}, {0, 10}},                   // no IMU sample, but an image: augmentState runs
      {"mixed_sizes", {1, 5, 3}, {0, 4, 2}, {10, 10, 10}},         // a slice whose windows differ, all of them allow it
      {"mixed_refusals", {6, 5, 5}, {5, 5, -1}, {10, 10, SKIP}},   // full, then seen, then skipped: the first trajectory names the reason
      {"single", {5}, {4}, {10}},
  };
  for (const Slice& s : slices) print(s, 1, 0, 4, true, 0, false, false);
  // every refusal that does not come from the windows, on a slice that would otherwise take the order
  const Slice& ok = slices[0];
  print(ok, 0, 0, 4, true, 0, false, false);     // the handle asks for order 0
  print(ok, 1, 1, 4, true, 0, false, false);     // the side-stream overlap owns the early k_feature
  print(ok, 1, 0, 8, true, 0, false, false);     // a double handle
  print(ok, 1, 0, 4, false, 0, false, false);    // Householder TSQR route: the selection is k_select's launch
  print(ok, 1, 0, 4, true, 1, false, false);     // diagonal and full Q_imu in one range: two propagate launches
  print(ok, 1, 0, 4, true, 2, false, false);     // every trajectory with a full Q_imu: one launch
  print(ok, 1, 0, 4, true, 0, true, false);      // the call's first frame
  print(ok, 1, 0, 4, true, 0, false, true);      // stage profile on
  print(ok, 1, 0, 4, true, 0, true, true);
  print(ok, 0, 0, 8, false, 1, true, true);      // everything at once: the setting is asked first
  print(slices[6], 1, 0, 8, true, 0, false, false);   // a double handle is refused before its windows are looked at
  return 0;
}
