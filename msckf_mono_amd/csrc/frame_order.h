// frame_order.h -- in which order a frame of run_frames enqueues its first launches, stated once and free of device calls.
//
// The frame step's own order is propagate + augmentState, k_feature, selection, ... (propagate first).  k_feature reads
// only what the previous frame's prune left -- camera states and P blocks of the slots below the newest one, gravity, the
// window size "after the next augment" in ncam_upd -- unless a track observes the camera state this frame's augmentState adds.
// feature_ahead says whether that holds for every trajectory of a slice's frame; two callers ask it:
//   * set_feature_overlap's side stream (the early k_feature of Batch<S>::enqueue_frame), and
//   * frame_order, the feature-first order: k_feature, then ONE launch with the selection's workgroups and
//     the propagate + augmentState workgroups side by side (k_propagate's HEAD instance, kernels_state.hip), then the rest of the update.
// No HIP header: a host compiler accepts this file on its own (tests/cpp/frame_order_host.cpp prints the decision over a grid).
#ifndef MSCKF_FRAME_ORDER_H
#define MSCKF_FRAME_ORDER_H

#include <cstddef>

namespace msckf {
namespace routes {

// why a slice's frame keeps the propagate-first order; FO_TAKEN: it does not
enum FrameOrderRefusal {
  FO_TAKEN = 0,
  FO_SETTING,       // the handle does not ask for it (msckf_hip_set_frame_order), or asks for the side-stream overlap instead
  FO_SCALAR,        // a double handle: its propagate body needs 254 registers, the joint launch would spill or lose residency
  FO_ROUTE,         // the update's selection is not k_select_diag's launch (Householder TSQR route), or the range mixes
                    // diagonal and full Q_imu (two propagate launches)
  FO_FIRST_FRAME,   // the call's first frame: the previous call need not have ended with a prune, ncam_upd may be stale
  FO_PROFILE,       // the stage profile times propagate, augment, features and selection apart
  FO_WINDOW_FULL,   // a trajectory's window is full: augmentState adds nothing (it reports STAT_ERR_NCAP), ncam_upd is one too many
  FO_SKIPPED,       // a skipped cell: no augmentState on this frame, ncam_upd is one too many
  FO_NEWEST_SEEN    // a track of the frame observes the camera state that augmentState is about to add
};
inline const char* frame_order_text(FrameOrderRefusal r) {
  switch (r) {
    case FO_TAKEN: return "feature_first";
    case FO_SETTING: return "setting";
    case FO_SCALAR: return "double";
    case FO_ROUTE: return "route";
    case FO_FIRST_FRAME: return "first_frame";
    case FO_PROFILE: return "profile";
    case FO_WINDOW_FULL: return "window_full";
    case FO_SKIPPED: return "skipped";
    case FO_NEWEST_SEEN: return "newest_seen";
  }
  return "?";
}

// May the frame's k_feature run before its augmentState, for EVERY trajectory of the range?  ncam: the host mirror of the window
// sizes before the frame; maxslot: the largest camera slot of each trajectory's work-list (-1: none); k: the cells' sample
// counts, skip_mark where the cell has no image.  The first trajectory that refuses names the reason.
inline FrameOrderRefusal feature_ahead(int nb, const int* ncam, const int* maxslot, const int* k, int skip_mark, int n_cap, bool first_frame, bool prof) {
  if (first_frame) return FO_FIRST_FRAME;
  if (prof) return FO_PROFILE;
  for (int i = 0; i < nb; ++i) {
    if (ncam[i] >= n_cap) return FO_WINDOW_FULL;
    if (k[i] == skip_mark) return FO_SKIPPED;
    const int n_after = ncam[i] + 1;                 // (<= n_cap)
    if (maxslot[i] > n_after - 2) return FO_NEWEST_SEEN;
  }
  return FO_TAKEN;
}

// Does the slice's frame take the feature-first order?  setting: msckf_hip_set_frame_order; overlap_feature: the side-stream
// setting (it owns the early k_feature when on); select_diag: routes::compress_route's; qroute: launch_propagate's (0 | 1 | 2).
inline FrameOrderRefusal frame_order(int setting, int overlap_feature, size_t scalar, bool select_diag, int qroute,
                                     int nb, const int* ncam, const int* maxslot, const int* k, int skip_mark, int n_cap, bool first_frame, bool prof) {
  if (!setting || overlap_feature) return FO_SETTING;
  if (scalar != 4) return FO_SCALAR;
  if (!select_diag || qroute == 1) return FO_ROUTE;
  return feature_ahead(nb, ncam, maxslot, k, skip_mark, n_cap, first_frame, prof);
}

// ---------------------------------------------------------------- order 2: propagate + augmentState inside the Gram Cholesky's launch
// The frame still enqueues k_feature first; the selection keeps a launch of its own (k_select_diag), k_gram follows, and
// propagate + augmentState ride in the one-level Gram Cholesky's launch, one workgroup per trajectory beside the factorization's
// (k_propagate's CHOL instances, kernels_state.hip).  The selection, k_gram and the Cholesky take the window size from ncam_upd.
// Nothing reads what propagate + augmentState write before the PHt product, the launch behind.
// why a slice's frame that could take it keeps order 1 (or 0); FC_TAKEN: it does not
enum FrameOrderCholRefusal {
  FC_TAKEN = 0,
  FC_SETTING,      // the handle asks for order 0 (msckf_hip_set_frame_order) or switched the form off (msckf_hip_set_frame_order_chol)
  FC_ORDER1,       // order 1 is not taken (frame_order names the reason): nothing has run k_feature ahead of augmentState
  FC_LEVELS,       // the compression is not the information form with a ONE-level Cholesky (TSQR, or two levels beyond 192 columns:
                   // its first level is followed by k_trsm_rows, and only the CH_GRAM instances have the joint form)
  FC_SMALL,        // some trajectory of the slice's frame has its update in k_update_small: no Cholesky launch to ride in
                   // (SMALL_ONLY), or one that leaves the small trajectories' workgroups at once (SMALL_AND_CHAIN)
  FC_LITERAL       // a trajectory of the batch is on the literal anisotropic route: its launches sit between k_gram and the Cholesky
};
inline const char* frame_order_chol_text(FrameOrderCholRefusal r) {
  switch (r) {
    case FC_TAKEN: return "in_cholesky";
    case FC_SETTING: return "setting";
    case FC_ORDER1: return "order1_refused";
    case FC_LEVELS: return "chol_levels";
    case FC_SMALL: return "small_update";
    case FC_LITERAL: return "literal";
  }
  return "?";
}
// Does the slice's frame take order 2?  setting: the handle's effective order (FrameSettings::effective: 2 asks for it, the default); order1: frame_order's answer for the
// same frame; info, chol_levels: routes::compress_route's; chain_only: routes::small_route's kind is CHAIN_ONLY for the slice's
// frame; n_lit: trajectories of the batch on the literal anisotropic route.
inline FrameOrderCholRefusal frame_order_chol(int setting, FrameOrderRefusal order1, bool info, int chol_levels, bool chain_only, int n_lit) {
  if (setting < 2) return FC_SETTING;
  if (order1 != FO_TAKEN) return FC_ORDER1;
  if (!info || chol_levels != 1) return FC_LEVELS;
  if (!chain_only) return FC_SMALL;
  if (n_lit > 0) return FC_LITERAL;
  return FC_TAKEN;
}

}  // namespace routes
}  // namespace msckf
#endif
