// host_lists.h -- the per-trajectory host bookkeeping of the filter, free of device calls.
//
// What the reference keeps on the host side of its hot loop -- the integer / std::find bookkeeping of MSCKF::update /
// addFeatures / removeTrackedFeature / marginalize's work-list / pruneRedundantStates / pruneEmptyStates (msckf.h:215-332,
// 336-371, 453-717, 1049-1098, 1469-1485) -- as list surgery on one HostTraj plus plain arrays that came back from the device.
// Every rule is stated once here; the drivers of msckf_hip.hip (one trajectory with single calls, or a range in lockstep)
// differ only in how they talk to the device.  No HIP header, no batch type: a host compiler accepts this file on its own.
// A step that can fail returns a negative errno code; the driver words the message.
#ifndef MSCKF_HOST_LISTS_H
#define MSCKF_HOST_LISTS_H

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace msckf_lists {

struct CamMeta { int state_id; double time; int last_correlated_id; std::vector<uint64_t> tracked; };
struct PrunedState { int state_id; double time; int last_correlated_id; double pose[7]; };   // camState at the moment it was pruned (msckf.h:631,714)
struct Track { uint64_t id; std::vector<double> obs; std::vector<int> cam_ids; bool initialized = false; double p_f_G[3] = {0, 0, 0}; };
struct TrackToResid { uint64_t id; std::vector<double> obs; std::vector<int> slots; };
struct HostTraj {
  bool initialized = false;
  int max_cam_states = 0, min_track_length = 0, max_track_length = 0;
  double redundancy_angle_thresh = 0, redundancy_distance_thresh = 0;
  std::vector<CamMeta> cams;
  std::vector<Track> tracks;
  std::vector<uint64_t> tracked_ids;
  std::vector<TrackToResid> to_resid;
  std::vector<PrunedState> pruned;
  std::vector<double> map;   // xyz triples of the last marginalize
  int map_pending = 0;       // > 0: the last marginalize()'s triangulated points of this many tracks are still on the device
                             // (read back when somebody asks -- getMap(), pruneRedundantStates(), a copy -- or dropped by the next marginalize())
  int wl_F = 0;              // tracks in the device work-list of this trajectory
};
// one trajectory's tracks for the device: observations per track, camera slots and coordinates track after track
struct WorkList {
  std::vector<int> M, slots; std::vector<double> obs;
  void clear() { M.clear(); slots.clear(); obs.clear(); }
};
// the per-track status bits of the feature kernel that the bookkeeping reads (dev_common.h: ST_*; msckf_hip.hip asserts the match)
enum { TRK_MOTION_OK = 1, TRK_TRI_VALID = 2, TRK_MOTION_SKIPPED = 16 };

// The rule for one scenario cell's IMU sample count k (0 .. K of the scenario) and its flags (CELL_SKIP: the trajectory's
// sequence has no image on this frame, so the cell carries nothing): null when the cell is acceptable, else why it is not
enum { CELL_SKIP = 1 };
inline const char* cell_refusal(int k, int K, int F, int n_drop, int flags) {
  if (flags & ~CELL_SKIP) return "unknown cell flag bit";
  if (k < 0) return "negative IMU sample count k";
  if (k > K) return "IMU sample count k exceeds the scenario's K (msckf_hip_scenario_alloc)";
  if ((flags & CELL_SKIP) && (k != 0 || F != 0 || n_drop != 0)) return "a skipped cell carries no IMU samples, no tracks and no drop";
  return nullptr;
}

// The pruned-state log's host mirror: which image's camera a record is.  The frame loop drops oldest-first, so per trajectory
// fifo holds the augment ordinals of the states in the window, oldest first (-1: a state that was there at enable / reset
// time or came in through another call), and aug the popped ordinal of every stored record.  ncam: the host mirror of the
// window sizes.  An empty mirror (the log is off) takes every step as a no-op.
struct PrunedFifo {
  std::vector<std::vector<int>> fifo, aug;
  void clear() { fifo.clear(); aug.clear(); }
  // no records, and a window of unknown states: the log was enabled or reset
  void start(const std::vector<int>& ncam) { fifo.assign(ncam.size(), std::vector<int>()); aug.assign(ncam.size(), std::vector<int>()); forget(ncam); }
  // every state in the window becomes one whose image is unknown (ordinal -1)
  void forget(const std::vector<int>& ncam) { for (size_t b = 0; b < fifo.size(); ++b) fifo[b].assign(ncam[b], -1); }
  // a trajectory whose window changed size behind the log's back (any call but the frame loop) holds unknown states
  void resync(const std::vector<int>& ncam) { for (size_t b = 0; b < fifo.size(); ++b) if ((int)fifo[b].size() != ncam[b]) fifo[b].assign(ncam[b], -1); }
  // one cell of the frame loop, where the window size takes the same steps: the augment pushes the frame's ordinal, the drop
  // pops the nd oldest into the ordinals of the records the frame stores -- as long as the log's capacity lasts
  void mirror(int b, bool augmented, int nd, int ordinal, int cap) {
    std::vector<int>& q = fifo[b];
    if (augmented) q.push_back(ordinal);
    for (int k = 0; k < nd; ++k) if ((int)aug[b].size() < cap) aug[b].push_back(q[k]);
    q.erase(q.begin(), q.begin() + nd);
  }
};

inline void remove_tracked_feature(HostTraj& t, uint64_t fid, std::vector<int>& slots) {
  slots.clear();
  for (size_t c = 0; c < t.cams.size(); ++c) {
    auto& ids = t.cams[c].tracked;
    auto it = std::find(ids.begin(), ids.end(), fid);
    if (it != ids.end()) { ids.erase(it); slots.push_back((int)c); }
  }
}

// augmentState's host half (msckf.h:148-149): the new camera state joins the window and map_ is cleared -- the points of the
// previous marginalize() still on the device belong to the map just cleared
inline void begin_image(HostTraj& t, int state_id, double time) {
  t.cams.push_back(CamMeta{state_id, time, -1, {}});
  t.map.clear(); t.map_pending = 0;
}

// key -> int table without a heap node per key (open addressing, power-of-two capacity, one instance per host thread reused
// from call to call): the bookkeeping below makes a few hundred to a few thousand look-ups per image and trajectory, and a
// std::unordered_map's allocations were most of their cost
struct FlatIndex {
  std::vector<uint64_t> key; std::vector<int> val; unsigned shift = 64; size_t mask = 0;
  void reset(size_t n) {
    size_t cap = 16; unsigned lg = 4;
    while (cap < 2 * n + 2) { cap <<= 1; ++lg; }
    if (key.size() < cap) key.resize(cap);
    val.assign(cap, -1);
    mask = cap - 1; shift = 64 - lg;
  }
  size_t slot(uint64_t k) const { return (size_t)((k * 0x9E3779B97F4A7C15ull) >> shift) & mask; }
  // keeps the FIRST value given for a key (std::find returns the first occurrence); returns the value held
  int insert_first(uint64_t k, int v) {
    for (size_t s = slot(k);; s = (s + 1) & mask) {
      if (val[s] < 0) { key[s] = k; val[s] = v; return v; }
      if (key[s] == k) return val[s];
    }
  }
  int find(uint64_t k) const {
    for (size_t s = slot(k);; s = (s + 1) & mask) {
      if (val[s] < 0) return -1;
      if (key[s] == k) return val[s];
    }
  }
};

// update(), msckf.h:215-300, with the reference's results and none of its quadratic searches.  The reference looks every tracked
// feature up in the incoming ids by linear search (:226), removes an ended feature from every camera state's list by linear
// search + erase (removeTrackedFeature :1469-1485) and erases the ended tracks one by one (:283-298): O(tracked x incoming) +
// O(ended x cameras x tracked) per image -- 43 us of the single filter's 286 us at 50 features per image (round-5 verdict), tens of
// milliseconds per filter at the benchmark's 200.  Here: one table of the incoming ids (first occurrence, as std::find
// returns), one table "ended feature -> camera slots that list it" built from the lists as they stand after this image's
// registrations, ONE stable filter pass per camera list and per track list.  Every list ends in the order the reference leaves it.
// (t.cams is not empty: the caller checks.)
inline void update_lists(HostTraj& t, const double* meas, const uint64_t* ids, int n) {
  t.to_resid.clear();
  static thread_local FlatIndex first, where;
  first.reset((size_t)n);
  for (int k = 0; k < n; ++k) first.insert_first(ids[k], k);                  // keeps the first occurrence (std::find, :226)
  // pass 1 (:224-247): register this image's observation; which tracks end here
  const size_t nt = t.tracked_ids.size();
  static thread_local std::vector<char> ended;
  ended.assign(nt, 0);
  size_t n_ended = 0;
  for (size_t i = 0; i < nt; ++i) {
    const uint64_t fid = t.tracked_ids[i];
    Track& tr = t.tracks[i];
    const int k = first.find(fid);
    const bool valid = k >= 0;
    if (valid) {
      tr.obs.push_back(meas[2 * (size_t)k]); tr.obs.push_back(meas[2 * (size_t)k + 1]);
      t.cams.back().tracked.push_back(fid);
      tr.cam_ids.push_back(t.cams.back().state_id);
    }
    if (!valid || tr.obs.size() / 2 >= (size_t)t.max_track_length) { ended[i] = 1; ++n_ended; }
  }
  if (!n_ended) return;
  // pass 2 (:249-265 + removeTrackedFeature): the camera slots that list an ended feature, in camera order
  where.reset(n_ended);
  std::vector<std::vector<int>> slots_of(n_ended);
  {
    int e = 0;
    for (size_t i = 0; i < nt; ++i) if (ended[i]) where.insert_first(t.tracked_ids[i], e++);
  }
  for (size_t c = 0; c < t.cams.size(); ++c) {
    auto& lst = t.cams[c].tracked;
    size_t w = 0;
    for (size_t r = 0; r < lst.size(); ++r) {
      const int e = where.find(lst[r]);
      if (e >= 0 && (slots_of[e].empty() || slots_of[e].back() != (int)c)) { slots_of[e].push_back((int)c); continue; }   // first occurrence in this list leaves it
      lst[w++] = lst[r];
    }
    lst.resize(w);
  }
  {
    int e = 0;
    for (size_t i = 0; i < nt; ++i) {
      if (!ended[i]) continue;
      Track& tr = t.tracks[i];
      std::vector<int>& slots = slots_of[e++];
      if (slots.size() >= (size_t)t.min_track_length) {
        TrackToResid r;
        r.id = tr.id; r.obs = std::move(tr.obs); r.slots = std::move(slots);   // (the track is erased below: its observations move, they are not copied)
        t.to_resid.push_back(std::move(r));
      }
    }
  }
  // pass 3 (:283-298): last_correlated_id of the camera states an ended track leaves empty, then the tracks themselves
  for (size_t i = 0; i < nt; ++i) {
    if (!ended[i] || t.tracks[i].cam_ids.empty()) continue;
    const int last_id = t.tracks[i].cam_ids.back();
    for (int idx : t.tracks[i].cam_ids)
      for (auto& cs : t.cams)
        if (cs.state_id == idx) { if (cs.tracked.empty()) cs.last_correlated_id = last_id; break; }
  }
  {
    size_t w = 0;
    for (size_t i = 0; i < nt; ++i) {
      if (ended[i]) continue;
      if (w != i) { t.tracks[w] = std::move(t.tracks[i]); t.tracked_ids[w] = t.tracked_ids[i]; }
      ++w;
    }
    t.tracks.resize(w); t.tracked_ids.resize(w);
  }
}

// addFeatures(), msckf.h:302-332.  -EEXIST: a new id is already being tracked (:328-329 prints and returns); the features
// before it stay added.  (t.cams is not empty: the caller checks.)
inline int add_features_lists(HostTraj& t, const double* meas, const uint64_t* ids, int n) {
  static thread_local FlatIndex known;
  known.reset(t.tracked_ids.size() + (size_t)n);
  for (size_t i = 0; i < t.tracked_ids.size(); ++i) known.insert_first(t.tracked_ids[i], (int)i);
  for (int i = 0; i < n; ++i) {
    if (known.find(ids[i]) >= 0) return -EEXIST;
    known.insert_first(ids[i], (int)t.tracked_ids.size());
    Track tr; tr.id = ids[i];
    tr.obs.push_back(meas[2 * i]); tr.obs.push_back(meas[2 * i + 1]);
    t.cams.back().tracked.push_back(ids[i]);
    tr.cam_ids.push_back(t.cams.back().state_id);
    t.tracks.push_back(std::move(tr));
    t.tracked_ids.push_back(ids[i]);
  }
  return 0;
}

// marginalize(), msckf.h:336-449: feature_tracks_to_residualize_ as the device's positional work-list
inline void build_worklist(const std::vector<TrackToResid>& to_resid, WorkList& wl) {
  wl.clear();
  for (const TrackToResid& r : to_resid) {
    wl.M.push_back((int)r.slots.size());
    wl.slots.insert(wl.slots.end(), r.slots.begin(), r.slots.end());
    wl.obs.insert(wl.obs.end(), r.obs.begin(), r.obs.end());
  }
}

// msckf.h:371 (map_.push_back(p_f_G)): the triangulated points of the F tracks of a marginalize that got as far as a valid
// triangulation (status: the feature kernel's bits per track, pf3: xyz per track)
inline void append_map(HostTraj& t, const int* status, const double* pf3, int F) {
  for (int k = 0; k < F; ++k)
    if ((status[k] & (TRK_MOTION_SKIPPED | TRK_MOTION_OK)) && (status[k] & TRK_TRI_VALID)) t.map.insert(t.map.end(), pf3 + 3 * k, pf3 + 3 * k + 3);
}

// findRedundantCamStates, msckf.h:1049-1098 (poses7: n x 7 = q_CG(w,x,y,z) p_C_G); rm: sorted state ids, empty or at least two
inline void find_redundant(const HostTraj& t, const double* poses7, std::vector<int>& rm) {
  const int n = (int)t.cams.size();
  if (n < 5) return;
  auto qp = [&](int i) { return poses7 + 7 * i; };
  int kf = 0;
  const int prot = n - 3;
  int next = 1;
  while (next != prot) {
    const double* a = qp(kf); const double* c = qp(next);
    const double dx = c[4] - a[4], dy = c[5] - a[5], dz = c[6] - a[6];
    const double distance = std::sqrt(dx * dx + dy * dy + dz * dz);
    // Eigen angularDistance: d = kf_q * conj(cam_q); 2*atan2(|vec(d)|, |d.w|)
    const double aw = a[0], ax = a[1], ay = a[2], az = a[3], bw = c[0], bx = -c[1], by = -c[2], bz = -c[3];
    const double dw = aw * bw - ax * bx - ay * by - az * bz;
    const double vx = aw * bx + ax * bw + ay * bz - az * by, vy = aw * by + ay * bw + az * bx - ax * bz, vz = aw * bz + az * bw + ax * by - ay * bx;
    const double angle = 2 * std::atan2(std::sqrt(vx * vx + vy * vy + vz * vz), std::fabs(dw));
    if (distance < t.redundancy_distance_thresh && angle < t.redundancy_angle_thresh) rm.push_back(t.cams[next].state_id);
    else kf = next;
    ++next;
    if (n - (int)rm.size() <= t.max_cam_states) break;
  }
  const int over = (n - (int)rm.size()) - t.max_cam_states;
  for (int i = 0; i < over; i++)
    if (std::find(rm.begin(), rm.end(), t.cams[i].state_id) == rm.end()) rm.push_back(t.cams[i].state_id);
  if (rm.size() < 2) rm.clear();
  std::sort(rm.begin(), rm.end());
}

// the camera states of rm that observed the track, in rm's order
inline std::vector<int> involved_of(const Track& tr, const std::vector<int>& rm) {
  std::vector<int> inv;
  for (int cam_id : rm) if (std::find(tr.cam_ids.begin(), tr.cam_ids.end(), cam_id) != tr.cam_ids.end()) inv.push_back(cam_id);
  return inv;
}
inline int slot_of(const HostTraj& t, int cam_id) {
  for (size_t i = 0; i < t.cams.size(); ++i) if (t.cams[i].state_id == cam_id) return (int)i;
  return -1;
}
inline void erase_involved(Track& tr, const std::vector<int>& involved) {
  for (int cam_id : involved) {
    auto it = std::find(tr.cam_ids.begin(), tr.cam_ids.end(), cam_id);
    if (it != tr.cam_ids.end()) {
      const size_t idx = (size_t)(it - tr.cam_ids.begin());
      tr.cam_ids.erase(it);
      tr.obs.erase(tr.obs.begin() + 2 * idx, tr.obs.begin() + 2 * idx + 2);
    }
  }
}

// MSCKF::pruneRedundantStates, msckf.h:453-682, host side.  The driver runs, per trajectory:
//   redundant_select            -> device: checkMotion + triangulation of cand_wl (if any)
//   redundant_apply_candidates
//   redundant_second_update     -> device: stored positions + second measurement update of wl (if any)
//   redundant_finish            -> device: poses, prune of plan.rm (retire_plan / retire_commit)
// With no camera state to remove (plan.rm empty) every step is a no-op and both work-lists come back empty.
struct RedundantPlan {
  std::vector<int> rm;            // state ids to remove, sorted
  std::vector<size_t> cand;       // tracks not yet initialized with >= 2 involved states: need motion check + triangulation
  std::vector<size_t> used;       // tracks of the second update
};

// keyframe selection and the first loop (:466-495): a track with one involved state loses that observation, the candidates go
// to cand_wl with their camera states in camera order (feature_associated_cam_states).  -E2BIG: more candidates than f_cap
inline int redundant_select(HostTraj& t, const double* poses7, int f_cap, RedundantPlan& plan, WorkList& cand_wl) {
  plan.rm.clear(); plan.cand.clear(); plan.used.clear(); cand_wl.clear();
  find_redundant(t, poses7, plan.rm);
  if (plan.rm.empty()) return 0;
  for (size_t i = 0; i < t.tracks.size(); ++i) {
    Track& tr = t.tracks[i];
    const std::vector<int> inv = involved_of(tr, plan.rm);
    if (inv.empty()) continue;
    if (inv.size() == 1) { erase_involved(tr, inv); continue; }
    if (!tr.initialized) plan.cand.push_back(i);
  }
  if (plan.cand.size() > (size_t)f_cap) return -E2BIG;
  for (size_t ci : plan.cand) {
    const Track& tr = t.tracks[ci];
    int m = 0;
    for (size_t p = 0; p < t.cams.size(); ++p) {
      auto it = std::find(tr.cam_ids.begin(), tr.cam_ids.end(), t.cams[p].state_id);
      if (it == tr.cam_ids.end()) continue;
      const size_t k = (size_t)(it - tr.cam_ids.begin());
      cand_wl.slots.push_back((int)p); cand_wl.obs.push_back(tr.obs[2 * k]); cand_wl.obs.push_back(tr.obs[2 * k + 1]); ++m;
    }
    cand_wl.M.push_back(m);
  }
  return 0;
}

// :496-528 with the device's answer for cand_wl: a candidate that failed checkMotion or the triangulation loses its involved
// observations, the others are initialized with their point, which also joins the map
inline void redundant_apply_candidates(HostTraj& t, const RedundantPlan& plan, const int* status, const double* pf3) {
  for (size_t c = 0; c < plan.cand.size(); ++c) {
    Track& tr = t.tracks[plan.cand[c]];
    const double* pc = pf3 + 3 * c;
    if (!((status[c] & TRK_MOTION_OK) && (status[c] & TRK_TRI_VALID))) erase_involved(tr, involved_of(tr, plan.rm));
    else { tr.initialized = true; std::copy(pc, pc + 3, tr.p_f_G); t.map.insert(t.map.end(), pc, pc + 3); }
  }
}

// second loop (:545-607): the involved observations of every track that still has some, and the track's stored p_f_G
// (pf3: room for f_cap triples).  -E2BIG: more such tracks than f_cap -- checked before anything of the track is written
inline int redundant_second_update(const HostTraj& t, RedundantPlan& plan, int f_cap, WorkList& wl, double* pf3) {
  wl.clear();
  if (plan.rm.empty()) return 0;
  for (size_t i = 0; i < t.tracks.size(); ++i) {
    const Track& tr = t.tracks[i];
    const std::vector<int> inv = involved_of(tr, plan.rm);
    if (inv.empty()) continue;
    if (wl.M.size() >= (size_t)f_cap) return -E2BIG;
    for (int cam_id : inv) {
      const size_t k = (size_t)(std::find(tr.cam_ids.begin(), tr.cam_ids.end(), cam_id) - tr.cam_ids.begin());
      wl.slots.push_back(slot_of(t, cam_id)); wl.obs.push_back(tr.obs[2 * k]); wl.obs.push_back(tr.obs[2 * k + 1]);
    }
    std::copy(tr.p_f_G, tr.p_f_G + 3, pf3 + 3 * wl.M.size());
    wl.M.push_back((int)inv.size());
    plan.used.push_back(i);
  }
  return 0;
}

// :596-606: the tracks of the second update lose their involved observations
inline void redundant_finish(HostTraj& t, const RedundantPlan& plan) {
  for (size_t i : plan.used) erase_involved(t.tracks[i], involved_of(t.tracks[i], plan.rm));
}

// pruneEmptyStates, msckf.h:685-717: the leading camera states 0 .. last_to_remove go (-1: nothing to prune)
inline int plan_prune_empty(const HostTraj& t) {
  const int max_states = t.max_cam_states, num = (int)t.cams.size();
  if (num < max_states || !t.cams.front().tracked.empty()) return -1;
  int last_to_remove = num - max_states - 1;
  for (int i = 1; i < num - max_states; i++)
    if (!t.cams[i].tracked.empty()) { last_to_remove = i - 1; break; }
  return last_to_remove;
}

// Retiring camera states (:616-681, :704-717) in two halves, so that the host lists change only once the device has pruned:
// retire_plan records the states that go as pruned_states_ keeps them (the whole camState, pose as read from the device:
// poses7 = n x 7) and the ascending slots that stay; retire_commit applies that to the trajectory.
struct Retirement { std::vector<PrunedState> pruned; std::vector<int> keep; };
template <class Removed> void retire_plan(const HostTraj& t, const double* poses7, Removed removed, Retirement& r) {
  r.pruned.clear(); r.keep.clear();
  for (int i = 0; i < (int)t.cams.size(); ++i) {
    if (!removed(i)) { r.keep.push_back(i); continue; }
    PrunedState ps{t.cams[i].state_id, t.cams[i].time, t.cams[i].last_correlated_id, {0}};
    std::copy(poses7 + 7 * (size_t)i, poses7 + 7 * (size_t)i + 7, ps.pose);
    r.pruned.push_back(ps);
  }
}
inline void retire_plan_ids(const HostTraj& t, const double* poses7, const std::vector<int>& sorted_ids, Retirement& r) {
  retire_plan(t, poses7, [&](int i) { return std::binary_search(sorted_ids.begin(), sorted_ids.end(), t.cams[i].state_id); }, r);
}
inline void retire_plan_leading(const HostTraj& t, const double* poses7, int last_to_remove, Retirement& r) {
  retire_plan(t, poses7, [&](int i) { return i <= last_to_remove; }, r);
}
inline void retire_commit(HostTraj& t, const Retirement& r) {
  if (r.pruned.empty()) return;
  t.pruned.insert(t.pruned.end(), r.pruned.begin(), r.pruned.end());
  std::vector<CamMeta> kept;
  kept.reserve(r.keep.size());
  for (int i : r.keep) kept.push_back(std::move(t.cams[i]));
  t.cams = std::move(kept);
}

}  // namespace msckf_lists

#endif  // MSCKF_HOST_LISTS_H
