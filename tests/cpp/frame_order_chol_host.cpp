// The frame step's order 2 (msckf_mono_amd/csrc/frame_order.h, frame_order_chol) on its own: no HIP header, a host compiler only.
// The rule's inputs come from where the frame step takes them: order 1's answer from frame_order over a slice, the Cholesky's
// levels from routes::compress_route over a handle's geometry, CHAIN_ONLY from routes::small_route over the slice's windows.
// Prints one line per case, "name key=value ... : order1 decision"; tests/test_frame_order_chol.py reads it.
#include <cstdio>
#include <vector>

#include "../../msckf_mono_amd/csrc/frame_order.h"
#include "../../msckf_mono_amd/csrc/update_routes.h"

using namespace msckf::routes;

static const int SKIP = -1, F_CAP = 16;

struct Slice { const char* name; std::vector<int> ncam, maxslot, k; };

// a float or double handle of n_cap cameras; small: MSCKF_HIP_SMALL_UPDATE (columns); override_route: msckf_hip_set_compression (-1 default)
static void print(const Slice& s, int setting, size_t scalar, int n_cap, int small, int override_route, int n_lit, bool first) {
  const int nb = (int)s.ncam.size();
  const Geometry g = geometry(nb, n_cap, F_CAP, n_cap, scalar);
  const int compress = effective_compress(g.compress, override_route, n_lit);
  const CompressRoute cr = compress_route(compress, g.ldR, g.has_Mp, g.lam_parts, 0);
  const FrameOrderRefusal o1 = frame_order(setting, 0, scalar, cr.select_diag, 0, nb, s.ncam.data(), s.maxslot.data(), s.k.data(), SKIP, n_cap, first, false);
  const int limit = small_limit(small, F_CAP, scalar, true);
  const SmallRoute sr = small_route(nb, [&](int i) { return window_cols(s.ncam[i], 1, s.k[i] == SKIP, n_cap); }, limit, compress, n_lit, 0, F_CAP, scalar, true);
  const FrameOrderCholRefusal r = frame_order_chol(setting, o1, cr.info, cr.chol_levels, sr.kind == CHAIN_ONLY, n_lit);
  std::printf("%s setting=%d scalar=%c n_cap=%d small=%d route=%d n_lit=%d first=%d blocks=%d levels=%d kind=%d : %s %s\n", s.name, setting, scalar == 4 ? 'f' : 'd', n_cap,
              small, override_route, n_lit, first ? 1 : 0, cr.nb_a, cr.chol_levels, (int)sr.kind, frame_order_text(o1), frame_order_chol_text(r));
}

int main() {
  // window sizes are those BEFORE the frame's augmentState; the update sees one camera state more
  const Slice steady30{"steady", {29, 29, 29}, {27, 28, 20}, {10, 10, 10}};
  const Slice steady14{"steady", {13, 13, 13}, {12, 11, 12}, {10, 10, 10}};
  const Slice steady10{"steady", {9, 9, 9}, {8, 8, 8}, {10, 10, 10}};
  const Slice steady40{"steady", {39, 39}, {38, 38}, {10, 10}};
  const Slice fill_small{"fill_small", {9, 9, 9}, {8, 8, 8}, {10, 10, 10}};        // 10 cameras at the update: k_update_small's at the default limit
  // (the default limit asks for 84 columns; 72 fit k_update_small at this f_cap -- small_limit, update_routes.h: (15 + n) n <= 7 168)
  const Slice fill_edge{"fill_edge", {11, 11, 11}, {10, 10, 10}, {10, 10, 10}};    // 12 cameras = 72 columns: the last small window
  const Slice fill_over{"fill_over", {12, 12, 12}, {11, 11, 11}, {10, 10, 10}};    // 13 cameras: the chain
  const Slice mixed{"mixed", {16, 16, 11}, {15, 15, 10}, {10, 10, 10}};            // trajectory 2 is k_update_small's, the others the chain's
  const Slice empty{"empty", {0, 0}, {-1, -1}, {10, 10}};                          // one camera state when the update runs: k_update_small's
  const Slice newest{"newest_seen", {29, 29, 29}, {28, 29, 28}, {10, 10, 10}};
  const Slice skipped{"skipped", {29, 29, 29}, {28, 28, -1}, {10, 10, SKIP}};
  const Slice full{"full", {30, 29, 29}, {28, 28, 28}, {10, 10, 10}};
  // every window shape at 30 cameras, default settings
  for (const Slice* s : {&steady30, &fill_small, &fill_edge, &fill_over, &mixed, &empty, &newest, &skipped, &full}) print(*s, 2, 4, 30, 84, -1, 0, false);
  // the joint instances: 4, 8 and 12 column blocks, and the two-level factorization that has none
  print(steady14, 2, 4, 14, 60, -1, 0, false);
  print(steady14, 2, 4, 14, 84, -1, 0, false);     // 14 cameras are beyond the 72 columns that fit: the chain at the default limit too
  print(steady10, 2, 4, 10, 0, -1, 0, false);
  print(steady10, 2, 4, 10, 84, -1, 0, false);
  print(steady40, 2, 4, 40, 84, -1, 0, false);     // 241 columns: two levels
  print(steady40, 2, 4, 60, 84, -1, 0, false);
  // the handle and the call
  print(steady30, 1, 4, 30, 84, -1, 0, false);     // the handle asks for order 1
  print(steady30, 0, 4, 30, 84, -1, 0, false);
  print(steady30, 2, 8, 30, 84, -1, 0, false);     // a double handle
  print(steady30, 2, 4, 30, 84, 0, 0, false);      // Householder TSQR
  print(steady30, 2, 4, 30, 84, -1, 1, false);     // a trajectory on the literal anisotropic route
  print(steady30, 2, 4, 30, 84, 0, 1, false);      // ... which brings the information form back
  print(steady30, 2, 4, 30, 84, -1, 0, true);      // the call's first frame
  print(mixed, 2, 4, 30, 0, -1, 0, false);         // the small update switched off: no slice is mixed
  return 0;
}
