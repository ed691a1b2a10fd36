// The update's launch routes (msckf_mono_amd/csrc/update_routes.h) on their own: no HIP header, a host compiler only.
// Prints one line per case, "TABLE key=value ... : route", over a grid of handles; each table spans the inputs its function
// takes.  With --runs the same tables are folded without loss: at every key, consecutive grid values whose whole sub-table is
// equal share an entry ("n_cap=11..21", "nb=16..130": the grid's values in that span), the sub-table indented below it.  That
// is the form of tests/golden/update_routes.txt: every threshold shows as the end of one run and the start of the next, and a
// key that a route does not depend on shows as one run over all its values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../msckf_mono_amd/csrc/update_routes.h"

using namespace msckf::routes;

static bool g_runs = false;
struct Row { std::vector<std::string> key; std::string out; };
struct Table {
  const char* name; std::vector<const char*> keys; std::vector<Row> rows;
  // the lines of rows [b, e) from key level l on, runs of equal sub-tables merged
  std::vector<std::string> fold(size_t l, size_t b, size_t e) const {
    if (l == keys.size()) return {": " + rows[b].out};
    std::vector<std::string> lines, prev; std::string first, last;
    auto close = [&]() {
      const std::string label = std::string(keys[l]) + "=" + first + (first == last ? "" : ".." + last);
      bool one = true;   // the sub-table is one entry (a line, or a heading with its own sub-table): it joins this key's line
      for (size_t i = 1; i < prev.size(); ++i) one = one && prev[i].compare(0, 2, "  ") == 0;
      lines.push_back(one ? label + " " + prev[0] : label);
      for (size_t i = one ? 1 : 0; i < prev.size(); ++i) lines.push_back((one ? "" : "  ") + prev[i]);
    };
    for (size_t i = b; i < e;) {
      size_t j = i;
      while (j < e && rows[j].key[l] == rows[i].key[l]) ++j;
      std::vector<std::string> sub = fold(l + 1, i, j);
      if (i != b && sub == prev) last = rows[i].key[l];
      else { if (i != b) close(); prev = sub; first = last = rows[i].key[l]; }
      i = j;
    }
    close();
    return lines;
  }
  void add(std::vector<std::string> key, const std::string& out) { rows.push_back({key, out}); }
  void print() const {
    if (g_runs) { std::printf("%s\n", name); for (auto& x : fold(0, 0, rows.size())) std::printf("  %s\n", x.c_str()); return; }
    for (auto& r : rows) {
      std::printf("%s", name);
      for (size_t l = 0; l < keys.size(); ++l) std::printf(" %s=%s", keys[l], r.key[l].c_str());
      std::printf(" : %s\n", r.out.c_str());
    }
  }
};
static std::string str(int v) { return std::to_string(v); }
template <class... A> static std::string fmt(const char* f, A... a) { char b[256]; std::snprintf(b, sizeof b, f, a...); return b; }
static std::string lim(int v) { return v == ALL_LO ? "lo" : v == ALL_HI ? "hi" : fmt("%d", v); }

static const size_t SCALARS[] = {4, 8};
static const int M_CAPS[] = {4, 12, 30, 31, 40, 45, 46, 47, 60, 62, 63, 64}, F_CAPS[] = {8, 200, 512, 513, 1024, 1025};
static const int BNB[][2] = {{1, 1}, {6, 2}, {64, 16}, {64, 64}, {96, 24}, {128, 128}, {130, 130}};
static std::string sc(size_t s) { return s == 4 ? "f" : "d"; }

static std::string feature_text(const FeatureRoute& r) {
  std::string s = r.n ? "" : "none";
  for (int i = 0; i < r.n; ++i) {
    const FeatureLaunch& l = r.l[i];
    if (i) s += " + ";
    // "(m_lo,m_hi]": the track lengths the launch takes; the pair kernel with its single flag and items, k_feature<LONG> "staged" or not
    if (l.pair) s += fmt("pair lm=%d (%s,%s] single=%d items=%d", l.lm, lim(l.m_lo).c_str(), lim(l.m_hi).c_str(), l.single, l.items);
    else s += fmt("k_feature<%d> lm=%d (%s,%s]%s", l.long_form ? 1 : 0, l.lm, lim(l.m_lo).c_str(), lim(l.m_hi).c_str(), l.staged ? " staged" : "");
  }
  return s;
}
static std::string compress_text(const CompressRoute& r) {
  if (!r.info) return "select tsqr";
  std::string s = fmt("select_diag gram parts=%d ", r.gram_parts);
  if (r.chol_levels == 1) s += fmt("CH_GRAM<%d>", r.nb_a);
  else if (r.chol_levels == 2) s += fmt("CH_GRAM_A<%d> TR_GRAM items=%d CH_GRAM_B<%d>", r.nb_a, r.trsm_items, r.nb_b);
  else s += "none";
  return s;
}
static std::string tsqr_text(const TsqrRoute& r) {
  return fmt("tsqr NC=%d RW=%d tri=%s lds=%zu nchunk=%d merge=%d", r.nc, r.rw, r.tri_lds ? "lds" : "global", r.lds_bytes, r.nchunk, r.merge ? 1 : 0);
}
static std::string kalman_text(const KalmanRoute& r, size_t scalar) {
  const char* S = scalar == 4 ? "float" : "double";
  std::string s = fmt("fused=%d ", r.s_fused ? 1 : 0);
  const std::string ci = fmt("k_chol_inv<%s,%s> lds=%zu", S, r.chol_inv_lds ? "true" : "false", r.chol_inv_bytes);
  switch (r.solve) {
    case GAIN_NONE: return s + "none";
    case GAIN_BLOCKED: return s + fmt("blocked<%d,%d,%d>", BLOCKED_GAIN[r.blocked].nb, BLOCKED_GAIN[r.blocked].na, BLOCKED_GAIN[r.blocked].npart);
    case GAIN_W: return s + fmt("k_gain_w<%s,%d,%d>", S, r.nbn, r.npart);
    case GAIN_LARGE: return s + fmt("large CH_S_A<%d> TR_S21 items=%d CH_S_B<%d> TR_W<%d> items=%d k_dx_wz", r.nb_a, r.items_s21, r.nb_b, r.nb_w, r.items_w);
    case GAIN_CHOL_INV: return s + ci + " OP_W k_dx_w";
    case GAIN_K: return s + fmt("k_gain<%s,%d> k_inject<true>", S, r.nbn);
    case GAIN_K_CHOL_INV: return s + ci + " OP_W OP_K k_inject<false>";
  }
  return s + "?";
}
static void small_case(Table& V, const char* name, const int* cols, int nb, int limit, int compress, int n_lit, int joseph, size_t scalar) {
  const SmallRoute r = small_route(nb, [&](int i) { return cols[i]; }, limit, compress, n_lit, joseph, 200, scalar, true);
  const char* kind = r.kind == CHAIN_ONLY ? "chain" : r.kind == SMALL_ONLY ? "small" : "mixed";
  V.add({sc(scalar), str(limit), str(compress), str(n_lit), str(joseph), name}, fmt("%s split=%d nsmall=%d segb=%d", kind, r.small_split, r.nsmall, r.segb));
}

// --handle scalar B nb n_cap f_cap m_cap form fused_s gain_parts small_update override cameras...: the routes of ONE update of ONE
// handle, composed the way launch_update composes them (one line per stage: G geometry, F features, C compression, Q the
// k_qr_update instantiation where the compression is the Householder TSQR, V the small-window decision over the range's
// windows, K Kalman stage); tests/test_gpu_update_kernels.py asserts with it that each
// of its cases reaches the kernels it was written for.  scalar: f | d; cameras: the window size of each trajectory of the range.
// --handle-lit: the same handle with a trajectory on the literal anisotropic route in it (n_lit > 0: no k_update_small, the
// information form whatever the override says; tests/test_gpu_literal_kernels.py)
static int one_handle(int argc, char** argv, int n_lit) {
  if (argc < 13) { std::fprintf(stderr, "--handle needs 11 values and the windows\n"); return 2; }
  const size_t s = argv[2][0] == 'f' ? 4 : 8;
  int a[10];
  for (int i = 0; i < 10; ++i) a[i] = std::atoi(argv[3 + i]);
  const int B = a[0], nb = a[1], n_cap = a[2], f_cap = a[3], m_cap = a[4], form = a[5], fused_s = a[6], gain_parts = a[7], small_update = a[8], ov = a[9];
  std::vector<int> cols;
  for (int i = 13; i < argc; ++i) cols.push_back(window_cols(std::atoi(argv[i]), 0, false, n_cap));
  if ((int)cols.size() != nb) { std::fprintf(stderr, "--handle: %d windows for nb = %d\n", (int)cols.size(), nb); return 2; }
  const Geometry g = geometry(B, n_cap, f_cap, m_cap, s);
  const int cmp = effective_compress(g.compress, ov, n_lit), limit = small_limit(small_update, f_cap, s, true);
  const SmallRoute r = small_route(nb, [&](int i) { return cols[i]; }, limit, cmp, n_lit, form, f_cap, s, true);
  std::printf("G %s ld=%d ldR=%d compress=%d Mp=%d Mp2=%d lam_parts=%d\n", g.refusal == GEO_OK ? "ok" : "refused", g.ld, g.ldR, g.compress, g.has_Mp, g.has_Mp2, g.lam_parts);
  std::printf("F %s\n", feature_text(feature_route(s, f_cap, m_cap, nb, 1, cmp)).c_str());
  std::printf("C compress=%d %s\n", cmp, compress_text(compress_route(cmp, g.ldR, g.has_Mp, g.lam_parts, GRAM_PARTS)).c_str());
  if (!cmp) std::printf("Q %s\n", tsqr_text(tsqr_route(s, g.n6cap, g.ldR, g.nchunk)).c_str());
  std::printf("V limit=%d %s split=%d nsmall=%d segb=%d\n", limit, r.kind == CHAIN_ONLY ? "chain" : r.kind == SMALL_ONLY ? "small" : "mixed", r.small_split, r.nsmall, r.segb);
  std::printf("K %s\n", kalman_text(kalman_route(s, n_cap, B, nb, form, fused_s, gain_parts, g.has_Mp2), s).c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "--handle")) return one_handle(argc, argv, 0);
  if (argc > 1 && !std::strcmp(argv[1], "--handle-lit")) return one_handle(argc, argv, 1);
  g_runs = argc > 1 && !std::strcmp(argv[1], "--runs");
  // G: what alloc derives from n_cap and f_cap; N: from B; A: what it refuses (the scalar and m_cap enter only there)
  Table G{"G", {"f_cap", "n_cap"}, {}}, N{"N", {"B"}, {}}, A{"A", {"scalar", "m_cap", "n_cap"}, {}};
  for (int f_cap : F_CAPS)
    for (int n_cap = 1; n_cap <= N_CAP_MAX + 1; ++n_cap) {
      const Geometry g = geometry(64, n_cap, f_cap, 12, 4);
      G.add({str(f_cap), str(n_cap)}, fmt("%s ld=%d ldR=%d compress=%d Mp=%d Mp2=%d lam_parts=%d", g.refusal == GEO_OK ? "ok" : "refused", g.ld, g.ldR, g.compress, g.has_Mp, g.has_Mp2, g.lam_parts));
    }
  for (int B : {1, 6, 64, 96, 128, 130}) N.add({str(B)}, fmt("nchunk=%d", geometry(B, 10, 200, 12, 4).nchunk));
  for (size_t s : SCALARS)
    for (int m_cap : M_CAPS)
      for (int n_cap = 1; n_cap <= N_CAP_MAX + 1; ++n_cap) {
        const GeometryRefusal r = geometry(64, n_cap, 200, m_cap, s).refusal;
        A.add({sc(s), str(m_cap), str(n_cap)}, r == GEO_OK ? "ok" : r == GEO_N_CAP ? "refused n_cap" : "refused m_cap");
      }
  G.print(); N.print(); A.print();
  // F: feature route.  The launches' shape follows the scalar, the route, feat_pair and m_cap (every m_cap at one f_cap and nb); the
  // pair kernel's single flag and items follow feat_pair, f_cap and nb (every f_cap and nb at the m_cap on either side of M_REG
  // and at M_STAGED): the cross through those points instead of the whole product, every bound with both its neighbours
  Table F{"F", {"scalar", "compress", "feat_pair", "m_cap", "f_cap", "nb"}, {}};
  for (size_t s : SCALARS)
    for (int compress : {0, 3})
      for (int fp = 0; fp <= 3; ++fp)
        for (int m_cap : M_CAPS)
          for (int f_cap : F_CAPS)
            for (auto& bn : BNB)
              if ((f_cap == 200 && bn[1] == 16) || m_cap == M_REG || m_cap == M_REG + 1 || m_cap == M_STAGED)
                F.add({sc(s), str(compress), str(fp), str(m_cap), str(f_cap), str(bn[1])}, feature_text(feature_route(s, f_cap, m_cap, bn[1], fp, compress)));
  F.print();
  // S: k_update_small's fit per window size; L: the limit a handle routes by
  Table S{"S", {"scalar", "granted", "f_cap", "n_cap"}, {}}, L{"L", {"scalar", "f_cap", "small_update"}, {}};
  for (size_t s : SCALARS)
    for (int granted = 1; granted >= 0; --granted)
      for (int f_cap : F_CAPS)
        for (int n_cap = 1; n_cap <= N_CAP_MAX; ++n_cap)
          if (granted || n_cap == 10) S.add({sc(s), str(granted), str(f_cap), str(n_cap)}, fmt("fits=%d segb=%d", update_small_fits(6 * n_cap, f_cap, s, granted != 0), update_small_segb(6 * n_cap)));
  for (size_t s : SCALARS)
    for (int f_cap : F_CAPS)
      for (int su : {0, 5, 6, 60, 84, 85, 90, 378, 1000}) L.add({sc(s), str(f_cap), str(su)}, fmt("limit=%d", small_limit(su, f_cap, s, true)));
  S.print(); L.print();
  // V: the small-window decision of a range, by its windows' camera columns (window_cols)
  Table V{"V", {"scalar", "limit", "compress", "n_lit", "form", "windows"}, {}};
  {
    const int all_short[] = {30, 60, 48}, all_long[] = {90, 96, 120}, mixed[] = {60, 90, 48, 126}, with_empty[] = {0, 60, 90}, only_empty[] = {0, 0};
    const int empty_long[] = {0, 96}, at_limit[] = {66, 72, 78};
    // run_frames: the update is enqueued one augmentState ahead of the host mirror; a skipped cell has none ahead
    const int ahead[] = {window_cols(9, 1, false, 12), window_cols(11, 1, false, 12), window_cols(12, 1, false, 12)};
    const int skipped[] = {window_cols(12, 1, true, 20), window_cols(12, 1, false, 20)};
    for (size_t s : SCALARS) {
      const int limit = small_limit(84, 200, s, true);   // the default setting at f_cap 200
      small_case(V, "all_short", all_short, 3, limit, 3, 0, 0, s);
      small_case(V, "all_long", all_long, 3, limit, 3, 0, 0, s);
      small_case(V, "mixed", mixed, 4, limit, 3, 0, 0, s);
      small_case(V, "with_empty", with_empty, 3, limit, 3, 0, 0, s);
      small_case(V, "only_empty", only_empty, 2, limit, 3, 0, 0, s);
      small_case(V, "empty_long", empty_long, 2, limit, 3, 0, 0, s);
      small_case(V, "at_limit", at_limit, 3, limit, 3, 0, 0, s);
      small_case(V, "ahead", ahead, 3, limit, 3, 0, 0, s);
      small_case(V, "skipped", skipped, 2, limit, 3, 0, 0, s);
      small_case(V, "mixed", mixed, 4, 0, 3, 0, 0, s);
      small_case(V, "mixed", mixed, 4, limit, 0, 0, 0, s);
      small_case(V, "mixed", mixed, 4, limit, 3, 1, 0, s);
      small_case(V, "mixed", mixed, 4, limit, 3, 0, 1, s);
      small_case(V, "mixed", mixed, 4, limit, 3, 0, 2, s);
      small_case(V, "mixed", mixed, 4, 48, 3, 0, 0, s);
      small_case(V, "all_long", all_long, 3, 378, 3, 0, 0, s);   // a limit beyond what fits the kernel: the chain takes everybody
    }
  }
  V.print();
  // C: compression route (the geometry of n_cap and f_cap, the handle's override, trajectories on the literal route)
  Table C{"C", {"override", "n_lit", "f_cap", "n_cap"}, {}};
  for (int ov : {-1, 3, 0})
    for (int n_lit = 0; n_lit <= 1; ++n_lit)
      for (int f_cap : F_CAPS)
        for (int n_cap = 1; n_cap <= N_CAP_MAX; ++n_cap) {
          const Geometry g = geometry(64, n_cap, f_cap, 12, 4);
          const int cmp = effective_compress(g.compress, ov, n_lit);
          C.add({str(ov), str(n_lit), str(f_cap), str(n_cap)}, fmt("compress=%d ", cmp) + compress_text(compress_route(cmp, g.ldR, g.has_Mp, g.lam_parts, GRAM_PARTS)));
        }
  C.print();
  // Q: the Householder TSQR's instantiation (every window at one batch size; every batch size on either side of a chunk count at one window)
  Table Q{"Q", {"scalar", "B", "n_cap"}, {}};
  for (size_t s : SCALARS)
    for (int B : {1, 32, 33, 64, 65, 128, 129, 130})
      for (int n_cap = 1; n_cap <= N_CAP_MAX; ++n_cap)
        if (B == 64 || n_cap == 22) {
          const Geometry g = geometry(B, n_cap, 1025, 12, s);
          Q.add({sc(s), str(B), str(n_cap)}, tsqr_text(tsqr_route(s, g.n6cap, g.ldR, g.nchunk)));
        }
  Q.print();
  // K: Kalman route (the window first: a bound in n_cap then shows once, over everything that does not move it)
  Table K{"K", {"n_cap", "scalar", "form", "fused_s", "gain_parts", "B,nb"}, {}};
  for (int n_cap = 1; n_cap <= N_CAP_MAX; ++n_cap)
    for (size_t s : SCALARS)
      for (int form = 0; form <= 2; ++form)
        for (int fused = 0; fused <= 1; ++fused)
          for (int parts : {0, 2, 4})
            for (auto& bn : BNB) {
              const Geometry g = geometry(bn[0], n_cap, 200, 12, s);
              K.add({str(n_cap), sc(s), str(form), str(fused), str(parts), str(bn[0]) + "," + str(bn[1])}, kalman_text(kalman_route(s, n_cap, bn[0], bn[1], form, fused, parts, g.has_Mp2), s));
            }
  K.print();
  return 0;
}
