// The track compiler (msckf_mono_amd/csrc/track_compile.h) on its own: no HIP header, a host compiler only.  A recording
// traced by hand with (max_cam_states, min_track_length, max_track_length) = (3, 2, 4): a track that ends by loss, two that
// end by length with an observation in the newest camera, one too short to be listed, a duplicated and an untracked id in a
// `cur` list, drops by pruneEmptyStates, and every refusal with its code and text.
// With a file name as argument: a recording is read from it and its cells are printed (tests/test_track_compile.py).
//   file:    "P max_cam_states min_track_length max_track_length", then per image "I n_cur n_new" followed by n_cur + n_new
//            lines "id x y" (hexadecimal floats)
//   output:  per image "C F entries n_drop window live", then per track "T id M" and M lines "slot x y"
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../msckf_mono_amd/csrc/track_compile.h"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

using msckf_compile::Compiler;
using msckf_compile::ImageSummary;
using msckf_compile::Refusal;

// the measurement of feature id on image k
static double mx(int k, uint64_t id) { return k + 0.125 * (double)id; }
static double my(int k, uint64_t id) { return -k - 0.0625 * (double)id; }
struct Lists { std::vector<double> m; std::vector<uint64_t> ids; };
static Lists lists(int k, std::initializer_list<uint64_t> ids) {
  Lists l;
  for (uint64_t id : ids) { l.ids.push_back(id); l.m.push_back(mx(k, id)); l.m.push_back(my(k, id)); }
  return l;
}
static Refusal image(Compiler& c, int k, std::initializer_list<uint64_t> cur, std::initializer_list<uint64_t> fresh, ImageSummary& s) {
  const Lists a = lists(k, cur), b = lists(k, fresh);
  return c.image(a.m.data(), a.ids.data(), (int)a.ids.size(), b.m.data(), b.ids.data(), (int)b.ids.size(), s);
}
static bool summary_is(const ImageSummary& s, int F, int entries, int n_drop, int window, int live) {
  return s.F == F && s.entries == entries && s.n_drop == n_drop && s.window == window && s.live == live;
}
// track t of the last work-list: id, and its observations (slot, image) pairs
static bool track_is(const Compiler& c, size_t t, uint64_t id, std::initializer_list<std::pair<int, int>> obs) {
  if (t >= c.wl.M.size() || c.ids[t] != id || c.wl.M[t] != (int)obs.size()) return false;
  size_t o = 0;
  for (size_t i = 0; i < t; ++i) o += (size_t)c.wl.M[i];
  for (const auto& so : obs) {
    if (c.wl.slots[o] != so.first || c.wl.obs[2 * o] != mx(so.second, id) || c.wl.obs[2 * o + 1] != my(so.second, id)) return false;
    ++o;
  }
  return true;
}

static int by_hand() {
  CHECK(Compiler::create_refusal(3, 2, 4).code == 0);
  for (int bad = 0; bad < 3; ++bad) {
    const Refusal r = Compiler::create_refusal(bad == 0 ? 0 : 3, bad == 1 ? -1 : 2, bad == 2 ? 0 : 4);
    CHECK(r.code == -EINVAL && r.why && std::strstr(r.why, "must be positive"));
  }
  Compiler c(3, 2, 4);
  ImageSummary s{};
  // image 0: three new features
  CHECK(image(c, 0, {}, {1, 2, 3}, s).code == 0 && summary_is(s, 0, 0, 0, 1, 3));
  // image 1: all tracked; 4 and 5 are new
  CHECK(image(c, 1, {1, 2, 3}, {4, 5}, s).code == 0 && summary_is(s, 0, 0, 0, 2, 5));
  // image 2: 3 is lost (two observations: listed), 5 is lost (one: never listed); 4 twice -- the first occurrence wins --; 77 is nobody's
  {
    Lists a = lists(2, {1, 2, 4});
    a.ids.push_back(4); a.m.push_back(99.0); a.m.push_back(-99.0);
    a.ids.push_back(77); a.m.push_back(5.0); a.m.push_back(5.0);
    CHECK(c.image(a.m.data(), a.ids.data(), (int)a.ids.size(), nullptr, nullptr, 0, s).code == 0 && summary_is(s, 1, 2, 0, 3, 3));
    CHECK(track_is(c, 0, 3, {{0, 0}, {1, 1}}));
  }
  // image 3: 1 and 2 reach max_track_length with an observation in the newest camera, 4 is lost; every camera is left empty, the
  // window of 4 goes back to max_cam_states
  CHECK(image(c, 3, {1, 2}, {}, s).code == 0 && summary_is(s, 3, 10, 1, 4, 0));
  CHECK(track_is(c, 0, 1, {{0, 0}, {1, 1}, {2, 2}, {3, 3}}) && track_is(c, 1, 2, {{0, 0}, {1, 1}, {2, 2}, {3, 3}}) && track_is(c, 2, 4, {{1, 1}, {2, 2}}));
  CHECK(c.t.pruned.empty() && c.t.cams.size() == 3);
  {
    int M[3]; int slots[10]; double obs[20]; uint64_t ids[3];
    CHECK(c.cell_refusal(3, 10).code == 0);
    Refusal r = c.cell_refusal(2, 10); CHECK(r.code == -E2BIG && std::strstr(r.why, "capacities"));
    r = c.cell_refusal(3, 9); CHECK(r.code == -E2BIG);
    r = c.cell_refusal(-1, 10); CHECK(r.code == -EINVAL && std::strstr(r.why, "negative capacity"));
    (void)M; (void)slots; (void)obs; (void)ids;
  }
  // image 4: nothing tracked, 9 is new: the oldest empty camera goes
  CHECK(image(c, 4, {}, {9}, s).code == 0 && summary_is(s, 0, 0, 1, 4, 1));
  // refusals of an image, in order: the counts, then the pointers
  {
    const double z[2] = {0, 0}; const uint64_t id = 50;
    Refusal r = c.image(z, &id, -1, z, &id, 0, s); CHECK(r.code == -EINVAL && std::strstr(r.why, "negative feature count"));
    r = c.image(nullptr, &id, 1, nullptr, nullptr, 0, s); CHECK(r.code == -EINVAL && std::strstr(r.why, "null feature list"));
    r = c.image(z, &id, 0, z, nullptr, 1, s); CHECK(r.code == -EINVAL && std::strstr(r.why, "null feature list"));
    CHECK(c.t.cams.size() == 3 && !c.broken);                              // a refused call changes nothing
  }
  // image 5: 9 comes as new again
  {
    const Refusal r = image(c, 5, {9}, {10, 9, 11}, s);
    CHECK(r.code == -EEXIST && std::strstr(r.why, "already being tracked") && c.broken);
    const Refusal again = image(c, 6, {}, {}, s);
    CHECK(again.code == -EIO && std::strstr(again.why, "unusable"));
    CHECK(c.cell_refusal(100, 100).code == -EIO);
  }
  return failures;
}

static int from_file(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) { std::printf("cannot open %s\n", path); return 1; }
  int a, b, d;
  if (std::fscanf(f, " P %d %d %d", &a, &b, &d) != 3) { std::fclose(f); return 1; }
  Compiler c(a, b, d);
  int n_cur, n_new;
  while (std::fscanf(f, " I %d %d", &n_cur, &n_new) == 2) {
    Lists l[2];
    for (int w = 0; w < 2; ++w)
      for (int i = 0; i < (w ? n_new : n_cur); ++i) {
        unsigned long long id; double x, y;
        if (std::fscanf(f, " %llu %la %la", &id, &x, &y) != 3) { std::fclose(f); return 1; }
        l[w].ids.push_back(id); l[w].m.push_back(x); l[w].m.push_back(y);
      }
    ImageSummary s{};
    const Refusal r = c.image(l[0].m.data(), l[0].ids.data(), n_cur, l[1].m.data(), l[1].ids.data(), n_new, s);
    if (r.code) { std::printf("R %d %s\n", r.code, r.why); std::fclose(f); return 0; }
    std::printf("C %d %d %d %d %d\n", s.F, s.entries, s.n_drop, s.window, s.live);
    size_t o = 0;
    for (size_t t = 0; t < c.wl.M.size(); ++t) {
      std::printf("T %llu %d\n", (unsigned long long)c.ids[t], c.wl.M[t]);
      for (int i = 0; i < c.wl.M[t]; ++i, ++o) std::printf("%d %a %a\n", c.wl.slots[o], c.wl.obs[2 * o], c.wl.obs[2 * o + 1]);
    }
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return from_file(argv[1]);
  if (by_hand()) return 1;
  std::printf("track compile ok\n");
  return 0;
}
