// The staged input layouts (msckf_mono_amd/csrc/input_layouts.h) on their own: no HIP header, a host compiler only.  Every block
// handed to the header is a heap block of exactly the size the header asked for, so a sanitizer sees any byte written outside.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../msckf_mono_amd/csrc/input_layouts.h"

using namespace msckf_inputs;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)
using VI = std::vector<int>;
using VZ = std::vector<size_t>;

// a heap block of exactly n bytes (operator new[]: aligned for every scalar type)
struct Block {
  std::unique_ptr<unsigned char[]> p; size_t n;
  explicit Block(size_t n_) : p(new unsigned char[n_ ? n_ : 1]), n(n_) { std::memset(p.get(), 0xA5, n_); }   // (a zero-byte block: one byte nobody is told about)
  unsigned char* at(size_t o = 0) { return p.get() + o; }
};

// ---- the streamed frame block: section offsets
static void frame_block_spot_case(size_t esz, const VZ& want, size_t empty_end) {
  const FrameLayout L(3, 2, 4, esz);
  VZ got;
  for (int s = 0; s < N_SECTIONS; ++s) got.push_back(L.block_at(s, 5));
  got.push_back(L.bytes(5));
  CHECK(got == want);
  CHECK(L.off_obs(0) == L.at[SEC_SLOTS] && L.off_obs(0) == empty_end && L.bytes(0) == empty_end);
}

// ---- the single-call block
template <class S> static void single_block_spot_case() {
  const SingleBlock w(5, 3);
  CHECK(w.f4 == 8 && w.ib == 28);
  const int F = 2, M[2] = {3, 1}, slots[4] = {4, 0, 2, 1};
  const double obs[8] = {0.1, -0.2, 0.3, -0.4, 0.5, -0.6, 0.7, -0.8};
  CHECK(w.ints(F) == 18 && w.scalars(F) == 12 && w.coords_at(w.ints(F)) == 80);
  Block blk(w.staged_bytes(w.ints(F), w.scalars(F), sizeof(S)));
  CHECK(blk.n == 80 + 12 * sizeof(S));
  int* I = reinterpret_cast<int*>(blk.at()); S* O = reinterpret_cast<S*>(blk.at(w.coords_at(w.ints(F))));
  w.pack(I, O, F, M, slots, obs);
  VI want(18, 0);
  want[0] = 2; want[4] = 3; want[5] = 1; want[12] = 4; want[13] = 0; want[14] = 2; want[15] = 1;
  CHECK(VI(I, I + 18) == want);
  CHECK(w.N_AT == 0 && w.M_AT == 4 && w.slots_at() == 12);
  std::vector<S> wo(12, S(0));
  for (int e = 0; e < 3; ++e) { wo[2 * e] = (S)obs[2 * e]; wo[2 * e + 1] = (S)obs[2 * e + 1]; }
  wo[6] = (S)obs[6]; wo[7] = (S)obs[7];                       // track 1's row starts m_cap pairs on
  CHECK(std::vector<S>(O, O + 12) == wo);
  // no track: the head and the lengths, no scalar
  Block none(w.staged_bytes(w.ints(0), w.scalars(0), sizeof(S)));
  CHECK(none.n == 48 && w.scalars(0) == 0);
  w.pack(reinterpret_cast<int*>(none.at()), reinterpret_cast<S*>(none.at(w.coords_at(w.ints(0)))), 0, nullptr, nullptr, nullptr);
  CHECK(VI(reinterpret_cast<int*>(none.at()), reinterpret_cast<int*>(none.at()) + 12) == VI(12, 0));
  // a range: whole blocks side by side, the last one full (f_cap tracks of m_cap) reaches its last row and no further
  const int nb = 2;
  const size_t nI = (size_t)nb * w.ib, nO = (size_t)nb * w.ib * 2;
  Block rng(w.staged_bytes(nI, nO, sizeof(S)));
  int* rI = reinterpret_cast<int*>(rng.at()); S* rO = reinterpret_cast<S*>(rng.at(w.coords_at(nI)));
  const VI fullM(5, 3); VI fullS; std::vector<double> fullO;
  for (int t = 0; t < 5; ++t) for (int k = 0; k < 3; ++k) { fullS.push_back(k + t % 2); fullO.push_back(t + 0.25 * k); fullO.push_back(-t - 0.5 * k); }
  w.pack(rI, rO, F, M, slots, obs);
  w.pack(rI + w.ib, rO + 2 * w.ib, 5, fullM.data(), fullS.data(), fullO.data());
  CHECK(VI(rI, rI + 18) == want && rI[w.ib] == 5 && rI[w.ib + w.slots_at() + 14] == fullS[14] && rO[2 * w.ib + 29] == (S)fullO[29]);
}

// ---- the work-list rules: n_cap 8, f_cap 24, m_cap 7 as tests/test_gpu_parity.py gives them
static bool refused(const VI& M, const VI& slots, int code, const char* why, int f_cap = 24, int m_cap = 7, int n_cap = 8) {
  const Refusal r = worklist_refusal((int)M.size(), M.data(), slots.data(), f_cap, m_cap, n_cap);
  return r.code == code && (why ? r.why && std::string(r.why) == why : r.why == nullptr);
}
static void worklist_rules() {
  VI many_M(25, 2), many_s;
  for (int t = 0; t < 25; ++t) { many_s.push_back(0); many_s.push_back(1); }
  CHECK(refused(many_M, many_s, -E2BIG, "more tracks than f_cap"));
  CHECK(refused({8}, {0, 1, 2, 3, 4, 5, 6, 7}, -E2BIG, "track longer than m_cap"));
  CHECK(refused({3}, {0, -1, 2}, -EINVAL, "camera slot out of range"));
  CHECK(refused({3}, {0, 8, 2}, -EINVAL, "camera slot out of range"));
  CHECK(refused({3}, {0, 1, 1}, -EINVAL, "camera slot repeated within a track"));
  CHECK(E2BIG == 7 && EINVAL == 22);
  CHECK(refused({3, 2}, {0, 1, 2, 6, 7}, 0, nullptr) && refused({}, {}, 0, nullptr));
  { const Refusal r = worklist_refusal(-1, nullptr, nullptr, 24, 7, 8); CHECK(r.code == -E2BIG && std::string(r.why) == "more tracks than f_cap"); }
  CHECK(refused({-1}, {}, -E2BIG, "track longer than m_cap"));
  // several violations: the count first (nothing else is read), then every length before any slot, then per track range before repetition
  many_s[0] = -5;
  many_M[3] = 9;
  CHECK(refused(many_M, many_s, -E2BIG, "more tracks than f_cap"));
  CHECK(refused({2, 8}, {-1, -1, 0, 1, 2, 3, 4, 5, 6, 7}, -E2BIG, "track longer than m_cap"));           // a bad slot in track 0, a long track 1
  CHECK(refused({3, 2}, {1, 1, 9, 0, 1}, -EINVAL, "camera slot out of range"));                         // track 0 repeats AND is out of range
  CHECK(refused({2, 2}, {1, 1, 0, 9}, -EINVAL, "camera slot repeated within a track"));                 // track 0 repeats, track 1 is out of range
  // slots 64 apart share a bit of the repetition test's word and are not taken for each other
  CHECK(refused({2}, {3, 67}, 0, nullptr, 24, 7, 98) && repeated_slot(VI({63, 5, 63}).data(), 3));
}

// ---- the readings chunk
template <class S> struct Chunk { int kk; std::vector<S> rows; VI cnt; };
template <class S> static std::vector<Chunk<S>> chunks_of(const Readings& in, int rd_cap) {
  std::vector<Chunk<S>> out;
  for (int k0 = 0; k0 < in.kmax; k0 += rd_cap) {
    const int kk = in.rows(k0, rd_cap);
    Block blk(in.staged_bytes(kk, sizeof(S)));
    S* rows = reinterpret_cast<S*>(blk.at());
    int* cnt = in.Kb ? reinterpret_cast<int*>(blk.at(in.counts_at(kk, sizeof(S)))) : nullptr;
    CHECK(!in.Kb || (in.counts_at(kk, sizeof(S)) % 16 == 0 && blk.n == in.counts_at(kk, sizeof(S)) + in.nb * sizeof(int)));
    CHECK(in.Kb || blk.n == in.scalars(kk) * sizeof(S));
    in.pack(rows, cnt, k0, kk, rd_cap);
    out.push_back(Chunk<S>{kk, std::vector<S>(rows, rows + in.scalars(kk)), cnt ? VI(cnt, cnt + in.nb) : VI()});
  }
  return out;
}
template <class S> static void readings() {
  const int rd_cap = 64, K[4] = {0, 64, 65, 130};
  std::vector<double> rd((size_t)(2 * 130) * RD_ROW);      // 0 + 64 + 65 + 130 rows with counts, 2 x 130 with one K
  for (size_t i = 0; i < rd.size(); ++i) rd[i] = 1.0 + 0.001 * (double)i;      // no reading is zero
  const Readings in(rd.data(), 4, K);
  const auto ch = chunks_of<S>(in, rd_cap);
  CHECK(ch.size() == 3);
  if (ch.size() != 3) return;
  CHECK(ch[0].kk == 64 && ch[1].kk == 64 && ch[2].kk == 2);
  CHECK(ch[0].cnt == VI({0, 64, 64, 64}) && ch[1].cnt == VI({0, 0, 1, 64}) && ch[2].cnt == VI({0, 0, 0, 2}));
  const size_t row0[4] = {0, 0, 64, 129};
  for (size_t c = 0; c < 3; ++c)
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < ch[c].kk; ++k)
        for (int x = 0; x < RD_ROW; ++x) {
          const S got = ch[c].rows[((size_t)i * ch[c].kk + k) * RD_ROW + x];
          const S want = k < ch[c].cnt[i] ? (S)rd[(row0[i] + c * rd_cap + k) * RD_ROW + x] : S(0);
          if (got != want) { CHECK(got == want); return; }
        }
  // one K for all: no count array, the rows of counts (K, K)
  const int KK[2] = {130, 130};
  const auto eq = chunks_of<S>(Readings(rd.data(), 2, 130), rd_cap), cn = chunks_of<S>(Readings(rd.data(), 2, KK), rd_cap);
  CHECK(eq.size() == 3 && cn.size() == 3);
  for (size_t c = 0; c < eq.size() && c < cn.size(); ++c) CHECK(eq[c].kk == cn[c].kk && eq[c].rows == cn[c].rows && eq[c].cnt.empty() && cn[c].cnt == VI(2, c < 2 ? 64 : 2));
  CHECK(chunks_of<S>(Readings(rd.data(), 3, 0), rd_cap).empty());
}

// ---- the scenario's store, the frame blocks and the reading rule
struct Cell { int f, b, k; bool skip; VI M, slots; int n_drop; };
static double reading(int f, int b, int s, int c) { return 0.1 + f + 0.01 * b + 0.001 * s + 0.0001 * c; }
static double coord(int f, int b, size_t e, int c) { return (c ? -1.0 : 1.0) * (1.0 / 3.0 + f + 0.1 * b + 0.01 * (double)e); }
template <class S> static void stage(ScenarioStore& sc, const Cell& c, int K) {
  std::vector<double> rd((size_t)K * RD_ROW), ob(2 * c.slots.size());
  for (int s = 0; s < K; ++s) for (int x = 0; x < RD_ROW; ++x) rd[(size_t)s * RD_ROW + x] = reading(c.f, c.b, s, x);
  for (size_t e = 0; e < c.slots.size(); ++e) { ob[2 * e] = coord(c.f, c.b, e, 0); ob[2 * e + 1] = coord(c.f, c.b, e, 1); }
  sc.set_cell<S>(c.f, c.b, rd.data(), c.k, c.skip, (int)c.M.size(), c.M.data(), c.slots.data(), ob.data(), c.n_drop);
}
// the resident copy a commit makes: one array per section, heap blocks of the sections' sizes
struct Resident {
  std::vector<Block> dev;
  explicit Resident(const ScenarioStore& sc) {
    for (int s = 0; s < N_SECTIONS; ++s) dev.emplace_back(s < N_FIXED ? sc.fixed[s].size() : sc.total() * sc.lay.entry_bytes(s));
    for (int s = 0; s < N_FIXED; ++s) std::memcpy(dev[s].at(), sc.fixed[s].data(), sc.fixed[s].size());
    for (int f = 0; f < sc.frames; ++f)
      sc.gather(f, reinterpret_cast<int*>(dev[SEC_SLOTS].at(sc.lay.resident_at(SEC_SLOTS, f, sc.fr_base[f]))), dev[SEC_OBS].at(sc.lay.resident_at(SEC_OBS, f, sc.fr_base[f])));
  }
};
// every cell of frame f from b0 on, read through `in` the way the kernels do (wl_first: entry = off[i * f_cap + t] + k), against
// what was staged
template <class S> static void read_frame(const FrameIn<S>& in, const std::vector<Cell>& cells, int f, int b0, int B, int K, int f_cap) {
  for (int b = b0; b < B; ++b) {
    const int i = b - b0;
    const Cell* c = nullptr;
    for (const Cell& q : cells) if (q.f == f && q.b == b) c = &q;      // the last one staged
    if (!c) {   // never set: no track, no drop, K samples of zero readings
      CHECK(in.n[i] == 0 && in.drop[i] == 0 && in.k[i] == K);
      for (int t = 0; t < f_cap; ++t) CHECK(in.M[i * f_cap + t] == 0);
      for (int s = 0; s < K * RD_ROW; ++s) CHECK(in.rd[(size_t)i * K * RD_ROW + s] == S(0));
      continue;
    }
    CHECK(in.n[i] == (int)c->M.size() && in.drop[i] == c->n_drop && in.k[i] == (c->skip ? NO_IMAGE : c->k));
    for (int s = 0; s < K; ++s) for (int x = 0; x < RD_ROW; ++x) CHECK(in.rd[((size_t)i * K + s) * RD_ROW + x] == (s < c->k ? (S)reading(f, b, s, x) : S(0)));
    size_t e = 0;
    for (int t = 0; t < f_cap; ++t) {
      const int M = t < (int)c->M.size() ? c->M[t] : 0;
      CHECK(in.M[i * f_cap + t] == M);
      for (int k = 0; k < M; ++k, ++e) {
        const long at = (long)in.off[i * f_cap + t] + k;
        CHECK(in.slots[at] == c->slots[e] && in.obs[2 * at] == (S)coord(f, b, e, 0) && in.obs[2 * at + 1] == (S)coord(f, b, e, 1));
      }
    }
  }
}
template <class S> static void check_scenario(const ScenarioStore& sc, const std::vector<Cell>& cells, int B, int K, int f_cap) {
  Resident res(sc);
  for (int f = 0; f < sc.frames; ++f) {
    Block blk(sc.lay.bytes(sc.entries(f)));
    sc.write_block(f, blk.at());
    for (int b0 : {0, 2}) {
      read_frame<S>(frame_in<S>(sc.lay, b0, [&](int s) { return res.dev[s].at(sc.lay.resident_at(s, f, sc.fr_base[f])); }), cells, f, b0, B, K, f_cap);
      read_frame<S>(frame_in<S>(sc.lay, b0, [&](int s) { return blk.at(sc.lay.block_at(s, sc.entries(f))); }), cells, f, b0, B, K, f_cap);
    }
  }
}
template <class S> static void scenario() {
  const int frames = 3, B = 3, K = 2, f_cap = 4;   // m_cap 3, n_cap 6
  std::vector<Cell> cells = {
      {0, 0, 2, false, {}, {}, 0},                                           // an empty cell
      {0, 1, 0, true, {}, {}, 0},                                            // a skipped cell
      {0, 2, 1, false, {2, 3, 1, 2}, {0, 1, 2, 3, 4, 5, 1, 5}, 2},           // F = f_cap, one track of M = m_cap
      // frame 1: no entry at all (cell (1, 1) is never set, the others carry no track)
      {1, 0, 2, false, {}, {}, 1},
      {1, 2, 0, false, {}, {}, 0},
      {2, 0, 2, false, {3, 2}, {1, 2, 3, 0, 4}, 0},
      {2, 1, 1, false, {2, 2, 2}, {0, 1, 1, 2, 2, 3}, 1},                    // the middle cell that is patched below
      {2, 2, 2, false, {1}, {5}, 3},
  };
  ScenarioStore sc;
  sc.reset(frames, B, K, f_cap, sizeof(S));
  for (const Cell& c : cells) stage<S>(sc, c, K);
  CHECK(sc.index());
  CHECK(sc.fr_base == VZ({0, 8, 8, 20}) && sc.total() == 20 && sc.entries(1) == 0 && sc.largest_frame() == 12);
  CHECK(sc.maxslot == VI({-1, -1, 5, -1, -1, -1, 4, 3, 5}));
  const int* off = sc.ints(SEC_OFF);
  CHECK(VI(off, off + 12) == VI({0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 5, 6}));
  CHECK(VI(off + 24, off + 36) == VI({0, 3, 5, 5, 5, 7, 9, 11, 11, 12, 12, 12}));
  check_scenario<S>(sc, cells, B, K, f_cap);
  // patch: the middle cell again with fewer tracks; what lies behind it moves by the difference
  const VI off_before(off, off + 36); const VZ base_before = sc.fr_base;
  cells.push_back({2, 1, 2, false, {2}, {4, 5}, 0});
  stage<S>(sc, cells.back(), K);
  CHECK(sc.index());
  for (int c = 0; c < 9; ++c)
    for (int t = 0; t < f_cap; ++t)
      if (c != 7) CHECK(off[c * f_cap + t] == off_before[c * f_cap + t] - (c > 7 ? 4 : 0));      // the frame's later cell moves by 6 - 2 entries
  CHECK(VI(off + 28, off + 32) == VI({5, 7, 7, 7}));                                              // the cell itself: one track, the rest behind it
  CHECK(sc.fr_base == VZ({base_before[0], base_before[1], base_before[2], base_before[3] - 4}) && sc.maxslot[7] == 5);
  check_scenario<S>(sc, cells, B, K, f_cap);
  // the same as a store that was staged that way from the start
  ScenarioStore fresh;
  fresh.reset(frames, B, K, f_cap, sizeof(S));
  for (const Cell& c : cells) if (!(c.f == 2 && c.b == 1 && c.M.size() == 3)) stage<S>(fresh, c, K);
  CHECK(fresh.index());
  for (int s = 0; s < N_FIXED; ++s) CHECK(fresh.fixed[s] == sc.fixed[s]);
  CHECK(fresh.slots == sc.slots && fresh.obs == sc.obs && fresh.fr_base == sc.fr_base && fresh.maxslot == sc.maxslot);
  for (int f = 0; f < frames; ++f) {
    Block a(sc.lay.bytes(sc.entries(f))), b(fresh.lay.bytes(fresh.entries(f)));
    sc.write_block(f, a.at()); fresh.write_block(f, b.at());
    CHECK(a.n == b.n && std::memcmp(a.at(), b.at(), a.n) == 0);
  }
}

int main() {
  frame_block_spot_case(4, {0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048}, 1536);
  frame_block_spot_case(8, {0, 512, 768, 1024, 1280, 1536, 1792, 2048, 2304}, 1792);
  single_block_spot_case<float>(); single_block_spot_case<double>();
  worklist_rules();
  readings<float>(); readings<double>();
  scenario<float>(); scenario<double>();
  if (failures) return 1;
  std::printf("input layouts ok\n");
  return 0;
}
