// input_layouts.h -- the byte layouts of the inputs that only the host writes and every kernel reads, free of device calls.
//
// Four layouts, each stated once here; msckf_hip.hip keeps what talks to the device (allocations, copies, events, the pinned
// ring, the page-locked chunks) and asks this file where everything sits:
//   1. SingleBlock    the padded single-call work-list block [n, 0, 0, 0 | M[f4] | slots[f_cap][m_cap]] of one trajectory, the
//                     coordinates beside it at twice the stride; worklist_refusal: the rules a work-list must meet before it is packed
//   2. Readings       the propagate staging chunk of rd_cap samples per trajectory, with or without per-trajectory counts
//   3. ScenarioStore  the compact scenario cells on the host and the frame index over them
//   4. SECTIONS       the sections of a frame, [rd | n | drop | k | M | off | slots | obs]: the resident arrays (one per section,
//                     frames after each other) and the streamed block of one frame (sections at 256-byte offsets), and frame_in,
//                     the ONE place that turns "where section s of this frame starts" into the pointers a slice's kernels get
// A further per-cell input costs one entry of SECTIONS, its line in ScenarioStore::set_cell and its use in enqueue_frame:
// the allocation, the commit, the block fill and both FrameIn forms follow from the table.
// No HIP header, no Dev<S>, no batch type: a host compiler accepts this file on its own.  The device reads these layouts
// through wl_first (dev_common.h); tests/cpp/input_layouts_host.cpp reads them the same way without a device.
#ifndef MSCKF_INPUT_LAYOUTS_H
#define MSCKF_INPUT_LAYOUTS_H

#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstring>
#include <vector>

namespace msckf_inputs {

constexpr int RD_ROW = 7;      // scalars of one IMU reading (dev_common.h: RD_STRIDE; msckf_hip.hip asserts the match)
constexpr int NO_IMAGE = -1;   // a cell's sample count when its trajectory has no image on the frame (dev_common.h: IMU_SKIP)
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- 1. the single-call work-list block
// Per trajectory ib ints [n, 0, 0, 0 | M[f4] | slots[f_cap][m_cap]] (one copy per set_tracks instead of three) and 2 ib scalars
// of coordinates [f_cap][m_cap][2]: the kernels index both with the same stride.  Only the F rows in use are ever written.
struct SingleBlock {
  int f_cap = 0, m_cap = 0, f4 = 0; long ib = 0;
  static constexpr int N_AT = 0, M_AT = 4;   // the count word, the track lengths
  SingleBlock() {}
  SingleBlock(int f_cap_, int m_cap_) : f_cap(f_cap_), m_cap(m_cap_), f4((f_cap_ + 3) & ~3), ib((4 + f4 + (long)f_cap_ * m_cap_ + 3) & ~3L) {}
  int slots_at() const { return M_AT + f4; }
  size_t ints(int F) const { return (size_t)slots_at() + (size_t)F * m_cap; }   // what the first F rows occupy
  size_t scalars(int F) const { return (size_t)F * m_cap * 2; }
  // one pinned area for n_ints ints and the scalars behind them: where the scalars start, and its size
  static size_t coords_at(size_t n_ints) { return align_up(n_ints * sizeof(int), 16); }
  static size_t staged_bytes(size_t n_ints, size_t n_scalars, size_t esz) { return coords_at(n_ints) + n_scalars * esz; }
  // one work-list into its block: I[0 .. ints(F)), O[0 .. scalars(F))
  template <class S> void pack(int* I, S* O, int F, const int* M, const int* slots, const double* obs) const {
    std::memset(I, 0, ints(F) * sizeof(int));
    std::memset(O, 0, scalars(F) * sizeof(S));
    I[N_AT] = F;
    int* hM = I + M_AT; int* hS = I + slots_at();
    size_t o = 0;
    for (int t = 0; t < F; o += M[t++]) {
      hM[t] = M[t];
      for (int k = 0; k < M[t]; ++k) {
        hS[(size_t)t * m_cap + k] = slots[o + k];
        O[((size_t)t * m_cap + k) * 2] = (S)obs[2 * (o + k)];
        O[((size_t)t * m_cap + k) * 2 + 1] = (S)obs[2 * (o + k) + 1];
      }
    }
  }
};

// The rules for one trajectory's work-list (set_tracks, set_tracks_range, scenario_set), checked before anything of it is
// staged or written: the number of tracks, then every track's length, then track by track its slots' range and repetition
// (a track observes a camera at most once: the kernels rely on it -- slot -> observation map, contiguous-range test).
// code 0: acceptable; else a negative errno code and the reason.
struct Refusal { int code; const char* why; };
inline bool repeated_slot(const int* s, int M) {
  unsigned long long seen = 0;
  for (int k = 0; k < M; ++k) { const unsigned long long bit = 1ull << (s[k] & 63); if (s[k] >= 0 && s[k] < 64 && (seen & bit)) return true; seen |= bit; }
  return false;
}
inline Refusal worklist_refusal(int F, const int* M, const int* slots, int f_cap, int m_cap, int n_cap) {
  if (F < 0 || F > f_cap) return {-E2BIG, "more tracks than f_cap"};
  for (int t = 0; t < F; ++t) if (M[t] > m_cap || M[t] < 0) return {-E2BIG, "track longer than m_cap"};
  size_t o = 0;
  for (int t = 0; t < F; o += M[t++]) {
    for (int k = 0; k < M[t]; ++k) if (slots[o + k] < 0 || slots[o + k] >= n_cap) return {-EINVAL, "camera slot out of range"};
    if (repeated_slot(slots + o, M[t])) return {-EINVAL, "camera slot repeated within a track"};
  }
  return {0, nullptr};
}

// ---- 2. the readings chunk
// The IMU samples of nb trajectories travel in chunks of at most rd_cap rows per trajectory: [nb][kk][RD_ROW] scalars and, with a
// count per trajectory, [nb] ints behind them.  With counts (rd holds K[0] rows, then K[1] rows, ...) the chunks are cut per
// trajectory: in the chunk at k0 trajectory i has clamp(K[i] - k0, 0, rd_cap) samples -- the chunks of its own run with K[i]
// alone, so the same launches see the same samples -- and zero rows up to the chunk's longest trajectory.  With one K for all
// ([nb][K] rows) there is no count array.
struct Readings {
  const double* rd; int nb; const int* Kb; int K; int kmax = 0;
  std::vector<size_t> row0;   // trajectory i's first row in rd
  Readings(const double* rd_, int nb_, int K_) : Readings(rd_, nb_, nullptr, K_) {}
  Readings(const double* rd_, int nb_, const int* Kb_, int K_ = 0) : rd(rd_), nb(nb_), Kb(Kb_), K(K_), row0(nb_) {
    size_t o = 0;
    for (int i = 0; i < nb; ++i) { const int ki = Kb ? Kb[i] : K; row0[i] = o; o += ki; kmax = std::max(kmax, ki); }
  }
  int rows(int k0, int rd_cap) const { return std::min(rd_cap, kmax - k0); }        // kk of the chunk at k0
  size_t scalars(int kk) const { return (size_t)nb * kk * RD_ROW; }
  size_t counts_at(int kk, size_t esz) const { return align_up(scalars(kk) * esz, 16); }
  size_t staged_bytes(int kk, size_t esz) const { return Kb ? counts_at(kk, esz) + nb * sizeof(int) : scalars(kk) * esz; }
  // the chunk [k0, k0 + kk): rows [nb][kk][RD_ROW]; cnt [nb] with counts, untouched without
  template <class S> void pack(S* rows_out, int* cnt, int k0, int kk, int rd_cap) const {
    for (int i = 0; i < nb; ++i) {
      const int have = Kb ? std::max(0, std::min(Kb[i] - k0, rd_cap)) : kk;
      if (Kb) cnt[i] = have;
      for (int k = 0; k < kk; ++k)
        for (int c = 0; c < RD_ROW; ++c) rows_out[((size_t)i * kk + k) * RD_ROW + c] = k < have ? (S)rd[(row0[i] + k0 + k) * RD_ROW + c] : S(0);
    }
  }
};

// ---- 4 (before 3, which is built from it). a frame's sections
// The six fixed sections hold a fixed number of elements per trajectory; the two variable ones hold the frame's compact
// work-list entries, one int / one coordinate pair each (a track finds its first through off).  Order and alignment are DESIGN §2's.
enum Section { SEC_RD, SEC_N, SEC_DROP, SEC_K, SEC_M, SEC_OFF, N_FIXED, SEC_SLOTS = N_FIXED, SEC_OBS, N_SECTIONS };
struct SectionRow { bool scalar; int per_sample, per_track, once; };   // elements per trajectory = per_sample K + per_track f_cap + once
constexpr SectionRow SECTIONS[N_SECTIONS] = {
    /* rd    */ {true, RD_ROW, 0, 0},   // the cell's IMU readings, K rows (those beyond its k are padding that nothing reads)
    /* n     */ {false, 0, 0, 1},       // tracks of the cell
    /* drop  */ {false, 0, 0, 1},       // camera states the frame's prune drops
    /* k     */ {false, 0, 0, 1},       // the cell's own number of IMU samples, or NO_IMAGE
    /* M     */ {false, 0, 1, 0},       // track lengths, zero beyond n
    /* off   */ {false, 0, 1, 0},       // first entry of each track, counted from the frame's first entry
    /* slots */ {false, 0, 0, 0},       // per entry: the camera slot
    /* obs   */ {true, 0, 0, 0},        // per entry: the coordinate pair
};
struct FrameLayout {
  int B = 0, K = 0, f_cap = 0; size_t esz = 0;
  size_t stride[N_FIXED] = {0};        // bytes per trajectory of a fixed section
  size_t at[N_FIXED + 1] = {0};        // streamed block: 256-byte-aligned offsets of the fixed sections and of slots
  FrameLayout() {}
  FrameLayout(int B_, int K_, int f_cap_, size_t esz_) : B(B_), K(K_), f_cap(f_cap_), esz(esz_) {
    for (int s = 0; s < N_FIXED; ++s) {
      stride[s] = (size_t)(SECTIONS[s].per_sample * K + SECTIONS[s].per_track * f_cap + SECTIONS[s].once) * elem(s);
      at[s + 1] = align_up(at[s] + (size_t)B * stride[s], 256);
    }
  }
  size_t elem(int s) const { return SECTIONS[s].scalar ? esz : sizeof(int); }
  size_t frame_bytes(int s) const { return (size_t)B * stride[s]; }                 // a fixed section of one frame
  size_t entry_bytes(int s) const { return s == SEC_OBS ? 2 * esz : sizeof(int); }   // a variable section, per entry
  // streamed block of a frame with nf entries
  size_t off_obs(size_t nf) const { return align_up(at[SEC_SLOTS] + nf * sizeof(int), 256); }
  size_t bytes(size_t nf) const { return align_up(off_obs(nf) + 2 * nf * esz, 256); }
  size_t block_at(int s, size_t nf) const { return s == SEC_OBS ? off_obs(nf) : at[s]; }
  // resident arrays (one per section, all frames): where frame f starts, `base` entries before it
  size_t resident_at(int s, int f, size_t base) const { return s < N_FIXED ? (size_t)f * frame_bytes(s) : base * entry_bytes(s); }
};

// where a frame's inputs are, for a slice that starts at trajectory b0: per-trajectory arrays already offset to b0, slots / obs
// the frame's compact entries (tracks find theirs through off)
template <class S> struct FrameIn { const S* rd; const int* n; const int* M; const int* off; const int* slots; const S* obs; const int* drop; const int* k; };
// where(s): the start of section s of this frame (trajectory 0)
template <class S, class Where> FrameIn<S> frame_in(const FrameLayout& L, int b0, Where where) {
  auto p = [&](int s) { return static_cast<const unsigned char*>(where(s)) + (s < N_FIXED ? (size_t)b0 * L.stride[s] : 0); };
  auto i = [&](int s) { return reinterpret_cast<const int*>(p(s)); };
  auto x = [&](int s) { return reinterpret_cast<const S*>(p(s)); };
  return FrameIn<S>{x(SEC_RD), i(SEC_N), i(SEC_M), i(SEC_OFF), i(SEC_SLOTS), x(SEC_OBS), i(SEC_DROP), i(SEC_K)};
}

// ---- 3. the scenario's host store
// Work-lists are COMPACT: a cell (frame, trajectory) holds sum M_j (slot, observation) entries, track t of the cell starts at
// off[cell][t] counted from the frame's first entry -- not [f_cap][m_cap] padded rows (1.9x the payload at cfg3's track lengths,
// on the host, in HBM and in every per-frame upload).  Scalars (readings, coordinates) are kept as bytes of esz each.
struct ScenarioStore {
  int frames = 0;
  FrameLayout lay;
  std::vector<unsigned char> fixed[N_FIXED];                        // [frames][B] cells of each fixed section
  std::vector<std::vector<int>> slots; std::vector<std::vector<unsigned char>> obs;   // per cell: its entries
  std::vector<int> maxslot;                                         // per cell the largest camera slot its work-list touches, or -1
  std::vector<size_t> fr_base;                                      // [frames + 1] first entry of a frame among all entries
  int* ints(int s) { return reinterpret_cast<int*>(fixed[s].data()); }
  const int* ints(int s) const { return reinterpret_cast<const int*>(fixed[s].data()); }
  // every cell: no track, no drop, K samples of zero readings
  void reset(int n_frames, int B, int K, int f_cap, size_t esz) {
    lay = FrameLayout(B, K, f_cap, esz);
    const size_t FB = (size_t)n_frames * B;
    for (int s = 0; s < N_FIXED; ++s) fixed[s].assign((size_t)n_frames * lay.frame_bytes(s), 0);
    std::fill(ints(SEC_K), ints(SEC_K) + FB, K);
    slots.assign(FB, std::vector<int>()); obs.assign(FB, std::vector<unsigned char>());
    maxslot.assign(FB, -1);
    fr_base.assign((size_t)n_frames + 1, 0);
    frames = n_frames;
  }
  // one cell (the caller has checked it: worklist_refusal, cell_refusal); off waits for index()
  template <class S> void set_cell(int f, int b, const double* rd, int k, bool skip, int F, const int* M, const int* sl, const double* ob, int n_drop) {
    const size_t cell = (size_t)f * lay.B + b;
    size_t tot = 0;
    for (int t = 0; t < F; ++t) tot += M[t];
    S* hr = reinterpret_cast<S*>(fixed[SEC_RD].data()) + cell * lay.K * RD_ROW;
    for (int s = 0; s < lay.K; ++s) for (int c = 0; c < RD_ROW; ++c) hr[s * RD_ROW + c] = s < k ? (S)rd[s * RD_ROW + c] : S(0);   // (padding beyond k: never read again)
    ints(SEC_N)[cell] = F; ints(SEC_DROP)[cell] = n_drop; ints(SEC_K)[cell] = skip ? NO_IMAGE : k;
    for (int t = 0; t < lay.f_cap; ++t) ints(SEC_M)[cell * lay.f_cap + t] = t < F ? M[t] : 0;
    slots[cell].assign(sl, sl + tot);
    obs[cell].resize(2 * tot * sizeof(S));
    S* co = reinterpret_cast<S*>(obs[cell].data());
    int mx = -1;
    for (size_t e = 0; e < tot; ++e) { mx = std::max(mx, sl[e]); co[2 * e] = (S)ob[2 * e]; co[2 * e + 1] = (S)ob[2 * e + 1]; }
    maxslot[cell] = mx;
  }
  // every off and fr_base from the cells as they stand; false: a frame holds more than 2^31 - 1 entries
  bool index() {
    const size_t B = lay.B, f_cap = lay.f_cap;
    int* off = ints(SEC_OFF); const int* M = ints(SEC_M);
    size_t total = 0;
    for (int f = 0; f < frames; ++f) {
      fr_base[f] = total;
      size_t in_frame = 0;
      for (size_t b = 0; b < B; ++b) {
        const size_t cell = (size_t)f * B + b;
        size_t o = in_frame;
        for (size_t t = 0; t < f_cap; ++t) { off[cell * f_cap + t] = (int)o; o += M[cell * f_cap + t]; }
        in_frame += slots[cell].size();
      }
      if (in_frame > 0x7fffffffu) return false;
      total += in_frame;
    }
    fr_base[frames] = total;
    return true;
  }
  size_t total() const { return fr_base[frames]; }
  size_t entries(int f) const { return fr_base[f + 1] - fr_base[f]; }
  size_t largest_frame() const { size_t mx = 0; for (int f = 0; f < frames; ++f) mx = std::max(mx, entries(f)); return mx; }
  // the compact cells of frame f, trajectory after trajectory, as one contiguous block: slots to hs, coordinates to ho
  void gather(int f, int* hs, unsigned char* ho) const {
    size_t o = 0;
    for (int b = 0; b < lay.B; ++b) {
      const size_t cell = (size_t)f * lay.B + b, n = slots[cell].size();
      if (n) { std::memcpy(hs + o, slots[cell].data(), n * sizeof(int)); std::memcpy(ho + 2 * o * lay.esz, obs[cell].data(), 2 * n * lay.esz); }
      o += n;
    }
  }
  // where frame f's cells of a fixed section start in the store
  const unsigned char* frame_cells(int s, int f) const { return fixed[s].data() + lay.resident_at(s, f, 0); }
  // frame f's streamed block, lay.bytes(entries(f)) bytes: the sections at their offsets (the gaps between them are not written)
  void write_block(int f, unsigned char* blk) const {
    for (int s = 0; s < N_FIXED; ++s) std::memcpy(blk + lay.at[s], frame_cells(s, f), lay.frame_bytes(s));
    gather(f, reinterpret_cast<int*>(blk + lay.at[SEC_SLOTS]), blk + lay.off_obs(entries(f)));
  }
};

}  // namespace msckf_inputs

#endif  // MSCKF_INPUT_LAYOUTS_H
