// msckf_hip.hip -- host side of libmsckf_hip.so: batch handle, track bookkeeping, C-ABI (include/msckf_hip.h).
//
// The host keeps exactly what the reference keeps on the host side of its hot loop -- the integer /
// std::find bookkeeping of MSCKF::update / addFeatures / removeTrackedFeature / pruneEmptyStates
// (msckf.h:215-332, 685-717, 1469-1485) -- and turns it into positional work-lists for the device.
// Everything numerical (msckf.h:101-212, 336-449, 905-1423) runs in the HIP kernels of kernels_*.hip; there
// is no CPU fallback: if no HIP device is usable msckf_hip_create fails.
// A handle is a BatchCore -- everything that is the same for float and double: streams, staging, the frame loops run_frames /
// run_frames_streamed -- with the typed half Batch<S> on top: the device
// buffers, the launches, the conversions between S and double.  What one frame of a scenario enqueues is
// Batch<S>::enqueue_frame; the per-filter entries are the range entries with nb = 1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>
#include <pthread.h>
#include <sched.h>

#include "../../include/msckf_hip.h"
#include "dev_common.h"
#include "frame_order.h"
#include "host_lists.h"
#include "input_layouts.h"
#include "nees_plan.h"
#include "traj_plan.h"
#include "replay_plan.h"
#include "settings.h"
#include "slice_policy.h"
#include "track_compile.h"

namespace {
using namespace msckf;
using namespace msckf_lists;
using msckf_settings::Settings;
namespace inputs = msckf_inputs;
static_assert(inputs::RD_ROW == RD_STRIDE && inputs::NO_IMAGE == IMU_SKIP, "input_layouts.h restates the reading's stride and the skipped cell's count");
static_assert(TRK_MOTION_OK == ST_MOTION_OK && TRK_TRI_VALID == ST_TRI_VALID && TRK_MOTION_SKIPPED == ST_MOTION_SKIPPED, "host_lists.h reads the feature kernel's status bits");

// rocTX ranges under the reference's stage names (asl_msckf.cpp:229-296: imu_prop, msckf_augment_state, msckf_update,
// msckf_add_features, msckf_marginalize, msckf_prune_redundant, msckf_prune_empty_states) around the host side of every stage,
// so that a `rocprofv3 --marker-trace` timeline of a caller reads like the reference's StageTiming message.  Off unless
// MSCKF_HIP_ROCTX=1; the marker library is opened at run time (no link dependency).
struct Roctx {
  int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
  Roctx() {
    const char* e = getenv("MSCKF_HIP_ROCTX");
    if (!e || !atoi(e)) return;
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!push || !pop) { push = nullptr; pop = nullptr; }
  }
};
const Roctx& roctx() { static Roctx r; return r; }
struct StageRange {
  bool on;
  explicit StageRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
  ~StageRange() { if (on) roctx().pop(); }
};

// the text behind msckf_hip_last_error(), per calling thread
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return fail(-EIO, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

constexpr int NSTAGE = 13;   // 0..7: msckf_hip_profile_read; 8 k_lit_pre, 9 k_lit_gamma, 10 k_literal, 11 k_replay_expand, 12 k_replay_walk_scan (msckf_hip_profile_read_ex)

// Persistent enqueue threads of a batch (one per slice of run_frames / run_frames_streamed): a K-frame window is a few
// milliseconds, creating and joining three std::threads per call was 1-2 % of it.
struct Workers {
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv, cv_done;
  std::function<void(int)> job;
  unsigned long gen = 0;
  int active = 0, pending = 0;
  bool stop = false;
  // worker idx runs on cpus[idx + 1] (cpus[0] is the calling thread's: the uploader of run_frames_streamed) when a list was
  // given (msckf_hip_set_host_affinity): the hand-overs between the uploading thread and the slices' enqueue threads are
  // spin waits, and a waiter that the scheduler moves or parks costs a frame's worth of time
  std::vector<int> cpus;
  // cpu >= 0: pin the calling worker to it (its original mask is saved on the first pin); cpu < 0: back to the original mask
  static void pin_self(int cpu, cpu_set_t* orig, bool* have_orig) {
    if (cpu < 0) {
      if (*have_orig) (void)pthread_setaffinity_np(pthread_self(), sizeof(*orig), orig);
      return;
    }
    if (!*have_orig) { if (pthread_getaffinity_np(pthread_self(), sizeof(*orig), orig) == 0) *have_orig = true; }
    cpu_set_t set; CPU_ZERO(&set); CPU_SET(cpu, &set);
    (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
  }
  void loop(int idx) {
    unsigned long seen = 0;
    int pinned = -2;
    cpu_set_t orig; bool have_orig = false;
    for (;;) {
      std::function<void(int)> f;
      {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen;
        if (idx >= active) continue;
        f = job;
        const int want = idx + 1 < (int)cpus.size() ? cpus[idx + 1] : -1;
        if (want != pinned) { pin_self(want, &orig, &have_orig); pinned = want; }
      }
      f(idx);
      { std::lock_guard<std::mutex> lk(m); if (--pending == 0) cv_done.notify_all(); }
    }
  }
  // run f(0) .. f(n - 1) on the worker threads (not on the caller); wait() returns when all have finished
  void start(int n, std::function<void(int)> f) {
    while ((int)th.size() < n) { const int idx = (int)th.size(); th.emplace_back([this, idx] { loop(idx); }); }
    { std::lock_guard<std::mutex> lk(m); job = std::move(f); active = n; pending = n; ++gen; }
    cv.notify_all();
  }
  void wait() { std::unique_lock<std::mutex> lk(m); cv_done.wait(lk, [&] { return pending == 0; }); }
  ~Workers() {
    { std::lock_guard<std::mutex> lk(m); stop = true; }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
};

struct BatchCore {
  int B = 0, n_cap = 0, f_cap = 0, m_cap = 0, dtype = 0, device = 0;
  bool h16 = false;   // dtype MSCKF_HIP_F16H_F32P: fp16 measurement Jacobian, f32 state and covariance
  size_t esz = 0;     // sizeof(S) of the typed half (set with the handle's dtype): element size of every buffer the core only moves as bytes
  std::vector<HostTraj> traj;
  hipStream_t st = nullptr;
  static constexpr int MAXS = 8;     // run_frames can run up to MAXS slices of the batch concurrently
  hipStream_t stx[MAXS] = {nullptr}; // stx[0] == st
  hipEvent_t ev_fork = nullptr, ev_join[MAXS] = {nullptr};
  std::vector<void*> allocs;
  // pinned host staging of the per-call inputs (single-filter API): filled, copied asynchronously, reused only after
  // ev_stage says the previous copy has left it -- the calls themselves do not wait for the device
  // (a ring of NSTG areas: a call takes the next one and only waits if the copy made out of it NSTG calls ago is still in
  // flight -- with a single area every propagate() of the per-sample API waited for the previous sample's copy)
  static constexpr int NSTG = 8;
  unsigned char* h_stage[NSTG] = {nullptr}; size_t h_stage_bytes[NSTG] = {0}; hipEvent_t ev_stage[NSTG] = {nullptr}; bool stage_busy[NSTG] = {false};
  int stage_cur = 0;
  // host mirror of ncam[] (every call that changes the window size updates it)
  std::vector<int> h_ncam;
  hipStream_t sty[MAXS] = {nullptr}; hipEvent_t ev_fa[MAXS] = {nullptr}, ev_fb[MAXS] = {nullptr};
  // every tunable of the handle (settings.h: defaults, environment variables, what a copy takes over); the typed half's
  // apply_settings() carries them into the kernel argument
  Settings settings;
  msckf_settings::FrameSettings frame_settings;   // the frame step's launch order (settings.h)
  // frames of a slice (one count per slice and frame) that took the feature-first order (routes::frame_order) since the handle
  // was created; the slices' enqueue threads count concurrently
  std::atomic<long long> n_feature_first{0};
  // ... and those of them that took order 2, propagate + augmentState inside the Gram Cholesky's launch (routes::frame_order_chol)
  std::atomic<long long> n_in_cholesky{0};
  int small_limit = 0;      // settings.small_update as far as it fits k_update_small at this handle's dtype and f_cap (apply_settings): the per-trajectory limit launch_update routes by
  bool info_form = false;    // the information form's buffers exist (Dev::trk_B; set by the typed half's create)
  std::vector<double> h_uv;  // [B][2] u_var', v_var' as initialize() got them
  std::vector<char> h_imu_ok;   // [B] the typed half's host copy of the IMU state is current (see Batch<S>::h_imu)
  std::vector<char> h_lit;   // [B] trajectory runs the literal route
  std::vector<char> h_qfull; // [B] trajectory carries a full Q_imu (its qf flag): k_propagate's full-Q instantiation runs it
  // launch_propagate's qroute for [b0, b0 + nb): 0 no trajectory with a full Q_imu, 1 some, 2 all
  int qroute(int b0, int nb) const {
    int n = 0;
    for (int b = b0; b < b0 + nb; ++b) n += h_qfull[b] ? 1 : 0;
    return n == 0 ? 0 : (n == nb ? 2 : 1);
  }
  int n_lit = 0;
  // the device arrays of plain integers, as the typed half's create allocated them (Dev::ncam, ::n_resid, ::stats)
  int* dv_ncam = nullptr; long long* dv_nres = nullptr; int* dv_stats = nullptr;
  int rd_cap = 0;   // samples per trajectory that the single-call staging of propagate holds
  void* h_rb = nullptr;   // page-locked landing area of the single-filter state read (get_cams_known): [n_cap][CAM_STRIDE] + [IMU_STRIDE] scalars
  // single-call work-lists (input_layouts.h, SingleBlock): per trajectory wl_blk.ib ints on the device, the typed half's
  // coordinates beside them
  inputs::SingleBlock wl_blk; int* wl_i = nullptr;
  // scenario (input_layouts.h): the staged cells and the frame index on the host (sc; sc.frames == 0: none), and the resident
  // copy a commit makes of them, one device array per section (SECTIONS), sc_total entries in the two variable ones
  inputs::ScenarioStore sc;
  bool committed = false;
  unsigned char* sc_dev[inputs::N_SECTIONS] = {nullptr}; size_t sc_total = 0;
  std::vector<void*> sc_allocs;
  // streamed inputs (run_frames_streamed): frame f's block (input_layouts.h, FrameLayout) is copied from page-locked
  // host memory into one of `ring` device staging sets on a copy stream, `ring` - 1 frames ahead of the kernels that read it.
  // Page-locked blocks are built on demand (scen_pin, or the first streamed run over a frame), only for frames that are
  // streamed: a run_frames-only user never pays for them.
  static constexpr int RING_MAX = 8;
  hipStream_t stc = nullptr; hipEvent_t ev_up[RING_MAX] = {nullptr}; hipEvent_t ev_use[RING_MAX][MAXS] = {{nullptr}};
  unsigned char* sg_blk[RING_MAX] = {nullptr}; size_t sg_bytes = 0;
  struct PinFrame { unsigned char* p = nullptr; size_t bytes = 0; int chunk = -1; };
  struct PinChunk { void* p = nullptr; int live = 0; };   // page-locked block of several frames; freed when its last frame is invalidated
  std::vector<PinFrame> pinf; std::vector<PinChunk> pin_chunks;
  void unpin_frame(int f) {
    const int c = pinf[f].chunk;
    if (c >= 0 && c < (int)pin_chunks.size() && pin_chunks[c].p && --pin_chunks[c].live == 0) {
      if (stc) (void)hipStreamSynchronize(stc);     // the last copy out of the block has completed
      (void)hipHostFree(pin_chunks[c].p);
      pin_chunks[c].p = nullptr;
    }
    pinf[f] = PinFrame();
  }
  void unpin_host() {
    for (auto& q : pin_chunks) if (q.p) hipHostFree(q.p);
    pin_chunks.clear();
    for (auto& pf : pinf) pf = PinFrame();
  }
  // Monte-Carlo replay (replay_plan.h; kernels_replay.hip): the plan on the host; on the device the sequence store (one array
  // per section as a resident scenario has them, scalars double), the assignment with every frame's bases, one expanded frame
  // block per slice (rp_blk: slices are at different frames at the same time, and where a trajectory's entries start depends on
  // the frame) and the scratch block of replay_expand.  rp_cells: per slice the host's k / drop / maxslot of the frame's cells,
  // looked up through seq_of by the slice's enqueue thread.  Under the Q_imu model (rp.model) rp_sigma holds sigma_uv, and the
  // factors, the scales and the walk table [frames + 1][B][6] (k_replay_walk_scan; rp.walk_planned) are on the device as well.
  msckf_replay::Plan rp;
  unsigned char* rp_dev[inputs::N_SECTIONS] = {nullptr}; std::vector<int> rp_maxcell;   // rp_maxcell [frames]: entries of the frame's largest sequence cell
  int* rp_seq_of = nullptr; uint64_t* rp_seed = nullptr; double* rp_sigma = nullptr; int* rp_base = nullptr; size_t rp_base_count = 0;
  bool rp_uploaded = false;                                  // the assignment and the bases on the device are the plan's
  double* rp_L = nullptr; double* rp_scale = nullptr; double* rp_wstart = nullptr; size_t rp_wstart_count = 0;
  unsigned char* rp_blk[MAXS] = {nullptr}; size_t rp_blk_bytes = 0;
  unsigned char* rp_scratch = nullptr; size_t rp_scratch_bytes = 0;
  // the fault record fault4[B][4] (zeros while none is set; rp.faults_uploaded) and replay_expand_faults' codes, one per entry of
  // the largest expanded frame
  double* rp_fault = nullptr; int* rp_code = nullptr; size_t rp_code_count = 0;
  // the timing record timing4[B][4] (zeros while none is set; rp.timing_uploaded), the sequences' image tables as commit built
  // them (time / frame_of [S][frames], base [frames][S]) and replay_expand_timing's deltas, one per entry of the largest frame
  double* rp_timing = nullptr; double* rp_img_time = nullptr; int* rp_img_frame = nullptr; int* rp_img_base = nullptr;
  double* rp_delta = nullptr; size_t rp_delta_count = 0;
  // the calibration records imucal[B][31] and camcal[B][8] (the identity and zeros while none is set; rp.calib_uploaded) and
  // replay_expand_calib's outputs: rd_cal / clip [K][6], obs_cal one pair per entry of the largest frame
  double* rp_imucal = nullptr; double* rp_camcal = nullptr; double* rp_rdcal = nullptr; int* rp_clip = nullptr; size_t rp_rdcal_count = 0;
  double* rp_obscal = nullptr; size_t rp_obscal_count = 0;
  std::vector<int> rp_cells[MAXS];
  Workers workers;   // enqueue threads of the slices
  // frame log (msckf_hip_frame_log_*; kernels_log.hip): [log_cap][B][LOG_STRIDE] scalars of esz bytes, null unless enabled.  log_n
  // counts the records written; a run_frames / run_frames_streamed call over [f0, f1) writes the records log_base + (f - f0)
  // (log_base = log_n at its start, read by the slices' enqueue threads) and advances log_n when it has succeeded
  void* log_buf = nullptr; int log_cap = 0, log_n = 0, log_base = 0;
  // A cursor log (kernels_log.hip): buf [B][cap][stride] scalars of esz bytes and the device cursors found[B] (records found
  // per trajectory, stored or not), null unless enabled.  ord counts the frame ordinals handed out; a run_frames /
  // run_frames_streamed call over [f0, f1) stamps its records with ordinal(f, f0) (base = ord at its start, read by the
  // slices' enqueue threads) and advances ord when it has succeeded.  name and api word the messages.
  struct CursorLog {
    int stride; const char* name; const char* api;
    void* buf = nullptr; int* found = nullptr; int cap = 0, ord = 0, base = 0;
    int ordinal(int f, int f0) const { return base + (f - f0); }
  };
  // map log (msckf_hip_map_log_*): one record per triangulated track
  CursorLog map{MAP_STRIDE, "map log", "msckf_hip_map_log"};
  // pruned-state log (msckf_hip_pruned_log_*): one record per dropped camera state.  While it is on no frame's prune rides on
  // the downdate (fuse_frame): the record is read between the update and the prune launch.  prn_list (host_lists.h) knows
  // which image's camera a record is; it is written by the enqueue thread of the trajectory's slice only (the loop at the end
  // of enqueue_frame that mirrors augment and drop into h_ncam).
  CursorLog prn{PRN_STRIDE, "pruned-state log", "msckf_hip_pruned_log"};
  PrunedFifo prn_list;
  // NEES log (msckf_hip_nees_log_*; nees_plan.h, kernels_log.hip): dense like the frame log, [nees_cap][B][REC] doubles whatever
  // the handle's dtype, null unless enabled; nees_n / nees_base as log_n / log_base.  The truth table it is taken against
  // (msckf_hip_truth_set): tru [tru_frames][tru_rows][TRUTH_ROW] doubles and tru_row_of[B] on the device, tru_frames == 0: none;
  // tru_walk: row f + 1 of the replay's walk table is added to the true biases of frame f (run_frames_replay only).
  // nees_replay: the call in flight is the replay's (set by the reserve, read by the slices' enqueue threads)
  double* nees_buf = nullptr; int nees_cap = 0, nees_n = 0, nees_base = 0; bool nees_replay = false;
  double* tru = nullptr; int* tru_row_of = nullptr; int tru_frames = 0, tru_rows = 0; bool tru_walk = false;
  // profiling
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool[NSTAGE];
  size_t ev_used[NSTAGE] = {0};
  double prof_ms[NSTAGE] = {0}; int prof_cnt[NSTAGE] = {0};

  // `count` zeroed elements of `elem` bytes on the device, freed with the handle
  template <class T> int dalloc(T** p, size_t count, size_t elem = sizeof(T)) {
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, std::max<size_t>(count, 1) * elem));
    HIPCHK(hipMemsetAsync(q, 0, std::max<size_t>(count, 1) * elem, st));
    allocs.push_back(q);
    *p = (T*)q;
    return 0;
  }
  // the settings the environment gives, the device's tables, streams and events, host mirrors; then the typed half's buffers
  int create() {
    { std::string err; if (!msckf_settings::settings_from_env(settings, err)) return fail(-EINVAL, err); }
    HIPCHK(hipSetDevice(device));
    feature_device_setup(); qr_device_setup(); kalman_device_setup(); gram_device_setup(); literal_device_setup();   // per device: constant tables, dynamic-LDS limits
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (int i = 0; i < NSTG; ++i) HIPCHK(hipEventCreateWithFlags(&ev_stage[i], hipEventDisableTiming));
    stx[0] = st;
    // every stream up front, in this order: the runtime places a stream on a hardware queue when it is made, and this order is
    // the one whose placement is measured (the slices' streams on queues of their own as far as the budget goes).  Making them
    // when a frame loop first needs them changed the placement: measured, 3 slices on 4 queues and 4 slices on 8 queues then
    // lost a third of their rate (profiles/hw_queue_slices.md, "streams made on first use")
    for (int i = 1; i < MAXS; ++i) HIPCHK(hipStreamCreateWithFlags(&stx[i], hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    for (int i = 1; i < MAXS; ++i) HIPCHK(hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming));
    for (int i = 0; i < MAXS; ++i) {
      HIPCHK(hipStreamCreateWithFlags(&sty[i], hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&ev_fa[i], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&ev_fb[i], hipEventDisableTiming));
    }
    h_ncam.assign(B, 0); h_uv.assign((size_t)2 * B, 0.0); h_lit.assign(B, 0); h_qfull.assign(B, 0); h_imu_ok.assign(B, 0);
    traj.assign(B, HostTraj());
    return alloc();
  }
  virtual ~BatchCore() {
    hipSetDevice(device);
    if (st) hipStreamSynchronize(st);
    for (void* p : allocs) hipFree(p);
    release_logs();
    free_replay_device();
    if (h_rb) hipHostFree(h_rb);
    for (int s = 0; s < NSTAGE; ++s) for (auto& e : ev_pool[s]) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (int i = 1; i < MAXS; ++i) { if (stx[i]) hipStreamDestroy(stx[i]); if (ev_join[i]) hipEventDestroy(ev_join[i]); }
    for (int i = 0; i < MAXS; ++i) { if (sty[i]) hipStreamDestroy(sty[i]); if (ev_fa[i]) hipEventDestroy(ev_fa[i]); if (ev_fb[i]) hipEventDestroy(ev_fb[i]); }
    if (ev_fork) hipEventDestroy(ev_fork);
    for (int i = 0; i < NSTG; ++i) if (ev_stage[i]) hipEventDestroy(ev_stage[i]);
    unpin_host();
    for (int k = 0; k < RING_MAX; ++k) { if (ev_up[k]) hipEventDestroy(ev_up[k]); for (int i = 0; i < MAXS; ++i) if (ev_use[k][i]) hipEventDestroy(ev_use[k][i]); if (sg_blk[k]) hipFree(sg_blk[k]); }
    if (stc) hipStreamDestroy(stc);

    for (int i = 0; i < NSTG; ++i) if (h_stage[i]) hipHostFree(h_stage[i]);
    if (st) hipStreamDestroy(st);
  }
  // ---- what the head of an entry checks
  int chk(int b) const { return (b < 0 || b >= B) ? -EINVAL : 0; }
  int chk_range(int b0, int nb) const { return (b0 < 0 || nb < 0 || b0 + nb > B) ? -EINVAL : 0; }
  // A run_frames / run_frames_streamed call that failed after some of its frames were enqueued leaves the slices at different
  // frames: which covariance buffer is current (the fused prune flips them per frame) and whether a window size is still
  // deferred differ per slice, and nothing can put that right.  The handle refuses further work instead of answering from a
  // stale buffer; the caller destroys it.
  bool poisoned = false;
  int poison(int rc, const std::string& msg) {
    (void)hipDeviceSynchronize();
    poisoned = true;
    return fail(rc, msg + " -- frames of this call were already enqueued: the filter states of this handle are undefined, destroy it");
  }
  // `if (int rc = guard()) return rc;` at the head of an entry that must not answer from a poisoned handle
  int guard() const { return poisoned ? fail(-EIO, "handle unusable after a failed run_frames call (destroy it)") : 0; }
  // `if (int rc = enter()) return rc;` before an entry's first device call: this handle's device is current, and the IMU samples
  // of propagate() calls that have not reached the device yet (see propagate()) are on their way
  int enter() {
    HIPCHK(hipSetDevice(device));
    return pend_b >= 0 ? flush_pending() : 0;
  }
  // the same after the check of the entry's trajectory index, or of its range
  int enter_traj(int b) { return chk(b) ? fail(-EINVAL, "trajectory index out of range") : enter(); }
  int enter_range(int b0, int nb) { return chk_range(b0, nb) ? fail(-EINVAL, "trajectory range out of bounds") : enter(); }
  // pinned staging area of at least `bytes`, safe to overwrite (the previous asynchronous copy out of it has finished)
  int stage_acquire(size_t bytes, unsigned char** out) {
    stage_cur = (stage_cur + 1) % NSTG;
    const int rc = stage_grow(stage_cur, bytes, true);
    *out = h_stage[stage_cur];
    return rc;
  }
  int stage_release() { HIPCHK(hipEventRecord(ev_stage[stage_cur], st)); stage_busy[stage_cur] = true; return 0; }
  // slot k of the ring at least `bytes`; wait: first for the copy still in flight out of it (a slot that is re-allocated is
  // always waited for)
  int stage_grow(int k, size_t bytes, bool wait) {
    const bool grow = bytes > h_stage_bytes[k];
    if ((wait || grow) && stage_busy[k]) { HIPCHK(hipEventSynchronize(ev_stage[k])); stage_busy[k] = false; }
    if (!grow) return 0;
    if (h_stage[k]) HIPCHK(hipHostFree(h_stage[k]));
    h_stage[k] = nullptr; h_stage_bytes[k] = 0;
    const size_t nb = std::max<size_t>(bytes, 1 << 12);
    HIPCHK(hipHostMalloc((void**)&h_stage[k], nb, hipHostMallocDefault));
    h_stage_bytes[k] = nb;
    return 0;
  }
  // every slot of the ring at least `bytes` (a commit walks the ring once per frame: without this each slot would be freed and
  // re-allocated as the frames grow)
  int stage_reserve(size_t bytes) {
    for (int k = 0; k < NSTG; ++k) { const int rc = stage_grow(k, bytes, false); if (rc) return rc; }
    return 0;
  }
  // copy on st + wait: what the getters and setters of single values do
  int read_back(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  int write_dev(void* dst, const void* src, size_t bytes) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  // ---- profiling helpers
  void stage_begin(int s, hipStream_t q) {
    if (!prof) return;
    if (ev_used[s] == ev_pool[s].size()) {
      hipEvent_t a, b2; hipEventCreate(&a); hipEventCreate(&b2);
      ev_pool[s].push_back({a, b2});
    }
    hipEventRecord(ev_pool[s][ev_used[s]].first, q);
  }
  void stage_end(int s, hipStream_t q) {
    if (!prof) return;
    hipEventRecord(ev_pool[s][ev_used[s]].second, q);
    ev_used[s]++;
  }

  // the rules for one trajectory's work-list (input_layouts.h), checked before anything of it is staged or written
  int check_worklist(int F, const int* M, const int* slots) const {
    const inputs::Refusal r = inputs::worklist_refusal(F, M, slots, f_cap, m_cap, n_cap);
    return r.code ? fail(r.code, r.why) : 0;
  }
  void invalidate_imu(int b0, int nb) { for (int b = b0; b < b0 + nb && b < B; ++b) h_imu_ok[b] = 0; }
  // Single-filter API (the shim's propagate(), one call per IMU sample, msckf.h:101): while the host copy of the IMU state is
  // valid it answers getImuState(), so the samples need not reach the device one by one -- they wait here and go as ONE copy +
  // ONE k_propagate launch when anything else touches the device (enter() at the head of every other entry).  Ten calls per
  // image were ten pinned-memory copies and ten launches (~6 us of host time each) for the same device-side result.
  std::vector<double> pend_rd; int pend_b = -1;
  int flush_pending(bool then_augment = false) {
    if (pend_b < 0) return 0;
    const int b = pend_b; pend_b = -1;
    std::vector<double> rd; rd.swap(pend_rd);
    if (hipSetDevice(device) != hipSuccess) { h_imu_ok[b] = 0; return fail(-EIO, "hipSetDevice failed"); }
    const int rc = propagate_device(inputs::Readings(rd.data(), 1, (int)(rd.size() / RD_STRIDE)), b, then_augment);
    if (rc) h_imu_ok[b] = 0;   // the samples are gone and the device never saw them: the host copy is ahead of the filter, drop it (getImuState() re-reads the device)
    return rc;
  }
  int propagate(int b0, int nb, const double* rd, int K, bool mirror = false) {
    if (int rc = guard()) return rc;
    if (chk_range(b0, nb)) return fail(-EINVAL, "trajectory range out of bounds");
    if (K < 0) return fail(-EINVAL, "negative sample count");
    if (mirror && nb == 1 && h_imu_ok[b0]) {
      if (pend_b >= 0 && pend_b != b0) { const int rc = flush_pending(); if (rc) return rc; }   // first: a failure here must not leave b0's host copy advanced with nothing queued
      mirror_advance(b0, rd, K);
      pend_b = b0; pend_rd.insert(pend_rd.end(), rd, rd + (size_t)K * RD_STRIDE);
      return 0;
    }
    if (!(mirror && nb == 1)) invalidate_imu(b0, nb);
    if (int rc = enter()) return rc;
    return propagate_device(inputs::Readings(rd, nb, K), b0);
  }
  // propagate() with a sample count per trajectory: rd holds K[0] rows, then K[1] rows, ...
  int propagate_counts(int b0, int nb, const double* rd, const int* K) {
    if (int rc = guard()) return rc;
    if (chk_range(b0, nb)) return fail(-EINVAL, "trajectory range out of bounds");
    for (int i = 0; i < nb; ++i) if (K[i] < 0) return fail(-EINVAL, "negative sample count K[" + std::to_string(i) + "]");
    for (int i = 0; i < nb; ++i) if (K[i] > 0) invalidate_imu(b0 + i, 1);
    if (int rc = enter()) return rc;
    return propagate_device(inputs::Readings(rd, nb, K), b0);
  }
  // ---- the device's integer arrays
  // last_stats of a marginalize() that had nothing to residualize (the reference returns early, msckf.h:337)
  int clear_stats(int b) {
    if (int rc = enter_traj(b)) return rc;
    HIPCHK(hipMemsetAsync(dv_stats + (size_t)b * STAT_STRIDE, 0, sizeof(int) * STAT_ERR, st));
    return 0;
  }
  int clear_errors(int b) {
    if (int rc = enter_traj(b)) return rc;
    HIPCHK(hipMemsetAsync(dv_stats + (size_t)b * STAT_STRIDE + STAT_ERR, 0, sizeof(int), st));
    return 0;
  }
  // the window size from the host's own count (kept through every entry that changes it): no device read.  A poisoned handle's
  // count is not to be trusted (its slices may have stopped at different frames)
  int ncam_host(int b) const {
    if (chk(b)) return fail(-EINVAL, "trajectory index out of range");
    return poisoned ? guard() : h_ncam[b];
  }
  int get_ncam(int b, int* n) {
    if (int rc = guard()) return rc;
    if (int rc = enter_traj(b)) return rc;
    return read_back(n, dv_ncam + b, sizeof(int));
  }
  int get_nres(int b, long long* n) {
    if (int rc = enter_traj(b)) return rc;
    return read_back(n, dv_nres + b, sizeof(long long));
  }
  int set_nres(int b, long long n) {
    if (int rc = enter_traj(b)) return rc;
    return write_dev(dv_nres + b, &n, sizeof(long long));
  }
  int stats(int b, int* out) {
    if (int rc = guard()) return rc;
    if (int rc = enter_traj(b)) return rc;
    int tmp[STAT_STRIDE];
    if (const int rc = read_back(tmp, dv_stats + (size_t)b * STAT_STRIDE, sizeof(tmp))) return rc;
    for (int i = 0; i < 7; ++i) out[i] = tmp[i];
    if (tmp[STAT_ERR] & STAT_ERR_NCAP) return fail(-EOVERFLOW, "camera-state capacity n_cap exceeded in augmentState");
    if (tmp[STAT_ERR] & STAT_ERR_PIVOT)
      return fail(-EDOM, "non-positive pivot in the factorization of S = T_H P T_H^T + R_n: the covariance lost positive definiteness "
                         "(msckf_hip_set_covariance_update(h, 1) selects the reference's Joseph form)");
    return 0;
  }
  int error_flags(int b, int* flags) {
    if (int rc = enter_traj(b)) return rc;
    return read_back(flags, dv_stats + (size_t)b * STAT_STRIDE + STAT_ERR, sizeof(int));
  }
  // ---- scenario
  void free_scenario_device() {
    for (void* q : sc_allocs) {                                  // a previous scenario is replaced, not leaked
      hipFree(q);
      allocs.erase(std::remove(allocs.begin(), allocs.end(), q), allocs.end());
    }
    sc_allocs.clear();
    for (auto& p : sc_dev) p = nullptr;
    sc_total = 0;
  }
  template <class T> int sc_dalloc(T** p, size_t count, size_t elem = sizeof(T)) {
    const size_t mark = allocs.size();
    const int rc = dalloc(p, count, elem);
    sc_allocs.insert(sc_allocs.end(), allocs.begin() + mark, allocs.end());
    return rc;
  }
  int scen_alloc(int n_frames, int K) {
    if (n_frames <= 0 || K <= 0) return fail(-EINVAL, "bad scenario size");
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(st));
    free_scenario_device();
    committed = false;
    unpin_host();
    sc.reset(n_frames, B, K, f_cap, esz);
    pinf.assign((size_t)n_frames, PinFrame());
    int rc = 0;
    for (int s = 0; s < inputs::N_FIXED; ++s) rc |= sc_dalloc(&sc_dev[s], sc.fixed[s].size(), 1);
    if (rc) sc.frames = 0;
    return rc;
  }
  // H2D of everything staged.  The host copy is kept, so cells may be patched with scenario_set and committed again.
  int scen_commit() {
    using namespace inputs;
    if (sc.frames <= 0) return fail(-EINVAL, "no scenario allocated");
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(st));
    if (!sc.index()) return fail(-E2BIG, "a frame's work-lists exceed 2^31 observations");
    const size_t total = sc.total();
    if (total != sc_total || !sc_dev[SEC_SLOTS]) {          // patched cells may have changed the compact size
      int rc = 0;
      for (int s = N_FIXED; s < N_SECTIONS; ++s) {
        if (void* q = sc_dev[s]) { hipFree(q); allocs.erase(std::remove(allocs.begin(), allocs.end(), q), allocs.end()); sc_allocs.erase(std::remove(sc_allocs.begin(), sc_allocs.end(), q), sc_allocs.end()); }
        sc_dev[s] = nullptr;
      }
      for (int s = N_FIXED; s < N_SECTIONS; ++s) rc |= sc_dalloc(&sc_dev[s], total, sc.lay.entry_bytes(s));
      if (rc) return rc;
      sc_total = total;
    }
    if (int rc = upload_store(sc, sc_dev)) return rc;
    committed = true;
    return 0;
  }
  // an indexed store's cells into its resident arrays dev[N_SECTIONS] (one per section, sized for it), and the wait for the copies
  int upload_store(const inputs::ScenarioStore& q, unsigned char* const* dev) {
    using namespace inputs;
    const size_t per_entry = q.lay.entry_bytes(SEC_SLOTS) + q.lay.entry_bytes(SEC_OBS);
    for (int s = 0; s < N_FIXED; ++s) HIPCHK(hipMemcpyAsync(dev[s], q.fixed[s].data(), q.fixed[s].size(), hipMemcpyHostToDevice, st));
    if (int rc = stage_reserve(q.largest_frame() * per_entry)) return rc;   // the pinned staging ring once, for the largest frame
    for (int f = 0; f < q.frames; ++f) {             // one frame at a time through the pinned staging area (bounded host memory)
      const size_t nf = q.entries(f);
      if (!nf) continue;
      unsigned char* raw = nullptr;
      int rc = stage_acquire(nf * per_entry, &raw);
      if (rc) return rc;
      unsigned char* h[N_SECTIONS] = {nullptr};
      h[SEC_SLOTS] = raw; h[SEC_OBS] = raw + nf * q.lay.entry_bytes(SEC_SLOTS);
      q.gather(f, reinterpret_cast<int*>(h[SEC_SLOTS]), h[SEC_OBS]);
      for (int s = N_FIXED; s < N_SECTIONS; ++s)
        HIPCHK(hipMemcpyAsync(dev[s] + q.lay.resident_at(s, f, q.fr_base[f]), h[s], nf * q.lay.entry_bytes(s), hipMemcpyHostToDevice, st));
      rc = stage_release();
      if (rc) return rc;
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  // page-locked per-frame blocks for run_frames_streamed, frames [f0, f1) that do not have one yet; also sizes the device
  // staging ring.  Called by run_frames_streamed itself; call it beforehand to keep the pinning out of a timed region.
  int scen_pin(int f0, int f1) {
    if (f0 < 0 || f1 > sc.frames || f0 > f1) return fail(-EINVAL, "frame range out of bounds");
    if (!committed) return fail(-EINVAL, "scenario not committed");
    if (int rc = enter()) return rc;
    size_t need = 0, maxb = sg_bytes;
    std::vector<int> todo;
    for (int f = f0; f < f1; ++f) {
      const size_t bytes = sc.lay.bytes(sc.entries(f));
      maxb = std::max(maxb, bytes);
      if (pinf[f].p) continue;
      pinf[f].bytes = bytes;
      need += bytes; todo.push_back(f);
    }
    if (!todo.empty()) {
      unsigned char* chunk = nullptr;
      if (hipHostMalloc((void**)&chunk, need, hipHostMallocDefault) != hipSuccess) {
        for (int f : todo) pinf[f] = PinFrame();
        return fail(-ENOMEM, "could not page-lock the frames to stream (run_frames on the resident scenario is unaffected)");
      }
      int ci = -1;
      for (size_t q = 0; q < pin_chunks.size(); ++q) if (!pin_chunks[q].p) { ci = (int)q; break; }
      if (ci < 0) { pin_chunks.push_back(PinChunk()); ci = (int)pin_chunks.size() - 1; }
      pin_chunks[ci].p = chunk; pin_chunks[ci].live = (int)todo.size();
      size_t o = 0;
      for (int f : todo) {
        unsigned char* blk = chunk + o;
        sc.write_block(f, blk);
        pinf[f].p = blk; pinf[f].chunk = ci;
        o += pinf[f].bytes;
      }
    }
    if (maxb > sg_bytes || !sg_blk[0]) {
      HIPCHK(hipStreamSynchronize(st));
      if (stc) HIPCHK(hipStreamSynchronize(stc));
      for (int k = 0; k < RING_MAX; ++k) { if (sg_blk[k]) hipFree(sg_blk[k]); sg_blk[k] = nullptr; }
      for (int k = 0; k < RING_MAX; ++k) HIPCHK(hipMalloc((void**)&sg_blk[k], maxb));
      sg_bytes = maxb;
    }
    return 0;
  }
  int set_upload_ring(int depth, int mode) {
    if (depth < 2 || depth > RING_MAX || mode < 0 || mode > 1) return fail(-EINVAL, "ring depth 2..8; mode 0 host hand-over, 1 device-side event waits");
    settings.ring = depth;
    return store(&Settings::up_mode, mode);
  }
  // ---- the frame loop of a scenario (run_frames, run_frames_streamed)
  // Trajectories are independent, so the batch may be cut into slices that run the same kernel sequence on separate streams:
  // the latency-bound stages of one slice (gain solve, Cholesky, propagate: one workgroup per trajectory) overlap with the
  // chip-filling stages of the others.  One host thread per slice enqueues that slice's kernels for all frames of the call
  // (~13 launches per frame and slice would otherwise serialise on one thread and make more than two slices launch-bound).
  // Stage profiling forces a single stream.  settings.nstreams is an upper bound: slices that would share a hardware queue run
  // one after the other, so the count is sized to the queues the process has (slice_policy.h states the rule, nothing here decides)
  // hw_queues: the hardware queues of the process, the runtime's default until the caller says otherwise (msckf_hip_set_hw_queues:
  // the library reads no variable of the runtime's); slices_exact: run the request whatever the queues (A/B runs).  Both are
  // plumbing of this process and stay with their handle when its state is copied.
  int hw_queues = msckf::slices::HW_QUEUES_DEFAULT; bool slices_exact = false;
  int n_slices(bool streamed) const {
    return msckf::slices::effective_slices(settings.nstreams, B, msckf::slices::handle_queue_budget(hw_queues), streamed, slices_exact, prof);
  }
  int set_hw_queues(int n) {
    if (n < 1 || n > msckf::slices::HW_QUEUES_MAX) return fail(-EINVAL, "1 to 32 hardware queues");
    hw_queues = n;
    return 0;
  }
  // slice hh of nh on its enqueue thread: trajectories [b0, b0 + nb) on stream q.  A frame whose prune rides on the downdate
  // leaves the covariance in the other buffer (flipped: the slice's current one is the handle's spare) and the new window size
  // for the next k_propagate to commit (pending)
  struct Slice { int hh, b0, nb; hipStream_t q; bool flipped, pending; };
  Slice begin_slice(int hh, int nh) {
    (void)hipSetDevice(device);
    (void)hipGetLastError();
    const int b0 = (int)((long)B * hh / nh);
    return Slice{hh, b0, (int)((long)B * (hh + 1) / nh) - b0, stx[hh], false, false};
  }
  // fork: the slices' streams (and the copy stream of a streamed run) start after what is queued on st
  int fork_slices(int nh, hipStream_t extra = nullptr) {
    if (nh <= 1 && !extra) return 0;
    HIPCHK(hipEventRecord(ev_fork, st));
    for (int i = 1; i < nh; ++i) HIPCHK(hipStreamWaitEvent(stx[i], ev_fork, 0));
    if (extra) HIPCHK(hipStreamWaitEvent(extra, ev_fork, 0));
    return 0;
  }
  // the end of a call whose frames are enqueued: st waits for the slices (and the copy stream); a launch error of any slice
  // (slice_rc: hipGetLastError is per host thread, a failed launch must not vanish with its thread) makes the handle
  // unusable; otherwise the covariance buffer that is current now becomes the handle's
  int finish_slices(int nh, const int* slice_rc, int f0, int f1, hipStream_t extra = nullptr) {
    for (int i = 1; i < nh; ++i)
      if (hipEventRecord(ev_join[i], stx[i]) != hipSuccess || hipStreamWaitEvent(st, ev_join[i], 0) != hipSuccess) return poison(-EIO, "joining the slices' streams failed");
    if (extra && (hipEventRecord(ev_join[1], extra) != hipSuccess || hipStreamWaitEvent(st, ev_join[1], 0) != hipSuccess)) return poison(-EIO, "joining the copy stream failed");
    for (int i = 0; i < nh; ++i)
      if (slice_rc[i]) return poison(-EIO, std::string("kernel launch failed on slice ") + std::to_string(i) + ": " + hipGetErrorString((hipError_t)slice_rc[i]));
    commit_buffer_parity(f0, f1);
    advance_logs(f1 - f0);
    return 0;
  }
  // ---- the device logs of the frame loop: the frame log (dense: record = frame), the map log and the pruned-state log (cursor
  // logs).  Enabled with a capacity, or (0) switched off: either way a log that exists is freed and its records are dropped.
  template <class T> static void dfree(T*& p) { if (p) (void)hipFree(p); p = nullptr; }
  // what every *_log_enable does first; the handle's stream is idle when the old storage goes
  int log_enable_enter(int capacity) {
    if (int rc = guard()) return rc;
    if (capacity < 0) return fail(-EINVAL, "negative capacity");
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  // a log's storage of `bytes` and, for a cursor log, its B cursors at zero.  A step that fails gives back what the earlier
  // ones got: the log stays off and the handle as it was
  int log_alloc(const char* name, size_t bytes, void** buf, int** cursors) {
    void* q = nullptr; void* c = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess || (cursors && hipMalloc(&c, (size_t)B * sizeof(int)) != hipSuccess)) {
      (void)hipGetLastError();
      dfree(q);
      return fail(-ENOMEM, std::string("could not allocate the ") + name + " (it stays disabled; the handle is unaffected)");
    }
    if (cursors && (hipMemsetAsync(c, 0, (size_t)B * sizeof(int), st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
      dfree(q); dfree(c);
      return fail(-EIO, std::string("could not clear the ") + name + "'s cursors (it stays disabled)");
    }
    *buf = q;
    if (cursors) *cursors = static_cast<int*>(c);
    return 0;
  }
  // head of run_frames / run_frames_streamed / run_frames_replay (replay_loop), before anything of the call's frames is enqueued,
  // in the order frame, map, pruned, NEES: a log that refuses the call leaves the later ones untouched
  int reserve_logs(int f0, int f1, bool replay_loop = false) {
    if (int rc = frame_log_reserve(f0, f1)) return rc;
    if (int rc = cursor_log_reserve(map, f0, f1)) return rc;
    if (int rc = pruned_log_reserve(f0, f1)) return rc;
    return nees_log_reserve(f0, f1, replay_loop);
  }
  // finish_slices, when the call's frames have succeeded
  void advance_logs(int frames) {
    if (log_buf) log_n += frames;
    for (CursorLog* g : {&map, &prn}) if (g->buf) g->ord += frames;
    if (nees_buf) nees_n += frames;
  }
  void release_logs() {
    dfree(log_buf);
    for (CursorLog* g : {&map, &prn}) { dfree(g->buf); dfree(g->found); }
    dfree(nees_buf); dfree(tru); dfree(tru_row_of);
  }
  // ---- frame log
  int frame_log_enable(int capacity_frames) {
    if (int rc = log_enable_enter(capacity_frames)) return rc;
    dfree(log_buf); log_cap = 0; log_n = 0;
    if (!capacity_frames) return 0;
    if (int rc = log_alloc("frame log", (size_t)capacity_frames * B * LOG_STRIDE * esz, &log_buf, nullptr)) return rc;
    log_cap = capacity_frames;
    return 0;
  }
  int frame_log_reset() { log_n = 0; return 0; }
  int frame_log_count() const { return log_n; }
  // the call's records fit, and start at log_n
  int frame_log_reserve(int f0, int f1) {
    if (!log_buf) return 0;
    if ((long)log_n + (f1 - f0) > log_cap) return fail(-ENOSPC, "frame log full: the call's frames do not fit behind the records written (msckf_hip_frame_log_reset, or a larger msckf_hip_frame_log_enable); nothing was run");
    log_base = log_n;
    return 0;
  }
  // ---- cursor logs
  int cursor_log_enable(CursorLog& g, int capacity) {
    if (int rc = log_enable_enter(capacity)) return rc;
    dfree(g.buf); dfree(g.found); g.cap = 0; g.ord = 0;
    if (!capacity) return 0;
    if (int rc = log_alloc(g.name, (size_t)capacity * B * g.stride * esz, &g.buf, &g.found)) return rc;
    g.cap = capacity;
    return 0;
  }
  // cursors and frame ordinal <- 0 (the storage stays); ordered on st before the next call's frames
  int cursor_log_reset(CursorLog& g) {
    if (int rc = guard()) return rc;
    g.ord = 0;
    if (!g.buf) return 0;
    if (int rc = enter()) return rc;
    HIPCHK(hipMemsetAsync(g.found, 0, (size_t)B * sizeof(int), st));
    return 0;
  }
  // the call's ordinals start at ord and stay exact in a float record
  int cursor_log_reserve(CursorLog& g, int f0, int f1) {
    if (!g.buf) return 0;
    if ((long)g.ord + (f1 - f0) > (1L << 24)) return fail(-ENOSPC, std::string(g.name) + ": the call's frame ordinals would pass 2^24 (" + g.api + "_reset); nothing was run");
    g.base = g.ord;
    return 0;
  }
  int cursor_log_enabled(const CursorLog& g) const { return g.buf ? 0 : fail(-EINVAL, std::string(g.name) + " not enabled (" + g.api + "_enable)"); }
  // after the handle's stream: per trajectory of [b0, b0 + nb) the records found and how many of them are stored -- found
  // counts on beyond the capacity, stored does not
  int cursor_log_counts(CursorLog& g, int b0, int nb, int* stored, int* found) {
    if (int rc = guard()) return rc;
    if (int rc = cursor_log_enabled(g)) return rc;
    if (int rc = enter_range(b0, nb)) return rc;
    std::vector<int> tmp(std::max(nb, 1));
    if (nb) HIPCHK(hipMemcpyAsync(tmp.data(), g.found + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < nb; ++i) {
      if (found) found[i] = tmp[i];
      if (stored) stored[i] = std::min(tmp[i], g.cap);
    }
    return 0;
  }
  // what a read checks: the cursor first, then the range [r0, r0 + n) against trajectory b's stored records
  int cursor_log_check_range(CursorLog& g, int b, int r0, int n) {
    int stored = 0;
    if (int rc = cursor_log_counts(g, b, 1, &stored, nullptr)) return rc;
    if (r0 < 0 || n < 0 || (long)r0 + n > stored) return fail(-EINVAL, std::string("record range beyond the records stored (") + g.api + "_counts)");
    return 0;
  }
  // what a metrics call checks first: the log is on and [q0, q1) lies within the ordinals handed out
  int cursor_log_check_ordinals(const CursorLog& g, int q0, int q1) const {
    if (int rc = cursor_log_enabled(g)) return rc;
    if (q0 < 0 || q1 < q0 || q1 > g.ord) return fail(-EINVAL, std::string("frame ordinal range beyond the ordinals handed out (") + g.api + "_frames)");
    return 0;
  }
  // One metrics call: the block [ground truth | out | ints] goes to the device on st, launch(gt, out, ints) enqueues the
  // kernel there, out[no] comes back; the block is freed on every way out and the first error of the two (enqueueing,
  // waiting) is the one reported
  template <class Launch>
  int log_metrics_call(const char* what, const double* gt, size_t ng, const int* ints, size_t ni, double* out, size_t no, Launch launch) {
    double* dg = nullptr;
    if (hipMalloc((void**)&dg, (std::max<size_t>(ng, 1) + no) * sizeof(double) + std::max<size_t>(ni, 1) * sizeof(int)) != hipSuccess) { (void)hipGetLastError(); return fail(-ENOMEM, "could not allocate the ground truth on the device"); }
    double* dout = dg + std::max<size_t>(ng, 1);
    int* di = reinterpret_cast<int*>(dout + no);
    hipError_t e = ng ? hipMemcpyAsync(dg, gt, ng * sizeof(double), hipMemcpyHostToDevice, st) : hipSuccess;
    if (e == hipSuccess && ni) e = hipMemcpyAsync(di, ints, ni * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) { launch(dg, dout, di); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, no * sizeof(double), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(dg);
    if (e != hipSuccess || es != hipSuccess) return fail(-EIO, std::string(what) + ": " + hipGetErrorString(e != hipSuccess ? e : es));
    return 0;
  }
  // ---- map log
  int map_log_enable(int capacity) { return cursor_log_enable(map, capacity); }
  int map_log_reset() { return cursor_log_reset(map); }
  int map_log_frames() const { return map.ord; }
  int map_log_counts(int b0, int nb, int* stored, int* found) { return cursor_log_counts(map, b0, nb, stored, found); }
  // what map_log_metrics checks before anything reaches the device: the ordinal range, and off as CSR over its cells
  int map_log_check_gt(int q0, int q1, const double* gt_xyz, const int* gt_off) {
    if (int rc = cursor_log_check_ordinals(map, q0, q1)) return rc;
    if ((gt_xyz == nullptr) != (gt_off == nullptr)) return fail(-EINVAL, "gt_xyz and gt_off: both or neither");
    if (!gt_off) return 0;
    const size_t cells = (size_t)(q1 - q0) * B;
    if (gt_off[0] < 0) return fail(-EINVAL, "gt_off starts below 0");
    for (size_t c = 0; c < cells; ++c)
      if (gt_off[c + 1] < gt_off[c]) return fail(-EINVAL, "gt_off decreases at cell " + std::to_string(c) + " (CSR offsets over the cells (frame - q0) * B + b)");
    return 0;
  }
  // ---- pruned-state log: a cursor log, and the host mirror of which image's camera a record is
  // switching it off gives the fused prune back
  int pruned_log_enable(int capacity) {
    const int rc = cursor_log_enable(prn, capacity);
    if (!prn.buf) prn_list.clear();              // off, or the old log went and no new one came
    else if (!rc) prn_list.start(h_ncam);
    return rc;
  }
  int pruned_log_reset() {
    if (int rc = cursor_log_reset(prn)) return rc;
    if (prn.buf) prn_list.start(h_ncam);
    return 0;
  }
  int pruned_log_frames() const { return prn.ord; }
  int pruned_log_reserve(int f0, int f1) {
    if (int rc = cursor_log_reserve(prn, f0, f1)) return rc;
    prn_list.resync(h_ncam);
    return 0;
  }
  int pruned_log_counts(int b0, int nb, int* stored, int* found) { return cursor_log_counts(prn, b0, nb, stored, found); }
  // ---- NEES log and its truth table (nees_plan.h has every check)
  bool replay_model_q() const { return rp.assigned && rp.model == msckf_replay::MODEL_Q; }
  // truth16 [n_frames][n_rows][16] and row_of[B] to the device; n_frames == 0 frees the table.  A refused or failed call leaves
  // the table that was there
  int truth_set(int n_frames, int n_rows, const double* truth16, const int* row_of, int add_walk) {
    using namespace msckf_nees;
    if (int rc = guard()) return rc;
    if (int rc = refuse(truth_refusal(n_frames, n_rows, truth16, row_of, B, add_walk, replay_model_q()))) return rc;
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(st));                        // the last run's log launches have read the old table
    double* t = nullptr; int* r = nullptr;
    if (n_frames) {
      const size_t bytes = (size_t)n_frames * n_rows * TRUTH_ROW * sizeof(double);
      if (hipMalloc((void**)&t, bytes) != hipSuccess || hipMalloc((void**)&r, (size_t)B * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        dfree(t);
        return fail(-ENOMEM, "could not allocate the truth table (the one set before stays)");
      }
      if (hipMemcpy(t, truth16, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(r, row_of, (size_t)B * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        dfree(t); dfree(r);
        return fail(-EIO, "could not copy the truth table to the device (the one set before stays)");
      }
    }
    dfree(tru); dfree(tru_row_of);
    tru = t; tru_row_of = r; tru_frames = n_frames; tru_rows = n_frames ? n_rows : 0; tru_walk = n_frames && add_walk;
    return 0;
  }
  int nees_log_enable(int capacity_frames) {
    if (int rc = log_enable_enter(capacity_frames)) return rc;
    dfree(nees_buf); nees_cap = 0; nees_n = 0;
    if (!capacity_frames) return 0;
    void* q = nullptr;
    if (int rc = log_alloc("NEES log", (size_t)capacity_frames * B * msckf_nees::REC * sizeof(double), &q, nullptr)) return rc;
    nees_buf = static_cast<double*>(q); nees_cap = capacity_frames;
    return 0;
  }
  int nees_log_reset() { nees_n = 0; return 0; }
  int nees_log_count() const { return nees_n; }
  // the call's frames are covered by the truth table and their records fit, starting at nees_n
  int nees_log_reserve(int f0, int f1, bool replay_loop) {
    if (!nees_buf) return 0;
    if (int rc = refuse(msckf_nees::reserve_refusal(f0, f1, tru_frames, tru_walk ? 1 : 0, replay_loop, replay_model_q(), nees_n, nees_cap))) return rc;
    nees_base = nees_n; nees_replay = replay_loop;
    return 0;
  }
  // records [r0, r0 + n) of trajectories [b0, b0 + nb), out [n][nb][8]: one strided copy, one wait
  int nees_log_read(int r0, int n, int b0, int nb, double* out) {
    using namespace msckf_nees;
    if (int rc = guard()) return rc;
    if (int rc = refuse(read_refusal(r0, n, nees_n))) return rc;
    if (int rc = enter_range(b0, nb)) return rc;
    if (n && nb)
      HIPCHK(hipMemcpy2DAsync(out, (size_t)nb * REC * sizeof(double), nees_buf + record_at(r0, b0, B), (size_t)B * REC * sizeof(double),
                              (size_t)nb * REC * sizeof(double), (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  // the records [r0, r1) reduced over the groups of trajectories on the device (k_nees_ensemble): out [r1 - r0][n_groups][14]
  int nees_log_ensemble(int r0, int r1, const int* group_of, int n_groups, double* out) {
    using namespace msckf_nees;
    if (int rc = guard()) return rc;
    if (int rc = refuse(ensemble_refusal(r0, r1, nees_n, group_of, B, n_groups))) return rc;
    if (int rc = enter()) return rc;
    if (r1 == r0) return 0;
    return log_metrics_call("nees_log_ensemble", nullptr, 0, group_of, (size_t)B, out, (size_t)(r1 - r0) * n_groups * ENS, [&](const double*, double* dout, const int* dgroup) {
      launch_nees_ensemble(nees_buf, B, r0, r1, n_groups, dgroup, dout, st);
    });
  }
  // ---- aligned trajectory error (traj_plan.h has the modes, the rows and every check; kernels_traj.hip the kernels).  None of
  // the four calls touches filters, inputs or logs.
  // The ints of one call, [r0b | r1b | lags]: on the device r0b sits at 0, r1b at nt, the lags behind the ranges given
  static std::vector<int> traj_ints(const int* r0b, const int* r1b, int nt, const int* lags, int n_lags) {
    std::vector<int> v;
    if (r0b) { v.assign(r0b, r0b + nt); v.insert(v.end(), r1b, r1b + nt); }
    if (lags) v.insert(v.end(), lags, lags + n_lags);
    return v;
  }
  // the frame log's records [r0, r1) against gt_pose7 [r1 - r0][B][7]: lags null: the alignment `mode`, out [B][20]; else the
  // relative pose error, out [B][n_lags][4].  The record range is refused as frame_log_metrics refuses it
  int frame_log_traj(const char* what, int r0, int r1, const int* r0b, const int* r1b, const double* gt, int mode, const int* lags, int n_lags, double* out) {
    using namespace msckf_traj;
    if (int rc = guard()) return rc;
    if (r0 < 0 || r1 < r0 || r1 > log_n) return fail(-EINVAL, "record range beyond the records written (msckf_hip_frame_log_count)");
    if (int rc = refuse(lags ? rpe_refusal(r0, r1, r0b, r1b, B, gt, lags, n_lags) : align_refusal(r0, r1, r0b, r1b, B, gt, mode))) return rc;
    if (int rc = enter()) return rc;
    const std::vector<int> ints = traj_ints(r0b, r1b, B, lags, n_lags);
    const size_t no = lags ? (size_t)B * n_lags * RPE_ROW : (size_t)B * ALIGN_ROW;
    return log_metrics_call(what, gt, (size_t)(r1 - r0) * B * POSE, ints.data(), ints.size(), out, no, [&](const double* dg, double* dout, const int* di) {
      const int* d0 = r0b ? di : nullptr; const int* d1 = r0b ? di + B : nullptr; const int* dl = di + (r0b ? 2 * B : 0);
      if (esz == sizeof(float)) {
        if (lags) launch_traj_rpe_log<float>(static_cast<const float*>(log_buf), B, r0, r1, d0, d1, dg, dl, n_lags, dout, st);
        else launch_traj_align_log<float>(static_cast<const float*>(log_buf), B, r0, r1, d0, d1, dg, mode, dout, st);
      } else {
        if (lags) launch_traj_rpe_log<double>(static_cast<const double*>(log_buf), B, r0, r1, d0, d1, dg, dl, n_lags, dout, st);
        else launch_traj_align_log<double>(static_cast<const double*>(log_buf), B, r0, r1, d0, d1, dg, mode, dout, st);
      }
    });
  }
  // the same on poses the caller hands over, est and gt [n_rec][n_traj][7]; n_traj is free of the handle's B, which only supplies
  // the device and the stream.  The block on the device is [gt | est]
  int pose_traj(const char* what, int n_rec, int nt, const double* est, const double* gt, const int* r0b, const int* r1b, int mode, const int* lags, int n_lags, double* out) {
    using namespace msckf_traj;
    if (int rc = guard()) return rc;
    if (int rc = refuse(shape_refusal(n_rec, nt))) return rc;
    if (int rc = refuse(lags ? rpe_refusal(0, n_rec, r0b, r1b, nt, gt, lags, n_lags) : align_refusal(0, n_rec, r0b, r1b, nt, gt, mode))) return rc;
    if (int rc = enter()) return rc;
    const size_t np = (size_t)n_rec * nt * POSE;
    std::vector<double> both(gt, gt + np);
    both.insert(both.end(), est, est + np);
    const std::vector<int> ints = traj_ints(r0b, r1b, nt, lags, n_lags);
    const size_t no = lags ? (size_t)nt * n_lags * RPE_ROW : (size_t)nt * ALIGN_ROW;
    return log_metrics_call(what, both.data(), both.size(), ints.data(), ints.size(), out, no, [&](const double* dg, double* dout, const int* di) {
      const int* d0 = r0b ? di : nullptr; const int* d1 = r0b ? di + nt : nullptr; const int* dl = di + (r0b ? 2 * nt : 0);
      if (lags) launch_traj_rpe_pose(dg + np, nt, n_rec, d0, d1, dg, dl, n_lags, dout, st);
      else launch_traj_align_pose(dg + np, nt, n_rec, d0, d1, dg, mode, dout, st);
    });
  }
  int run_frames(int f0, int f1) {
    if (int rc = guard()) return rc;
    if (f0 < 0 || f1 > sc.frames || f0 > f1) return fail(-EINVAL, "frame range out of bounds");
    if (!committed) return fail(-EINVAL, "scenario not committed");
    if (int rc = reserve_logs(f0, f1)) return rc;
    if (int rc = enter()) return rc;
    const int nh = n_slices(false);
    const int rc = fork_slices(nh);
    if (rc) return rc;
    int slice_rc[MAXS] = {0};
    auto enqueue = [&](int hh) {
      Slice s = begin_slice(hh, nh);
      for (int f = f0; f < f1; ++f) enqueue_frame(s, f, f0, f1, -1);
      slice_rc[hh] = (int)hipGetLastError();
    };
    if (nh == 1) enqueue(0);
    else {
      workers.start(nh - 1, [&](int idx) { enqueue(idx + 1); });
      enqueue(0);
      workers.wait();
    }
    return finish_slices(nh, slice_rc, f0, f1);
  }
  // run_frames with the inputs handed over per frame, as the reference's callers do (asl_msckf.cpp:227-284: IMU samples and
  // the image's tracks arrive with the image): frame f's block -- IMU samples + compact work-list, what the frame really
  // holds, not a padded maximum -- goes from page-locked host memory into staging set f % ring on a copy stream, up to
  // ring - 1 frames ahead of the kernels that consume it.  Hand-over (up_mode 0): the uploading thread waits for its copy on
  // the HOST and publishes the frame number; a slice's enqueue thread launches frame f only after that, and the uploader
  // reuses a set only after every slice's "consumed" event of frame f - ring has completed -- no stream ever waits for
  // another stream's event on the device (those waits cost 0.15-0.25 ms per frame with two staging sets).  up_mode 1 keeps
  // the device-side hipStreamWaitEvent protocol, for comparison.
  int run_frames_streamed(int f0, int f1) {
    if (int rc = guard()) return rc;
    if (f0 < 0 || f1 > sc.frames || f0 > f1) return fail(-EINVAL, "frame range out of bounds");
    if (!committed) return fail(-EINVAL, "scenario not committed");
    if (int rc = reserve_logs(f0, f1)) return rc;
    if (int rc = enter()) return rc;
    {
      bool all = sg_blk[0] != nullptr;
      for (int f = f0; f < f1 && all; ++f) all = pinf[f].p != nullptr;
      if (!all) { int rc = scen_pin(f0, f1); if (rc) return rc; }
    }
    if (!stc) {
      HIPCHK(hipStreamCreateWithFlags(&stc, hipStreamNonBlocking));
      for (int k = 0; k < RING_MAX; ++k) {
        HIPCHK(hipEventCreateWithFlags(&ev_up[k], hipEventDisableTiming));
        for (int i = 0; i < MAXS; ++i) HIPCHK(hipEventCreateWithFlags(&ev_use[k][i], hipEventDisableTiming));
      }
    }
    const int nh = n_slices(true);
    const int R = settings.ring, mode = settings.up_mode;
    const int rc = fork_slices(nh, stc);
    if (rc) return rc;
    // up_rdy = frames whose block may be read (mode 0: the copy has completed; mode 1: copy + event record are enqueued --
    // an event must be recorded before a wait on it is enqueued); use_enq[s] = frames whose "consumed" record is enqueued.
    std::atomic<int> up_rdy{f0};
    std::atomic<int> use_enq[MAXS];
    for (int i = 0; i < MAXS; ++i) use_enq[i].store(f0);
    std::atomic<int> failed{0};
    int slice_rc[MAXS] = {0};
    auto slice = [&](int hh) {
      Slice s = begin_slice(hh, nh);
      for (int f = f0; f < f1; ++f) {
        while (up_rdy.load(std::memory_order_acquire) <= f && !failed.load()) std::this_thread::yield();
        if (failed.load()) break;
        const int k = (f - f0) % R;
        if (mode == 1) (void)hipStreamWaitEvent(s.q, ev_up[k], 0);
        enqueue_frame(s, f, f0, f1, k);
        (void)hipEventRecord(ev_use[k][hh], s.q);
        use_enq[hh].store(f + 1, std::memory_order_release);
      }
      slice_rc[hh] = (int)hipGetLastError();
    };
    // the uploading (calling) thread on its own core for the duration of the call, when a list of cores was given
    cpu_set_t old_mask; bool repin = false;
    if (!workers.cpus.empty() && workers.cpus[0] >= 0 && pthread_getaffinity_np(pthread_self(), sizeof(old_mask), &old_mask) == 0) {
      cpu_set_t one; CPU_ZERO(&one); CPU_SET(workers.cpus[0], &one);
      (void)pthread_setaffinity_np(pthread_self(), sizeof(one), &one); repin = true;
    }
    workers.start(nh, slice);
    int rc_up = 0;
    for (int f = f0; f < f1 && !rc_up; ++f) {
      const int k = (f - f0) % R;
      if (f - f0 >= R)
        for (int i = 0; i < nh && !rc_up; ++i) {   // the set is free again once every slice has consumed frame f - R
          while (use_enq[i].load(std::memory_order_acquire) <= f - R) std::this_thread::yield();
          const hipError_t e = mode == 0 ? hipEventSynchronize(ev_use[k][i]) : hipStreamWaitEvent(stc, ev_use[k][i], 0);
          if (e != hipSuccess) rc_up = -EIO;
        }
      if (!rc_up && (f == settings.test_fail_upload || hipMemcpyAsync(sg_blk[k], pinf[f].p, pinf[f].bytes, hipMemcpyHostToDevice, stc) != hipSuccess)) rc_up = -EIO;
      if (!rc_up && (mode == 0 ? hipStreamSynchronize(stc) : hipEventRecord(ev_up[k], stc)) != hipSuccess) rc_up = -EIO;
      if (rc_up) failed.store(1);
      up_rdy.store(f + 1, std::memory_order_release);
    }
    workers.wait();
    if (repin) (void)pthread_setaffinity_np(pthread_self(), sizeof(old_mask), &old_mask);
    if (rc_up) return poison(rc_up, "input upload failed");
    return finish_slices(nh, slice_rc, f0, f1, stc);
  }
  // ---- Monte-Carlo replay (replay_plan.h): shared sequences, expanded per frame on the device (k_replay_expand)
  int refuse(const inputs::Refusal& r) const { return r.code ? fail(r.code, r.why) : 0; }
  void free_replay_device() {
    for (auto& p : rp_dev) dfree(p);
    dfree(rp_seq_of); dfree(rp_seed); dfree(rp_sigma); dfree(rp_base); rp_base_count = 0;
    dfree(rp_L); dfree(rp_scale); dfree(rp_wstart); rp_wstart_count = 0;
    for (auto& p : rp_blk) dfree(p);
    rp_blk_bytes = 0;
    dfree(rp_scratch); rp_scratch_bytes = 0;
    dfree(rp_fault); dfree(rp_code); rp_code_count = 0;
    dfree(rp_timing); dfree(rp_img_time); dfree(rp_img_frame); dfree(rp_img_base); dfree(rp_delta); rp_delta_count = 0;
    dfree(rp_imucal); dfree(rp_camcal); dfree(rp_rdcal); dfree(rp_clip); rp_rdcal_count = 0; dfree(rp_obscal); rp_obscal_count = 0;
    rp_uploaded = false;
  }
  int replay_alloc(int n_seq, int n_frames, int K) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(msckf_replay::Plan::alloc_refusal(n_seq, n_frames, K))) return rc;
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(st));
    free_replay_device();
    rp.alloc(n_seq, n_frames, K, B, f_cap);
    return 0;
  }
  int replay_set_cell(int f, int s, const double* rd, int k, int F, const int* M, const int* slots, const double* obs, int n_drop, int flags) {
    if (int rc = refuse(rp.cell_refusal(f, s, rd, k, F, M, slots, n_drop, flags, m_cap, n_cap))) return rc;
    rp.set_cell(f, s, rd, k, F, M, slots, obs, n_drop, flags);
    return 0;
  }
  // H2D of the sequences as they stand (the host copy is kept: cells may be patched and committed again)
  int replay_commit() {
    using namespace inputs;
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.commit_refusal())) return rc;
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = refuse(rp.commit())) return rc;
    rp.committed = false;                                    // until the device holds them
    const ScenarioStore& q = rp.seq;
    for (auto& p : rp_dev) dfree(p);
    for (int s = 0; s < N_SECTIONS; ++s)
      HIPCHK(hipMalloc((void**)&rp_dev[s], std::max<size_t>(s < N_FIXED ? q.fixed[s].size() : q.total() * q.lay.entry_bytes(s), 16)));
    if (int rc = upload_store(q, rp_dev)) return rc;
    // the image tables of the timed expansion (replay_plan.h, TIMING)
    dfree(rp_img_time); dfree(rp_img_frame); dfree(rp_img_base);
    HIPCHK(hipMalloc((void**)&rp_img_time, rp.img_time.size() * sizeof(double))); HIPCHK(hipMalloc((void**)&rp_img_frame, rp.img_frame.size() * sizeof(int))); HIPCHK(hipMalloc((void**)&rp_img_base, rp.img_base.size() * sizeof(int)));
    HIPCHK(hipMemcpy(rp_img_time, rp.img_time.data(), rp.img_time.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(rp_img_frame, rp.img_frame.data(), rp.img_frame.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(rp_img_base, rp.img_base.data(), rp.img_base.size() * sizeof(int), hipMemcpyHostToDevice));
    rp_maxcell.assign(q.frames, 0);
    for (int f = 0; f < q.frames; ++f) for (int s = 0; s < rp.S; ++s) rp_maxcell[f] = std::max(rp_maxcell[f], (int)rp.entries(s, f));
    rp.committed = true;
    rp_uploaded = false;
    return 0;
  }
  // may be called again between runs
  int replay_assign(const int* seq_of, const uint64_t* seed, const double* sigma4) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.assign_refusal(seq_of, sigma4))) return rc;
    rp.assign(seq_of, seed, sigma4);
    rp_uploaded = false;
    return 0;
  }
  // the Q_imu model's assignment (replay_plan.h, MODEL); a later replay_assign returns to the sigma4 model
  int replay_assign_q(const int* seq_of, const uint64_t* seed, const double* Q144, const double* scale, const double* sigma_uv) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.assign_q_refusal(seq_of, Q144, scale, sigma_uv))) return rc;
    rp.assign_q(seq_of, seed, Q144, scale, sigma_uv);
    rp_uploaded = false;
    return 0;
  }
  // the fault record (replay_plan.h, FAULTS), or null for none; may be called between runs, stays through assign, assign_q and
  // commit, and replay_alloc clears it.  A refused call leaves the previous record in force.
  int replay_set_faults(const double* fault4) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.faults_refusal(fault4))) return rc;
    rp.set_faults(fault4);
    return 0;
  }
  // the timing record (replay_plan.h, TIMING), or null for none; may be called between runs, stays through assign, assign_q,
  // set_faults and commit, and replay_alloc clears it.  A refused call leaves the previous record in force.
  int replay_set_timing(const double* timing4) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.timing_refusal(timing4))) return rc;
    rp.set_timing(timing4);
    return 0;
  }
  // the calibration records (replay_plan.h, CALIB), or null for none; may be called between runs, stay through assign, assign_q,
  // set_faults, set_timing and commit, and replay_alloc clears them.  A refused call leaves the previous record in force.
  int replay_set_imu_calib(const double* imucal) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.imu_calib_refusal(imucal))) return rc;
    rp.set_imu_calib(imucal);
    return 0;
  }
  int replay_set_cam_calib(const double* camcal) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.cam_calib_refusal(camcal))) return rc;
    rp.set_cam_calib(camcal);
    return 0;
  }
  // msckf_hip_replay_image_table: sequence seq's image table as commit built it -- time / frame_of [images], base [frames], each
  // or null -- and the image count
  int replay_image_table(int seq, double* time, int* frame_of, int* base) {
    if (int rc = guard()) return rc;
    if (rp.frames() <= 0) return fail(-EINVAL, "no replay allocated");
    if (!rp.committed) return fail(-EINVAL, "replay not committed");
    if (seq < 0 || seq >= rp.S) return fail(-EINVAL, "replay cell out of range");
    const int F = rp.frames(), n = rp.img_n[seq];
    if (time) std::copy(rp.img_time.begin() + (size_t)seq * F, rp.img_time.begin() + (size_t)seq * F + n, time);
    if (frame_of) std::copy(rp.img_frame.begin() + (size_t)seq * F, rp.img_frame.begin() + (size_t)seq * F + n, frame_of);
    if (base) for (int f = 0; f < F; ++f) base[f] = rp.img_base[rp.cell(f, seq)];
    return n;
  }
  // the timing part of the timed expansion's arguments on frame f
  ReplayTimingIn replay_timing(int f) const { return ReplayTimingIn{rp_timing, rp_img_time, rp_img_frame, rp_img_base + (size_t)f * rp.S, rp.frames()}; }
  // before a run or an expansion (after enter()): the bases of every frame, and with the assignment and the fault record on the device
  int replay_upload_plan() {
    if (rp.planned && rp_uploaded && rp.faults_uploaded && rp.timing_uploaded && rp.calib_uploaded) return 0;
    if (int rc = refuse(rp.index_trajectories())) return rc;
    HIPCHK(hipStreamSynchronize(st));                        // the last run's kernels have read the old ones
    if (!rp_seq_of) {
      HIPCHK(hipMalloc((void**)&rp_seq_of, (size_t)B * sizeof(int))); HIPCHK(hipMalloc((void**)&rp_seed, (size_t)B * sizeof(uint64_t)));
      HIPCHK(hipMalloc((void**)&rp_sigma, (size_t)B * msckf_replay::N_SIGMA * sizeof(double)));
      HIPCHK(hipMalloc((void**)&rp_fault, (size_t)B * msckf_replay::N_FAULT * sizeof(double)));
      HIPCHK(hipMalloc((void**)&rp_timing, (size_t)B * msckf_replay::N_TIMING * sizeof(double)));
      HIPCHK(hipMalloc((void**)&rp_imucal, (size_t)B * msckf_replay::IMU_CAL * sizeof(double)));
      HIPCHK(hipMalloc((void**)&rp_camcal, (size_t)B * msckf_replay::CAM_CAL * sizeof(double)));
    }
    if (rp.base.size() != rp_base_count) { dfree(rp_base); rp_base_count = 0; HIPCHK(hipMalloc((void**)&rp_base, rp.base.size() * sizeof(int))); rp_base_count = rp.base.size(); }
    HIPCHK(hipMemcpy(rp_seq_of, rp.seq_of.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(rp_seed, rp.seed.data(), (size_t)B * sizeof(uint64_t), hipMemcpyHostToDevice));
    const bool model = rp.model == msckf_replay::MODEL_Q;
    const std::vector<double>& sg = model ? rp.sigma_uv : rp.sigma;   // (rp_sigma has room for the larger of the two)
    HIPCHK(hipMemcpy(rp_sigma, sg.data(), sg.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(rp_base, rp.base.data(), rp.base.size() * sizeof(int), hipMemcpyHostToDevice));
    if (model) {
      if (!rp_L) { HIPCHK(hipMalloc((void**)&rp_L, (size_t)B * msckf_replay::L_SIZE * sizeof(double))); HIPCHK(hipMalloc((void**)&rp_scale, (size_t)B * sizeof(double))); }
      HIPCHK(hipMemcpy(rp_L, rp.L.data(), rp.L.size() * sizeof(double), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(rp_scale, rp.scale.data(), rp.scale.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (rp.fault.empty()) HIPCHK(hipMemset(rp_fault, 0, (size_t)B * msckf_replay::N_FAULT * sizeof(double)));
    else HIPCHK(hipMemcpy(rp_fault, rp.fault.data(), rp.fault.size() * sizeof(double), hipMemcpyHostToDevice));
    if (rp.timing.empty()) HIPCHK(hipMemset(rp_timing, 0, (size_t)B * msckf_replay::N_TIMING * sizeof(double)));
    else HIPCHK(hipMemcpy(rp_timing, rp.timing.data(), rp.timing.size() * sizeof(double), hipMemcpyHostToDevice));
    {
      std::vector<double> ic = rp.imucal;                    // (no record: the identity)
      if (ic.empty()) { ic.resize((size_t)B * msckf_replay::IMU_CAL); for (int b = 0; b < B; ++b) msckf_replay::imu_calib_identity(ic.data() + (size_t)b * msckf_replay::IMU_CAL); }
      HIPCHK(hipMemcpy(rp_imucal, ic.data(), ic.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (rp.camcal.empty()) HIPCHK(hipMemset(rp_camcal, 0, (size_t)B * msckf_replay::CAM_CAL * sizeof(double)));
    else HIPCHK(hipMemcpy(rp_camcal, rp.camcal.data(), rp.camcal.size() * sizeof(double), hipMemcpyHostToDevice));
    rp_uploaded = rp.faults_uploaded = rp.timing_uploaded = rp.calib_uploaded = true;
    return 0;
  }
  // msckf_hip_replay_fault_counts: the faults of the frames [f0, f1) per trajectory, out [B][6], counted on the device from the
  // sequences, the seeds and the fault record alone (k_replay_fault_counts): no run, no log
  int replay_fault_counts(int f0, int f1, long long* out) {
    using namespace inputs;
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.run_refusal(f0, f1))) return rc;
    if (int rc = enter()) return rc;
    if (int rc = replay_upload_plan()) return rc;
    constexpr size_t W = msckf_replay::N_FAULT_COUNT;
    long long* dout = nullptr;
    HIPCHK(hipMalloc((void**)&dout, (size_t)B * W * sizeof(long long)));
    auto i = [&](int s) { return reinterpret_cast<const int*>(rp_dev[s]); };
    launch_replay_fault_counts(i(SEC_N), i(SEC_M), i(SEC_OFF), ReplayTrajIn{rp_seq_of, rp_seed, rp_sigma, rp_base, rp_fault}, f0, f1, rp.S, f_cap, B, dout, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)B * W * sizeof(long long), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(dout);
    if (e != hipSuccess || es != hipSuccess) return fail(-EIO, std::string("replay_fault_counts: ") + hipGetErrorString(e != hipSuccess ? e : es));
    return 0;
  }
  // msckf_hip_replay_imu_sums: per trajectory the count, the summed omega, a and dT of the IMU samples a run over [f0, f1) would
  // hand its propagate, out [B][8] (replay_plan.h, ImuSum), summed on the device from the sequences and the assignment alone
  // (k_replay_imu_sums): no run, no log, nothing of the filters changes
  int replay_imu_sums(int f0, int f1, double* out) {
    using namespace inputs;
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.sums_refusal(f0, f1))) return rc;
    if (int rc = enter()) return rc;
    if (int rc = replay_upload_plan()) return rc;
    if (int rc = replay_walk_table()) return rc;
    constexpr size_t W = msckf_replay::IMU_SUM_ROW;
    double* dout = nullptr;
    HIPCHK(hipMalloc((void**)&dout, (size_t)B * W * sizeof(double)));
    launch_replay_imu_sums(reinterpret_cast<const double*>(rp_dev[SEC_RD]), reinterpret_cast<const int*>(rp_dev[SEC_K]), ReplayTrajIn{rp_seq_of, rp_seed, rp_sigma, rp_base},
                           replay_model(0), f0, f1, rp.S, rp.K(), B, esz == sizeof(float), dout, st, rp.imu_calibrated ? rp_imucal : nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)B * W * sizeof(double), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(dout);
    if (e != hipSuccess || es != hipSuccess) return fail(-EIO, std::string("replay_imu_sums: ") + hipGetErrorString(e != hipSuccess ? e : es));
    return 0;
  }
  // msckf_hip_replay_calib_counts: per trajectory the samples of the frames [f0, f1) and the components the saturation clips,
  // out [B][8] (replay_plan.h, CalibCount), counted on the device from the sequences, the assignment and the IMU record alone
  // (k_replay_calib_counts): no run, no log, nothing of the filters changes
  int replay_calib_counts(int f0, int f1, long long* out) {
    using namespace inputs;
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.run_refusal(f0, f1))) return rc;
    if (int rc = enter()) return rc;
    if (int rc = replay_upload_plan()) return rc;
    if (int rc = replay_walk_table()) return rc;
    constexpr size_t W = msckf_replay::N_CALIB_COUNT;
    long long* dout = nullptr;
    HIPCHK(hipMalloc((void**)&dout, (size_t)B * W * sizeof(long long)));
    launch_replay_calib_counts(reinterpret_cast<const double*>(rp_dev[SEC_RD]), reinterpret_cast<const int*>(rp_dev[SEC_K]), ReplayTrajIn{rp_seq_of, rp_seed, rp_sigma, rp_base},
                               replay_model(0), rp_imucal, f0, f1, rp.S, rp.K(), B, dout, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)B * W * sizeof(long long), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(dout);
    if (e != hipSuccess || es != hipSuccess) return fail(-EIO, std::string("replay_calib_counts: ") + hipGetErrorString(e != hipSuccess ? e : es));
    return 0;
  }
  // what map_log_fault_metrics checks before anything reaches the device: the log and its ordinals, then the replay frames
  // [f0, f0 + (q1 - q0)) as a run would check them
  int map_log_check_faults(int q0, int q1, int f0) {
    if (int rc = cursor_log_check_ordinals(map, q0, q1)) return rc;
    return refuse(rp.run_refusal(f0, f0 + (q1 - q0)));
  }
  // under the Q_imu model, after replay_upload_plan(): the walk table of the cells and the assignment as they stand, tabulated on
  // the handle's stream (stage 12; the slices' streams fork from it) if it is not already
  int replay_walk_table() {
    using namespace inputs;
    if (rp.model != msckf_replay::MODEL_Q || rp.walk_planned) return 0;
    const size_t need = (size_t)(rp.frames() + 1) * B * msckf_replay::WALK_ROW;
    if (need != rp_wstart_count) {
      HIPCHK(hipStreamSynchronize(st));
      dfree(rp_wstart); rp_wstart_count = 0;
      HIPCHK(hipMalloc((void**)&rp_wstart, need * sizeof(double)));
      rp_wstart_count = need;
    }
    stage_begin(12, st);
    launch_replay_walk_scan(reinterpret_cast<const double*>(rp_dev[SEC_RD]), reinterpret_cast<const int*>(rp_dev[SEC_K]), ReplayTrajIn{rp_seq_of, rp_seed, rp_sigma, rp_base},
                            replay_model(0), rp_wstart, rp.frames(), rp.S, rp.K(), B, st);
    stage_end(12, st);
    HIPCHK(hipGetLastError());
    rp.walk_planned = true;
    return 0;
  }
  // the model's part of the expansion's arguments on frame f (all null under the sigma4 model)
  ReplayModelIn replay_model(int f) const {
    if (rp.model != msckf_replay::MODEL_Q) return ReplayModelIn{nullptr, nullptr, nullptr};
    return ReplayModelIn{rp_L, rp_scale, rp_wstart + (size_t)f * B * msckf_replay::WALK_ROW};
  }
  // msckf_hip_replay_walk: rows [f0, f1) of the walk table for the trajectories [b0, b0 + nb), out [f1 - f0][nb][6]
  int replay_walk(int f0, int f1, int b0, int nb, double* out) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.walk_refusal(f0, f1, b0, nb))) return rc;
    if (int rc = enter()) return rc;
    if (int rc = replay_upload_plan()) return rc;
    if (int rc = replay_walk_table()) return rc;
    constexpr int W = msckf_replay::WALK_ROW;
    std::vector<double> rows((size_t)(f1 - f0) * B * W);
    if (!rows.empty()) HIPCHK(hipMemcpyAsync(rows.data(), rp_wstart + (size_t)f0 * B * W, rows.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int f = 0; f < f1 - f0; ++f) std::copy(rows.begin() + ((size_t)f * B + b0) * W, rows.begin() + ((size_t)f * B + b0 + nb) * W, out + (size_t)f * nb * W);
    return 0;
  }
  // one expanded block per slice, each large enough for the largest expanded frame
  int replay_blocks(int nh) {
    const size_t need = rp.block_bytes(esz);
    if (need > rp_blk_bytes) {
      HIPCHK(hipStreamSynchronize(st));
      for (auto& p : rp_blk) dfree(p);
      rp_blk_bytes = need;
    }
    for (int i = 0; i < nh; ++i) if (!rp_blk[i]) HIPCHK(hipMalloc((void**)&rp_blk[i], rp_blk_bytes));
    return 0;
  }
  // run_frames with each frame's block expanded on the device from the sequences, on the slice's own stream ahead of the frame's
  // propagate; everything else is run_frames'
  int run_frames_replay(int f0, int f1) {
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.run_refusal(f0, f1))) return rc;
    if (int rc = enter()) return rc;
    if (int rc = replay_upload_plan()) return rc;
    if (int rc = replay_walk_table()) return rc;
    const int nh = n_slices(false);
    if (int rc = replay_blocks(nh)) return rc;
    if (int rc = reserve_logs(f0, f1, true)) return rc;
    for (int i = 0; i < nh; ++i) rp_cells[i].assign((size_t)3 * B, 0);
    const int rc = fork_slices(nh);
    if (rc) return rc;
    int slice_rc[MAXS] = {0};
    auto enqueue = [&](int hh) {
      Slice s = begin_slice(hh, nh);
      for (int f = f0; f < f1; ++f) enqueue_frame(s, f, f0, f1, IN_REPLAY);
      slice_rc[hh] = (int)hipGetLastError();
    };
    if (nh == 1) enqueue(0);
    else {
      workers.start(nh - 1, [&](int idx) { enqueue(idx + 1); });
      enqueue(0);
      workers.wait();
    }
    return finish_slices(nh, slice_rc, f0, f1);
  }
  // where a frame's inputs are, as enqueue_frame's `staged` says: resident, expanded by the replay, or (>= 0) in that staging set
  static constexpr int IN_RESIDENT = -1, IN_REPLAY = -2;
  // The host's copy of the frame's cells, indexed by trajectory: the sample count k (or IMU_SKIP), the drop, the largest camera
  // slot of the work-list.  A scenario's own cells, or for a replay those of each trajectory's sequence (slice hh's [b0, b0 + nb)).
  struct FrameCells { const int* k; const int* drop; const int* maxslot; };
  FrameCells frame_cells(int f, int staged, int hh, int b0, int nb) {
    using namespace inputs;
    if (staged != IN_REPLAY) {
      const size_t cell0 = (size_t)f * B;
      return FrameCells{sc.ints(SEC_K) + cell0, sc.ints(SEC_DROP) + cell0, sc.maxslot.data() + cell0};
    }
    int* c = rp_cells[hh].data();
    for (int b = b0; b < b0 + nb; ++b) {
      const size_t cell = rp.cell_of(f, b);
      c[b] = rp.seq.ints(SEC_K)[cell]; c[B + b] = rp.seq.ints(SEC_DROP)[cell]; c[2 * B + b] = rp.seq.maxslot[cell];
    }
    return FrameCells{c, c + B, c + 2 * B};
  }
  int sync() {
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  // the setters of the C interface: validate, store, apply
  int store(int Settings::* field, int v) { settings.*field = v; apply_settings(); return 0; }
  int set_feature_overlap(int on) { return store(&Settings::overlap_feature, on ? 1 : 0); }
  int set_frame_order(int order) {
    if (order != 0 && order != 1) return fail(-EINVAL, "order: 0 propagate first on every frame, 1 feature first where the frame allows it");
    frame_settings.order = order;
    return 0;
  }
  int set_frame_order_chol(int on) { frame_settings.in_cholesky = on ? 1 : 0; return 0; }
  int set_compression(int route) {
    if (route < -1 || route > 3) return fail(-EINVAL, "route: -1 default, 0 Householder TSQR, 1..3 information form (blocked matrix-core Cholesky; 1 and 2 named retired factorizations)");
    if (route >= 1 && !info_form) return fail(-ENOTSUP, "information form not available for this window size (6 n_cap + 1 > 384 or f_cap > 1024)");
    return store(&Settings::compress_route, route);
  }
  int set_gate_early(int on) { return store(&Settings::gate_early, on ? 1 : 0); }
  int set_cov_update(int form) {
    if (form < 0 || form > 2) return fail(-EINVAL, "form: 0 square-root gain (P - W W^T), 1 Joseph, 2 square-root gain with the register-resident solve");
    return store(&Settings::cov_update, form);
  }
  int set_host_affinity(const int* cpus, int n) {
    std::lock_guard<std::mutex> lk(workers.m);
    workers.cpus.assign(cpus, cpus + std::max(n, 0));
    return 0;
  }
  int set_streams(int n) {
    if (n < 1 || n > MAXS) return fail(-EINVAL, "1 to 8 streams");
    return store(&Settings::nstreams, n);
  }
  int prof_enable(int on) {
    prof = on != 0;
    for (int s = 0; s < NSTAGE; ++s) { ev_used[s] = 0; prof_ms[s] = 0; prof_cnt[s] = 0; }
    return 0;
  }
  // what an event pair with NOTHING between its records measures on this stream (the marker packets themselves): the stage
  // timers of prof_read hold one such pair per launch, so a single-kernel stage reads kernel time + this
  int prof_event_overhead(double* ms) {
    if (int rc = enter()) return rc;
    hipEvent_t a, b2;
    HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b2));
    HIPCHK(hipStreamSynchronize(st));
    double tot = 0; const int reps = 64;
    for (int i = 0; i < reps; ++i) {
      HIPCHK(hipEventRecord(a, st)); HIPCHK(hipEventRecord(b2, st));
      HIPCHK(hipEventSynchronize(b2));
      float t = 0; HIPCHK(hipEventElapsedTime(&t, a, b2));
      tot += t;
    }
    hipEventDestroy(a); hipEventDestroy(b2);
    *ms = tot / reps;
    return 0;
  }
  int prof_read(double* ms, int* cnt, int cap) {
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(st));
    for (int s = 0; s < NSTAGE; ++s) {
      for (size_t i = 0; i < ev_used[s]; ++i) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, ev_pool[s][i].first, ev_pool[s][i].second));
        prof_ms[s] += t; prof_cnt[s]++;
      }
      ev_used[s] = 0;
      if (s < cap) { ms[s] = prof_ms[s]; cnt[s] = prof_cnt[s]; }
    }
    return 0;
  }

  // ---- the typed steps (Batch<S>, msckf_hip.hip): everything that launches a kernel or converts between S and double
  virtual int alloc() = 0;   // create()'s typed part: Dev<S> and every device buffer
  virtual int init_core(int b, const double* cam, const double* noise, const double* q78, const double* P0, const double* params, const double* imu) = 0;
  virtual int init_full(int b, const double* cam, const double* uv2, const double* Q144, const double* P0_225, const double* params, const double* imu) = 0;
  virtual void mirror_advance(int b, const double* rd, int K) = 0;   // propagate()'s K samples on the host copy of the IMU state
  virtual int propagate_device(const inputs::Readings& in, int b0, bool then_augment = false) = 0;   // in.nb trajectories from b0 on
  virtual int augment(int b0, int nb) = 0;
  virtual int set_tracks(int b, int F, const int* M, const int* slots, const double* obs) = 0;
  virtual int marginalize(int b0, int nb, int mode = 0) = 0;   // mode 1: the second update of pruneRedundantStates (stored p_f_G per track, set_given_range)
  // range forms (one copy / one launch for trajectories b0 .. b0 + nb - 1): the batched image cycle (host_image_cycle), and
  // the per-filter entries with nb = 1
  virtual int set_tracks_range(int b0, int nb, const std::vector<WorkList>& wl) = 0;           // every trajectory's list in one pinned block, two copies
  virtual int cams_range(int b0, int nb, double* poses7) = 0;                                  // [nb][n_cap][7], one read + one wait
  virtual int feature_only_range(int b0, int nb, int* status, double* pf3, bool launch) = 0;   // checkMotion + triangulation of the work-lists: [nb][f_cap], [nb][f_cap][3]; launch = false: only read what the last launch left
  virtual int set_given_range(int b0, int nb, const double* pf3) = 0;                          // [nb][f_cap][3]
  virtual int prune_keep_range(int b0, int nb, const std::vector<std::vector<int>>& keep) = 0; // keep[i]: ascending slots of trajectory b0 + i
  virtual int drop_oldest(int b0, int nb, int n) = 0;
  virtual int get_imu(int b, double* o) = 0;
  virtual int set_imu(int b, const double* in) = 0;
  virtual int get_cams(int b, double* o, int cap, int* n) = 0;
  virtual int get_cams_known(int b, double* o, int n) = 0;   // n known to the caller: cameras + (into the host copy) the IMU state, one wait
  virtual int set_cam(int b, int slot, const double* in) = 0;
  virtual int get_cov(int b, double* P, int ldo) = 0;
  virtual int set_cov(int b, const double* P, int D) = 0;
  virtual int track_info(int b, double* out, int cap) = 0;
  virtual int track_blocks(int b, int* first, double* Hx, double* rw, double* Bh, int cap) = 0;
  virtual int deltax(int b, double* out, int cap) = 0;
  virtual int scen_set(int f, int b, const double* rd, int k, int F, const int* M, const int* slots, const double* obs, int n_drop, int flags) = 0;
  // THE frame step of run_frames / run_frames_streamed / run_frames_replay: frame f of a call over [f0, f1) for slice s, inputs
  // in staging set `staged` of the upload ring, or resident (IN_RESIDENT), or expanded by the replay (IN_REPLAY)
  virtual void enqueue_frame(Slice& s, int f, int f0, int f1, int staged) = 0;
  // the read-back of the calibrated expansion (msckf_hip_replay_expand_calib): each pointer or null
  struct CalibOut { double* rd_cal; int* clip; double* obs_cal; };
  virtual int replay_expand(int f, int b, double* rd, double* obs, int* ints, int* slots, int cap_entries, int* code = nullptr, double* delta = nullptr, const CalibOut* co = nullptr) = 0;
  virtual int map_log_fault_metrics(int q0, int q1, int f0, double* out) = 0;                  // out [B][8]
  virtual void commit_buffer_parity(int f0, int f1) = 0;   // after the frames [f0, f1): the covariance buffer that is current becomes the handle's
  virtual void apply_settings() = 0;   // the one place where `settings` reaches the kernel argument
  virtual int set_aniso(int mode, double tol) = 0;
  virtual int copy_from(BatchCore* src) = 0;
  virtual int lit_info(int b, int* out8) = 0;
  virtual int frame_log_read(int r0, int n, int b0, int nb, double* out) = 0;                  // [n][nb][LOG_STRIDE]
  // gt_p [r1 - r0][B][3], out [B][6]; r0b / r1b (both or neither): a record range per trajectory inside [r0, r1)
  virtual int frame_log_metrics(int r0, int r1, const double* gt_p, double* out, const int* r0b = nullptr, const int* r1b = nullptr) = 0;
  int frame_log_metrics_ranges(const int* r0b, const int* r1b, const double* gt_p, double* out) {
    int lo = INT32_MAX, hi = 0;
    for (int b = 0; b < B; ++b) {
      if (r0b[b] < 0 || r1b[b] < r0b[b] || r1b[b] > log_n)
        return fail(-EINVAL, "record range of trajectory " + std::to_string(b) + " beyond the records written (msckf_hip_frame_log_count)");
      lo = std::min(lo, r0b[b]); hi = std::max(hi, r1b[b]);
    }
    return frame_log_metrics(lo, hi, gt_p, out, r0b, r1b);
  }
  virtual int map_log_read(int b, int r0, int n, double* out) = 0;                              // [n][MAP_STRIDE]
  virtual int map_log_metrics(int q0, int q1, const double* gt_xyz, const int* gt_off, double* out) = 0;   // out [B][8]
  virtual int pruned_log_read(int b, int r0, int n, double* out, int* aug_ord) = 0;             // [n][PRN_STRIDE], [n]
  virtual int pruned_log_metrics(int q0, int q1, const double* gt_pose, int n_ord, double* out) = 0;       // gt_pose [n_ord][B][7], out [B][10]
};

int resolve_map(BatchCore* B, int b);   // (defined with the host-side bookkeeping below)

template <class S>
struct Batch : BatchCore {
  Dev<S> d{};
  S* P_spare = nullptr;   // second covariance buffer: target of a downdate that carries the frame's prune (Dev::Pout)
  // Host mirror of the IMU state for the single-filter API: getImuState() is called once per IMU sample by the reference's
  // runner (asl_msckf.cpp:231) and must be synchronously available on the host; between two images only
  // propagate() changes it, and propogateImuStateRK (msckf.h:1425-1467) is a few hundred FLOP -- so msckf_hip_propagate
  // advances this copy with the reference's own RK sequence while the device advances the state the filter uses, and
  // msckf_hip_get_imu_state answers from it without a device round trip.  Any other device-side change of the state
  // (marginalize, the batched calls) invalidates it (h_imu_ok); the next getter reads the device and re-validates.
  std::vector<S> h_imu;
  // single-call staging on device
  S* d_rd = nullptr;                                // [B][rd_cap][7]
  int* d_cnt = nullptr;                             // [B] sample counts of a propagate_range_counts chunk
  S* d_pfin = nullptr;                              // [B][f_cap][4] stored feature positions (mode 1)
  S* wl_obs = nullptr;         // the coordinates of the single-call work-lists: [B][2 wl_blk.ib], beside the core's wl_i

  int alloc() override {
    h_imu.assign((size_t)B * IMU_STRIDE, S(0));
    d.B = B; d.n_cap = n_cap; d.f_cap = f_cap; d.m_cap = m_cap;
    const routes::Geometry g = routes::geometry(B, n_cap, f_cap, m_cap, sizeof(S));   // update_routes.h: the routes read the same record
    d.n6cap = g.n6cap; d.ld = g.ld; d.ldR = g.ldR; d.nchunk = g.nchunk;
    // 6 n_cap + 1 <= 384 (n_cap <= 63): the compression kernels' column capacity; it also bounds everything indexed by a state
    // column or a camera slot further down (k_prune_inplace keeps ceil(ld / 16) x ceil(ld / 256) <= 25 x 2 elements per thread: ld <= 400; 6-bit slot fields of trk_first)
    if (g.refusal == routes::GEO_N_CAP) return fail(-ENOTSUP, "n_cap too large: 6*n_cap+1 must be <= 384 (at most 63 camera states)");
    const size_t Bz = B, pl = (size_t)d.ld * d.ld, nl = (size_t)d.n6cap * d.n6cap, dn = (size_t)d.ld * d.n6cap;
    const size_t TF = Bz * f_cap;
    int rc = 0;
    rc |= dalloc(&d.imu, Bz * IMU_STRIDE); rc |= dalloc(&d.cam, Bz * n_cap * CAM_STRIDE); rc |= dalloc(&d.prm, Bz * PRM_STRIDE);
    rc |= dalloc(&d.qf, Bz * QF_STRIDE);
    rc |= dalloc(&d.P, Bz * pl); rc |= dalloc(&P_spare, Bz * pl); d.Pout = nullptr; d.fuse_drop = nullptr; d.ncam_defer = 0;
    rc |= dalloc(&d.ncam, Bz); rc |= dalloc(&d.n_resid, Bz);
    rc |= dalloc(&d.trk_status, TF); rc |= dalloc(&d.trk_pf, TF * 4); rc |= dalloc(&d.trk_gamma, TF);
    d.h16 = h16 ? 1 : 0; d.trk_Hx = nullptr; d.trk_Hx16 = nullptr;
    if (h16) rc |= dalloc(&d.trk_Hx16, TF * m_cap * 12); else rc |= dalloc(&d.trk_Hx, TF * m_cap * 12);
    rc |= dalloc(&d.trk_V, TF * 2 * m_cap * 4); rc |= dalloc(&d.trk_Zf, TF * 3 * (size_t)d.ldR);
    rc |= dalloc(&d.trk_ro, TF * 2 * m_cap); rc |= dalloc(&d.trk_first, TF);
    rc |= dalloc(&d.row_start, Bz * (f_cap + 1)); rc |= dalloc(&d.trk_order, TF); rc |= dalloc(&d.stats, Bz * STAT_STRIDE);
    rc |= dalloc(&d.Rbuf, Bz * d.nchunk * (size_t)d.n6cap * d.ldR);
    // information-form compression (kernels_gram.hip + kernels_chol.hip)
    d.compress = g.compress;   // blocked matrix-core Cholesky (kernels_chol.hip), two levels beyond 192 columns
    d.Mp = nullptr; d.Mp2 = nullptr;
    if (g.has_Mp2) rc |= dalloc(&d.Mp2, Bz * 24 * 256);
    if (d.compress) {
      if (g.has_Mp) rc |= dalloc(&d.Mp, Bz * 12 * 256);
      rc |= dalloc(&d.trk_B, TF * 3 * (size_t)d.ldR); rc |= dalloc(&d.trk_rw, TF * 2 * m_cap); rc |= dalloc(&d.trk_inv, TF * n_cap);
      rc |= dalloc(&d.Dg, Bz * n_cap * DG_STRIDE);
      d.lam_part = g.lam_parts ? (long)(Bz * (size_t)d.ldR * d.ldR) : 0;     // up to four copies of Lam^ for the split-K SYRK (windows up to 31 cameras)
      d.gram_parts = routes::GRAM_PARTS;   // P = 4 (sixteen workgroups per trajectory) measured: k_gram 56 -> 54 us, the Cholesky's extra load round 64 -> 66 us
      rc |= dalloc(&d.Lam, Bz * (size_t)d.ldR * d.ldR * (d.lam_part ? 4 : 1));
    }
    rc |= dalloc(&d.PHt, Bz * dn); rc |= dalloc(&d.Smat, Bz * nl); rc |= dalloc(&d.Linv, Bz * nl); rc |= dalloc(&d.W, Bz * dn);
    rc |= dalloc(&d.K, Bz * dn); rc |= dalloc(&d.A, Bz * pl); rc |= dalloc(&d.AP, Bz * pl); rc |= dalloc(&d.X, Bz * pl); rc |= dalloc(&d.dx, Bz * d.ld);
    rc |= dalloc(&d.keep, Bz * n_cap); rc |= dalloc(&d.nkeep, Bz); rc |= dalloc(&d.ncam_upd, Bz); rc |= dalloc(&d.nres_upd, Bz);
    rc |= dalloc(&d_pfin, TF * 4); d.trk_pfin = d_pfin; d.mode = 0; d.ncam_bias = 0;
    d.small_split = 0;
    apply_settings();
    rc |= dalloc(&d.gain_bar, Bz * 32);
    rd_cap = 64;
    rc |= dalloc(&d_rd, Bz * rd_cap * RD_STRIDE); rc |= dalloc(&d_cnt, Bz);
    HIPCHK(hipHostMalloc(&h_rb, ((size_t)n_cap * CAM_STRIDE + IMU_STRIDE) * sizeof(S), hipHostMallocDefault));
    wl_blk = inputs::SingleBlock(f_cap, m_cap);
    rc |= dalloc(&wl_i, Bz * wl_blk.ib); rc |= dalloc(&wl_obs, Bz * wl_blk.ib * 2);
    dv_ncam = d.ncam; dv_nres = d.n_resid; dv_stats = d.stats; info_form = d.trk_B != nullptr;
    if (rc) return rc;
    use_single_worklists();
    if (g.refusal == routes::GEO_M_CAP) return fail(-EINVAL, "m_cap too large for the feature kernel's LDS budget");
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }
  void apply_settings() override {
    const Settings& s = settings;
    d.joseph = s.cov_update; d.gate_early = s.gate_early; d.gain_fused_s = s.fused_s; d.feat_pair = s.feat_pair; d.gain_parts = s.gain_parts;
    d.lit.serial = s.lit_serial; d.lit.route = s.lit_route;
    d.lit.tol = s.lit_tol >= 0 ? s.lit_tol : (sizeof(S) == 4 ? 8e-4 : 1e-10);
    small_limit = routes::small_limit(s.small_update, f_cap, sizeof(S), update_small_granted());
  }
  void use_single_worklists() {
    d.trk_n = wl_i + wl_blk.N_AT; d.trk_M = wl_i + wl_blk.M_AT; d.trk_slots = wl_i + wl_blk.slots_at(); d.trk_obs = wl_obs; d.trk_off = nullptr;
    d.wl_stride_n = wl_blk.ib; d.wl_stride_f = wl_blk.ib; d.wl_stride_o = wl_blk.ib;
  }
  // Dev view whose work-list pointers start at trajectory b0 (kernels index work-lists by b - b0)
  Dev<S> view(int b0) const {
    Dev<S> v = d;
    v.trk_n += (long)b0 * d.wl_stride_n; v.trk_M += (long)b0 * d.wl_stride_f;
    v.trk_slots += (long)b0 * d.wl_stride_o; v.trk_obs += 2 * (long)b0 * d.wl_stride_o;
    return v;
  }

  // The five derived noise parameters PRM_WU .. PRM_LIT of trajectory b for the batch's anisotropic-noise mode
  // (dev_common.h); allocates the literal route's work space when the first trajectory needs it.
  int derive_noise(int b, S* out5) {
    const double u = h_uv[2 * (size_t)b], v = h_uv[2 * (size_t)b + 1];
    const bool was = h_lit[b] != 0;
    bool lit = false;
    if (u == v) { out5[0] = 1; out5[1] = 1; out5[2] = (S)u; out5[3] = (S)u; out5[4] = 0; }
    else if (settings.aniso_mode == 0 && !h16 && d.trk_B) { out5[0] = 1; out5[1] = 1; out5[2] = 1; out5[3] = (S)u; out5[4] = 1; lit = true; }
    else { out5[0] = (S)(1.0 / std::sqrt(u)); out5[1] = (S)(1.0 / std::sqrt(v)); out5[2] = 1; out5[3] = 1; out5[4] = 0; }
    if (lit && !d.lit.W2) { const int rc = lit_alloc(); if (rc) return rc; }
    if (lit != was) { n_lit += lit ? 1 : -1; h_lit[b] = lit ? 1 : 0; }
    return 0;
  }
  // work space of kernels_literal.hip (a few (6 n_cap)^2 matrices per trajectory); only allocated when a trajectory has
  // u_var' != v_var' on the literal route
  int lit_alloc() {
    if (!literal_lds_available()) return fail(-ENOTSUP, "this device does not grant the 94 KB of LDS per workgroup the literal anisotropic route needs (msckf_hip_set_anisotropic_noise(h, 1, 0) selects pre-whitening)");
    LitBufs& L = d.lit;
    const size_t Bz = B, n1 = (size_t)d.n6cap + 1;
    L.ldx = ((f_cap * std::max(2 * m_cap - 3, 1) + 7) / 8) * 8;
    L.r_cap = d.n6cap + 15; L.ldg = f_cap * m_cap + 8; L.ldz = L.r_cap + (int)n1; L.kept_stride = 6 * (d.n6cap + 16) + 64;
    int rc = 0;
    rc |= dalloc(&L.tau, Bz * (2 * n1 + 2));
    rc |= dalloc(&L.Vf, Bz * f_cap * 2 * m_cap * 3); rc |= dalloc(&L.Tf, Bz * f_cap * 9);
    rc |= dalloc(&L.row0, Bz * (f_cap + 1)); rc |= dalloc(&L.obs0, Bz * (f_cap + 1)); rc |= dalloc(&L.otrk, Bz * L.ldg); rc |= dalloc(&L.kept, Bz * L.kept_stride);
    rc |= dalloc(&L.TH, Bz * L.r_cap * n1); rc |= dalloc(&L.Z, Bz * (size_t)L.ldz * L.ldz);
    L.w2_stride = lit_ws_doubles(d.n6cap, m_cap, L.r_cap);
    rc |= dalloc(&L.W2, Bz * (size_t)L.w2_stride);
    // the sweep over the dense stack (MSCKF_HIP_LITERAL_ROUTE=1: tests, A/B runs) needs the stack itself and the u-rows of A Q_1
    if (settings.lit_route == 1) { rc |= dalloc(&L.X, Bz * L.ldx * n1); rc |= dalloc(&L.G, Bz * (size_t)L.ldg * L.r_cap); }
    rc |= dalloc(&L.info, Bz * 8);
    rc |= dalloc(&L.BD, Bz * f_cap * 6 * (size_t)d.ldR); rc |= dalloc(&L.Gam, Bz * (size_t)d.ldR * d.ldR); rc |= dalloc(&L.Du, Bz * n_cap * 24);
    if (settings.lit_timers) rc |= dalloc(&L.tim, Bz * LIT_TIM_SLOTS);
    if (rc) { L.W2 = nullptr; return fail(-ENOMEM, "work space of the literal anisotropic route (msckf_hip_set_anisotropic_noise(h, 1, 0) selects pre-whitening)"); }
    return 0;
  }
  int set_aniso(int mode, double tol) override {
    if (mode < 0 || mode > 1) return fail(-EINVAL, "mode: 0 the reference's R_n = Q_1^T R_o Q_1 on the device, 1 pre-whitened rows");
    if (int rc = enter()) return rc;
    settings.aniso_mode = mode; settings.lit_tol = tol;
    apply_settings();
    for (int b = 0; b < B; ++b) {
      if (!traj[b].initialized) continue;
      S out5[5];
      const int rc = derive_noise(b, out5);
      if (rc) return rc;
      if (const int rc = write_dev(d.prm + (size_t)b * PRM_STRIDE + PRM_WU, out5, sizeof(out5))) return rc;
    }
    return 0;
  }
  int lit_info(int b, int* out8) override {
    if (chk(b)) return fail(-EINVAL, "trajectory index out of range");
    if (!d.lit.info) { for (int i = 0; i < 8; ++i) out8[i] = 0; return 0; }
    if (int rc = enter()) return rc;
    if (const int rc = read_back(out8, d.lit.info + (size_t)b * 8, 8 * sizeof(int))) return rc;
    if (d.lit.tim) {     // MSCKF_HIP_LITERAL_TIMERS=1 (profiling runs): phase durations of the last launch in microseconds on stderr
      long long t[LIT_TIM_SLOTS];
      if (const int rc = read_back(t, d.lit.tim + (size_t)b * LIT_TIM_SLOTS, sizeof(t))) return rc;
      std::fprintf(stderr, "[k_literal b=%d] us: explicit rows %.0f Gram %.0f sweep %.0f kept %.0f handed-through rows %.0f basis products %.0f Z fill %.0f eliminate %.0f store %.0f total %.0f\n", b,
                   (t[2] - t[1]) * 0.01, (t[3] - t[2]) * 0.01, (t[4] - t[3]) * 0.01, (t[5] - t[4]) * 0.01, (t[6] - t[5]) * 0.01,
                   (t[8] - t[6]) * 0.01, (t[10] - t[8]) * 0.01, (t[11] - t[10]) * 0.01, (t[9] - t[11]) * 0.01, (t[9] - t[0]) * 0.01);
      std::fprintf(stderr, "[k_literal b=%d] us: the sweep's panels = stage %.0f + core %.0f + rows / columns %.0f + results and trailing pass %.0f; basis products = staging %.0f + Z %.0f + rest %.0f\n", b,
                   t[12] * 0.01, t[13] * 0.01, t[14] * 0.01, t[15] * 0.01, (t[7] - t[6]) * 0.01, (t[23] - t[7]) * 0.01, (t[8] - t[23]) * 0.01);
      if (out8[6] > 0)
        std::fprintf(stderr, "[k_literal b=%d] us: the %d kept handed-through rows = column operations %.0f + Gram of the start %.0f + its products %.0f + reflectors %.0f + t~ %.0f + products with the explicit rows, Gam y %.0f + pair products %.0f\n", b, out8[6],
                     (t[16] - t[5]) * 0.01, (t[17] - t[16]) * 0.01, (t[18] - t[17]) * 0.01, (t[19] - t[18]) * 0.01, (t[20] - t[19]) * 0.01, (t[21] - t[20]) * 0.01, (t[22] - t[21]) * 0.01);
    }
    return 0;
  }
  // MSCKF::initialize with the whole noiseParams::Q_imu (12 x 12) and initial_imu_covar (15 x 15), column-major (types.h:90-91).
  // Q_imu enters the filter only through G Q_imu G^T in Phi (P_II + G Q_imu G^T dT) Phi^T, which msckf.h:143 symmetrises:
  // with X = G Q_imu G^T, (Phi (P + X dT) Phi^T + its transpose) / 2 = Phi (P + (X + X^T) / 2 dT) Phi^T for symmetric P_II, and
  // (X + X^T) / 2 = G ((Q_imu + Q_imu^T) / 2) G^T -- only the symmetric part of Q_imu ever reaches P, so that is what is stored.
  // initial_imu_covar is P_II as it is (msckf.h:86): it must be symmetric.  No off-diagonal entry anywhere: exactly init().
  int init_full(int b, const double* cam, const double* uv2, const double* Q144, const double* P0_225, const double* params, const double* imu) override {
    if (int rc = guard()) return rc;
    if (chk(b)) return fail(-EINVAL, "trajectory index out of range");
    double pmax = 0;
    for (int i = 0; i < 144; ++i) if (!std::isfinite(Q144[i])) return fail(-EINVAL, "Q_imu has a non-finite entry");
    for (int i = 0; i < 225; ++i) { if (!std::isfinite(P0_225[i])) return fail(-EINVAL, "initial_imu_covar has a non-finite entry"); pmax = std::max(pmax, std::fabs(P0_225[i])); }
    for (int j = 0; j < 15; ++j)
      for (int i = 0; i < j; ++i)
        if (std::fabs(P0_225[i + 15 * j] - P0_225[j + 15 * i]) > 1e-12 * pmax) return fail(-EINVAL, "initial_imu_covar is not symmetric (to 1e-12 of its largest entry)");
    double noise[29], qs[QF_STRIDE] = {0};
    noise[0] = uv2[0]; noise[1] = uv2[1];
    for (int i = 0; i < 12; ++i) noise[2 + i] = Q144[i + 12 * i];
    for (int i = 0; i < 15; ++i) noise[14 + i] = P0_225[i + 15 * i];
    bool full = false;
    for (int i = 0; i < 12; ++i)
      for (int j = i; j < 12; ++j) {
        qs[qf_index(i, j)] = i == j ? Q144[i + 12 * i] : (Q144[i + 12 * j] + Q144[j + 12 * i]) / 2;
        if (i != j && (S)qs[qf_index(i, j)] != S(0)) full = true;
      }
    return init_core(b, cam, noise, full ? qs : nullptr, P0_225, params, imu);
  }
  // q78: upper triangle of the symmetric Q_imu (qf_index), null = diagonal Q_imu (noise[2..13]); P0: the whole
  // initial_imu_covar (column-major), null = its diagonal noise[14..28]
  int init_core(int b, const double* cam, const double* noise, const double* q78, const double* P0, const double* params, const double* imu) override {
    if (int rc = guard()) return rc;
    if (chk(b)) return fail(-EINVAL, "trajectory index out of range");
    if (!(noise[0] > 0) || !(noise[1] > 0)) return fail(-EINVAL, "u_var_prime / v_var_prime must be positive");
    if (int rc = enter()) return rc;
    S prm[PRM_STRIDE] = {0}, st_imu[IMU_STRIDE] = {0}, qf[QF_STRIDE] = {0};
    if (q78) { for (int i = 0; i < QF_FLAG; ++i) qf[i] = (S)q78[i]; qf[QF_FLAG] = 1; }
    for (int i = 0; i < 12; ++i) prm[i] = (S)cam[i];
    prm[PRM_UVAR] = (S)noise[0]; prm[PRM_VVAR] = (S)noise[1];
    for (int i = 0; i < 12; ++i) prm[PRM_Q + i] = (S)noise[2 + i];
    for (int i = 0; i < 8; ++i) prm[PRM_GN + i] = (S)params[i];
    h_uv[2 * (size_t)b] = noise[0]; h_uv[2 * (size_t)b + 1] = noise[1];
    { const int rc0 = derive_noise(b, prm + PRM_WU); if (rc0) return rc0; }
    for (int i = 0; i < 29; ++i) st_imu[i] = (S)imu[i];
    for (int i = 0; i < 4; ++i) st_imu[IQN + i] = st_imu[IQ + i];        // msckf.h:83-85
    for (int i = 0; i < 3; ++i) { st_imu[IVN + i] = st_imu[IV + i]; st_imu[IPN + i] = st_imu[IP + i]; }
    std::vector<S> P((size_t)d.ld * d.ld, S(0));
    if (P0) { for (int j = 0; j < 15; ++j) for (int i = 0; i < 15; ++i) P[(size_t)j * d.ld + i] = (S)P0[i + 15 * j]; }
    else for (int i = 0; i < 15; ++i) P[(size_t)i * d.ld + i] = (S)noise[14 + i];
    std::copy(st_imu, st_imu + IMU_STRIDE, h_imu.begin() + (size_t)b * IMU_STRIDE); h_imu_ok[b] = 1;
    HIPCHK(hipMemcpyAsync(d.prm + (size_t)b * PRM_STRIDE, prm, sizeof(prm), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d.qf + (size_t)b * QF_STRIDE, qf, sizeof(qf), hipMemcpyHostToDevice, st));   // (a diagonal Q_imu clears the flag)
    h_qfull[b] = q78 ? 1 : 0;
    HIPCHK(hipMemcpyAsync(d.imu + (size_t)b * IMU_STRIDE, st_imu, sizeof(st_imu), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d.P + (size_t)b * d.ld * d.ld, P.data(), P.size() * sizeof(S), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d.ncam + b, 0, sizeof(int), st));
    h_ncam[b] = 0;
    HIPCHK(hipMemsetAsync(d.n_resid + b, 0, sizeof(long long), st));
    HIPCHK(hipMemsetAsync(d.stats + (size_t)b * STAT_STRIDE, 0, sizeof(int) * STAT_STRIDE, st));
    HIPCHK(hipMemsetAsync(wl_i + (size_t)b * wl_blk.ib + wl_blk.N_AT, 0, sizeof(int), st));
    HIPCHK(hipStreamSynchronize(st));
    HostTraj& t = traj[b];
    t = HostTraj();
    t.initialized = true;
    t.min_track_length = (int)params[5]; t.max_track_length = (int)params[6]; t.max_cam_states = (int)params[7];
    t.redundancy_angle_thresh = params[3]; t.redundancy_distance_thresh = params[4];
    return 0;
  }
  // propogateImuStateRK (msckf.h:1425-1467) + the anchors of msckf.h:138-141 on the host copy of trajectory b, in S arithmetic
  static void host_rk(S* x, const double* rd7) {
    const S dT = (S)rd7[6];
    const S w[3] = {(S)rd7[0] - x[IBG], (S)rd7[1] - x[IBG + 1], (S)rd7[2] - x[IBG + 2]};
    // 0.5 * omegaMat(w) applied to y = (-x, -y, -z, w) of q_IG (matrix_utils.h:19-30)
    auto op = [&](const S y[4], S o[4]) {
      o[0] = S(0.5) * (w[2] * y[1] - w[1] * y[2] + w[0] * y[3]);
      o[1] = S(0.5) * (-w[2] * y[0] + w[0] * y[2] + w[1] * y[3]);
      o[2] = S(0.5) * (w[1] * y[0] - w[0] * y[1] + w[2] * y[3]);
      o[3] = S(0.5) * (-w[0] * y[0] - w[1] * y[1] - w[2] * y[2]);
    };
    const S y0[4] = {-x[IQ + 1], -x[IQ + 2], -x[IQ + 3], x[IQ]};
    S k0[4], k1[4], k2[4], k3[4], k4[4], k5[4], t[4];
    op(y0, k0);
    for (int i = 0; i < 4; ++i) t[i] = y0[i] + (k0[i] / S(4)) * dT;
    op(t, k1);
    for (int i = 0; i < 4; ++i) t[i] = y0[i] + (k0[i] / S(8) + k1[i] / S(8)) * dT;
    op(t, k2);
    for (int i = 0; i < 4; ++i) t[i] = y0[i] + (-k1[i] / S(2) + k2[i]) * dT;
    op(t, k3);
    for (int i = 0; i < 4; ++i) t[i] = y0[i] + (k0[i] * S(3) / S(16) + k3[i] * S(9) / S(16)) * dT;
    op(t, k4);
    for (int i = 0; i < 4; ++i) t[i] = y0[i] + (-k0[i] * S(3) / S(7) + k1[i] * S(2) / S(7) + k2[i] * S(12) / S(7) - k3[i] * S(12) / S(7) + k4[i] * S(8) / S(7)) * dT;
    op(t, k5);
    S yt[4];
    for (int i = 0; i < 4; ++i) yt[i] = y0[i] + (S(7) * k0[i] + S(32) * k2[i] + S(12) * k3[i] + S(32) * k4[i] + S(7) * k5[i]) * dT / S(90);
    S q[4] = {yt[3], -yt[0], -yt[1], -yt[2]};
    const S nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    // v += (C_IG^T (a - b_a) + g) dT with the OLD attitude, p += v_old dT
    const S qw = x[IQ], qx = x[IQ + 1], qy = x[IQ + 2], qz = x[IQ + 3];
    const S R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)},
                       {2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)},
                       {2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)}};
    const S am[3] = {(S)rd7[3] - x[IBA], (S)rd7[4] - x[IBA + 1], (S)rd7[5] - x[IBA + 2]};
    for (int i = 0; i < 3; ++i) x[IP + i] += x[IV + i] * dT;
    for (int i = 0; i < 3; ++i) x[IV + i] += (R[0][i] * am[0] + R[1][i] * am[1] + R[2][i] * am[2] + x[IG + i]) * dT;
    for (int i = 0; i < 4; ++i) x[IQ + i] = q[i] / nq;
    for (int i = 0; i < 4; ++i) x[IQN + i] = x[IQ + i];
    for (int i = 0; i < 3; ++i) { x[IVN + i] = x[IV + i]; x[IPN + i] = x[IP + i]; }
  }
  void mirror_advance(int b, const double* rd, int K) override {
    for (int k = 0; k < K; ++k) host_rk(h_imu.data() + (size_t)b * IMU_STRIDE, rd + (size_t)k * RD_STRIDE);
  }
  // then_augment: augmentState follows for the same trajectories -- k_propagate's fused variant on the last chunk (as run_frames)
  // With a count per trajectory (in.Kb) a trajectory that has run out has none in the later chunks: k_propagate leaves it alone
  int propagate_device(const inputs::Readings& in, int b0, bool then_augment) override {
    const int nb = in.nb;
    for (int k0 = 0; k0 < in.kmax; k0 += rd_cap) {
      const int kk = in.rows(k0, rd_cap);
      unsigned char* raw = nullptr;
      int rc = stage_acquire(in.staged_bytes(kk, sizeof(S)), &raw);
      if (rc) return rc;
      S* tmp = reinterpret_cast<S*>(raw); int* hc = reinterpret_cast<int*>(raw + in.counts_at(kk, sizeof(S)));
      in.pack(tmp, hc, k0, kk, rd_cap);
      HIPCHK(hipMemcpyAsync(d_rd, tmp, in.scalars(kk) * sizeof(S), hipMemcpyHostToDevice, st));
      if (in.Kb) HIPCHK(hipMemcpyAsync(d_cnt, hc, nb * sizeof(int), hipMemcpyHostToDevice, st));
      rc = stage_release();
      if (rc) return rc;
      if (in.Kb) launch_propagate<S>(d, b0, nb, d_rd, (long)kk * RD_STRIDE, kk, st, false, qroute(b0, nb), d_cnt);
      else launch_propagate<S>(d, b0, nb, d_rd, (long)kk * RD_STRIDE, kk, st, then_augment && k0 + kk >= in.K, qroute(b0, nb));
      HIPCHK(hipGetLastError());
    }
    return 0;
  }
  int augment(int b0, int nb) override {
    if (int rc = guard()) return rc;
    if (chk_range(b0, nb)) return fail(-EINVAL, "trajectory range out of bounds");
    HIPCHK(hipSetDevice(device));
    if (pend_b >= 0 && pend_b == b0 && nb == 1 && !pend_rd.empty()) {     // the image's IMU samples are still here: one launch for both
      const int rc = flush_pending(true);
      if (rc) return rc;
    } else {
      if (int rc = enter()) return rc;
      launch_augment<S>(d, b0, nb, st);
    }
    for (int b = b0; b < b0 + nb; ++b) if (h_ncam[b] < n_cap) h_ncam[b]++;
    HIPCHK(hipGetLastError());
    return 0;
  }
  int set_tracks(int b, int F, const int* M, const int* slots, const double* obs) override {
    if (chk(b)) return fail(-EINVAL, "trajectory index out of range");
    int rc = check_worklist(F, M, slots);
    if (rc) return rc;
    if (int rc = enter()) return rc;
    // only the F rows in use travel, as the device holds them: the ints in one copy, the coordinates in a second one, both out
    // of one pinned block
    const size_t nI = wl_blk.ints(F), nO = wl_blk.scalars(F);
    unsigned char* raw = nullptr;
    rc = stage_acquire(wl_blk.staged_bytes(nI, nO, sizeof(S)), &raw);
    if (rc) return rc;
    int* hI = reinterpret_cast<int*>(raw); S* hO = reinterpret_cast<S*>(raw + wl_blk.coords_at(nI));
    wl_blk.pack(hI, hO, F, M, slots, obs);
    HIPCHK(hipMemcpyAsync(wl_i + (size_t)b * wl_blk.ib, hI, (F ? nI : (size_t)wl_blk.M_AT) * sizeof(int), hipMemcpyHostToDevice, st));
    if (F) HIPCHK(hipMemcpyAsync(wl_obs + (size_t)b * wl_blk.ib * 2, hO, nO * sizeof(S), hipMemcpyHostToDevice, st));
    rc = stage_release();
    if (rc) return rc;
    traj[b].wl_F = F;
    return 0;
  }
  int set_tracks_range(int b0, int nb, const std::vector<WorkList>& wl) override {
    if (chk_range(b0, nb) || (int)wl.size() != nb) return fail(-EINVAL, "trajectory range out of bounds");
    for (int i = 0; i < nb; ++i) { const int rc = check_worklist((int)wl[i].M.size(), wl[i].M.data(), wl[i].slots.data()); if (rc) return rc; }
    if (int rc = enter()) return rc;
    // the device's padded single-call layout for the whole range: nb whole blocks of ints and of coordinates, out of one
    // pinned block, two copies
    const size_t nI = (size_t)nb * wl_blk.ib, nO = (size_t)nb * wl_blk.ib * 2;
    unsigned char* raw = nullptr;
    int rc = stage_acquire(wl_blk.staged_bytes(nI, nO, sizeof(S)), &raw);
    if (rc) return rc;
    int* hI = reinterpret_cast<int*>(raw); S* hO = reinterpret_cast<S*>(raw + wl_blk.coords_at(nI));
    parallel_for(nb, [&](int i) {
      wl_blk.pack(hI + (size_t)i * wl_blk.ib, hO + (size_t)i * wl_blk.ib * 2, (int)wl[i].M.size(), wl[i].M.data(), wl[i].slots.data(), wl[i].obs.data());
      return 0;
    });
    HIPCHK(hipMemcpyAsync(wl_i + (size_t)b0 * wl_blk.ib, hI, nI * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(wl_obs + (size_t)b0 * wl_blk.ib * 2, hO, nO * sizeof(S), hipMemcpyHostToDevice, st));
    rc = stage_release();
    if (rc) return rc;
    for (int i = 0; i < nb; ++i) traj[b0 + i].wl_F = (int)wl[i].M.size();
    return 0;
  }
  // Frame f of a call over [.., f1): does its prune ride on the downdate (the covariance lands, pruned, in the other buffer and
  // the next frame's k_propagate commits the window size)?  Never the call's last frame: it prunes with its own launch, so that
  // ncam is final when the call returns; and no frame while the pruned-state log is on: its record is the state between the update
  // and the prune, which only the prune's own launch leaves in reach.  The frame step and commit_buffer_parity both ask here.
  bool fuse_frame(int f, int f1) const { return settings.fuse_prune && !prof && !settings.overlap_feature && d.joseph == 0 && f + 1 < f1 && !prn.buf; }
  // every slice ran the same frames; each fused one flipped the buffers
  void commit_buffer_parity(int f0, int f1) override {
    int flips = 0;
    for (int f = f0; f < f1; ++f) flips += fuse_frame(f, f1) ? 1 : 0;
    if (flips & 1) std::swap(d.P, P_spare);
  }
  // compression route of an update's launches (routes::effective_compress).  Every launch of an update -- the early k_feature of
  // the overlap path too -- asks here.
  int update_compress() const { return routes::effective_compress(d.compress, settings.compress_route, n_lit); }
  // ncam_ahead: run_frames advances its host mirror of the window sizes after the frame's launches (the frame's augmentState is
  // not in h_ncam yet when its update is enqueued).  Which route a TRAJECTORY takes depends on its own window size only -- never
  // on its neighbours in the range, on how a batch is cut into slices or a frame range into calls, or on the API used
  // (bit-identical results either way).  A range whose windows all lie on one side of small_limit launches that side's sequence
  // alone; a range with windows on both sides launches both, and every kernel of either leaves the other's trajectories alone
  // (Dev::small_split, other_route).  Inside k_update_small the launch is still sized by the largest short window of the range
  // (LDS strides, and the column-segment width of chol(Lam^): 4 up to 63 columns, 8 beyond); neither changes the order of the
  // operations on any matrix element -- every element takes its rank-1 updates pivot by pivot whichever task holds it -- so the
  // bits are the trajectory's own (tests/test_gpu_ragged.py holds it: 5 .. 14 cameras alone and beside each other).
  // cell_k (run_frames: the frame's sample counts from b0 on): a skipped cell has no augmentState ahead.
  // select_done (the frame step's feature-first order): k_propagate's HEAD instance has run the selection and the block-diagonal sums already.
  // ride (the frame step's order 2, routes::frame_order_chol: k_feature has run, the range is CHAIN_ONLY on the one-level
  // information form, no literal trajectory): the frame's propagate + augmentState, not launched yet, go into the Gram Cholesky's
  // launch (launch_chol_gram_propagate); the selection, k_gram and that launch take the window size from ncam_upd.
  struct CholRide { const S* rd; long rd_stride; int K; int q_route; const int* cnt; int ncam_defer; };
  // the one-launch update's say on a range (routes::small_route) with the handle's own arguments: launch_update and the frame order ask
  routes::SmallRoute range_small_route(int compress, int b0, int nb, int ncam_ahead, const int* cell_k) const {
    return routes::small_route(nb, [&](int i) { return routes::window_cols(h_ncam[b0 + i], ncam_ahead, cell_k && cell_k[i] == IMU_SKIP, n_cap); },
                               small_limit, compress, n_lit, d.joseph, f_cap, sizeof(S), update_small_granted());
  }
  void launch_update(const Dev<S>& vin, int b0, int nb, hipStream_t q, bool feature_done = false, int ncam_ahead = 0, const int* cell_k = nullptr, bool select_done = false,
                     const CholRide* ride = nullptr) {
    invalidate_imu(b0, nb);            // the update corrects the IMU state on the device (msckf.h:1376-1383)
    Dev<S> v = vin;
    v.compress = update_compress();
    if (!feature_done) { stage_begin(2, q); launch_feature<S>(v, b0, nb, q); stage_end(2, q); }
    // information form: k_select and the block-diagonal reduction share a launch (both only read k_feature's outputs)
    const routes::CompressRoute cr = routes::compress_route(v.compress, d.ldR, d.Mp != nullptr, d.lam_part > 0, d.gram_parts);
    if (ride) {
      Dev<S> v2 = v; v2.ncam_bias = 1;
      launch_select_diag<S>(v2, b0, nb, q);
      launch_gram<S>(v2, b0, nb, q, 3);
      v2.ncam_defer = ride->ncam_defer;
      launch_chol_gram_propagate<S>(v2, b0, nb, ride->rd, ride->rd_stride, ride->K, q, ride->q_route, ride->cnt);
      launch_kalman<S>(v, b0, nb, q);
      return;
    }
    if (!select_done) { stage_begin(7, q); if (cr.select_diag) launch_select_diag<S>(v, b0, nb, q); else launch_select<S>(v, b0, nb, q); stage_end(7, q); }
    // short windows (single filters, BASELINE configs[1]): everything after the selection in ONE launch (k_update_small)
    const routes::SmallRoute sr = range_small_route(v.compress, b0, nb, ncam_ahead, cell_k);
    if (sr.kind != routes::CHAIN_ONLY) {
      v.small_split = sr.small_split;
      stage_begin(5, q); launch_update_small<S>(v, b0, nb, q, sr); stage_end(5, q);
      if (sr.kind == routes::SMALL_ONLY) return;
    }
    if (cr.info) {
      // anisotropic pixel noise, literal route: the information matrix of the reference's (T_H, r_n, R_n) replaces H_o^T H_o
      // for those trajectories (kernels_literal.hip)
      stage_begin(3, q);
      launch_gram<S>(v, b0, nb, q, 3);                    // (the literal route starts from the same f64 Gram matrix)
      stage_end(3, q);
      if (n_lit > 0) {
        if (prof) for (int part = 1; part <= 3; ++part) { stage_begin(7 + part, q); launch_literal<S>(v, b0, nb, q, part); stage_end(7 + part, q); }
        else launch_literal<S>(v, b0, nb, q);
      }
      stage_begin(4, q); launch_gram<S>(v, b0, nb, q, 2); stage_end(4, q);
    } else {
      stage_begin(3, q); launch_compress<S>(v, b0, nb, q, 1); stage_end(3, q);
      stage_begin(4, q); launch_compress<S>(v, b0, nb, q, 2); stage_end(4, q);
    }
    stage_begin(5, q); launch_kalman<S>(v, b0, nb, q); stage_end(5, q);
  }
  int marginalize(int b0, int nb, int mode) override {
    if (int rc = guard()) return rc;
    if (int rc = enter_range(b0, nb)) return rc;
    use_single_worklists();
    Dev<S> v = view(b0);
    v.mode = mode;
    launch_update(v, b0, nb, st);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // ---- range forms (host_image_cycle; the per-filter entries with nb = 1)
  int cams_range(int b0, int nb, double* poses7) override {
    if (int rc = guard()) return rc;
    if (int rc = enter_range(b0, nb)) return rc;
    const size_t per = (size_t)n_cap * CAM_STRIDE;
    std::vector<S> tmp(per * nb);
    if (const int rc = read_back(tmp.data(), d.cam + (size_t)b0 * per, tmp.size() * sizeof(S))) return rc;
    for (int i = 0; i < nb; ++i)
      for (int c = 0; c < n_cap; ++c)
        for (int k = 0; k < 7; ++k) poses7[((size_t)i * n_cap + c) * 7 + k] = (double)tmp[(size_t)i * per + (size_t)c * CAM_STRIDE + k];
    return 0;
  }
  int feature_only_range(int b0, int nb, int* status, double* pf3, bool launch) override {
    if (int rc = guard()) return rc;
    if (int rc = enter_range(b0, nb)) return rc;
    if (launch) { use_single_worklists(); launch_feature<S>(view(b0), b0, nb, st); HIPCHK(hipGetLastError()); }
    std::vector<int> stt((size_t)nb * f_cap); std::vector<S> pf((size_t)nb * f_cap * 4);
    HIPCHK(hipMemcpyAsync(stt.data(), d.trk_status + (size_t)b0 * f_cap, stt.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pf.data(), d.trk_pf + (size_t)b0 * f_cap * 4, pf.size() * sizeof(S), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t t = 0; t < stt.size(); ++t) { status[t] = stt[t]; for (int k = 0; k < 3; ++k) pf3[3 * t + k] = (double)pf[4 * t + k]; }
    return 0;
  }
  int set_given_range(int b0, int nb, const double* pf3) override {
    if (int rc = enter_range(b0, nb)) return rc;
    const size_t cnt = (size_t)nb * f_cap * 4;
    unsigned char* raw = nullptr;
    int rc = stage_acquire(cnt * sizeof(S), &raw);
    if (rc) return rc;
    S* tmp = reinterpret_cast<S*>(raw);
    for (size_t t = 0; t < (size_t)nb * f_cap; ++t) { for (int k = 0; k < 3; ++k) tmp[4 * t + k] = (S)pf3[3 * t + k]; tmp[4 * t + 3] = S(0); }
    HIPCHK(hipMemcpyAsync(d_pfin + (size_t)b0 * f_cap * 4, tmp, cnt * sizeof(S), hipMemcpyHostToDevice, st));
    return stage_release();
  }
  int prune_keep_range(int b0, int nb, const std::vector<std::vector<int>>& keep) override {
    if (int rc = guard()) return rc;
    if (chk_range(b0, nb) || (int)keep.size() != nb) return fail(-EINVAL, "trajectory range out of bounds");
    if (int rc = enter()) return rc;
    // [nb][n_cap] slots + [nb] counts through the pinned ring, two copies, one launch (a trajectory that keeps everything is a no-op
    // there).  Like every other input: no wait for the stream in the middle of an image's chain (the update before it, k_prune and
    // the state read after it are one uninterrupted queue)
    const size_t nI = (size_t)nb * n_cap + nb;
    unsigned char* raw = nullptr;
    int rc = stage_acquire(nI * sizeof(int), &raw);
    if (rc) return rc;
    int* hk = reinterpret_cast<int*>(raw); int* hn = hk + (size_t)nb * n_cap;
    std::memset(hk, 0, nI * sizeof(int));
    for (int i = 0; i < nb; ++i) {
      const int nk = (int)keep[i].size();
      if (nk > n_cap) return fail(-EINVAL, "keep list longer than n_cap");
      hn[i] = nk;
      for (int k = 0; k < nk; ++k) hk[(size_t)i * n_cap + k] = keep[i][k];
    }
    HIPCHK(hipMemcpyAsync(d.keep + (size_t)b0 * n_cap, hk, (size_t)nb * n_cap * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d.nkeep + b0, hn, nb * sizeof(int), hipMemcpyHostToDevice, st));
    rc = stage_release();
    if (rc) return rc;
    launch_prune<S>(d, b0, nb, st);
    for (int i = 0; i < nb; ++i) h_ncam[b0 + i] = (int)keep[i].size();
    HIPCHK(hipGetLastError());
    return 0;
  }
  int drop_oldest(int b0, int nb, int n) override {
    if (int rc = guard()) return rc;
    if (int rc = enter_range(b0, nb)) return rc;
    launch_prune<S>(d, b0, nb, st, nullptr, std::max(n, 0));
    for (int b = b0; b < b0 + nb; ++b) h_ncam[b] -= std::max(0, std::min(n, h_ncam[b]));
    HIPCHK(hipGetLastError());
    return 0;
  }
  int get_imu(int b, double* o) override {
    if (int rc = guard()) return rc;
    if (chk(b)) return fail(-EINVAL, "trajectory index out of range");
    S* tmp = h_imu.data() + (size_t)b * IMU_STRIDE;
    if (!h_imu_ok[b]) {
      if (int rc = enter()) return rc;
      if (const int rc = read_back(tmp, d.imu + (size_t)b * IMU_STRIDE, IMU_STRIDE * sizeof(S))) return rc;
      h_imu_ok[b] = 1;
    }
    for (int i = 0; i < 29; ++i) o[i] = (double)tmp[i];
    return 0;
  }
  int set_imu(int b, const double* in) override {
    if (int rc = enter_traj(b)) return rc;
    S tmp[IMU_STRIDE] = {0};
    for (int i = 0; i < 29; ++i) tmp[i] = (S)in[i];
    if (const int rc = write_dev(d.imu + (size_t)b * IMU_STRIDE, tmp, sizeof(tmp))) return rc;
    std::copy(tmp, tmp + IMU_STRIDE, h_imu.begin() + (size_t)b * IMU_STRIDE); h_imu_ok[b] = 1;
    return 0;
  }
  int get_cams(int b, double* o, int cap, int* nout) override {
    if (int rc = guard()) return rc;
    int n = 0;
    int rc = get_ncam(b, &n);
    if (rc) return rc;
    *nout = n;
    if (n > cap) return fail(-E2BIG, "output buffer too small");
    std::vector<S> tmp((size_t)std::max(n, 1) * CAM_STRIDE);
    if (n) HIPCHK(hipMemcpyAsync(tmp.data(), d.cam + (size_t)b * n_cap * CAM_STRIDE, (size_t)n * CAM_STRIDE * sizeof(S), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) for (int k = 0; k < 7; ++k) o[7 * i + k] = (double)tmp[(size_t)i * CAM_STRIDE + k];
    return 0;
  }
  // the single-filter API knows its window size on the host: no count read first, and the IMU state rides along into the host
  // copy (nothing changes it between an update and the next propagate), so that the getImuState() that follows costs no wait
  int get_cams_known(int b, double* o, int n) override {
    if (int rc = guard()) return rc;
    if (chk(b) || n < 0 || n > n_cap) return fail(-EINVAL, "index out of range");
    if (int rc = enter()) return rc;
    S* tmp = static_cast<S*>(h_rb); S* tim = tmp + (size_t)n_cap * CAM_STRIDE;        // (page-locked: a pageable destination goes through the runtime's own staging copy)
    if (n) HIPCHK(hipMemcpyAsync(tmp, d.cam + (size_t)b * n_cap * CAM_STRIDE, (size_t)n * CAM_STRIDE * sizeof(S), hipMemcpyDeviceToHost, st));
    const bool want_imu = !h_imu_ok[b];
    if (want_imu) HIPCHK(hipMemcpyAsync(tim, d.imu + (size_t)b * IMU_STRIDE, IMU_STRIDE * sizeof(S), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (want_imu) { std::copy(tim, tim + IMU_STRIDE, h_imu.begin() + (size_t)b * IMU_STRIDE); h_imu_ok[b] = 1; }
    for (int i = 0; i < n; ++i) for (int k = 0; k < 7; ++k) o[7 * i + k] = (double)tmp[(size_t)i * CAM_STRIDE + k];
    return 0;
  }
  int set_cam(int b, int slot, const double* in) override {
    if (chk(b) || slot < 0 || slot >= n_cap) return fail(-EINVAL, "index out of range");
    if (int rc = enter()) return rc;
    S tmp[CAM_STRIDE] = {0};
    for (int k = 0; k < 7; ++k) tmp[k] = (S)in[k];
    return write_dev(d.cam + ((size_t)b * n_cap + slot) * CAM_STRIDE, tmp, sizeof(tmp));
  }
  int get_cov(int b, double* P, int ldo) override {
    if (int rc = guard()) return rc;
    int n = 0;
    int rc = get_ncam(b, &n);
    if (rc) return rc;
    const int D = 15 + 6 * n;
    if (ldo < D) return fail(-EINVAL, "ld smaller than D");
    std::vector<S> tmp((size_t)d.ld * d.ld);
    if (const int rc = read_back(tmp.data(), d.P + (size_t)b * d.ld * d.ld, tmp.size() * sizeof(S))) return rc;
    for (int j = 0; j < D; ++j) for (int i = 0; i < D; ++i) P[(size_t)j * ldo + i] = (double)tmp[(size_t)j * d.ld + i];
    return 0;
  }
  int set_cov(int b, const double* P, int D) override {
    if (chk(b)) return fail(-EINVAL, "trajectory index out of range");
    if (D < 15 || (D - 15) % 6 || (D - 15) / 6 > n_cap) return fail(-EINVAL, "bad covariance dimension");
    if (int rc = enter()) return rc;
    std::vector<S> tmp((size_t)d.ld * d.ld, S(0));
    for (int j = 0; j < D; ++j) for (int i = 0; i < D; ++i) tmp[(size_t)j * d.ld + i] = (S)P[(size_t)j * D + i];
    const int n = (D - 15) / 6;
    HIPCHK(hipMemcpyAsync(d.P + (size_t)b * d.ld * d.ld, tmp.data(), tmp.size() * sizeof(S), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d.ncam + b, &n, sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    h_ncam[b] = n;
    return 0;
  }
  // value semantics of the reference object (MSCKF<_S> is copyable, msckf.h:31-67): the filter state of every trajectory
  // -- IMU / camera states, parameters, covariance, window size, counters, flags -- and the host-side track bookkeeping;
  // work buffers and a resident scenario are not state and are not copied
  int copy_from(BatchCore* src) override {
    if (int rc = guard()) return rc;
    Batch<S>* o = dynamic_cast<Batch<S>*>(src);
    // (a literal work space allocated without the dense stack cannot take over the sweep over it: lit_alloc sizes by lit_route)
    if (!o || o->B != B || o->n_cap != n_cap || o->f_cap != f_cap || o->m_cap != m_cap || o->h16 != h16 || (d.lit.W2 && !d.lit.X && o->settings.lit_route == 1))
      return fail(-EINVAL, "copy_state: handles differ in shape or dtype");
    if (o->poisoned) return fail(-EIO, "copy_state: the source handle is unusable after a failed run_frames call (its filter states are undefined)");
    { const int rcf = o->flush_pending(); if (rcf) return rcf; }
    for (int b = 0; b < o->B; ++b) { const int rcm = resolve_map(o, b); if (rcm) return rcm; }   // (work buffers are not copied: points still on the device first)
    if (int rc = enter()) return rc;
    HIPCHK(hipStreamSynchronize(o->st));
    const size_t Bz = B, pl = (size_t)d.ld * d.ld;
    auto cp = [&](void* dst, const void* sp, size_t bytes) { return hipMemcpyAsync(dst, sp, bytes, hipMemcpyDeviceToDevice, st); };
    HIPCHK(cp(d.imu, o->d.imu, Bz * IMU_STRIDE * sizeof(S))); HIPCHK(cp(d.cam, o->d.cam, Bz * n_cap * CAM_STRIDE * sizeof(S)));
    HIPCHK(cp(d.prm, o->d.prm, Bz * PRM_STRIDE * sizeof(S))); HIPCHK(cp(d.P, o->d.P, Bz * pl * sizeof(S)));
    HIPCHK(cp(d.qf, o->d.qf, Bz * QF_STRIDE * sizeof(S)));
    HIPCHK(cp(d.ncam, o->d.ncam, Bz * sizeof(int))); HIPCHK(cp(d.n_resid, o->d.n_resid, Bz * sizeof(long long)));
    HIPCHK(cp(d.stats, o->d.stats, Bz * STAT_STRIDE * sizeof(int))); HIPCHK(cp(d.ncam_upd, o->d.ncam_upd, Bz * sizeof(int)));
    traj = o->traj; h_ncam = o->h_ncam; h_uv = o->h_uv; h_imu = o->h_imu; h_imu_ok = o->h_imu_ok; h_qfull = o->h_qfull;
    settings.take_over(o->settings); frame_settings.take_over(o->frame_settings);
    prn_list.forget(h_ncam);   // (the log stays with its handle; the states taken over are none of its images)
    HIPCHK(hipStreamSynchronize(st));
    std::fill(h_lit.begin(), h_lit.end(), 0); n_lit = 0;   // which trajectories run the literal route is re-derived from the copied parameters
    return set_aniso(settings.aniso_mode, settings.lit_tol);   // applies the settings, re-derives the per-trajectory noise parameters, allocates the literal route's work space if needed
  }
  int track_info(int b, double* out, int cap) override {
    if (int rc = enter_traj(b)) return rc;
    int tmp[STAT_STRIDE];
    if (const int rc = read_back(tmp, d.stats + (size_t)b * STAT_STRIDE, sizeof(tmp))) return rc;
    const int F = tmp[STAT_NTRACKS];
    if (F > cap) return fail(-E2BIG, "output buffer too small");
    std::vector<int> stt(std::max(F, 1)); std::vector<S> gm(std::max(F, 1)), pf((size_t)std::max(F, 1) * 4);
    if (F) {
      HIPCHK(hipMemcpyAsync(stt.data(), d.trk_status + (size_t)b * f_cap, F * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(gm.data(), d.trk_gamma + (size_t)b * f_cap, F * sizeof(S), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(pf.data(), d.trk_pf + (size_t)b * f_cap * 4, (size_t)F * 4 * sizeof(S), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    for (int t = 0; t < F; ++t) {
      double* o = out + 8 * t;
      const bool skipped = stt[t] & ST_MOTION_SKIPPED;
      o[0] = (skipped || (stt[t] & ST_MOTION_OK)) ? 1 : 0;
      o[1] = (stt[t] & ST_TRI_VALID) ? 1 : 0; o[2] = (stt[t] & ST_GATE_PASS) ? 1 : 0; o[3] = (stt[t] & ST_INCLUDED) ? 1 : 0;
      o[4] = (double)gm[t]; o[5] = (double)pf[4 * t]; o[6] = (double)pf[4 * t + 1]; o[7] = (double)pf[4 * t + 2];
    }
    return F;
  }
  // what the feature kernels left per track for the information form, as stored (entries beyond a track's observations or
  // outside its slot range are whatever the buffers held): first [F], Hx [F][m_cap][12], rw [F][m_cap][2], Bh [F][3][6 n_cap + 1]
  int track_blocks(int b, int* first, double* Hx, double* rw, double* Bh, int cap) override {
    if (int rc = enter_traj(b)) return rc;
    if (!d.trk_B || !(d.h16 ? (const void*)d.trk_Hx16 : (const void*)d.trk_Hx) || !d.trk_rw) return fail(-ENOTSUP, "the per-track blocks exist on the information-form route only");
    int tmp[STAT_STRIDE];
    if (const int rc = read_back(tmp, d.stats + (size_t)b * STAT_STRIDE, sizeof(tmp))) return rc;
    const int F = tmp[STAT_NTRACKS];
    if (F > cap) return fail(-E2BIG, "output buffer too small");
    if (!F) return 0;
    const size_t tb = (size_t)b * f_cap, nh = (size_t)F * m_cap * 12, nr = (size_t)F * 2 * m_cap, ldR = (size_t)d.ldR, nB = (size_t)F * 3 * ldR, nc = 6 * (size_t)n_cap + 1;
    std::vector<S> hx(d.h16 ? 0 : nh), r(nr); std::vector<__half> hx16(d.h16 ? nh : 0); std::vector<double> bb(nB);
    HIPCHK(hipMemcpyAsync(first, d.trk_first + tb, F * sizeof(int), hipMemcpyDeviceToHost, st));
    if (d.h16) HIPCHK(hipMemcpyAsync(hx16.data(), d.trk_Hx16 + tb * m_cap * 12, nh * sizeof(__half), hipMemcpyDeviceToHost, st));   // as stored: fp16, widened below
    else HIPCHK(hipMemcpyAsync(hx.data(), d.trk_Hx + tb * m_cap * 12, nh * sizeof(S), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(r.data(), d.trk_rw + tb * 2 * m_cap, nr * sizeof(S), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(bb.data(), d.trk_B + tb * 3 * ldR, nB * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (d.h16) for (size_t i = 0; i < nh; ++i) Hx[i] = (double)__half2float(hx16[i]);
    else for (size_t i = 0; i < nh; ++i) Hx[i] = (double)hx[i];
    for (size_t i = 0; i < nr; ++i) rw[i] = (double)r[i];
    for (size_t q = 0; q < (size_t)F * 3; ++q) for (size_t c = 0; c < nc; ++c) Bh[q * nc + c] = bb[q * ldR + c];
    return F;
  }
  int deltax(int b, double* out, int cap) override {
    int n = 0;
    int rc = get_ncam(b, &n);
    if (rc) return rc;
    const int D = 15 + 6 * n;
    if (D > cap) return fail(-E2BIG, "output buffer too small");
    std::vector<S> tmp(D);
    if (const int rc = read_back(tmp.data(), d.dx + (size_t)b * d.ld, D * sizeof(S))) return rc;
    for (int i = 0; i < D; ++i) out[i] = (double)tmp[i];
    return D;
  }
  int scen_set(int f, int b, const double* rd, int k, int F, const int* M, const int* slots, const double* obs, int n_drop, int flags) override {
    if (f < 0 || f >= sc.frames || chk(b)) return fail(-EINVAL, "scenario cell out of range");
    { const int rc = check_worklist(F, M, slots); if (rc) return rc; }   // before the staged cell is touched
    if (n_drop < 0) return fail(-EINVAL, "negative n_drop");
    if (const char* why = cell_refusal(k, sc.lay.K, F, n_drop, flags)) return fail(-EINVAL, why);
    if (k > 0 && !rd) return fail(-EINVAL, "null readings for a cell with samples");
    sc.set_cell<S>(f, b, rd, k, (flags & CELL_SKIP) != 0, F, M, slots, obs, n_drop);
    committed = false;               // offsets move: the resident copy and the frame's page-locked block are stale until the next commit
    unpin_frame(f);                  // (its chunk is released with the last of its frames: patch -> commit -> stream cycles do not grow)
    return 0;
  }
  // a frame's inputs on the device for a slice that starts at trajectory b0 (input_layouts.h, frame_in): resident, or as
  // uploaded into staging set k
  using FrameIn = inputs::FrameIn<S>;
  FrameIn resident_frame(int f, int b0) const {
    return inputs::frame_in<S>(sc.lay, b0, [&](int s) { return sc_dev[s] + sc.lay.resident_at(s, f, sc.fr_base[f]); });
  }
  FrameIn staged_frame(int f, int k, int b0) const {
    return inputs::frame_in<S>(sc.lay, b0, [&](int s) { return sg_blk[k] + sc.lay.block_at(s, sc.entries(f)); });
  }
  // the replay's three views of frame f: the sequence cells, the assignment with the frame's bases, and the sections of an
  // expanded block (the ordinary frame block of rp.nf[f] entries) to write (replay_out) or to read (replay_frame)
  ReplaySeqIn replay_seq(int f) const {
    using namespace inputs;
    const ScenarioStore& q = rp.seq;
    auto at = [&](int s) { return rp_dev[s] + q.lay.resident_at(s, f, q.fr_base[f]); };
    auto i = [&](int s) { return reinterpret_cast<const int*>(at(s)); };
    return ReplaySeqIn{reinterpret_cast<const double*>(at(SEC_RD)), i(SEC_N), i(SEC_DROP), i(SEC_K), i(SEC_M), i(SEC_OFF), i(SEC_SLOTS), reinterpret_cast<const double*>(at(SEC_OBS))};
  }
  // (the fault record only while some trajectory has a non-zero probability, or the timed form runs: otherwise the unfaulted
  // form is launched)
  ReplayTrajIn replay_traj(int f, bool calib = false) const { return ReplayTrajIn{rp_seq_of, rp_seed, rp_sigma, rp_base + (size_t)f * B, rp.faulted || rp.timed || rp.calibrated() || calib ? rp_fault : nullptr}; }
  // THE expansion's launch, for the frame loop and the read-backs: the timed form while some timing record is non-zero
  // (replay_plan.h, TIMING), otherwise the un-timed launch as it always was
  // calib (the read-back's outputs on the device, or null): the calibrated form -- what runs anyway while some calibration
  // record is non-trivial (replay_plan.h, CALIB), and under trivial records writes the bits of the other forms
  void replay_launch(const ReplayOut<S>& o, int f, int b0, int nb, hipStream_t q, int* code = nullptr, double* delta = nullptr, const ReplayCalibIn* calib = nullptr) {
    if (rp.calibrated() || calib) {
      const ReplayCalibIn c{rp_imucal, rp_camcal, rp.timed, calib ? calib->rd_cal : nullptr, calib ? calib->clip : nullptr, calib ? calib->obs_cal : nullptr};
      launch_replay_expand_calib<S>(replay_seq(f), replay_traj(f, true), replay_model(f), replay_timing(f), c, o, f, b0, nb, rp.K(), f_cap, q, m_cap, code, delta);
    } else if (rp.timed) launch_replay_expand_timed<S>(replay_seq(f), replay_traj(f), replay_model(f), replay_timing(f), o, f, b0, nb, rp.K(), f_cap, q, m_cap, code, delta);
    else launch_replay_expand<S>(replay_seq(f), replay_traj(f), replay_model(f), o, f, b0, nb, rp.K(), f_cap, rp_maxcell[f], q, m_cap, code);
  }
  ReplayOut<S> replay_out(unsigned char* blk, int f) const {
    using namespace inputs;
    const FrameLayout L = rp.out_layout(sizeof(S));
    auto at = [&](int s) { return blk + L.block_at(s, rp.nf[f]); };
    auto i = [&](int s) { return reinterpret_cast<int*>(at(s)); };
    return ReplayOut<S>{reinterpret_cast<S*>(at(SEC_RD)), i(SEC_N), i(SEC_DROP), i(SEC_K), i(SEC_M), i(SEC_OFF), i(SEC_SLOTS), reinterpret_cast<S*>(at(SEC_OBS))};
  }
  FrameIn replay_frame(int f, int hh, int b0) const {
    const inputs::FrameLayout L = rp.out_layout(sizeof(S));
    return inputs::frame_in<S>(L, b0, [&](int s) { return rp_blk[hh] + L.block_at(s, rp.nf[f]); });
  }
  // msckf_hip_replay_expand / _ints: k_replay_expand for trajectory b alone into the scratch block, and what it wrote there --
  // rd [K][7] and the cell's coordinate pairs as doubles; ints [3 + 2 f_cap] = n, drop, k, M[f_cap], off[f_cap] and the cell's
  // slots (each pair null or not); code (or null): per SEQUENCE entry 0 kept, 1 outlier, 2 missed, from the same launch.  Under
  // faults M holds the survivors and slots / obs are in partition order.  Returns the cell's entries.  Nothing of the handle's
  // filters, inputs or logs changes.
  // co (msckf_hip_replay_expand_calib): the noise-free calibrated samples rd_cal [K][6], the 6-bit masks of clipped components
  // clip [K] and the mapped noise-free coordinates obs_cal per SEQUENCE entry, from the same launch.
  int replay_expand(int f, int b, double* rd, double* obs, int* ints, int* slots, int cap_entries, int* code = nullptr, double* delta = nullptr, const CalibOut* co = nullptr) override {
    using namespace inputs;
    if (int rc = guard()) return rc;
    if (int rc = refuse(rp.expand_refusal(f, b))) return rc;
    if (int rc = enter()) return rc;
    if (int rc = replay_upload_plan()) return rc;
    if (int rc = replay_walk_table()) return rc;
    const int K = rp.K(), E = (int)rp.entries(rp.seq_of[b], f);
    if (E > cap_entries) return fail(-E2BIG, "output buffer too small for the cell's entries");
    const size_t need = rp.block_bytes(sizeof(S));
    if (need > rp_scratch_bytes) {
      HIPCHK(hipStreamSynchronize(st));
      dfree(rp_scratch); rp_scratch_bytes = 0;
      HIPCHK(hipMalloc((void**)&rp_scratch, need));
      rp_scratch_bytes = need;
    }
    const bool coded = code && (rp.faulted || rp.timed || rp.calibrated());   // (without faults every code is 0: FAULT_KEPT)
    const bool timed = delta && rp.timed;                      // (without timing every delta is 0)
    if (timed && rp.largest > rp_delta_count) {
      HIPCHK(hipStreamSynchronize(st));
      dfree(rp_delta); rp_delta_count = 0;
      HIPCHK(hipMalloc((void**)&rp_delta, rp.largest * sizeof(double)));
      rp_delta_count = rp.largest;
    }
    if (coded && rp.largest > rp_code_count) {
      HIPCHK(hipStreamSynchronize(st));
      dfree(rp_code); rp_code_count = 0;
      HIPCHK(hipMalloc((void**)&rp_code, rp.largest * sizeof(int)));
      rp_code_count = rp.largest;
    }
    if (co && ((size_t)K * 6 > rp_rdcal_count || rp.largest > rp_obscal_count)) {
      HIPCHK(hipStreamSynchronize(st));
      dfree(rp_rdcal); dfree(rp_clip); dfree(rp_obscal); rp_rdcal_count = rp_obscal_count = 0;
      HIPCHK(hipMalloc((void**)&rp_rdcal, (size_t)K * 6 * sizeof(double))); HIPCHK(hipMalloc((void**)&rp_clip, (size_t)K * 6 * sizeof(int)));
      HIPCHK(hipMalloc((void**)&rp_obscal, std::max<size_t>(rp.largest, 1) * 2 * sizeof(double)));
      rp_rdcal_count = (size_t)K * 6; rp_obscal_count = rp.largest;
    }
    const ReplayOut<S> o = replay_out(rp_scratch, f);
    const ReplayCalibIn cal{rp_imucal, rp_camcal, rp.timed, rp_rdcal, rp_clip, rp_obscal};
    replay_launch(o, f, b, 1, st, coded ? rp_code : nullptr, timed ? rp_delta : nullptr, co ? &cal : nullptr);
    HIPCHK(hipGetLastError());
    const size_t base = (size_t)rp.base[(size_t)f * B + b];
    std::vector<S> hr((size_t)K * RD_STRIDE), ho((size_t)2 * std::max(E, 1));
    std::vector<int> hi((size_t)3 + 2 * f_cap), hs(std::max(E, 1));
    HIPCHK(hipMemcpyAsync(hr.data(), o.rd + (size_t)b * K * RD_STRIDE, hr.size() * sizeof(S), hipMemcpyDeviceToHost, st));
    if (E) HIPCHK(hipMemcpyAsync(ho.data(), o.obs + 2 * base, (size_t)2 * E * sizeof(S), hipMemcpyDeviceToHost, st));
    if (E) HIPCHK(hipMemcpyAsync(hs.data(), o.slots + base, (size_t)E * sizeof(int), hipMemcpyDeviceToHost, st));
    if (code) std::fill(code, code + E, (int)msckf_replay::FAULT_KEPT);
    if (coded && E) HIPCHK(hipMemcpyAsync(code, rp_code + base, (size_t)E * sizeof(int), hipMemcpyDeviceToHost, st));
    if (delta) std::fill(delta, delta + E, 0.0);
    if (timed && E) HIPCHK(hipMemcpyAsync(delta, rp_delta + base, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, st));
    std::vector<int> hclip(co ? (size_t)K * 6 : 0);
    if (co && co->rd_cal) HIPCHK(hipMemcpyAsync(co->rd_cal, rp_rdcal, (size_t)K * 6 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (co && co->clip) HIPCHK(hipMemcpyAsync(hclip.data(), rp_clip, (size_t)K * 6 * sizeof(int), hipMemcpyDeviceToHost, st));
    if (co && co->obs_cal && E) HIPCHK(hipMemcpyAsync(co->obs_cal, rp_obscal + 2 * base, (size_t)2 * E * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hi[0], o.n + b, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hi[1], o.drop + b, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hi[2], o.k + b, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hi[3], o.M + (size_t)b * f_cap, (size_t)f_cap * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hi[3 + f_cap], o.off + (size_t)b * f_cap, (size_t)f_cap * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (rd) for (size_t i = 0; i < hr.size(); ++i) rd[i] = (double)hr[i];
    if (obs) for (int i = 0; i < 2 * E; ++i) obs[i] = (double)ho[i];
    if (ints) std::copy(hi.begin(), hi.end(), ints);
    if (slots) std::copy(hs.begin(), hs.begin() + E, slots);
    if (co && co->clip) for (int i = 0; i < K; ++i) { co->clip[i] = 0; for (int c = 0; c < 6; ++c) co->clip[i] |= hclip[(size_t)i * 6 + c] << c; }
    return E;
  }
  // THE frame step: frame f of a call over [f0, f1) for slice s, inputs in staging set `staged`, resident or the replay's --
  // propagate + augmentState, the update, the prune (on the downdate or with its own launch, fuse_frame), the host mirror of
  // the window size.
  // may_overlap (resident inputs only): k_feature reads only what the previous frame's prune left behind -- camera states and
  // P blocks of slots below the newest one, the constant gravity vector -- unless a track observes the camera this frame's
  // augmentState adds.  When none does (host mirror of the window sizes, slots known since scenario_set) and the handle asks
  // for it (set_feature_overlap) it runs on a side stream concurrently with the latency-bound propagate + augment.
  // The same condition, for resident, staged and replay inputs alike (frame_cells has every kind's largest slot), lets a float
  // handle take the feature-first order (routes::frame_order; frame_settings.order, the default): k_feature, then ONE launch
  // with the selection and propagate + augmentState side by side, on the slice's own stream -- no second stream, no event, and
  // the frame's prune rides on the downdate as on every other frame (fuse_frame does not ask about the order).
  void enqueue_frame(Slice& s, int f, int f0, int f1, int staged) override {
    const int b0 = s.b0, nb = s.nb, hh = s.hh;
    const bool replay = staged == IN_REPLAY;
    const FrameIn in = replay ? replay_frame(f, hh, b0) : staged == IN_RESIDENT ? resident_frame(f, b0) : staged_frame(f, staged, b0);
    const bool may_overlap = staged == IN_RESIDENT;
    hipStream_t q = s.q;
    const FrameCells cells = frame_cells(f, staged, hh, b0, nb);   // the host's copy of the frame's cells
    const int* cell_k = cells.k; const int* cell_drop = cells.drop;
    const int K = replay ? rp.K() : sc.lay.K;
    // replay: the slice's trajectories of this frame's block, from the sequences (outside the frame step's own stage timers)
    if (replay) { stage_begin(11, q); replay_launch(replay_out(rp_blk[hh], f), f, b0, nb, q); stage_end(11, q); }
    Dev<S> v = d;
    v.P = s.flipped ? P_spare : d.P; v.ncam_defer = s.pending ? 1 : 0;
    const bool fuse = fuse_frame(f, f1);
    v.trk_n = in.n; v.trk_M = in.M; v.trk_off = in.off; v.trk_slots = in.slots; v.trk_obs = in.obs;
    v.wl_stride_n = 1; v.wl_stride_f = f_cap; v.wl_stride_o = 0;
    // may k_feature run before this frame's augmentState?  (frame_order.h: never on the call's first frame -- the previous call need
    // not have ended with a prune -- nor beside a skipped cell, which gets no camera state: ncam_upd would be one too many)
    const int q_route = qroute(b0, nb);
    const bool select_diag = routes::compress_route(update_compress(), d.ldR, d.Mp != nullptr, d.lam_part > 0, d.gram_parts).select_diag;
    const routes::CompressRoute c_route = routes::compress_route(update_compress(), d.ldR, d.Mp != nullptr, d.lam_part > 0, d.gram_parts);
    const routes::FrameOrderRefusal order1 = routes::frame_order(frame_settings.order, settings.overlap_feature, sizeof(S), select_diag, q_route, nb, h_ncam.data() + b0,
                                                                 cells.maxslot + b0, cell_k + b0, IMU_SKIP, n_cap, f == f0, prof);
    const bool feature_first = order1 == routes::FO_TAKEN;
    // order 2 (frame_order.h): propagate + augmentState wait for the Gram Cholesky's launch, the selection keeps its own
    const bool in_cholesky = routes::frame_order_chol(frame_settings.effective(), order1, c_route.info, c_route.chol_levels,
                                                      range_small_route(update_compress(), b0, nb, 1, cell_k + b0).kind == routes::CHAIN_ONLY, n_lit) == routes::FC_TAKEN;
    const bool early = may_overlap && settings.overlap_feature &&
                       routes::feature_ahead(nb, h_ncam.data() + b0, cells.maxslot + b0, cell_k + b0, IMU_SKIP, n_cap, f == f0, prof) == routes::FO_TAKEN;
    if (feature_first) {
      // feature-first order, on the slice's own stream: k_feature from what the previous frame's prune left (window size from ncam_upd),
      // then the selection's workgroups and propagate + augmentState side by side in one launch (k_propagate's HEAD instance), then the rest of the update;
      // order 2 launches k_feature alone here, the rest in launch_update
      StageRange r("msckf_marginalize(features)+imu_prop+msckf_augment_state");
      Dev<S> v2 = v; v2.ncam_bias = 1;
      v2.compress = update_compress();
      launch_feature<S>(v2, b0, nb, q);
      if (!in_cholesky) launch_frame_head<S>(v2, b0, nb, in.rd, (long)K * RD_STRIDE, K, q, q_route, in.k);
      n_feature_first.fetch_add(1, std::memory_order_relaxed);
      if (in_cholesky) n_in_cholesky.fetch_add(1, std::memory_order_relaxed);
    }
    if (early) {
      (void)hipEventRecord(ev_fa[hh], q);
      (void)hipStreamWaitEvent(sty[hh], ev_fa[hh], 0);
      Dev<S> v2 = v; v2.ncam_bias = 1;
      v2.compress = update_compress();
      launch_feature<S>(v2, b0, nb, sty[hh]);
      (void)hipEventRecord(ev_fb[hh], sty[hh]);
    }
    // propagate and augmentState are always back to back here: one launch (the per-stage profile keeps them apart)
    if (!feature_first) {
      StageRange r("imu_prop+msckf_augment_state");
      stage_begin(0, q); launch_propagate<S>(v, b0, nb, in.rd, (long)K * RD_STRIDE, K, q, !prof, q_route, in.k); stage_end(0, q);
      if (prof) { stage_begin(1, q); launch_augment<S>(v, b0, nb, q, in.k); stage_end(1, q); }
    }
    if (early) (void)hipStreamWaitEvent(q, ev_fb[hh], 0);
    const CholRide ride{in.rd, (long)K * RD_STRIDE, K, q_route, in.k, v.ncam_defer};
    v.ncam_defer = 0;
    if (fuse) { v.Pout = s.flipped ? d.P : P_spare; v.fuse_drop = in.drop; }
    { StageRange r(fuse ? "msckf_marginalize+msckf_prune_empty_states" : "msckf_marginalize"); launch_update(v, b0, nb, q, early || feature_first, 1, cell_k + b0, feature_first, in_cholesky ? &ride : nullptr); }
    if (fuse) s.flipped = !s.flipped;
    else {
      // pruned-state log: the states this frame drops, as the update left them (v.P: in place), with frame ordinal
      // prn.ordinal(f, f0), behind the trajectories' cursors; outside the stage timers
      if (prn.buf) launch_pruned_log<S>(v, b0, nb, q, in.drop, prn.ordinal(f, f0), prn.cap, static_cast<S*>(prn.buf), prn.found);
      StageRange r("msckf_prune_empty_states");
      stage_begin(6, q);
      launch_prune<S>(v, b0, nb, q, in.drop, 0);
      stage_end(6, q);
    }
    s.pending = fuse;
    // frame log: the state the frame leaves -- the covariance buffer that is current after the flip, the window size where the
    // prune left it (ncam_upd while it is pending) -- as record log_base + (f - f0); outside the stage timers
    if (log_buf) launch_frame_log<S>(d, b0, nb, q, s.flipped ? P_spare : d.P, s.pending, static_cast<S*>(log_buf) + (size_t)(log_base + (f - f0)) * B * LOG_STRIDE);
    // NEES log: the same state against frame f's rows of the truth table (and, for a replay whose table asks for it, row f + 1 of
    // the walk table) as record nees_base + (f - f0); the reserve has checked that the table covers f
    if (nees_buf)
      launch_nees_log<S>(d, b0, nb, q, s.flipped ? P_spare : d.P, in.k, tru + msckf_nees::truth_at(f, 0, tru_rows), tru_row_of,
                         tru_walk && nees_replay ? rp_wstart + (size_t)(f + 1) * B * msckf_replay::WALK_ROW : nullptr, f, nees_buf + msckf_nees::record_at(nees_base + (f - f0), 0, B));
    // map log: the tracks of the work-list the update read (in.n, in.M: resident or staged) with frame ordinal
    // map.ordinal(f, f0), behind the trajectories' cursors; also outside the stage timers
    if (map.buf) launch_map_log<S>(d, b0, nb, q, in.n, in.M, map.ordinal(f, f0), map.cap, static_cast<S*>(map.buf), map.found);
    for (int b = b0; b < b0 + nb; ++b) {   // host mirror of the window size: augment (not for a skipped cell), then drop n_drop (clamped as k_make_keep does)
      const bool augmented = h_ncam[b] < n_cap && cell_k[b] != IMU_SKIP;
      if (augmented) h_ncam[b]++;
      const int nd = std::max(0, std::min(cell_drop[b], h_ncam[b]));
      h_ncam[b] -= nd;
      if (prn.buf) prn_list.mirror(b, augmented, nd, prn.ordinal(f, f0), prn.cap);
    }
  }
  // records [r0, r0 + n) of trajectories [b0, b0 + nb) as doubles: one strided copy, one wait
  int frame_log_read(int r0, int n, int b0, int nb, double* out) override {
    if (int rc = guard()) return rc;
    if (r0 < 0 || n < 0 || (long)r0 + n > log_n) return fail(-EINVAL, "record range beyond the records written (msckf_hip_frame_log_count)");
    if (int rc = enter_range(b0, nb)) return rc;
    const size_t row = (size_t)nb * LOG_STRIDE;
    std::vector<S> tmp(std::max<size_t>(row * n, 1));
    if (n && nb)
      HIPCHK(hipMemcpy2DAsync(tmp.data(), row * sizeof(S), static_cast<const S*>(log_buf) + ((size_t)r0 * B + b0) * LOG_STRIDE, (size_t)B * LOG_STRIDE * sizeof(S),
                              row * sizeof(S), (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t i = 0; i < row * n; ++i) out[i] = (double)tmp[i];
    return 0;
  }
  // the records [r0, r1) against ground-truth positions, reduced on the device (k_log_metrics): per trajectory n, sum |e|^2,
  // max |e|, |e| at r1 - 1, sum e^T P_pp^-1 e, records with STAT_ERR != 0
  int frame_log_metrics(int r0, int r1, const double* gt_p, double* out, const int* r0b, const int* r1b) override {
    if (int rc = guard()) return rc;
    if (r0 < 0 || r1 < r0 || r1 > log_n) return fail(-EINVAL, "record range beyond the records written (msckf_hip_frame_log_count)");
    if (int rc = enter()) return rc;
    std::vector<int> rb;                                       // r0b | r1b
    if (r0b) { rb.assign(r0b, r0b + B); rb.insert(rb.end(), r1b, r1b + B); }
    return log_metrics_call("frame_log_metrics", gt_p, (size_t)(r1 - r0) * B * 3, rb.data(), rb.size(), out, (size_t)B * 6, [&](const double* dg, double* dout, const int* dr) {
      launch_log_metrics<S>(static_cast<const S*>(log_buf), B, r0, r1, r0b ? dr : nullptr, r0b ? dr + B : nullptr, dg, dout, st);
    });
  }
  // stored records [r0, r0 + n) of trajectory b of a cursor log as doubles: one copy, after cursor_log_check_range
  int cursor_log_copy(const CursorLog& g, int b, int r0, int n, double* out) {
    if (!n) return 0;
    std::vector<S> tmp((size_t)n * g.stride);
    if (const int rc = read_back(tmp.data(), static_cast<const S*>(g.buf) + ((size_t)b * g.cap + r0) * g.stride, tmp.size() * sizeof(S))) return rc;
    for (size_t i = 0; i < tmp.size(); ++i) out[i] = (double)tmp[i];
    return 0;
  }
  int cursor_log_read(CursorLog& g, int b, int r0, int n, double* out) {
    if (int rc = cursor_log_check_range(g, b, r0, n)) return rc;
    return cursor_log_copy(g, b, r0, n, out);
  }
  int map_log_read(int b, int r0, int n, double* out) override { return cursor_log_read(map, b, r0, n, out); }
  // the stored records with frame ordinal in [q0, q1) against ground-truth landmarks (CSR per cell; both null: none), reduced on
  // the device (k_map_metrics): per trajectory records, matched, sum |e|^2, max |e|, gated records with their own gamma,
  // sum gamma, sum 2 M - 3, unmatched
  int map_log_metrics(int q0, int q1, const double* gt_xyz, const int* gt_off, double* out) override {
    if (int rc = guard()) return rc;
    if (int rc = map_log_check_gt(q0, q1, gt_xyz, gt_off)) return rc;
    if (int rc = enter()) return rc;
    const size_t cells = (size_t)(q1 - q0) * B, noff = gt_off ? cells + 1 : 0, ng = gt_off ? (size_t)gt_off[cells] * 3 : 0;
    return log_metrics_call("map_log_metrics", gt_xyz, ng, gt_off, noff, out, (size_t)B * 8, [&](const double* dg, double* dout, const int* doff) {
      launch_map_metrics<S>(static_cast<const S*>(map.buf), map.found, map.cap, B, q0, q1, gt_off ? dg : nullptr, gt_off ? doff : nullptr, dout, st);
    });
  }
  // the stored records with frame ordinal in [q0, q1), written by run_frames_replay contiguously from replay frame f0, against
  // the faults of their tracks (k_map_fault_metrics): per trajectory the gate's confusion table and the clean passed gamma sums
  int map_log_fault_metrics(int q0, int q1, int f0, double* out) override {
    using namespace inputs;
    if (int rc = guard()) return rc;
    if (int rc = map_log_check_faults(q0, q1, f0)) return rc;
    if (int rc = enter()) return rc;
    if (int rc = replay_upload_plan()) return rc;
    auto i = [&](int s) { return reinterpret_cast<const int*>(rp_dev[s]); };
    return log_metrics_call("map_log_fault_metrics", nullptr, 0, nullptr, 0, out, (size_t)B * msckf_replay::N_FAULT_METRIC, [&](const double*, double* dout, const int*) {
      launch_map_fault_metrics<S>(static_cast<const S*>(map.buf), map.found, map.cap, B, q0, q1, f0, i(SEC_N), i(SEC_M), i(SEC_OFF), replay_traj(0), rp.S, f_cap, dout, st);
    });
  }
  // the map log's read, and the augment ordinal of each record from the host mirror
  int pruned_log_read(int b, int r0, int n, double* out, int* aug_ord) override {
    if (int rc = cursor_log_check_range(prn, b, r0, n)) return rc;
    if (!n) return 0;
    const std::vector<int>& aug = prn_list.aug[b];
    if ((int)aug.size() < r0 + n) return fail(-EIO, "pruned-state log: fewer augment ordinals on the host than records on the device");
    if (int rc = cursor_log_copy(prn, b, r0, n, out)) return rc;
    if (aug_ord) std::copy(aug.begin() + r0, aug.begin() + r0 + n, aug_ord);
    return 0;
  }
  // the stored records with prune ordinal in [q0, q1) against ground-truth poses gt_pose[n_ord][B][7], matched through their
  // augment ordinals (uploaded here, off the frame path), reduced on the device (k_pruned_metrics): out [B][10]
  int pruned_log_metrics(int q0, int q1, const double* gt_pose, int n_ord, double* out) override {
    if (int rc = guard()) return rc;
    if (int rc = cursor_log_check_ordinals(prn, q0, q1)) return rc;
    if (n_ord < 0 || (n_ord > 0 && !gt_pose)) return fail(-EINVAL, "gt_pose: n_ord poses per trajectory, n_ord >= 0, null only with n_ord == 0");
    if (int rc = enter()) return rc;
    std::vector<int> aug((size_t)B * prn.cap, -1);
    for (int b = 0; b < B; ++b) std::copy(prn_list.aug[b].begin(), prn_list.aug[b].end(), aug.begin() + (size_t)b * prn.cap);
    return log_metrics_call("pruned_log_metrics", gt_pose, (size_t)n_ord * B * 7, aug.data(), aug.size(), out, (size_t)B * 10, [&](const double* dg, double* dout, const int* daug) {
      launch_pruned_metrics<S>(static_cast<const S*>(prn.buf), prn.found, prn.cap, B, q0, q1, daug, dg, n_ord, dout, st);
    });
  }
};

// -------------------------------------------------------------------------------------------------
// host bookkeeping shared by both dtypes (restates msckf.h:215-332, 685-717, 765-807, 1469-1485): the list work is
// host_lists.h, free of device calls; here are the drivers that put the device calls between its steps
// -------------------------------------------------------------------------------------------------
int host_update(BatchCore* B, int b, const double* meas, const uint64_t* ids, int n) {
  HostTraj& t = B->traj[b];
  if (!t.initialized) return fail(-EINVAL, "trajectory not initialized");
  if (t.cams.empty()) return fail(-EINVAL, "update() before augmentState() (msckf.h:238 dereferences cam_states_.end()-1)");
  update_lists(t, meas, ids, n);
  return 0;
}

int host_add_features(BatchCore* B, int b, const double* meas, const uint64_t* ids, int n) {
  HostTraj& t = B->traj[b];
  if (!t.initialized) return fail(-EINVAL, "trajectory not initialized");
  if (t.cams.empty()) return fail(-EINVAL, "addFeatures() before augmentState() (msckf.h:320)");
  if (add_features_lists(t, meas, ids, n)) return fail(-EEXIST, "added new feature that was already being tracked");
  return 0;
}

int set_tracks(BatchCore* B, int b, const WorkList& wl) { return B->set_tracks(b, (int)wl.M.size(), wl.M.data(), wl.slots.data(), wl.obs.data()); }

int host_marginalize(BatchCore* B, int b) {
  HostTraj& t = B->traj[b];
  t.map.clear(); t.map_pending = 0;
  WorkList wl;
  build_worklist(t.to_resid, wl);
  int rc = set_tracks(B, b, wl);
  if (rc) return rc;
  if (wl.M.empty()) return B->clear_stats(b);
  rc = B->marginalize(b, 1);
  if (rc) return rc;
  t.map_pending = (int)wl.M.size();   // map_ (msckf.h:371) is read back when it is asked for: no wait for the device inside marginalize()
  return 0;
}

// the triangulated points of the last marginalize() (msckf.h:371: map_.push_back(p_f_G)), fetched on demand
int resolve_map(BatchCore* B, int b) {
  HostTraj& t = B->traj[b];
  const int F = t.map_pending;
  if (F <= 0) return 0;
  t.map_pending = 0;
  std::vector<double> info((size_t)F * 8);
  const int rc = B->track_info(b, info.data(), F);
  if (rc < 0) return rc;
  // track_info's rows (motion passed or skipped, triangulation valid, ..., xyz) back as what append_map reads
  std::vector<int> status(F); std::vector<double> pf((size_t)F * 3);
  for (int i = 0; i < F; ++i) {
    status[i] = (info[8 * i] != 0 ? ST_MOTION_OK : 0) | (info[8 * i + 1] != 0 ? ST_TRI_VALID : 0);
    std::copy(&info[8 * i + 5], &info[8 * i + 5] + 3, &pf[3 * (size_t)i]);
  }
  append_map(t, status.data(), pf.data(), F);
  return 0;
}

// retire what every trajectory of the range planned: one prune launch for the range, then the host lists
static int prune_retired_range(BatchCore* B, int b0, const std::vector<Retirement>& ret) {
  const int nb = (int)ret.size();
  std::vector<std::vector<int>> keep(nb);
  for (int i = 0; i < nb; ++i) keep[i] = ret[i].keep;
  const int rc = B->prune_keep_range(b0, nb, keep);
  if (rc) return rc;
  for (int i = 0; i < nb; ++i) retire_commit(B->traj[b0 + i], ret[i]);
  return 0;
}

int host_prune_empty(BatchCore* B, int b) {
  HostTraj& t = B->traj[b];
  const int last_to_remove = plan_prune_empty(t);
  if (last_to_remove < 0) return 0;
  // pruned_states_ keeps the whole camState (msckf.h:714; read by asl_msckf.cpp:409-424): poses come back once, here
  const int num = (int)t.cams.size();
  std::vector<double> poses((size_t)num * 7);
  int rc = B->get_cams_known(b, poses.data(), num);
  if (rc) return rc;
  std::vector<Retirement> ret(1);
  retire_plan_leading(t, poses.data(), last_to_remove, ret[0]);
  return prune_retired_range(B, b, ret);
}

// MSCKF::pruneRedundantStates, msckf.h:453-682: keyframe selection and observation surgery on the host (host_lists.h),
// the triangulation of not-yet-initialized features and the second measurement update on the device.
int host_prune_redundant(BatchCore* B, int b) {
  HostTraj& t = B->traj[b];
  if (!t.initialized) return fail(-EINVAL, "trajectory not initialized");
  if (t.cams.size() < 20) return 0;                                           // :455
  const int n = (int)t.cams.size();
  std::vector<double> poses((size_t)n * 7);
  int rc = resolve_map(B, b);          // this call appends to map_ (:528) and reuses the device work-list
  if (rc) return rc;
  rc = B->get_cams_known(b, poses.data(), n);
  if (rc) return rc;
  RedundantPlan plan;
  WorkList wl;
  // ---- first loop :466-534
  if (redundant_select(t, poses.data(), B->f_cap, plan, wl)) return fail(-E2BIG, "more candidate features than f_cap");
  if (plan.rm.empty()) return 0;
  if (!wl.M.empty()) {
    rc = set_tracks(B, b, wl);
    if (rc) return rc;
    std::vector<int> status(B->f_cap); std::vector<double> pf(3 * (size_t)B->f_cap);
    rc = B->feature_only_range(b, 1, status.data(), pf.data(), true);
    if (rc) return rc;
    redundant_apply_candidates(t, plan, status.data(), pf.data());
  }
  // ---- second loop :545-607
  std::vector<double> pfin(3 * (size_t)B->f_cap);
  if (redundant_second_update(t, plan, B->f_cap, wl, pfin.data())) return fail(-E2BIG, "more features than f_cap");
  if (!wl.M.empty()) {
    rc = set_tracks(B, b, wl);
    if (rc) return rc;
    rc = B->set_given_range(b, 1, pfin.data());
    if (rc) return rc;
    rc = B->marginalize(b, 1, 1);
    if (rc) return rc;
  }
  redundant_finish(t, plan);
  // ---- prune the removed camera states :616-681, poses as corrected by the second update (msckf.h:614 precedes :631)
  rc = B->get_cams_known(b, poses.data(), n);
  if (rc) return rc;
  std::vector<Retirement> ret(1);
  retire_plan_ids(t, poses.data(), plan.rm, ret[0]);
  return prune_retired_range(B, b, ret);
}

int host_finish(BatchCore* B, int b) {
  HostTraj& t = B->traj[b];
  // D6: the reference appends to the stale feature_tracks_to_residualize_ of the previous update() (cleared only
  // at msckf.h:218), whose positional indices and pose copies are invalid once states were corrected/pruned;
  // the stale list is dropped here (oracle/msckf_oracle.hpp does the same).
  t.to_resid.clear();
  for (size_t i = 0; i < t.tracked_ids.size(); i++) {
    TrackToResid r;
    remove_tracked_feature(t, t.tracked_ids[i], r.slots);
    if (r.slots.size() >= (size_t)t.min_track_length) {
      for (auto& tr : t.tracks) if (tr.id == t.tracked_ids[i]) { r.id = tr.id; r.obs = tr.obs; break; }
      t.to_resid.push_back(r);
    }
  }
  return host_marginalize(B, b);
}

// -------------------------------------------------------------------------------------------------
// One image of the ASL runner's loop (asl_msckf.cpp:269-294) for trajectories b0 .. b0 + nb - 1 of a batch IN LOCKSTEP:
//   augmentState -> update -> addFeatures -> marginalize -> [pruneRedundantStates] -> [pruneEmptyStates]
// The bookkeeping of every trajectory runs on the host through the same functions as the per-filter entries above --
// host_update, host_add_features, and the steps of host_lists.h: build_worklist, append_map, redundant_select /
// _apply_candidates / _second_update / _finish, plan_prune_empty, retire_plan_* / retire_commit --, the device work of a stage
// goes out as ONE launch sequence over the range (the kernels index trajectories; a run of trajectories with nothing to do is
// skipped) and what a stage needs back -- poses for findRedundantCamStates, triangulated points of not-yet-initialized
// features, poses of the states about to be pruned -- comes back in one read and one wait per stage for the whole range,
// instead of one per filter.
// Same arithmetic per trajectory as the per-filter calls (tests/test_gpu_parity.py: bit for bit).
// -------------------------------------------------------------------------------------------------
// the bookkeeping of the trajectories of a range is independent: spread over host threads (created per call: tens of microseconds
// against milliseconds of list surgery at the benchmark's 200 tracks per image); fn(i) returns 0 or an error code.  fail() leaves
// its text with the thread it ran on: the first failure's code AND text come back to the caller's thread
template <class Fn> static int parallel_for(int n, Fn fn) {
  unsigned hw = std::thread::hardware_concurrency();
  int nt = (int)std::min<unsigned>(hw ? hw : 1u, 32u);
  if (const char* e = getenv("MSCKF_HIP_HOST_THREADS")) nt = std::max(1, atoi(e));
  nt = std::min(nt, n);
  if (nt <= 1) { for (int i = 0; i < n; ++i) { const int rc = fn(i); if (rc) return rc; } return 0; }
  std::atomic<int> next(0), err(0);
  std::string msg;   // written by the one thread that sets err, read after the join
  auto work = [&]() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= n || err.load()) return;
      const int rc = fn(i);
      int none = 0;
      if (rc && err.compare_exchange_strong(none, rc)) msg = g_err;
    }
  };
  std::vector<std::thread> th;
  for (int k = 1; k < nt; ++k) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
  if (err.load()) g_err = msg;
  return err.load();
}
template <class Fn> static int for_runs(const std::vector<char>& on, int b0, Fn fn) {
  const int nb = (int)on.size();
  for (int i = 0; i < nb;) {
    if (!on[i]) { ++i; continue; }
    int j = i;
    while (j < nb && on[j]) ++j;
    const int rc = fn(b0 + i, j - i);
    if (rc) return rc;
    i = j;
  }
  return 0;
}
static bool any_of(const std::vector<char>& on) { for (char c : on) if (c) return true; return false; }

int host_image_cycle(BatchCore* B, int b0, int nb, const int* state_ids, const double* times,
                     const double* upd_meas, const uint64_t* upd_ids, const int* upd_n,
                     const double* new_meas, const uint64_t* new_ids, const int* new_n, int flags) {
  if (b0 < 0 || nb <= 0 || b0 + nb > B->B) return fail(-EINVAL, "trajectory range out of bounds");
  const int n_cap = B->n_cap, f_cap = B->f_cap;
  for (int i = 0; i < nb; ++i) {
    const HostTraj& t = B->traj[b0 + i];
    if (!t.initialized) return fail(-EINVAL, "trajectory not initialized");
    if ((int)t.cams.size() >= n_cap) return fail(-EOVERFLOW, "camera-state capacity n_cap exceeded");
  }
  static const bool tim = getenv("MSCKF_HIP_CYCLE_TIMERS") != nullptr;
  double tph[8] = {0}; auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double tl = now();
  auto tick = [&](int k) { if (tim) { const double t2 = now(); tph[k] += t2 - tl; tl = t2; } };
  // ---- augmentState :148-212
  int rc = B->augment(b0, nb);
  if (rc) return rc;
  for (int i = 0; i < nb; ++i) begin_image(B->traj[b0 + i], state_ids[i], times ? times[i] : 0.0);
  tick(0);
  // ---- update :215-300, addFeatures :302-332 (host)
  {
    std::vector<size_t> ou(nb + 1, 0), on(nb + 1, 0);
    for (int i = 0; i < nb; ++i) { ou[i + 1] = ou[i] + (size_t)upd_n[i]; on[i + 1] = on[i] + (size_t)new_n[i]; }
    rc = parallel_for(nb, [&](int i) {
      int r2 = host_update(B, b0 + i, upd_meas + 2 * ou[i], upd_ids + ou[i], upd_n[i]);
      if (!r2) r2 = host_add_features(B, b0 + i, new_meas + 2 * on[i], new_ids + on[i], new_n[i]);
      return r2;
    });
    if (rc) return rc;
  }
  tick(1);
  // ---- marginalize :336-449
  {
    std::vector<char> has(nb, 0);
    std::vector<WorkList> wl(nb);
    parallel_for(nb, [&](int i) { build_worklist(B->traj[b0 + i].to_resid, wl[i]); return 0; });
    tick(2);
    rc = B->set_tracks_range(b0, nb, wl);
    if (rc) return rc;
    for (int i = 0; i < nb; ++i) {
      const int F = (int)wl[i].M.size();
      if (!F) { rc = B->clear_stats(b0 + i); if (rc) return rc; }
      has[i] = F > 0;
      B->traj[b0 + i].map_pending = F;
    }
    tick(3);
    rc = for_runs(has, b0, [&](int s0, int n) { return B->marginalize(s0, n); });
    if (rc) return rc;
  }
  tick(4);
  // ---- pruneRedundantStates :453-682
  if (flags & 1) {
    std::vector<char> act(nb, 0);
    for (int i = 0; i < nb; ++i) act[i] = B->traj[b0 + i].cams.size() >= 20;   // :455
    if (any_of(act)) {
      std::vector<int> status((size_t)nb * f_cap);
      std::vector<double> pf((size_t)nb * f_cap * 3), poses((size_t)nb * n_cap * 7);
      // what resolve_map() fetches per filter: the points of the marginalize just launched (the work-lists are reused below)
      rc = B->feature_only_range(b0, nb, status.data(), pf.data(), false);
      if (rc) return rc;
      rc = B->cams_range(b0, nb, poses.data());
      if (rc) return rc;
      std::vector<RedundantPlan> plan(nb);    // (a trajectory that is not active keeps an empty plan: every step skips it)
      std::vector<char> has_cand(nb, 0), has_upd(nb, 0);
      WorkList wl;
      // first loop :466-534
      for (int i = 0; i < nb; ++i) {
        if (!act[i]) continue;
        HostTraj& t = B->traj[b0 + i];
        append_map(t, &status[(size_t)i * f_cap], &pf[(size_t)i * f_cap * 3], t.map_pending);
        t.map_pending = 0;
        if (redundant_select(t, &poses[(size_t)i * n_cap * 7], f_cap, plan[i], wl)) return fail(-E2BIG, "more candidate features than f_cap");
        if (wl.M.empty()) continue;
        rc = set_tracks(B, b0 + i, wl);
        if (rc) return rc;
        has_cand[i] = 1;
      }
      // checkMotion + initializePosition of the not-yet-initialized features, every trajectory's in one launch per run
      if (any_of(has_cand)) {
        // (feature_only_range launches over the runs; the read-back covers the whole range once)
        rc = for_runs(has_cand, b0, [&](int s0, int n) { return B->feature_only_range(s0, n, status.data() + (size_t)(s0 - b0) * f_cap, pf.data() + (size_t)(s0 - b0) * f_cap * 3, true); });
        if (rc) return rc;
        for (int i = 0; i < nb; ++i)
          if (has_cand[i]) redundant_apply_candidates(B->traj[b0 + i], plan[i], &status[(size_t)i * f_cap], &pf[(size_t)i * f_cap * 3]);
      }
      // second loop :545-607: the work-lists of the second update
      std::vector<double> pfin((size_t)nb * f_cap * 3, 0.0);
      for (int i = 0; i < nb; ++i) {
        if (redundant_second_update(B->traj[b0 + i], plan[i], f_cap, wl, &pfin[(size_t)i * f_cap * 3])) return fail(-E2BIG, "more features than f_cap");
        if (wl.M.empty()) continue;
        rc = set_tracks(B, b0 + i, wl);
        if (rc) return rc;
        has_upd[i] = 1;
      }
      if (any_of(has_upd)) {
        rc = B->set_given_range(b0, nb, pfin.data());
        if (rc) return rc;
        rc = for_runs(has_upd, b0, [&](int s0, int n) { return B->marginalize(s0, n, 1); });
        if (rc) return rc;
      }
      bool anyrm = false;
      for (int i = 0; i < nb; ++i) { redundant_finish(B->traj[b0 + i], plan[i]); anyrm |= !plan[i].rm.empty(); }
      // prune the removed camera states :616-681 (poses as corrected by the second update: :614 precedes :631)
      if (anyrm) {
        rc = B->cams_range(b0, nb, poses.data());
        if (rc) return rc;
        std::vector<Retirement> ret(nb);
        for (int i = 0; i < nb; ++i) retire_plan_ids(B->traj[b0 + i], &poses[(size_t)i * n_cap * 7], plan[i].rm, ret[i]);
        rc = prune_retired_range(B, b0, ret);
        if (rc) return rc;
      }
    }
  }
  tick(5);
  // ---- pruneEmptyStates :685-761
  if (flags & 2) {
    std::vector<int> last(nb, -1);
    bool any = false;
    for (int i = 0; i < nb; ++i) { last[i] = plan_prune_empty(B->traj[b0 + i]); any |= last[i] >= 0; }
    if (any) {
      std::vector<double> poses((size_t)nb * n_cap * 7);
      rc = B->cams_range(b0, nb, poses.data());    // pruned_states_ keeps the whole camState (msckf.h:714)
      if (rc) return rc;
      std::vector<Retirement> ret(nb);
      for (int i = 0; i < nb; ++i) retire_plan_leading(B->traj[b0 + i], &poses[(size_t)i * n_cap * 7], last[i], ret[i]);
      rc = prune_retired_range(B, b0, ret);
      if (rc) return rc;
    }
  }
  tick(6);
  if (tim) fprintf(stderr, "cycle nb=%d ms: augment %.2f update+add %.2f lists %.2f upload %.2f launch %.2f redundant %.2f empty %.2f\n", nb, tph[0], tph[1], tph[2], tph[3], tph[4], tph[5], tph[6]);
  return 0;
}

BatchCore* H(msckf_hip_handle h) { return reinterpret_cast<BatchCore*>(h); }
}  // namespace

#ifdef MSCKF_ABLATE
namespace msckf { void qr_debug_set(int idx, int val); void feat_debug_set(int val); void featp_cycles_read(unsigned long long* out8, int reset); extern int g_gram_dbg; void chol_cycles_read(unsigned long long* out16, int reset); void chol_sub_read(unsigned long long* out32, int reset); void chol_debug_set(int v); void prop_cycles_read(unsigned long long* out8, int reset); void gram_cycles_read(unsigned long long* out40, int reset); void gemm_cycles_read(unsigned long long* out16, int reset); void gemm_trace_read(unsigned long long* out); void us_cycles_read(unsigned long long* out16, int reset); }
#endif

extern "C" {

#ifdef MSCKF_ABLATE
// ablation knobs of the -DMSCKF_ABLATE build (scripts/*_ablate.py); the product library does not export this symbol
void msckf_hip_debug_set(int idx, int val) {
  if (idx == 200) { msckf::feat_debug_set(val); return; }
  if (idx == 300) { msckf::g_gram_dbg = val; return; }
  if (idx == 400) { msckf::chol_debug_set(val); return; }
  msckf::qr_debug_set(idx, val);
}
void msckf_hip_debug_chol_cycles(unsigned long long* out16, int reset) { msckf::chol_cycles_read(out16, reset); }
void msckf_hip_debug_chol_sub(unsigned long long* out32, int reset) { msckf::chol_sub_read(out32, reset); }
void msckf_hip_debug_prop_cycles(unsigned long long* out8, int reset) { msckf::prop_cycles_read(out8, reset); }
void msckf_hip_debug_featp_cycles(unsigned long long* out8, int reset) { msckf::featp_cycles_read(out8, reset); }
void msckf_hip_debug_gram_cycles(unsigned long long* out40, int reset) { msckf::gram_cycles_read(out40, reset); }
void msckf_hip_debug_gemm_cycles(unsigned long long* out16, int reset) { msckf::gemm_cycles_read(out16, reset); }
void msckf_hip_debug_gemm_trace(unsigned long long* out) { msckf::gemm_trace_read(out); }
void msckf_hip_debug_us_cycles(unsigned long long* out16, int reset) { msckf::us_cycles_read(out16, reset); }
#endif

const char* msckf_hip_last_error(void) { return g_err.c_str(); }

int msckf_hip_create(int B, int n_cap, int f_cap, int m_cap, int dtype, int device, msckf_hip_handle* out) {
  if (!out) return fail(-EINVAL, "null out pointer");
  *out = nullptr;
  if (B <= 0 || n_cap <= 0 || f_cap <= 0 || m_cap < 2 || m_cap > 64) return fail(-EINVAL, "bad capacities (need B,n_cap,f_cap > 0 and 2 <= m_cap <= 64)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(-ENODEV, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(-ENODEV, "HIP device index out of range");
  if (dtype != MSCKF_HIP_F32 && dtype != MSCKF_HIP_F64 && dtype != MSCKF_HIP_F16H_F32P) return fail(-EINVAL, "dtype must be MSCKF_HIP_F32, MSCKF_HIP_F64 or MSCKF_HIP_F16H_F32P");
  BatchCore* b = dtype == MSCKF_HIP_F64 ? static_cast<BatchCore*>(new Batch<double>()) : new Batch<float>();
  b->B = B; b->n_cap = n_cap; b->f_cap = f_cap; b->m_cap = m_cap; b->dtype = dtype; b->device = device;
  b->h16 = dtype == MSCKF_HIP_F16H_F32P; b->esz = dtype == MSCKF_HIP_F64 ? sizeof(double) : sizeof(float);
  const int rc = b->create();
  if (rc) { delete b; return rc; }
  *out = reinterpret_cast<msckf_hip_handle>(b);
  return 0;
}
int msckf_hip_destroy(msckf_hip_handle h) { delete H(h); return 0; }

int msckf_hip_initialize(msckf_hip_handle h, int b, const double* cam12, const double* noise29, const double* params8, const double* imu29) {
  return H(h)->init_core(b, cam12, noise29, nullptr, nullptr, params8, imu29);
}
int msckf_hip_initialize_full(msckf_hip_handle h, int b, const double* cam12, const double* uv2, const double* Q144, const double* P0_225,
                              const double* params8, const double* imu29) {
  if (!h || !cam12 || !uv2 || !Q144 || !P0_225 || !params8 || !imu29) return fail(-EINVAL, "null argument");
  return H(h)->init_full(b, cam12, uv2, Q144, P0_225, params8, imu29);
}
int msckf_hip_propagate(msckf_hip_handle h, int b, const double* readings7, int K) { StageRange r("imu_prop"); return H(h)->propagate(b, 1, readings7, K, true); }
int msckf_hip_augment_state(msckf_hip_handle h, int b, int state_id, double time) {
  BatchCore* B = H(h);
  if (b < 0 || b >= B->B) return fail(-EINVAL, "trajectory index out of range");
  if ((int)B->traj[b].cams.size() >= B->n_cap) return fail(-EOVERFLOW, "camera-state capacity n_cap exceeded");
  StageRange r("msckf_augment_state");
  int rc = B->augment(b, 1);
  if (rc) return rc;
  begin_image(B->traj[b], state_id, time);
  return 0;
}
int msckf_hip_update(msckf_hip_handle h, int b, const double* meas2, const uint64_t* ids, int n) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  StageRange r("msckf_update");
  return host_update(H(h), b, meas2, ids, n);
}
int msckf_hip_add_features(msckf_hip_handle h, int b, const double* meas2, const uint64_t* ids, int n) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  StageRange r("msckf_add_features");
  return host_add_features(H(h), b, meas2, ids, n);
}
int msckf_hip_marginalize(msckf_hip_handle h, int b) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  StageRange r("msckf_marginalize");
  return host_marginalize(H(h), b);
}
int msckf_hip_prune_empty_states(msckf_hip_handle h, int b) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  StageRange r("msckf_prune_empty_states");
  return host_prune_empty(H(h), b);
}
int msckf_hip_image_cycle_range(msckf_hip_handle h, int b0, int nb, const int* state_ids, const double* times,
                                const double* upd_meas2, const uint64_t* upd_ids, const int* upd_n,
                                const double* new_meas2, const uint64_t* new_ids, const int* new_n, int flags) {
  if (!h) return fail(-EINVAL, "null handle");
  if (!state_ids || !upd_n || !new_n) return fail(-EINVAL, "null argument");
  StageRange r("msckf_image_cycle_range");
  return host_image_cycle(H(h), b0, nb, state_ids, times, upd_meas2, upd_ids, upd_n, new_meas2, new_ids, new_n, flags);
}
int msckf_hip_prune_redundant_states(msckf_hip_handle h, int b) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  StageRange r("msckf_prune_redundant");
  return host_prune_redundant(H(h), b);
}
int msckf_hip_finish(msckf_hip_handle h, int b) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  return host_finish(H(h), b);
}
int msckf_hip_get_num_cam_states(msckf_hip_handle h, int b) {   // cam_states_.size(): the host keeps the count (augment, prune, drop and run_frames all update it)
  return H(h)->ncam_host(b);
}
int msckf_hip_get_imu_state(msckf_hip_handle h, int b, double* imu29) { return H(h)->get_imu(b, imu29); }
int msckf_hip_get_cam_states(msckf_hip_handle h, int b, double* cam7, int* state_ids, int cap) {
  int n = 0;
  int rc = H(h)->get_cams(b, cam7, cap, &n);
  if (rc) return rc;
  if (state_ids) {
    const auto& cams = H(h)->traj[b].cams;
    for (int i = 0; i < n; ++i) state_ids[i] = i < (int)cams.size() ? cams[i].state_id : -1;
  }
  return n;
}
int msckf_hip_get_map(msckf_hip_handle h, int b, double* xyz, int cap) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  { const int rc = resolve_map(H(h), b); if (rc) return rc; }
  const auto& m = H(h)->traj[b].map;
  const int n = (int)m.size() / 3;
  if (n > cap) return fail(-E2BIG, "output buffer too small");
  std::copy(m.begin(), m.end(), xyz);
  return n;
}
static std::vector<PrunedState> sorted_pruned(const HostTraj& t) {
  std::vector<PrunedState> p = t.pruned;
  std::stable_sort(p.begin(), p.end(), [](const PrunedState& a, const PrunedState& c) { return a.state_id < c.state_id; });   // msckf.h:842-846
  return p;
}
int msckf_hip_get_pruned_state_ids(msckf_hip_handle h, int b, int* ids, int cap) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  const std::vector<PrunedState> p = sorted_pruned(H(h)->traj[b]);
  if ((int)p.size() > cap) return fail(-E2BIG, "output buffer too small");
  for (size_t i = 0; i < p.size(); ++i) ids[i] = p[i].state_id;
  return (int)p.size();
}
int msckf_hip_get_pruned_states(msckf_hip_handle h, int b, double* cam7, double* time, int* state_ids, int* last_correlated_ids, int cap) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  const std::vector<PrunedState> p = sorted_pruned(H(h)->traj[b]);
  if ((int)p.size() > cap) return fail(-E2BIG, "output buffer too small");
  for (size_t i = 0; i < p.size(); ++i) {
    if (cam7) std::copy(p[i].pose, p[i].pose + 7, cam7 + 7 * i);
    if (time) time[i] = p[i].time;
    if (state_ids) state_ids[i] = p[i].state_id;
    if (last_correlated_ids) last_correlated_ids[i] = p[i].last_correlated_id;
  }
  return (int)p.size();
}
int msckf_hip_get_cam_meta(msckf_hip_handle h, int b, double* time, int* n_tracked, int* last_correlated_ids, int cap) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  const auto& cams = H(h)->traj[b].cams;
  if ((int)cams.size() > cap) return fail(-E2BIG, "output buffer too small");
  for (size_t i = 0; i < cams.size(); ++i) {
    if (time) time[i] = cams[i].time;
    if (n_tracked) n_tracked[i] = (int)cams[i].tracked.size();
    if (last_correlated_ids) last_correlated_ids[i] = cams[i].last_correlated_id;
  }
  return (int)cams.size();
}
int msckf_hip_get_tracked_feature_ids(msckf_hip_handle h, int b, int cam_index, uint64_t* ids, int cap) {
  if (b < 0 || b >= H(h)->B) return fail(-EINVAL, "trajectory index out of range");
  const auto& cams = H(h)->traj[b].cams;
  if (cam_index < 0 || cam_index >= (int)cams.size()) return fail(-EINVAL, "camera index out of range");
  const auto& tr = cams[(size_t)cam_index].tracked;
  if ((int)tr.size() > cap) return fail(-E2BIG, "output buffer too small");
  std::copy(tr.begin(), tr.end(), ids);
  return (int)tr.size();
}
int msckf_hip_get_covariance(msckf_hip_handle h, int b, double* P, int ld) { return H(h)->get_cov(b, P, ld); }
int msckf_hip_set_covariance(msckf_hip_handle h, int b, const double* P, int D) { return H(h)->set_cov(b, P, D); }
int msckf_hip_set_imu_state(msckf_hip_handle h, int b, const double* imu29) { return H(h)->set_imu(b, imu29); }
int msckf_hip_set_cam_pose(msckf_hip_handle h, int b, int slot, const double* cam7) { return H(h)->set_cam(b, slot, cam7); }
int msckf_hip_get_num_residualized(msckf_hip_handle h, int b, long long* n) { return H(h)->get_nres(b, n); }
int msckf_hip_set_num_residualized(msckf_hip_handle h, int b, long long n) { return H(h)->set_nres(b, n); }
int msckf_hip_last_stats(msckf_hip_handle h, int b, int* out7) { return H(h)->stats(b, out7); }
int msckf_hip_clear_error_flags(msckf_hip_handle h, int b) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->clear_errors(b); }
int msckf_hip_last_tracks(msckf_hip_handle h, int b, double* out8, int cap) { return H(h)->track_info(b, out8, cap); }
int msckf_hip_last_deltax(msckf_hip_handle h, int b, double* dx, int cap) { return H(h)->deltax(b, dx, cap); }
int msckf_hip_last_track_blocks(msckf_hip_handle h, int b, int* first, double* Hx, double* rw, double* Bh, int cap) { return H(h)->track_blocks(b, first, Hx, rw, Bh, cap); }

int msckf_hip_set_tracks(msckf_hip_handle h, int b, int F, const int* M, const int* slots, const double* obs2) { return H(h)->set_tracks(b, F, M, slots, obs2); }
int msckf_hip_propagate_range(msckf_hip_handle h, int b0, int nb, const double* readings7, int K) { return H(h)->propagate(b0, nb, readings7, K); }
int msckf_hip_propagate_range_counts(msckf_hip_handle h, int b0, int nb, const double* readings7, const int* K) {
  if (!h || (nb > 0 && !K)) return fail(-EINVAL, "null argument");
  return H(h)->propagate_counts(b0, nb, readings7, K);
}
int msckf_hip_augment_range(msckf_hip_handle h, int b0, int nb) { return H(h)->augment(b0, nb); }
int msckf_hip_marginalize_range(msckf_hip_handle h, int b0, int nb) { return H(h)->marginalize(b0, nb, 0); }
int msckf_hip_drop_oldest_range(msckf_hip_handle h, int b0, int nb, int n_drop) { return H(h)->drop_oldest(b0, nb, n_drop); }

int msckf_hip_scenario_alloc(msckf_hip_handle h, int n_frames, int K) { return H(h)->scen_alloc(n_frames, K); }
int msckf_hip_scenario_set(msckf_hip_handle h, int frame, int b, const double* readings7, int F, const int* M, const int* slots, const double* obs2, int n_drop) {
  if (!h) return fail(-EINVAL, "null handle");
  return H(h)->scen_set(frame, b, readings7, H(h)->sc.lay.K, F, M, slots, obs2, n_drop, 0);
}
static_assert(MSCKF_HIP_CELL_SKIP == CELL_SKIP, "host_lists.h states the cell rule with the header's flag bit");
int msckf_hip_scenario_set_cell(msckf_hip_handle h, int frame, int b, const double* readings7, int k, int F, const int* M, const int* slots, const double* obs2, int n_drop, int flags) {
  if (!h) return fail(-EINVAL, "null handle");
  return H(h)->scen_set(frame, b, readings7, k, F, M, slots, obs2, n_drop, flags);
}
int msckf_hip_scenario_commit(msckf_hip_handle h) { return H(h)->scen_commit(); }
int msckf_hip_run_frames(msckf_hip_handle h, int f0, int f1) { return H(h)->run_frames(f0, f1); }
int msckf_hip_run_frames_streamed(msckf_hip_handle h, int f0, int f1) { return H(h)->run_frames_streamed(f0, f1); }
int msckf_hip_replay_alloc(msckf_hip_handle h, int n_seq, int n_frames, int K) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->replay_alloc(n_seq, n_frames, K); }
int msckf_hip_replay_set_cell(msckf_hip_handle h, int frame, int seq, const double* readings7, int k, int F, const int* M, const int* slots, const double* obs2, int n_drop, int flags) {
  if (!h) return fail(-EINVAL, "null handle");
  return H(h)->replay_set_cell(frame, seq, readings7, k, F, M, slots, obs2, n_drop, flags);
}
int msckf_hip_replay_assign(msckf_hip_handle h, const int* seq_of, const uint64_t* seed, const double* sigma4) { if (!h || !seq_of || !seed || !sigma4) return fail(-EINVAL, "null argument"); return H(h)->replay_assign(seq_of, seed, sigma4); }
int msckf_hip_replay_assign_q(msckf_hip_handle h, const int* seq_of, const uint64_t* seed, const double* Q144, const double* scale, const double* sigma_uv) {
  if (!h || !seq_of || !seed || !Q144 || !scale || !sigma_uv) return fail(-EINVAL, "null argument");
  return H(h)->replay_assign_q(seq_of, seed, Q144, scale, sigma_uv);
}
int msckf_hip_replay_walk(msckf_hip_handle h, int f0, int f1, int b0, int nb, double* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->replay_walk(f0, f1, b0, nb, out); }
int msckf_hip_replay_commit(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->replay_commit(); }
int msckf_hip_run_frames_replay(msckf_hip_handle h, int f0, int f1) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->run_frames_replay(f0, f1); }
int msckf_hip_replay_expand(msckf_hip_handle h, int frame, int b, double* rd, double* obs2, int cap_entries) { if (!h || !rd || !obs2) return fail(-EINVAL, "null argument"); return H(h)->replay_expand(frame, b, rd, obs2, nullptr, nullptr, cap_entries); }
int msckf_hip_replay_expand_ints(msckf_hip_handle h, int frame, int b, int* ints, int* slots, int cap_entries) { if (!h || !ints || !slots) return fail(-EINVAL, "null argument"); return H(h)->replay_expand(frame, b, nullptr, nullptr, ints, slots, cap_entries); }
int msckf_hip_replay_set_faults(msckf_hip_handle h, const double* fault4) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->replay_set_faults(fault4); }
int msckf_hip_replay_expand_faults(msckf_hip_handle h, int frame, int b, int* code, int cap_entries) { if (!h || !code) return fail(-EINVAL, "null argument"); return H(h)->replay_expand(frame, b, nullptr, nullptr, nullptr, nullptr, cap_entries, code); }
int msckf_hip_replay_set_timing(msckf_hip_handle h, const double* timing4) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->replay_set_timing(timing4); }
int msckf_hip_replay_image_table(msckf_hip_handle h, int seq, double* time, int* frame_of, int* base) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->replay_image_table(seq, time, frame_of, base); }
int msckf_hip_replay_expand_timing(msckf_hip_handle h, int frame, int b, double* delta, int cap_entries) { if (!h || !delta) return fail(-EINVAL, "null argument"); return H(h)->replay_expand(frame, b, nullptr, nullptr, nullptr, nullptr, cap_entries, nullptr, delta); }
int msckf_hip_replay_set_imu_calib(msckf_hip_handle h, const double* imucal) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->replay_set_imu_calib(imucal); }
int msckf_hip_replay_set_cam_calib(msckf_hip_handle h, const double* camcal) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->replay_set_cam_calib(camcal); }
int msckf_hip_replay_expand_calib(msckf_hip_handle h, int frame, int b, double* rd_cal, int* clip, double* obs_cal, int cap_entries) {
  if (!h) return fail(-EINVAL, "null handle");
  const BatchCore::CalibOut co{rd_cal, clip, obs_cal};
  return H(h)->replay_expand(frame, b, nullptr, nullptr, nullptr, nullptr, cap_entries, nullptr, nullptr, &co);
}
int msckf_hip_replay_calib_counts(msckf_hip_handle h, int f0, int f1, long long* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->replay_calib_counts(f0, f1, out); }
int msckf_hip_replay_fault_counts(msckf_hip_handle h, int f0, int f1, long long* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->replay_fault_counts(f0, f1, out); }
int msckf_hip_replay_imu_sums(msckf_hip_handle h, int f0, int f1, double* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->replay_imu_sums(f0, f1, out); }
// ---- the track compiler (track_compile.h): host code alone, no handle, no device
int msckf_hip_compile_create(int max_cam_states, int min_track_length, int max_track_length, msckf_hip_compiler* out) {
  if (!out) return fail(-EINVAL, "null out pointer");
  *out = nullptr;
  if (const msckf_compile::Refusal r = msckf_compile::Compiler::create_refusal(max_cam_states, min_track_length, max_track_length); r.code) return fail(r.code, r.why);
  *out = reinterpret_cast<msckf_hip_compiler>(new msckf_compile::Compiler(max_cam_states, min_track_length, max_track_length));
  return 0;
}
int msckf_hip_compile_destroy(msckf_hip_compiler c) { delete reinterpret_cast<msckf_compile::Compiler*>(c); return 0; }
int msckf_hip_compile_image(msckf_hip_compiler c, const double* upd_meas2, const uint64_t* upd_ids, int upd_n, const double* new_meas2, const uint64_t* new_ids, int new_n, int* out5) {
  if (!c || !out5) return fail(-EINVAL, "null argument");
  msckf_compile::ImageSummary s{0, 0, 0, 0, 0};
  if (const msckf_compile::Refusal r = reinterpret_cast<msckf_compile::Compiler*>(c)->image(upd_meas2, upd_ids, upd_n, new_meas2, new_ids, new_n, s); r.code) return fail(r.code, r.why);
  out5[0] = s.F; out5[1] = s.entries; out5[2] = s.n_drop; out5[3] = s.window; out5[4] = s.live;
  return 0;
}
int msckf_hip_compile_cell(msckf_hip_compiler c, int* M, int* slots, double* obs2, uint64_t* ids, int cap_tracks, int cap_entries) {
  if (!c) return fail(-EINVAL, "null argument");
  const msckf_compile::Compiler& k = *reinterpret_cast<const msckf_compile::Compiler*>(c);
  if (const msckf_compile::Refusal r = k.cell_refusal(cap_tracks, cap_entries); r.code) return fail(r.code, r.why);
  if ((!k.wl.M.empty() && (!M || !ids)) || (!k.wl.slots.empty() && (!slots || !obs2))) return fail(-EINVAL, "null output with a work-list to store");
  std::copy(k.wl.M.begin(), k.wl.M.end(), M);
  std::copy(k.ids.begin(), k.ids.end(), ids);
  std::copy(k.wl.slots.begin(), k.wl.slots.end(), slots);
  std::copy(k.wl.obs.begin(), k.wl.obs.end(), obs2);
  return (int)k.wl.M.size();
}
int msckf_hip_map_log_fault_metrics(msckf_hip_handle h, int q0, int q1, int f0, double* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->map_log_fault_metrics(q0, q1, f0, out); }
int msckf_hip_sync(msckf_hip_handle h) { return H(h)->sync(); }
int msckf_hip_profile_enable(msckf_hip_handle h, int on) { return H(h)->prof_enable(on); }
int msckf_hip_profile_read(msckf_hip_handle h, double* ms7, int* count7) { return H(h)->prof_read(ms7, count7, 8); }
int msckf_hip_profile_read_ex(msckf_hip_handle h, double* ms, int* count, int cap) { if (!h || !ms || !count || cap < 8) return fail(-EINVAL, "bad arguments"); for (int s = NSTAGE; s < cap; ++s) { ms[s] = 0; count[s] = 0; } return H(h)->prof_read(ms, count, cap); }
int msckf_hip_profile_event_overhead(msckf_hip_handle h, double* ms) { if (!h || !ms) return fail(-EINVAL, "null argument"); return H(h)->prof_event_overhead(ms); }
int msckf_hip_set_host_affinity(msckf_hip_handle h, const int* cpus, int n) { if (!h || (n > 0 && !cpus)) return fail(-EINVAL, "null argument"); return H(h)->set_host_affinity(cpus, n); }
int msckf_hip_set_streams(msckf_hip_handle h, int n) { return H(h)->set_streams(n); }
int msckf_hip_get_effective_streams(msckf_hip_handle h, int streamed, int* out) { if (!h || !out) return fail(-EINVAL, "null argument"); *out = H(h)->n_slices(streamed != 0); return 0; }
int msckf_hip_parse_hw_queues(const char* text) { return msckf::slices::parse_hw_queue_budget(text); }
int msckf_hip_set_hw_queues(msckf_hip_handle h, int n) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_hw_queues(n); }
int msckf_hip_set_slices_exact(msckf_hip_handle h, int on) { if (!h) return fail(-EINVAL, "null handle"); H(h)->slices_exact = on != 0; return 0; }
int msckf_hip_scenario_pin(msckf_hip_handle h, int f0, int f1) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->scen_pin(f0, f1); }
int msckf_hip_set_upload_ring(msckf_hip_handle h, int depth, int mode) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_upload_ring(depth, mode); }
int msckf_hip_set_feature_overlap(msckf_hip_handle h, int on) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_feature_overlap(on); }
int msckf_hip_set_frame_order(msckf_hip_handle h, int order) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_frame_order(order); }
int msckf_hip_get_frame_order_count(msckf_hip_handle h, long long* count) {
  if (!h || !count) return fail(-EINVAL, "null handle or null count");
  *count = H(h)->n_feature_first.load(std::memory_order_relaxed);
  return 0;
}
int msckf_hip_set_frame_order_chol(msckf_hip_handle h, int on) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_frame_order_chol(on); }
int msckf_hip_get_frame_order_chol_count(msckf_hip_handle h, long long* count) {
  if (!h || !count) return fail(-EINVAL, "null handle or null count");
  *count = H(h)->n_in_cholesky.load(std::memory_order_relaxed);
  return 0;
}
int msckf_hip_set_covariance_update(msckf_hip_handle h, int form) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_cov_update(form); }
int msckf_hip_set_compression(msckf_hip_handle h, int route) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_compression(route); }
int msckf_hip_set_gate_early_accept(msckf_hip_handle h, int on) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_gate_early(on); }
int msckf_hip_set_anisotropic_noise(msckf_hip_handle h, int mode, double tail_tol) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->set_aniso(mode, tail_tol); }
int msckf_hip_copy_state(msckf_hip_handle dst, msckf_hip_handle src) { if (!dst || !src) return fail(-EINVAL, "null handle"); return H(dst)->copy_from(H(src)); }
int msckf_hip_get_error_flags(msckf_hip_handle h, int b, int* flags) { if (!h || !flags) return fail(-EINVAL, "null argument"); return H(h)->error_flags(b, flags); }
int msckf_hip_frame_log_enable(msckf_hip_handle h, int capacity_frames) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->frame_log_enable(capacity_frames); }
int msckf_hip_frame_log_reset(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->frame_log_reset(); }
int msckf_hip_frame_log_count(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->frame_log_count(); }
int msckf_hip_frame_log_read(msckf_hip_handle h, int r0, int n, int b0, int nb, double* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->frame_log_read(r0, n, b0, nb, out); }
int msckf_hip_frame_log_metrics(msckf_hip_handle h, int r0, int r1, const double* gt_p, double* out) { if (!h || !gt_p || !out) return fail(-EINVAL, "null argument"); return H(h)->frame_log_metrics(r0, r1, gt_p, out); }
int msckf_hip_frame_log_metrics_ranges(msckf_hip_handle h, const int* r0, const int* r1, const double* gt_p, double* out) { if (!h || !r0 || !r1 || !gt_p || !out) return fail(-EINVAL, "null argument"); return H(h)->frame_log_metrics_ranges(r0, r1, gt_p, out); }
int msckf_hip_map_log_enable(msckf_hip_handle h, int capacity_per_trajectory) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->map_log_enable(capacity_per_trajectory); }
int msckf_hip_map_log_reset(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->map_log_reset(); }
int msckf_hip_map_log_frames(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->map_log_frames(); }
int msckf_hip_map_log_counts(msckf_hip_handle h, int b0, int nb, int* stored, int* found) { if (!h || !stored || !found) return fail(-EINVAL, "null argument"); return H(h)->map_log_counts(b0, nb, stored, found); }
int msckf_hip_map_log_read(msckf_hip_handle h, int b, int r0, int n, double* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->map_log_read(b, r0, n, out); }
int msckf_hip_map_log_metrics(msckf_hip_handle h, int q0, int q1, const double* gt_xyz, const int* gt_off, double* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->map_log_metrics(q0, q1, gt_xyz, gt_off, out); }
int msckf_hip_pruned_log_enable(msckf_hip_handle h, int capacity_per_trajectory) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->pruned_log_enable(capacity_per_trajectory); }
int msckf_hip_pruned_log_reset(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->pruned_log_reset(); }
int msckf_hip_pruned_log_frames(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->pruned_log_frames(); }
int msckf_hip_pruned_log_counts(msckf_hip_handle h, int b0, int nb, int* stored, int* found) { if (!h || !stored || !found) return fail(-EINVAL, "null argument"); return H(h)->pruned_log_counts(b0, nb, stored, found); }
int msckf_hip_pruned_log_read(msckf_hip_handle h, int b, int r0, int n, double* out, int* aug_ord) { if (!h || !out || !aug_ord) return fail(-EINVAL, "null argument"); return H(h)->pruned_log_read(b, r0, n, out, aug_ord); }
int msckf_hip_pruned_log_metrics(msckf_hip_handle h, int q0, int q1, const double* gt_pose, int n_ord, double* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->pruned_log_metrics(q0, q1, gt_pose, n_ord, out); }
int msckf_hip_truth_set(msckf_hip_handle h, int n_frames, int n_rows, const double* truth16, const int* row_of, int add_walk) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->truth_set(n_frames, n_rows, truth16, row_of, add_walk); }
int msckf_hip_nees_log_enable(msckf_hip_handle h, int capacity_frames) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->nees_log_enable(capacity_frames); }
int msckf_hip_nees_log_reset(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->nees_log_reset(); }
int msckf_hip_nees_log_count(msckf_hip_handle h) { if (!h) return fail(-EINVAL, "null handle"); return H(h)->nees_log_count(); }
int msckf_hip_nees_log_read(msckf_hip_handle h, int r0, int n, int b0, int nb, double* out) { if (!h || !out) return fail(-EINVAL, "null argument"); return H(h)->nees_log_read(r0, n, b0, nb, out); }
int msckf_hip_nees_log_ensemble(msckf_hip_handle h, int r0, int r1, const int* group_of, int n_groups, double* out) { if (!h || !group_of || !out) return fail(-EINVAL, "null argument"); return H(h)->nees_log_ensemble(r0, r1, group_of, n_groups, out); }
int msckf_hip_frame_log_align(msckf_hip_handle h, int r0, int r1, const int* r0b, const int* r1b, const double* gt_pose7, int mode, double* out) {
  if (const auto r = msckf_traj::pointer_refusal({h, gt_pose7, out}); r.code) return fail(r.code, r.why);
  return H(h)->frame_log_traj("frame_log_align", r0, r1, r0b, r1b, gt_pose7, mode, nullptr, 0, out);
}
int msckf_hip_frame_log_rpe(msckf_hip_handle h, int r0, int r1, const int* r0b, const int* r1b, const double* gt_pose7, const int* lags, int n_lags, double* out) {
  if (const auto r = msckf_traj::pointer_refusal({h, gt_pose7, lags, out}); r.code) return fail(r.code, r.why);
  return H(h)->frame_log_traj("frame_log_rpe", r0, r1, r0b, r1b, gt_pose7, 0, lags, n_lags, out);
}
int msckf_hip_traj_align(msckf_hip_handle h, int n_rec, int n_traj, const double* est_pose7, const double* gt_pose7, const int* r0b, const int* r1b, int mode, double* out) {
  if (const auto r = msckf_traj::pointer_refusal({h, est_pose7, gt_pose7, out}); r.code) return fail(r.code, r.why);
  return H(h)->pose_traj("traj_align", n_rec, n_traj, est_pose7, gt_pose7, r0b, r1b, mode, nullptr, 0, out);
}
int msckf_hip_traj_rpe(msckf_hip_handle h, int n_rec, int n_traj, const double* est_pose7, const double* gt_pose7, const int* r0b, const int* r1b, const int* lags, int n_lags, double* out) {
  if (const auto r = msckf_traj::pointer_refusal({h, est_pose7, gt_pose7, lags, out}); r.code) return fail(r.code, r.why);
  return H(h)->pose_traj("traj_rpe", n_rec, n_traj, est_pose7, gt_pose7, r0b, r1b, 0, lags, n_lags, out);
}
int msckf_hip_literal_info(msckf_hip_handle h, int b, int* out8) { if (!h || !out8) return fail(-EINVAL, "null argument"); return H(h)->lit_info(b, out8); }

}  // extern "C"
