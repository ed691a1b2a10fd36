/* msckf_hip.h -- C-ABI of the MI355X-native batched MSCKF filter core (libmsckf_hip.so).
 *
 * Drop-in boundary for the EKF hot path of daniilidis-group/msckf_mono.  The reference has no FFI layer:
 * its operator boundary is the public interface of the header-only class template
 *     msckf_mono::MSCKF<_S>            (include/msckf_mono/msckf.h:66-848)
 * instantiated as MSCKF<float> by src/ros_interface.cpp:80 and datasets/asl_msckf.cpp:57.  Each entry point
 * below replaces one member function of that class for ONE trajectory `b` of a batch handle (the reference
 * object is the B = 1 case); include/msckf_mono/msckf.h in this repository is the C++ shim that keeps the
 * reference's class/member names on top of these calls.
 *
 * Conventions: plain pointers and sizes only; every scalar crosses the boundary as double (narrowed to
 * the handle's dtype inside); matrices are column-major; quaternions are (w,x,y,z) in Eigen's Hamilton
 * convention; return value 0 = success, negative = -errno style failure (never throws; the reference
 * reports nothing at all, msckf.h:328,1405-1409).  A handle is bound to one HIP device and one stream; calls
 * on one handle must not be concurrent (the reference object is not re-entrant either).
 *
 * Packed argument layouts
 *   cam12    c_u c_v f_u f_v b | q_CI(w,x,y,z) | p_C_I(3)                               types.h:48-55
 *   noise29  u_var_prime v_var_prime | diag(Q_imu)(12) | diag(initial_imu_covar)(15)   types.h:86-92
 *            (every caller of the reference passes diagonal matrices: asl_msckf.cpp:86-108)
 *   uv2      u_var_prime v_var_prime                                                   types.h:87-88
 *   Q144     Q_imu, 12 x 12 column-major; noise order n_g n_wg n_a n_wa (calcG)         types.h:90
 *   P0_225   initial_imu_covar, 15 x 15 column-major; error-state order th b_g v b_a p  types.h:91
 *   params8  max_gn_cost_norm min_rcond translation_threshold redundancy_angle_thresh
 *            redundancy_distance_thresh min_track_length max_track_length max_cam_states types.h:94-99
 *   imu29    q_IG(4) b_g(3) v_I_G(3) b_a(3) p_I_G(3) g(3) q_IG_null(4) v_I_G_null(3) p_I_G_null(3)
 *                                                                                       types.h:69-76
 *   reading7 omega(3) a(3) dT                                                           types.h:78-84
 *   cam7     q_CG(4) p_C_G(3)                                                           types.h:57-67
 *   frame log record, 48 scalars per frame and trajectory, all as the frame's update and prune leave them:
 *            0-15  q_IG(4) b_g(3) v_I_G(3) b_a(3) p_I_G(3): the first 16 entries of imu29
 *            16-30 diagonal of P_II (error-state order th b_g v b_a p)
 *            31-36 upper triangle of the position block P[12..14][12..14]: xx xy xz yy yz zz
 *            37    window size (camera states)
 *            38-40 n_tracks, passed, sticky error flags of the update (out7[0], out7[4] of last_stats; get_error_flags)
 *            41-47 cam7 of camera slot 0: the oldest surviving camera, the fixed-lag estimate; zeros for an empty window
 *   map log record, 8 scalars per logged track (a track the reference's map_ would hold, msckf.h:371: motion check passed
 *            or skipped, triangulation valid), as the frame's update leaves them:
 *            0-2   p_f_G, the triangulated landmark
 *            3     gamma, the track's gate statistic (chi-square with 2 M - 3 degrees of freedom for a passed track)
 *            4     frame ordinal: frames run since msckf_hip_map_log_enable / _reset
 *            5     track index in the frame's work-list
 *            6     flags: 1 gate passed, 2 included in the update, 4 gamma is the early-accept bound
 *                  (msckf_hip_set_gate_early_accept), not the statistic
 *            7     M, the track's observation count
 *            (4-7 are integers below 2^24: exact in a float)
 *   pruned-state log record, 32 scalars per camera state that a frame drops, as the frame's update leaves it (before the prune):
 *            0-6   cam7 of the dropped state: its last, fully corrected pose -- the fixed-lag smoothed estimate
 *            7     prune frame ordinal: frames run since msckf_hip_pruned_log_enable / _reset
 *            8-28  upper triangle of the state's 6 x 6 posterior covariance block (error-state order th_C p_C), row by row:
 *                  (0,0) (0,1) .. (0,5) (1,1) .. (1,5) (2,2) .. (5,5)
 *            29    window size before the prune
 *            30    k: the state is the k-th oldest of those the frame drops (its camera slot before the prune)
 *            31    0
 *            (7, 29, 30 are integers below 2^24: exact in a float)
 *   NEES log record, 8 doubles per frame and trajectory whatever the handle's dtype, from the state the frame leaves and the
 *            frame's row of the truth table (msckf_hip_truth_set):
 *            0     NEES of the 15-state: e^T P_II^-1 e, e = [e_th ; b_g - b_g* ; v - v* ; b_a - b_a* ; p - p*] in P's own order
 *            1-5   NEES of the 3 x 3 diagonal blocks th, b_g, v, b_a, p on their own
 *            6     frame index f
 *            7     flags: 1 a diagonal entry or a pivot of P_II was not positive, 2 the cell was skipped (either: 0-5 are 0),
 *                  4 the trajectory's sticky error flags are set (0-5 are computed all the same)
 *
 * Pixel noise: with u_var_prime == v_var_prime (the configuration the throughput metric is quoted on) the update is
 * independent of the null-space basis and of the compression order and matches the reference to rounding.  With
 * u_var_prime != v_var_prime (EuRoC intrinsics, asl_msckf.cpp:77-78) the library builds the reference's own construction on
 * the device (msckf_hip_set_anisotropic_noise, mode 0, default): R_o_j = A_j^T R_j A_j with A_j the trailing columns of the
 * column-pivoted Householder Q of H_f_j (= JacobiSVD's trailing U columns, msckf.h:954-955), HouseholderQR of the stack in
 * the reference's column and row order with the zero-tail rule (rows 0..14 of H_o pass verbatim), R_n = Q_1^T R_o Q_1
 * (msckf.h:423-431, 1343-1366).  The reference's own result there is not reproducible beyond ~1e-4 in the biases per
 * update: a column that depends on the previous ones (the window's gauge directions) has a rounding-level tail, the
 * reflector built from it is rounding noise, and its row enters R_n with O(1) weight (measured with the reference's own
 * source under two roundings, tests/test_ref_vs_oracle.py).  tail_tol > 0 treats such a tail (below tail_tol * |column|) as
 * the zero it is in exact arithmetic -- the reference's algorithm in its exact-arithmetic limit, reproducible to rounding
 * and as close to either rounding of the reference as they are to each other; tail_tol = 0 is msckf.h's rule to the
 * letter (where rows exist below the first 15 + 6N the tail comes out of an f64 Gram matrix, which resolves it to ~1e-4 of
 * the column at best: tail_tol is taken no finer than 3e-4 there).  Mode 1 pre-whitens every observation row by 1/sigma_u resp. 1/sigma_v and runs the filter with unit noise (the
 * full generalized-least-squares update: statistically the better estimator, but not the reference's).
 */
#ifndef MSCKF_HIP_H
#define MSCKF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct msckf_hip_batch* msckf_hip_handle;

/* MSCKF_HIP_F16H_F32P (BASELINE.json configs[4]): state, covariance and every accumulation in f32 (Gram matrix in f64),
 * the 2 x 6 measurement Jacobian blocks H_x rounded to and stored as fp16. */
enum { MSCKF_HIP_F32 = 0, MSCKF_HIP_F64 = 1, MSCKF_HIP_F16H_F32P = 2 };

/* ---- lifecycle --------------------------------------------------------------------------------------- */
/* B trajectories; capacity n_cap camera states (>= max(max_cam_states, max_track_length)+1),
 * f_cap tracks per update, m_cap observations per track (<= 64).  replaces: MSCKF() ctor, msckf.h:69. */
int msckf_hip_create(int B, int n_cap, int f_cap, int m_cap, int dtype, int device, msckf_hip_handle* out);
int msckf_hip_destroy(msckf_hip_handle h);
/* Value semantics of the reference object (MSCKF<_S> is copyable, msckf.h:31-67): dst <- the filter state of every trajectory
 * of src (states, parameters, covariance, counters, flags, host-side track bookkeeping) and every setting of src that decides
 * numerics or which kernels run, whether a setter or the environment at src's creation chose it ("Settings":
 * the column "copy"): dst continues bit for bit as src would.  The staging ring, host affinity and test hooks stay dst's own.
 * Both handles must have been created with the same B, capacities and dtype (-EINVAL otherwise; also when src runs the
 * anisotropic sweep over the dense stack, MSCKF_HIP_LITERAL_ROUTE=1, and dst's literal work space was allocated without that
 * stack); work buffers and a resident scenario are not copied. */
int msckf_hip_copy_state(msckf_hip_handle dst, msckf_hip_handle src);
const char* msckf_hip_last_error(void);

/* ---- the reference's public member functions, per trajectory b ---------------------------------------- */
/* MSCKF::initialize(camera, noise_params, msckf_params, imu_state)                   msckf.h:72-97  */
int msckf_hip_initialize(msckf_hip_handle h, int b, const double* cam12, const double* noise29,
                         const double* params8, const double* imu29);
/* The same with the whole Q_imu and initial_imu_covar (msckf.h:86, :134) instead of their diagonals.  Q_imu is kept as its
 * symmetric part (Q + Q^T) / 2 -- exact: msckf.h:143 symmetrises Phi (P_II + G Q G^T dT) Phi^T, so only the symmetric part
 * of G Q G^T reaches the covariance.  initial_imu_covar becomes P_II as given and must be symmetric to 1e-12 of its largest
 * entry.  Non-finite entries or an asymmetric initial_imu_covar: -EINVAL (reason in msckf_hip_last_error()).  With every
 * off-diagonal entry of both matrices zero this is msckf_hip_initialize on the diagonals, bit for bit; a later
 * msckf_hip_initialize of the same b drops the full Q_imu again.  No positive-definiteness check (the reference has none). */
int msckf_hip_initialize_full(msckf_hip_handle h, int b, const double* cam12, const double* uv2, const double* Q144,
                              const double* P0_225, const double* params8, const double* imu29);
/* MSCKF::propagate(imuReading&), K consecutive readings fused into one launch        msckf.h:101-145 */
int msckf_hip_propagate(msckf_hip_handle h, int b, const double* readings7, int K);
/* MSCKF::augmentState(state_id, time)                                                msckf.h:148-212 */
int msckf_hip_augment_state(msckf_hip_handle h, int b, int state_id, double time);
/* MSCKF::update(measurements, feature_ids)   (host-side track bookkeeping)           msckf.h:215-299 */
int msckf_hip_update(msckf_hip_handle h, int b, const double* meas2, const uint64_t* ids, int n);
/* MSCKF::addFeatures(features, feature_ids)  (host-side track bookkeeping)           msckf.h:302-332 */
int msckf_hip_add_features(msckf_hip_handle h, int b, const double* meas2, const uint64_t* ids, int n);
/* MSCKF::marginalize()                                                               msckf.h:336-449 */
int msckf_hip_marginalize(msckf_hip_handle h, int b);
/* MSCKF::pruneEmptyStates()                                                          msckf.h:685-761 */
int msckf_hip_prune_empty_states(msckf_hip_handle h, int b);
/* MSCKF::pruneRedundantStates(): keyframe selection + observation surgery on the host, triangulation of
 * not-yet-initialized features and the second update on the device                   msckf.h:453-682 */
int msckf_hip_prune_redundant_states(msckf_hip_handle h, int b);
/* MSCKF::finish()                                                                    msckf.h:765-807 */
int msckf_hip_finish(msckf_hip_handle h, int b);
/* getters, msckf.h:810-848 */
int msckf_hip_get_num_cam_states(msckf_hip_handle h, int b);                 /* getNumCamStates :810 */
int msckf_hip_get_imu_state(msckf_hip_handle h, int b, double* imu29);       /* getImuState     :815 */
int msckf_hip_get_cam_states(msckf_hip_handle h, int b, double* cam7, int* state_ids, int cap); /* getCamStates :835 */
int msckf_hip_get_map(msckf_hip_handle h, int b, double* xyz, int cap);      /* getMap :820; returns count */
int msckf_hip_get_pruned_state_ids(msckf_hip_handle h, int b, int* ids, int cap);  /* getPrunedStates :840 */
/* getPrunedStates() :840-848 in full: the camState of every pruned state as it was when pruned (pose after the
 * last update that touched it, time, ids; types.h:57-67), sorted by state_id as the reference sorts them.  Any output
 * pointer may be NULL.  Read by asl_msckf.cpp:409-424 (pruned-camera path).  Returns the count. */
int msckf_hip_get_pruned_states(msckf_hip_handle h, int b, double* cam7, double* time, int* state_ids,
                                int* last_correlated_ids, int cap);
/* the non-pose members of getCamStates()[i] (types.h:57-67): time, tracked_feature_ids.size(), last_correlated_id
 * (asl_msckf.cpp:384-388 publishes them); host-side bookkeeping, no device access.  Returns the count. */
int msckf_hip_get_cam_meta(msckf_hip_handle h, int b, double* time, int* n_tracked, int* last_correlated_ids, int cap);
/* getCamState(i).tracked_feature_ids :830 */
int msckf_hip_get_tracked_feature_ids(msckf_hip_handle h, int b, int cam_index, uint64_t* ids, int cap);

/* ---- additive accessors (the reference keeps these private, msckf.h:52-54; needed for parity tests) ---- */
int msckf_hip_get_covariance(msckf_hip_handle h, int b, double* P, int ld);  /* D x D, D = 15 + 6 N */
int msckf_hip_set_covariance(msckf_hip_handle h, int b, const double* P, int D);
int msckf_hip_set_imu_state(msckf_hip_handle h, int b, const double* imu29);
int msckf_hip_set_cam_pose(msckf_hip_handle h, int b, int slot, const double* cam7);
int msckf_hip_get_num_residualized(msckf_hip_handle h, int b, long long* n);
int msckf_hip_set_num_residualized(msckf_hip_handle h, int b, long long n);
/* last marginalize: out[0..6] = n_tracks, motion-rejected, triangulation-rejected, gate-rejected, passed,
 * stacked rows m, kept rows r.  Also the place where the trajectory's sticky device-side error flags surface (out7 is
 * filled regardless): -EOVERFLOW camera-state capacity exceeded in augmentState; -EDOM a factorization of
 * S = T_H P T_H^T + R_n (msckf.h:1369) met a non-positive pivot since the flags were last cleared -- the covariance lost
 * positive definiteness (the pivot is clamped and the run continues; the reference's explicit S.inverse() would return
 * garbage silently).  (No kernel waits for another workgroup without a fall-back: the in-place prune is one workgroup per
 * trajectory, the gain solve's shared product is re-formed locally when a sibling does not show up.)
 *
 * The non-positive pivot report, stated once (held by tests/test_gpu_pivot_report.py at every factorization of S):
 *   - the flag is per trajectory and sticky until msckf_hip_clear_error_flags, and it is raised by every covariance-update form
 *     (0, 1, 2), every compression route (the literal anisotropic route has no factorization of S of its own, neither a Cholesky
 *     nor the reference's explicit inverse: it leaves its information matrix where k_gram leaves H_o^T H_o and the same kernels
 *     factor S from there) and both dtypes;
 *   - the other trajectories of the launch, of the frame range and of the handle are unaffected, bit for bit;
 *   - the failed trajectory's state and covariance are undefined from the failed update on, until they are overwritten
 *     (set_covariance, set_imu_state, set_cam_pose) or the trajectory is re-initialised; its counts and per-track results of that
 *     update are still the update's own;
 *   - the handle is otherwise reusable after msckf_hip_clear_error_flags: no scratch buffer carries anything of the failure
 *     into a later update, of that trajectory or of another.
 * The per-track gate factors N_j = H_x,j P H_x,j^T + R_j of the track's unprojected Jacobian; a track whose N_j is not positive
 * definite is gate-rejected (where the reference, which factors the projected A_j^T N_j A_j, may pass it) and raises no flag
 * of its own; such a P is no covariance, and the factorization of the joint S reports it in the same update. */
int msckf_hip_last_stats(msckf_hip_handle h, int b, int* out7);
int msckf_hip_clear_error_flags(msckf_hip_handle h, int b);
/* the sticky flags themselves, without turning them into a return code: bit 0 capacity overflow (-EOVERFLOW above), bit 1
 * non-positive pivot (-EDOM above).  For callers that poll many trajectories and want the statistics either way. */
int msckf_hip_get_error_flags(msckf_hip_handle h, int b, int* flags);
/* per track of the last marginalize: out[t*8 + ..] = motion_ok tri_valid gate_pass included gamma p_f_G(3) */
int msckf_hip_last_tracks(msckf_hip_handle h, int b, double* out8, int cap);
int msckf_hip_last_deltax(msckf_hip_handle h, int b, double* dx, int cap);
/* per track of the last marginalize, what the feature kernels stored for the information-form route (-ENOTSUP on handles without
 * it; an f16 Jacobian is read as stored and widened, so Hx holds exact binary16 values): first[t] = first | last << 8 camera slot
 * of the track; Hx[t][m_cap][12] the whitened 2 x 6 Jacobian block of every observation; rw[t][m_cap][2] the whitened residuals; Bh[t][3][6 n_cap + 1] the three rows of B^ (the
 * window's camera columns, c in column 6 n_cam).  Entries beyond a track's observations, and columns of B^ outside its slot
 * range, are whatever the buffers held.  Returns the number of tracks (at most cap). */
int msckf_hip_last_track_blocks(msckf_hip_handle h, int b, int* first, double* Hx, double* rw, double* Bh, int cap);

/* ---- batched path: work-lists ("front-end track dump": positional camera slots + normalized coords) ---- */
/* Replace trajectory b's work-list by F tracks; slots/obs are flattened over tracks (sum(M) entries).
 * This is what MSCKF::update() hands to marginalize() as feature_tracks_to_residualize_ (msckf.h:249-262). */
int msckf_hip_set_tracks(msckf_hip_handle h, int b, int F, const int* M, const int* slots, const double* obs2);
/* propagate / augment / marginalize / prune for the trajectory range [b0, b0+nb) in single launches */
int msckf_hip_propagate_range(msckf_hip_handle h, int b0, int nb, const double* readings7, int K); /* [nb][K][7] */
/* The same with a sample count per trajectory: readings7 holds the trajectories' samples one after the other, K[i] >= 0 rows for
 * trajectory b0 + i.  Bit for bit msckf_hip_propagate_range(h, b0 + i, 1, rows_i, K[i]) called trajectory by trajectory; a
 * trajectory with K[i] == 0 is not touched.  -EINVAL for a negative K[i] (nothing is propagated). */
int msckf_hip_propagate_range_counts(msckf_hip_handle h, int b0, int nb, const double* readings7, const int* K);
int msckf_hip_augment_range(msckf_hip_handle h, int b0, int nb);
int msckf_hip_marginalize_range(msckf_hip_handle h, int b0, int nb);
int msckf_hip_drop_oldest_range(msckf_hip_handle h, int b0, int nb, int n_drop);
/* The ASL runner's per-image cycle (datasets/asl_msckf.cpp:269-294: augmentState, update, addFeatures, marginalize,
 * pruneRedundantStates :289, pruneEmptyStates) for trajectories b0 .. b0 + nb - 1 IN LOCKSTEP: the feature bookkeeping of every
 * trajectory (msckf.h:215-332, 453-534, 685-717, 1049-1098) runs on the host through the same steps as the per-filter entries
 * (msckf_mono_amd/csrc/host_lists.h states each rule once; the two callers differ only in their device calls), every device stage is one
 * launch sequence over the range and every read-back (poses for findRedundantCamStates, triangulated points, pruned states' poses)
 * one copy + one wait for the whole range.  Same results per trajectory as msckf_hip_augment_state / _update / _add_features /
 * _marginalize / _prune_redundant_states / _prune_empty_states called filter by filter, bit for bit.  IMU samples go in beforehand
 * through msckf_hip_propagate_range.  state_ids[nb], times[nb] (may be null): augmentState's arguments; upd_* / new_*: update()'s
 * and addFeatures()'s arguments of the trajectories, concatenated (upd_n[i] / new_n[i] entries each; normalized coordinates, 2 per id).
 * flags: 1 = pruneRedundantStates, 2 = pruneEmptyStates. */
int msckf_hip_image_cycle_range(msckf_hip_handle h, int b0, int nb, const int* state_ids, const double* times,
                                const double* upd_meas2, const uint64_t* upd_ids, const int* upd_n,
                                const double* new_meas2, const uint64_t* new_ids, const int* new_n, int flags);

/* ---- batched path: HBM-resident scenario (inputs uploaded once, then frames run without host syncs) ---- */
int msckf_hip_scenario_alloc(msckf_hip_handle h, int n_frames, int K);
/* stage one (frame, trajectory) cell on the host side of the handle */
int msckf_hip_scenario_set(msckf_hip_handle h, int frame, int b, const double* readings7 /*[K][7]*/, int F,
                           const int* M, const int* slots, const double* obs2, int n_drop);
/* The same cell with its OWN number of IMU samples and, for batches whose sequences differ in length, a skip mark.
 *   k      0 <= k <= K of msckf_hip_scenario_alloc: only k rows of readings7 are read (null allowed when k == 0), by the host
 *          and by the device.  k == 0: the frame propagates nothing -- state and covariance are not rewritten -- and
 *          augments: bit for bit msckf_hip_augment_range alone.
 *   flags  bit 0 (MSCKF_HIP_CELL_SKIP): this trajectory's sequence has no image on this frame.  Nothing of the trajectory
 *          changes: no propagate, no camera state, no update, no prune; its frame-log record repeats the unchanged state.
 *          A skipped cell has k == 0, F == 0 and n_drop == 0.
 * -EINVAL for k out of range, a skipped cell that carries samples, tracks or a drop, or an unknown flag bit; the cell staged
 * before stays.  msckf_hip_scenario_set is this entry with k = K and flags = 0.  Like it, the call un-commits the scenario. */
enum { MSCKF_HIP_CELL_SKIP = 1 };
int msckf_hip_scenario_set_cell(msckf_hip_handle h, int frame, int b, const double* readings7 /*[k][7]*/, int k, int F,
                                const int* M, const int* slots, const double* obs2, int n_drop, int flags);
int msckf_hip_scenario_commit(msckf_hip_handle h);   /* H2D of everything staged */
/* one filter update per trajectory per frame: K x propagate + augmentState + marginalize + prune, for
 * frames [f0, f1), asynchronously on the handle's stream.  Results do not depend on how a range is cut into calls.
 * (In the square-root gain form the prune of every frame but a call's last rides on the covariance downdate, which
 * writes the pruned covariance into the handle's second buffer -- one launch less per frame; environment
 * MSCKF_HIP_FUSE_PRUNE=0 at create time keeps the separate prune launch, for A/B runs.) */
int msckf_hip_run_frames(msckf_hip_handle h, int f0, int f1);
/* The same frames with the inputs handed over per frame, as the reference's callers do (IMU samples and the image's
 * tracks arrive with the image, asl_msckf.cpp:227-284): frame f's IMU samples and its COMPACT work-list (sum M_j slot /
 * observation entries + per-track offsets, not padded [f_cap][m_cap] rows) are copied from page-locked host memory into one
 * of `depth` device staging sets on a copy stream, up to depth - 1 frames ahead of the kernels that read them.  Results are
 * bit-identical to msckf_hip_run_frames; the difference is the PCIe leg inside the timed region. */
int msckf_hip_run_frames_streamed(msckf_hip_handle h, int f0, int f1);
/* Build the page-locked per-frame blocks of frames [f0, f1) (and size the device staging ring) ahead of time;
 * msckf_hip_run_frames_streamed does it on first use otherwise.  Only frames that are streamed are ever page-locked;
 * -ENOMEM leaves msckf_hip_run_frames on the resident scenario unaffected. */
int msckf_hip_scenario_pin(msckf_hip_handle h, int f0, int f1);
/* Staging ring of msckf_hip_run_frames_streamed: depth 2..8 (default 6); mode 0 (default) hands frames over between the
 * uploading thread and the slices' enqueue threads on the HOST (no stream waits for another stream's event on the device),
 * mode 1 uses hipStreamWaitEvent hand-overs.  Same results. */
int msckf_hip_set_upload_ring(msckf_hip_handle h, int depth, int mode);
/* ---- Monte-Carlo replay: shared noise-free sequences, per-trajectory seeded noise added on the device -------------- */
/* n_seq SEQUENCES of n_frames cells are staged once (sequence values are kept as doubles); each of the handle's B trajectories
 * then names a sequence, a 64-bit seed and a noise model (four white levels, or the filter's Q_imu with its bias random walks:
 * msckf_hip_replay_assign_q below), and before each frame one kernel launch per slice expands the
 * frame's sequence cells into the ordinary per-trajectory frame block -- what msckf_hip_run_frames_streamed would have
 * uploaded -- so that B trajectories cost the host store, the page-locked memory and the PCIe traffic of none.
 * The noise is a pure function of (seed, frame, index), no state is carried between frames:
 *   mix(s, i)  = value i (0-based) of splitmix64 seeded s: z = s + (i + 1) 0x9E3779B97F4A7C15, z = (z ^ z >> 30) 0xBF58476D1CE4E5B9,
 *                z = (z ^ z >> 27) 0x94D049BB133111EB, z ^ z >> 31, modulo 2^64;   U(s, i) = (mix(s, i) >> 11) 2^-53
 *   pair(s, j) = (r cos(2 pi u2), r sin(2 pi u2)) with u1 = 1 - U(s, 2 j), u2 = U(s, 2 j + 1), r = sqrt(-2 ln u1)
 *   trajectory b with seed s_b on frame f: s_imu = mix(s_b, 2 f), s_obs = mix(s_b, 2 f + 1)
 *   IMU sample i < k of the cell takes pairs 3 i, 3 i + 1, 3 i + 2 of s_imu = (g_x, g_y), (g_z, a_x), (a_y, a_z):
 *     omega += sigma_g g, a += sigma_a a; dT is unchanged; rows from k on are zero
 *   entry e of the cell (its e-th (slot, observation) pair) takes pair e of s_obs: obs += (sigma_u n_u, sigma_v n_v)
 * Sums are formed in double and rounded once to the handle's scalar.  msckf_mono_amd/scenario.py holds the numpy twin.
 * msckf_hip_replay_alloc replaces a previous replay; a scenario staged with msckf_hip_scenario_* is independent of it. */
int msckf_hip_replay_alloc(msckf_hip_handle h, int n_seq, int n_frames, int K);
/* one (frame, sequence) cell: arguments and rules of msckf_hip_scenario_set_cell; un-commits the replay */
int msckf_hip_replay_set_cell(msckf_hip_handle h, int frame, int seq, const double* readings7 /*[k][7]*/, int k, int F,
                              const int* M, const int* slots, const double* obs2, int n_drop, int flags);
/* seq_of[B], seed[B], sigma4[B][4] = sigma_g sigma_a sigma_u sigma_v per trajectory.  -EINVAL for a seq_of outside
 * [0, n_seq) or a sigma that is negative or not finite; the assignment made before stays.  May be called again between runs. */
int msckf_hip_replay_assign(msckf_hip_handle h, const int* seq_of, const uint64_t* seed, const double* sigma4);
/* The Q_imu model in place of sigma4: the noise the filter assumes (msckf_hip_initialize_full's Q144), correlated, with the
 * two bias random walks.  Per trajectory Q[b] (12 x 12, column-major, noise order n_g n_wg n_a n_wa, taken as its symmetric
 * part 0.5 (Q + Q^T)), scale[b] >= 0 (the role of scenario.Trajectory's imu_noise_scale) and (sigma_u, sigma_v)[b].
 *   L = chol_psd(Q_sym), lower triangular, on the host in double: for column c, d = Q_cc - s, s = sum_{j < c} L_cj^2 (ascending j
 *     from 0); d < -1e-12 max_diag is refused; |d| <= 1e-12 max_diag makes the whole column zero (semi-definite input works: a
 *     zero walk density is the common case); otherwise L_cc = sqrt(d), L_rc = (Q_rc - sum_{j < c} L_rj L_cj) / L_cc
 *   IMU sample i < k of the cell takes pairs 6 i .. 6 i + 5 of s_imu as z[0 .. 11]: pair 6 i + p = (z[2 p], z[2 p + 1]);
 *     w_r = sum_{c <= r} L_rc z_c, c ascending from 0, each product rounded, then added
 *   with dT_i > 0: omega += (scale w[0:3]) / sqrt(dT_i), a += (scale w[6:9]) / sqrt(dT_i),
 *     delta_g = (scale w[3:6]) sqrt(dT_i), delta_a = (scale w[9:12]) sqrt(dT_i); a sample with dT_i <= 0 gets neither
 *   the walk, per component (gyro 0 .. 2, accelerometer 3 .. 5), summed sequentially in double: P(f, 0) = 0,
 *     P(f, i + 1) = P(f, i) + delta(f, i); Wstart(0) = 0, Wstart(f + 1) = Wstart(f) + P(f, k_f); skipped cells and cells with
 *     k = 0 add nothing.  Sample (f, i) stores (value + (Wstart(f) + P(f, i))) + noise: the bias starts at the sequence's constant
 *     bias, what the filter is initialised with.  Rows from k on are zero.  Observations as above: obs += (sigma_u n_u, sigma_v n_v).
 * Everything is summed in double and rounded once to the handle's scalar.  A one-off device scan tabulates Wstart (frames + 1
 * rows per trajectory) when an assignment or a commit has changed it, so single frames and cut ranges expand as before.
 * -EINVAL, in this order: "seq_of names no sequence of the replay", "Q, scale and sigma must be finite", "scale and sigma must
 * not be negative", "Q is not positive semi-definite"; the assignment made before stays.  May be called between runs; a later
 * msckf_hip_replay_assign returns the handle to the sigma4 model.  msckf_hip_run_frames_replay, msckf_hip_replay_expand and
 * _expand_ints serve whichever model is assigned. */
int msckf_hip_replay_assign_q(msckf_hip_handle h, const int* seq_of, const uint64_t* seed, const double* Q144 /*[B][144]*/,
                              const double* scale /*[B]*/, const double* sigma_uv /*[B][2]*/);
/* Rows [f0, f1) of Wstart, 0 <= f0 <= f1 <= frames + 1, for the trajectories [b0, b0 + nb): out [f1 - f0][nb][6] (gyro, then
 * accelerometer bias offset).  Row f + 1 is the true bias offset at the time of frame f's log record.  Builds the table if
 * needed.  -EINVAL "no replay allocated", "walk range out of bounds", "replay not committed", "replay not assigned through
 * msckf_hip_replay_assign_q", in this order. */
int msckf_hip_replay_walk(msckf_hip_handle h, int f0, int f1, int b0, int nb, double* out);
int msckf_hip_replay_commit(msckf_hip_handle h);   /* H2D of the sequences staged */
/* msckf_hip_run_frames over the frames [f0, f1) of the replay: same kernels, same slices, same logs; a frame's inputs are
 * expanded on the slice's own stream ahead of its propagate.  -EINVAL "frame range out of bounds", "replay not committed",
 * "replay not assigned", in this order. */
int msckf_hip_run_frames_replay(msckf_hip_handle h, int f0, int f1);
/* What the expansion kernel writes for trajectory b on `frame`, from a launch of the same kernel for that trajectory alone into
 * scratch memory: rd [K][7] and the cell's coordinate pairs obs2 [entries][2] as doubles (exact: the handle's scalar widened);
 * _ints: ints [3 + 2 f_cap] = n, drop, k, M[f_cap], off[f_cap] and slots [entries].  Returns the cell's entries; -E2BIG when
 * they exceed cap_entries.  Nothing of the handle's filters, inputs or logs changes. */
int msckf_hip_replay_expand(msckf_hip_handle h, int frame, int b, double* rd /*[K][7]*/, double* obs2, int cap_entries);
int msckf_hip_replay_expand_ints(msckf_hip_handle h, int frame, int b, int* ints, int* slots, int cap_entries);
/* Seeded front-end faults on top of either noise model: missed observations and outliers, per trajectory
 * fault4[b] = (p_miss, p_out, rho_u, rho_v) -- two probabilities in [0, 1], two radii in normalised image units, finite and >= 0.
 *   s_flt(f) = mix(mix(s_b, 2^63 + 1), f).  Frames use mix(s_b, 2 f) and mix(s_b, 2 f + 1), replay_initial_error (the twin)
 *     uses mix(s_b, 2^63): no frame index reaches either.
 *   entry e (0-based among the SEQUENCE cell's entries, in sequence order) takes u_miss = U(s_flt, 3 e), u_out = U(s_flt, 3 e + 1),
 *     u_ang = U(s_flt, 3 e + 2)
 *   raw_miss(e) = u_miss < p_miss.  A track that would keep fewer than two observations loses none: if M - #raw_miss < 2 then
 *     miss = false on the whole track (so the sequence's own tracks with M < 2 pass through unchanged); otherwise
 *     miss = raw_miss.  A tracker hands the filter no track of one observation.
 *   out(e) = !miss(e) && u_out < p_out
 *   obs = value + sigma noise exactly as without faults (pair e of s_obs, indexed by the sequence entry: a trajectory's Gaussian
 *     noise does not depend on its faults); where out(e) the pair becomes (x + rho_u cos a, y + rho_v sin a), a the rounded
 *     product 6.283185307179586 u_ang, each product rounded, then added, all in double, rounded once to the handle's scalar.
 *     A displacement of fixed size at a uniform angle, so that detection rate against outlier size is a clean curve.
 *   the expanded block: off[t], the trajectory's base, the frame's entry count, n, drop, k and rd are unchanged -- a track's
 *     range keeps the sequence's length.  M[t] is the number of surviving observations; the range is a stable partition, the
 *     survivors in sequence order, then the missed entries in sequence order; every entry carries its slot and coordinates.
 *     Nothing downstream reads beyond off[t] + M[t].
 * With NULL, or every trajectory at p_miss = p_out = 0, the expansion launched and every bit are those without faults.
 * -EINVAL, in this order: "no replay allocated", "fault probabilities must lie in [0, 1]", "fault radii must be finite and not
 * negative"; a refused call leaves the previous setting in force.  May be called between runs; survives msckf_hip_replay_assign,
 * _assign_q and _commit; msckf_hip_replay_alloc clears it.  msckf_hip_replay_expand / _expand_ints return what the faulted
 * kernel wrote: M = survivors, slots and coordinates in partition order; their return value is still the cell's entries. */
int msckf_hip_replay_set_faults(msckf_hip_handle h, const double* fault4 /*[B][4], NULL: none*/);
/* per SEQUENCE entry of trajectory b's cell on `frame`: 0 kept, 1 outlier, 2 missed, from the same launch as
 * msckf_hip_replay_expand.  Returns the cell's entries; -E2BIG when they exceed cap_entries. */
int msckf_hip_replay_expand_faults(msckf_hip_handle h, int frame, int b, int* code /*[entries]*/, int cap_entries);
/* The camera's clock, on top of either noise model and of the faults: a constant camera-IMU time offset, per-image timestamp
 * jitter and rolling-shutter readout, per trajectory timing4[b] = (t_d, r_y, y_0, sigma_j) -- the offset in seconds, the readout
 * slope in seconds per unit of normalised image y (a sensor of H rows read in t_r seconds: r_y = t_r f_v / H,
 * y_0 = (H / 2 - c_v) / f_v), the jitter in seconds; all finite, sigma_j >= 0.  A record is non-zero when t_d, r_y or sigma_j is.
 *   image table of a sequence, built at msckf_hip_replay_commit from its cells alone.  Frames in order with T = 0 (double),
 *     ord = 0, W = 0: a skipped cell changes nothing; any other cell adds its dT_i, i < k ascending, to T, sets ord += 1,
 *     W += 1, records time[ord - 1] = T, frame_of[ord - 1] = f, base(f) = ord - W, then sets W -= n_drop(f).  Camera slot s of
 *     frame f's cell is image base(f) + s: the window an empty start at frame 0 gives, always a suffix of the images.
 *   entry l of a track has the sequence value (x_l, y_l) and image i_l = base(f) + slot_l; it was exposed at time[i_l] + delta_l,
 *     delta_l = (t_d + r_y (y_l - y_0)) + sigma_j g(frame_of[i_l]): the difference, the product, the sum, the product sigma_j g,
 *     the sum, each rounded in double.  g(q) is the first component of pair(mix(s_b, 2^63 + 2), q): one draw per image and seed,
 *     shared by every observation of that image in whichever cell it surfaces (sigma_j == 0: no draw, the term is 0).
 *   the shift uses nodes of the same track, in sequence order: M = 1 unchanged; M = 2 both entries; M >= 3 the entries l0, l0 + 1,
 *     l0 + 2 with l0 = min(max(l - 1, 0), M - 3).  d_j = time[i_j] - time[i_l], relative to the entry's own time;
 *     w_j = prod_{m != j} (delta_l - d_m) / prod_{m != j} (d_j - d_m), m ascending, numerator and denominator each one product
 *     (three nodes) or one difference (two), then one division; the new value is sum_j w_j (x_j, y_j), j ascending, the first
 *     product, then each further product added: + - x / only, each rounded in double, no contraction.  delta_l == 0 exactly:
 *     the value itself.
 *   the Gaussian pixel noise and the outlier ring are then added to the shifted value exactly as without timing; a missed
 *     observation still serves its neighbours as a node; draws stay indexed by the sequence entry, so a seed's noise and faults
 *     do not depend on its timing.  Timing moves no IMU row.
 * With NULL, or every record zero (y_0 alone moves nothing), the expansion launched and every bit are those without timing.
 * -EINVAL, in this order: "no replay allocated", "timing values must be finite", "jitter must not be negative"; then, only
 * under a non-zero record (here on committed cells, and at msckf_hip_replay_commit while such a record is in force), with the
 * sequence, frame and track named ("timing: sequence S, frame F, track T: ..."): a cell that names a camera slot >= W(f), a track
 * whose slots do not ascend strictly, a track whose node times do not increase strictly.  A refused call leaves the previous
 * record in force.  May be called between runs; survives msckf_hip_replay_assign, _assign_q, _set_faults and _commit;
 * msckf_hip_replay_alloc clears it.  msckf_hip_replay_expand / _expand_ints / _expand_faults return what the timed kernel wrote. */
int msckf_hip_replay_set_timing(msckf_hip_handle h, const double* timing4 /*[B][4], NULL: none*/);
/* Sequence seq's image table as the last msckf_hip_replay_commit built it: time [images], frame_of [images], base [frames], each
 * or NULL.  Returns the image count (<= frames).  -EINVAL "no replay allocated", "replay not committed", "replay cell out of
 * range". */
int msckf_hip_replay_image_table(msckf_hip_handle h, int seq, double* time, int* frame_of, int* base);
/* per SEQUENCE entry of trajectory b's cell on `frame`: its delta in seconds (0 without timing), from the same launch as
 * msckf_hip_replay_expand.  Returns the cell's entries; -E2BIG when they exceed cap_entries. */
int msckf_hip_replay_expand_timing(msckf_hip_handle h, int frame, int b, double* delta /*[entries]*/, int cap_entries);
/* The faults of the frames [f0, f1) per trajectory, counted on the device from the sequences, the seeds and the fault record
 * alone (no run, no log): out [B][6] = entries, missed, outliers, tracks, tracks that lost at least one observation, tracks that
 * carry at least one outlier.  Integers: they equal the twin's exactly.  Refusals as msckf_hip_run_frames_replay. */
int msckf_hip_replay_fault_counts(msckf_hip_handle h, int f0, int f1, long long* out /*[B][6]*/);
/* The gate against the faults: the stored map-log records with ordinal in [q0, q1), where the record with ordinal q belongs to
 * replay frame f0 + (q - q0) -- the caller states that msckf_hip_run_frames_replay wrote the log contiguously from f0.  Whether
 * a record's track carries an outlier is recomputed on the device from (seed, frame, the sequence's off / M, fault4).
 * out [B][8] = 0 records in range, 1 clean and gate passed, 2 clean and rejected, 3 contaminated and passed, 4 contaminated and
 * rejected, 5 sum of gamma and 6 sum of 2 M - 3 over the clean gate-passed records without flag 4 (the mean of 5 / 6 is 1 for a
 * consistent filter), 7 records whose track index is >= the cell's n (unmatched, counted nowhere else).  Sums in double, in a
 * fixed order: the same log gives the same bits; sums and counts, so ranks add.  Contaminated tracks that fail the motion or
 * triangulation check are never logged: column 5 of msckf_hip_replay_fault_counts minus columns 3 + 4 here is their number.
 * -EINVAL while the map log is off, for ordinals beyond those handed out, for a frame outside the replay ("frame range out of
 * bounds"), and while the replay is not committed or not assigned. */
int msckf_hip_map_log_fault_metrics(msckf_hip_handle h, int q0, int q1, int f0, double* out /*[B][8]*/);
/* per trajectory, over the non-skipped cells of frames [f0, f1) as msckf_hip_run_frames_replay would expand them (either
 * noise model, walk included; faults do not touch IMU rows): out[B][8] = 0 samples, 1-3 sum omega, 4-6 sum a, 7 sum dT.
 * Each sample is the value the expansion writes -- rounded to the handle's scalar, widened to double -- summed in double in a
 * fixed order (same inputs, same bits).  Sums and counts: intervals add.  Refusals as msckf_hip_run_frames_replay.
 * One wavefront per trajectory: a lane takes the frames f0 + lane, f0 + lane + 64, ... in ascending order and a frame's
 * samples in ascending order, the 64 partial sums are combined by a fixed tree.  What a per-seed stand-still initialisation
 * needs (mean omega = the gyro bias, mean a = the attitude against gravity and the accelerometer bias), from samples that
 * exist only on the device.  Nothing of the handle's filters, inputs or logs changes. */
int msckf_hip_replay_imu_sums(msckf_hip_handle h, int f0, int f1, double* out /*[B][8]*/);
/* Calibration errors of the sensors, on top of either noise model, the faults and the timing (csrc/replay_plan.h, CALIB: the
 * arithmetic below is that file's inline functions calib_imu, calib_out and calib_cam, which the kernels compile).
 * The IMU record imucal[b] = [31]: T_g (0 .. 8, 3 x 3 row-major), T_a (9 .. 17), G (18 .. 26, the gyro's response to specific
 * force, rad/s per m/s^2), sat_g, sat_a (27, 28; 0: no saturation), lsb_g, lsb_a (29, 30; 0: no quantisation).  The identity
 * record is T_g = T_a = I and everything else 0; a record is non-trivial when it differs from that.  The matrices act on the
 * sequence's values, constant bias included: the cell holds omega + b_0 and a + b_0, and the shift (T - I) b_0 is a bias the
 * filter estimates anyway.
 *   sample i < k of a cell that is not skipped, v_g = cell[0:3], v_a = cell[3:6]: c_a[r] = sum_c T_a[r][c] v_a[c] and
 *     c_g[r] = sum_c T_g[r][c] v_g[c], the first product, then each further product added, c ascending; for the gyro then
 *     + G[r][0] v_a[0], + G[r][1] v_a[1], + G[r][2] v_a[2] in that order; every product and sum rounded in double.
 *   c takes the place of the sequence value in the noise rule: c + sigma g under sigma4, (c + W(f, i)) + n under the Q_imu
 *     model (no n when dT_i <= 0).  The bias walk stays an output bias: the walk table does not change.
 *   saturation where sat > 0: x = min(max(x, -sat), sat); a component is CLIPPED when its value before the clamp lies strictly
 *     outside [-sat, sat].  Quantisation where lsb > 0: x = lsb rint(x / lsb), the quotient rounded, rint to nearest even, then
 *     the product.  The result is rounded once to the handle's scalar.  dT, rows from k on and skipped cells are untouched.
 * -EINVAL, in this order: "no replay allocated", "calibration values must be finite", "saturation and quantisation must not be
 * negative"; a refused call leaves the previous record in force.  May be called between runs; survives msckf_hip_replay_assign,
 * _assign_q, _set_faults, _set_timing and _commit; msckf_hip_replay_alloc clears it.  msckf_hip_replay_imu_sums sums the
 * calibrated rows: a per-seed stand-still initialisation sees the scale and g-sensitivity error as it would on a real unit. */
int msckf_hip_replay_set_imu_calib(msckf_hip_handle h, const double* imucal /*[B][31], NULL: none*/);
/* The camera record camcal[b] = (e_u, e_v, d_u, d_v, k1, k2, p1, p2): the residual map, in normalised coordinates, between the
 * true camera and the calibration the front end undistorted with -- e the relative focal-length error, d the principal-point
 * error divided by the focal length, k and p the residual radial-tangential coefficients; all finite, all zero is trivial.
 * It applies to an entry's value (x, y): the sequence value, or what the timing shift made of it (delta keeps the sequence's y):
 *   xx = x x, yy = y y, xy = x y, r2 = xx + yy, rad = (1 + k1 r2) + k2 (r2 r2)
 *   xd = (x rad + (2 p1) xy) + p2 (r2 + 2 xx),  yd = (y rad + p1 (r2 + 2 yy)) + (2 p2) xy
 *   x' = (xd + e_u xd) + d_u,                   y' = (yd + e_v yd) + d_v
 * + - x only, each rounded in double, no contraction.  The Gaussian pixel noise and the outlier ring are then added to (x', y')
 * exactly as before; draws stay indexed by the sequence entry, so a seed's noise and faults do not depend on its calibration;
 * missed entries are mapped too.  -EINVAL, in this order: "no replay allocated", "calibration values must be finite".
 * Lifetime as the IMU record's.  While neither record is non-trivial for any trajectory, the kernels launched and every bit
 * they write are those without calibration; otherwise msckf_hip_replay_expand / _ints / _faults / _timing return what the
 * calibrated kernel wrote. */
int msckf_hip_replay_set_cam_calib(msckf_hip_handle h, const double* camcal /*[B][8], NULL: none*/);
/* From the same single-trajectory launch as msckf_hip_replay_expand, each pointer or NULL: rd_cal, the noise-free calibrated c
 * of every sample in double (rows from k on: the sequence's); clip, per sample the 6-bit mask of clipped components (bit c:
 * column c of the row; the noise is part of the clipped value); obs_cal, the mapped noise-free (x', y') per SEQUENCE entry.
 * Without records c and (x', y') are the sequence's (shifted) values and clip is 0.  Returns the cell's entries; -E2BIG when
 * they exceed cap_entries. */
int msckf_hip_replay_expand_calib(msckf_hip_handle h, int frame, int b, double* rd_cal /*[K][6]*/, int* clip /*[K]*/, double* obs_cal /*[entries][2]*/, int cap_entries);
/* The saturation of the frames [f0, f1) per trajectory, counted on the device without a run: the stored values are recomputed
 * from the sequences, the assignment and the IMU record.  out [B][8] = 0 samples (i < k of the non-skipped cells), 1-3 gyro
 * x, y, z clipped, 4-6 accelerometer x, y, z clipped, 7 samples with any component clipped.  Integers; ranges add.  One
 * wavefront per trajectory, a fixed order and a fixed tree, as msckf_hip_replay_imu_sums.  Refusals as
 * msckf_hip_run_frames_replay.  Nothing of the handle's filters, inputs or logs changes. */
int msckf_hip_replay_calib_counts(msckf_hip_handle h, int f0, int f1, long long* out /*[B][8]*/);
/* ---- the track compiler: a recorded feature-id stream into the cells of the frame loops (host code, no device) -------- */
/* The frame loops take positional work-lists per frame, (M, slots, obs2, n_drop); a recording is an id stream, the tracked and
 * the new features of every image.  Without pruneRedundantStates the bookkeeping that turns one into the other -- update(),
 * addFeatures(), marginalize()'s feature_tracks_to_residualize_, pruneEmptyStates() (msckf.h:215-332, 336-371, 685-717) -- reads
 * ids and max_cam_states / min_track_length / max_track_length and nothing of the estimate, so a recording compiles once,
 * offline, with the same host code msckf_hip_image_cycle_range (flags = 2) runs per image: the cycle of the reference's live
 * node (ros_interface.cpp never prunes redundant states).  pruneRedundantStates cannot be compiled: it selects keyframes from
 * the ESTIMATED camera poses (msckf.h:1049-1098); a run with it stays on msckf_hip_image_cycle_range.
 * These four calls need no GPU and no handle and work on a machine without a GPU, as msckf_hip_last_error does.
 * -EINVAL for non-positive parameters, negative counts or null pointers with positive counts; -EEXIST when a new id is already
 * tracked ("added new feature that was already being tracked": the features before it stay added, as in the reference), after
 * which the compiler is unusable (-EIO, "the compiler is unusable after a refused image").  Every refusal leaves its text
 * with msckf_hip_last_error(). */
typedef struct msckf_hip_compiler_s* msckf_hip_compiler;
int msckf_hip_compile_create(int max_cam_states, int min_track_length, int max_track_length, msckf_hip_compiler* out);
int msckf_hip_compile_destroy(msckf_hip_compiler c);
/* one image = augmentState, update, addFeatures, marginalize's work-list, pruneEmptyStates.
 * out5 = F tracks, entries (sum M), n_drop, window after the augment (before the drop), tracks still live */
int msckf_hip_compile_image(msckf_hip_compiler c, const double* upd_meas2, const uint64_t* upd_ids, int upd_n,
                            const double* new_meas2, const uint64_t* new_ids, int new_n, int* out5);
/* the last image's work-list, in feature_tracks_to_residualize_ order; returns F, -E2BIG beyond the caps */
int msckf_hip_compile_cell(msckf_hip_compiler c, int* M, int* slots, double* obs2, uint64_t* ids, int cap_tracks, int cap_entries);
int msckf_hip_sync(msckf_hip_handle h);
/* ---- per-frame device log of msckf_hip_run_frames / _streamed (off by default) ------------------------ */
/* Storage for capacity_frames records ("frame log record" above) of every trajectory, in the handle's dtype; 0 frees the
 * log and disables it.  Any call drops the records written so far.  -ENOMEM when the allocation fails: the log is then off and
 * the handle as usable as before.  While the log is on, every frame of a run_frames / run_frames_streamed call ends with one
 * small extra launch per stream that copies the record out of the filter state -- it reads the state and writes only the log,
 * so the filter computes the same bits with and without it -- and a call over [f0, f1) writes the records
 * count .. count + (f1 - f0) - 1.  A call whose frames do not fit behind the records written returns -ENOSPC and runs nothing.
 * The log launch is outside the stage timers.  msckf_hip_copy_state does not copy the log. */
int msckf_hip_frame_log_enable(msckf_hip_handle h, int capacity_frames);
int msckf_hip_frame_log_reset(msckf_hip_handle h);   /* records written <- 0 (the storage stays) */
int msckf_hip_frame_log_count(msckf_hip_handle h);   /* records written; advances when a run_frames call has succeeded */
/* Records [r0, r0 + n) of trajectories [b0, b0 + nb) as doubles, out[n][nb][48]; waits for the handle's stream like the other
 * getters.  -EINVAL for a range beyond the records written, -EIO on a handle that a failed run_frames call left unusable. */
int msckf_hip_frame_log_read(msckf_hip_handle h, int r0, int n, int b0, int nb, double* out);
/* The records [r0, r1) against ground-truth positions gt_p[r1 - r0][B][3], reduced on the device: out[B][6] = per trajectory
 * the number of records, sum |e|^2, max |e|, |e| at record r1 - 1, sum e^T P_pp^-1 e (P_pp the logged position block, 3 x 3
 * Cholesky), and the number of records with an error flag set; e = p_I_G - gt_p, unaligned (the filters start from ground
 * truth).  Accumulated in double in a fixed order: the same log gives the same bits.  Sums and counts, so that ranks and
 * sequences combine by addition (ATE = sqrt(sum |e|^2 / n), mean NEES = sum / n). */
int msckf_hip_frame_log_metrics(msckf_hip_handle h, int r0, int r1, const double* gt_p, double* out);
/* The same with a record range per trajectory, [r0[b], r1[b]) (r0[B], r1[B]): sequences of unequal length set r1[b] to their
 * own frame count, so that the records of their skipped tail stay out.  gt_p[max(r1) - min(r0)][B][3] is indexed from
 * min(r0); "|e| at record r1 - 1" is at r1[b] - 1.  With every range equal: the bits of msckf_hip_frame_log_metrics. */
int msckf_hip_frame_log_metrics_ranges(msckf_hip_handle h, const int* r0, const int* r1, const double* gt_p, double* out);
/* ---- per-track device log of msckf_hip_run_frames / _streamed: the landmark map (off by default) ------- */
/* Storage for capacity_per_trajectory records ("map log record" above) of every trajectory, in the handle's dtype, and a
 * cursor per trajectory; 0 frees the log and disables it.  Any call drops the records held so far.  -ENOMEM when the allocation
 * fails: the log is then off and the handle as usable as before.  While the log is on, every frame of a run_frames /
 * run_frames_streamed call ends with one small extra launch per stream that appends the frame's logged tracks, in track order,
 * behind the trajectory's records -- it reads the filter's arrays and writes only the log, so the filter computes the same
 * bits with and without it.  A trajectory that finds more than its capacity keeps the first capacity_per_trajectory records
 * in (frame, track) order and goes on counting (msckf_hip_map_log_counts).  A skipped cell and a cell without tracks log
 * nothing; the frame ordinal advances all the same.  Only run_frames / run_frames_streamed write the log (the per-filter
 * entries and msckf_hip_image_cycle_range return their map through msckf_hip_get_map); msckf_hip_copy_state does not copy it. */
int msckf_hip_map_log_enable(msckf_hip_handle h, int capacity_per_trajectory);
int msckf_hip_map_log_reset(msckf_hip_handle h);    /* cursors and frame ordinal <- 0 (the storage stays) */
int msckf_hip_map_log_frames(msckf_hip_handle h);   /* frame ordinals handed out; advances when a run_frames call has succeeded */
/* Trajectories [b0, b0 + nb): found[i] records found, stored[i] = min(found[i], capacity) of them held; found > stored: the log
 * overflowed.  Waits for the handle's stream.  -EINVAL while the log is off. */
int msckf_hip_map_log_counts(msckf_hip_handle h, int b0, int nb, int* stored, int* found);
/* Stored records [r0, r0 + n) of trajectory b as doubles, out[n][8].  -EINVAL for a range beyond stored (and while the log is
 * off), -EIO on a handle that a failed run_frames call left unusable. */
int msckf_hip_map_log_read(msckf_hip_handle h, int b, int r0, int n, double* out);
/* The stored records with frame ordinal in [q0, q1) (0 <= q0 <= q1 <= msckf_hip_map_log_frames) reduced on the device.
 * Ground truth: gt_off[(q1 - q0) * B + 1] is CSR over the cells (frame - q0) * B + b, non-decreasing (else -EINVAL); the
 * landmark of a record is gt_xyz[gt_off[cell] + track][3].  gt_xyz and gt_off both null: no ground truth.
 * out[B][8] = per trajectory: 0 records in range, 1 records matched to ground truth, 2 sum |e|^2 and 3 max |e| over those
 * (e = p_f_G - landmark), 4 gate-passed records that do not carry flag 4, 5 sum of gamma and 6 sum of 2 M - 3 over those,
 * 7 records whose track index is >= their cell's CSR length (unmatched, left out of the error sums).  Accumulated in double
 * in a fixed order: the same log gives the same bits.  Sums and counts, so that ranks combine by addition; mean normalised
 * gate statistic = column 5 / column 6 (1 for a consistent filter). */
int msckf_hip_map_log_metrics(msckf_hip_handle h, int q0, int q1, const double* gt_xyz, const int* gt_off, double* out);
/* ---- pruned-state device log of msckf_hip_run_frames / _streamed: the smoothed camera poses (off by default) ------- */
/* Storage for capacity_per_trajectory records ("pruned-state log record" above) of every trajectory, in the handle's dtype, and
 * a cursor per trajectory; 0 frees the log and disables it.  Any call drops the records held so far.  -EINVAL for a negative
 * capacity, -ENOMEM when the allocation fails: the log is then off and the handle as usable as before.  While the log is on,
 * every frame of a run_frames / run_frames_streamed call prunes with its own launch (no prune rides on the covariance downdate:
 * one more launch per frame and stream than with the log off) and one small launch before it appends every camera state the
 * frame is about to drop (the cell's n_drop oldest), oldest first, behind the trajectory's records: what getPrunedStates()
 * (msckf.h:631, 714) keeps, with the posterior covariance block added.  It reads the filter's arrays and writes only the log,
 * and a prune of its own computes the bits of one that rides: the filter's results are the same with and without the log.
 * A trajectory that drops more than its capacity keeps the first capacity_per_trajectory records and goes on counting.  A
 * skipped cell and a cell that drops nothing log nothing; the frame ordinal advances all the same.  Only run_frames /
 * run_frames_streamed write the log; msckf_hip_copy_state does not copy it. */
int msckf_hip_pruned_log_enable(msckf_hip_handle h, int capacity_per_trajectory);
int msckf_hip_pruned_log_reset(msckf_hip_handle h);    /* cursors and frame ordinal <- 0 (the storage stays) */
int msckf_hip_pruned_log_frames(msckf_hip_handle h);   /* frame ordinals handed out; advances when a run_frames call has succeeded */
/* Trajectories [b0, b0 + nb): found[i] states dropped, stored[i] = min(found[i], capacity) of them held.  Waits for the handle's
 * stream.  -EINVAL while the log is off. */
int msckf_hip_pruned_log_counts(msckf_hip_handle h, int b0, int nb, int* stored, int* found);
/* Stored records [r0, r0 + n) of trajectory b as doubles, out[n][32], and aug_ord[n]: per record the ordinal of the frame whose
 * augmentState created the state (run_frames drops oldest-first, so the host keeps the window's ordinals in a queue), or -1
 * for a state that was in the window when the log was enabled or reset, or that another call than run_frames /
 * run_frames_streamed put there.  -EINVAL for a range beyond stored (and while the log is off), -EIO on a handle that a failed
 * run_frames call left unusable. */
int msckf_hip_pruned_log_read(msckf_hip_handle h, int b, int r0, int n, double* out, int* aug_ord);
/* The stored records with prune ordinal in [q0, q1) (0 <= q0 <= q1 <= msckf_hip_pruned_log_frames) against ground-truth camera
 * poses gt_pose[n_ord][B][7] (cam7 of the camera of frame ordinal o, trajectory b), reduced on the device.  A record is matched
 * through its augment ordinal; -1 or >= n_ord: unmatched.  n_ord < 0, or a null gt_pose with n_ord > 0: -EINVAL.
 * Pose error e = [e_th ; e_p]: e_p = p_C_G - p_gt; e_th is the error-state angle of the filter's own update (buildUpdateQuat,
 * msckf.h:851-872): q_CG = buildUpdateQuat(e_th) * q_gt, e_th = -2 vec(q_CG * q_gt^-1) with a non-negative scalar part.
 * out[B][10] = per trajectory: 0 records in range, 1 matched, 2 sum |e_p|^2, 3 max |e_p|, 4 sum |e_th|^2, 5 max |e_th|,
 * 6 sum e^T P6^-1 e over the matched records whose logged block has a Cholesky factor, 7 their number, 8 matched records with
 * a non-positive pivot (left out of 6), 9 unmatched.  Accumulated in double in a fixed order: the same log gives the same bits.
 * Sums and counts, so that ranks combine by addition: position ATE = sqrt(col 2 / col 1), mean NEES = col 6 / col 7 (6 for a
 * consistent filter). */
int msckf_hip_pruned_log_metrics(msckf_hip_handle h, int q0, int q1, const double* gt_pose, int n_ord, double* out);
/* ---- full-state NEES log of the frame loops, reduced per frame across trajectories (off by default) ------------------- */
/* The truth the NEES log is taken against, resident on the device: truth16[n_frames][n_rows][16] holds the first 16 entries of
 * imu29 (q_IG b_g v b_a p), the true state at the time of frame f's log record, in double; row_of[B] names each trajectory's
 * row in [0, n_rows) -- its sequence for a replay, itself for a plain scenario.  add_walk = 1: row f + 1 of the replay's walk
 * table (msckf_hip_replay_walk) is added to the true b_g and b_a of frame f; accepted only while a msckf_hip_replay_assign_q
 * assignment is in force and honoured only by msckf_hip_run_frames_replay.  n_frames = 0 frees the table.
 * -EINVAL: "truth table: row_of names no row of the table", "truth table: entry not finite", "truth table: quaternion norm off
 * by more than 1e-6", "truth table: add_walk needs an assignment through msckf_hip_replay_assign_q"; the table set before stays. */
int msckf_hip_truth_set(msckf_hip_handle h, int n_frames, int n_rows, const double* truth16, const int* row_of, int add_walk);
/* Storage for capacity_frames records ("NEES log record" above) of every trajectory, always doubles; 0 frees the log and
 * disables it.  Any call drops the records written so far.  -ENOMEM when the allocation fails: the log is then off and the
 * handle as usable as before.  A dense log like the frame log: while it is on, every frame of a run_frames / _streamed / _replay
 * call ends with one more small launch per stream, after the frame log's, that reads the state and the truth and writes only
 * the log -- the filter computes the same bits with and without it -- and a call over [f0, f1) writes the records count ..
 * count + (f1 - f0) - 1.  The head of such a call reserves the log fourth, after the frame, map and pruned-state logs, before
 * anything of its frames is enqueued: -EINVAL "NEES log on without a truth table", "the truth table does not cover the call's
 * frames", "the truth table adds the replay's walk, only msckf_hip_run_frames_replay honours it" (run_frames / _streamed),
 * -ENOSPC when the frames do not fit behind the records written; nothing was run.
 * The record: e_th is the error-state angle of the filter's own update (buildUpdateQuat, msckf.h:851-872), q_IG =
 * buildUpdateQuat(e_th) * q_IG*, e_th = -2 vec(q_IG * q_IG*^-1) with a non-negative scalar part, as msckf_hip_pruned_log_metrics
 * defines it for q_CG.  With D = diag P_II the correlation matrix C = D^-1/2 P_II D^-1/2 = L L^T is factored in double and
 * NEES = |L^-1 D^-1/2 e|^2; each 3 x 3 diagonal block of P_II gets a Cholesky factorisation of its own.  P_II's upper
 * triangle is read.  msckf_hip_copy_state copies neither the log nor the truth table. */
int msckf_hip_nees_log_enable(msckf_hip_handle h, int capacity_frames);
int msckf_hip_nees_log_reset(msckf_hip_handle h);   /* records written <- 0 (the storage stays) */
int msckf_hip_nees_log_count(msckf_hip_handle h);   /* records written; advances when a frame loop's call has succeeded */
/* Records [r0, r0 + n) of trajectories [b0, b0 + nb), out[n][nb][8]: one strided copy; waits for the handle's stream.
 * -EINVAL for a range beyond the records written, -EIO on a handle that a failed run_frames call left unusable. */
int msckf_hip_nees_log_read(msckf_hip_handle h, int r0, int n, int b0, int nb, double* out);
/* The records [r0, r1) reduced across trajectories on the device, per record and group: group_of[B] in [-1, n_groups) names a
 * trajectory's group (the seeds of one sequence), -1 leaves it out.  out[r1 - r0][n_groups][14] = 0 members with flags = 0,
 * 1 members left out for a flag, 2-7 the sums of columns 0-5 over the unflagged members, 8-13 the sums of their squares; an
 * empty group gives zeros.  Accumulated in a fixed order: the same log gives the same bits.  Sums and counts, so that ranks
 * combine by addition; ANEES = column 2 / column 0, consistent over n seeds when n ANEES lies between the chi-square(15 n)
 * quantiles the caller chooses.  -EINVAL "record range beyond the records written", "NEES ensemble: group_of outside
 * [-1, n_groups)", "NEES ensemble: at least one group". */
int msckf_hip_nees_log_ensemble(msckf_hip_handle h, int r0, int r1, const int* group_of, int n_groups, double* out);
/* ---- aligned trajectory error on the device: yaw and SE(3) ATE, and the relative pose error -------------------------- */
/* The frame log's records [r0, r1) against ground-truth poses gt_pose7[r1 - r0][B][7] (q_IG w x y z, then p; indexed from r0),
 * reduced on the device after an alignment g ~ R p + t of each trajectory's estimate p onto its ground truth g: mode 0 none
 * (R = I, t = 0), 1 a rotation about the global z axis (gravity is (0, 0, -9.81)) plus a translation -- the gauge of a VIO --,
 * 2 a rotation and a translation (SE(3)); no scale.  r0b / r1b (both NULL: [r0, r1) for every trajectory): the trajectory's own
 * range [r0b[b], r1b[b]) inside [r0, r1), as msckf_hip_frame_log_metrics_ranges takes it.
 * out[B][20] = per trajectory: 0 records n, 1-9 R row by row, 10-12 t, 13 cond, and over e = R p + t - g: 14 sum |e|^2, 15 max |e|,
 * 16 |e| at the last record; over the error-state angle e_th (msckf_hip_pruned_log_metrics defines it) of the aligned attitude
 * C(q_IG) R^T against the truth: 17 sum |e_th|^2, 18 max |e_th|; 19 sum |p - g|^2 before alignment (column 1 of
 * msckf_hip_frame_log_metrics).  Yaw: theta = atan2(W10 - W01, W00 + W11) of W = sum g_c p_c^T (_c: centred on its own mean),
 * cond = hypot(W10 - W01, W00 + W11) / sqrt(sum |p_c,xy|^2 sum |g_c,xy|^2).  SE(3): R from the eigenvector of largest
 * eigenvalue of Horn's 4 x 4 matrix (Jacobi, in double), always a proper rotation, cond = (l1 - l2) / l1.  cond lies in [0, 1];
 * 0: the data do not fix R -- n <= 1, no extent (yaw: no horizontal extent) give R = I; collinear points under SE(3) give one
 * of the minimisers.  t = mean g - R mean p.  The sums are centred in a pass of their own, not expanded from raw moments.
 * Accumulated in double in a fixed order: the same input gives the same bits.  Sums and counts, so that ranks, sequences and
 * seeds combine by addition (aligned ATE = sqrt(col 14 / col 0)).
 * -EINVAL, in this order: "null argument"; "record range beyond the records written"; "trajectory alignment: mode is ...";
 * "trajectory ranges: r0b and r1b, both or neither"; "trajectory ranges: a trajectory's range lies outside [r0, r1)";
 * "ground-truth poses: entry not finite"; "ground-truth poses: quaternion norm off by more than 1e-6".  -EIO on a handle that a
 * failed run_frames call left unusable.  Nothing of the handle's filters, inputs or logs changes. */
int msckf_hip_frame_log_align(msckf_hip_handle h, int r0, int r1, const int* r0b, const int* r1b, const double* gt_pose7, int mode, double* out);
/* The relative pose error of the same records over lags[n_lags] (1 <= n_lags <= 8, every lag >= 1 record), gauge-free: over
 * the pairs (r, r + lag) inside the trajectory's range, e_t = C(q_r) (p_{r+lag} - p_r) - C(g_r) (g_{r+lag} - g_r) (each
 * displacement in its own body frame at r) and e_th the error-state angle of q_{r+lag} * q_r^-1 against the truth's.
 * out[B][n_lags][4] = 0 pairs, 1 sum |e_t|^2, 2 sum |e_th|^2, 3 max |e_t|; a lag longer than the range gives zeros.
 * -EINVAL as above with "relative pose error: between 1 and 8 lags" / "... a lag is at least 1 record" in the mode's place. */
int msckf_hip_frame_log_rpe(msckf_hip_handle h, int r0, int r1, const int* r0b, const int* r1b, const double* gt_pose7, const int* lags, int n_lags, double* out);
/* The same two reductions on poses the caller hands over -- a pruned-state log's read-back, another run's outputs, a trajectory
 * from elsewhere: est_pose7 and gt_pose7 [n_rec][n_traj][7], r0b / r1b inside [0, n_rec) or both NULL, out[n_traj][20] and
 * out[n_traj][n_lags][4].  n_traj is free of the handle's B: the handle supplies the device and the stream.  -EINVAL "pose
 * arrays: n_rec >= 0 and n_traj >= 1 are needed" takes the place of the record range. */
int msckf_hip_traj_align(msckf_hip_handle h, int n_rec, int n_traj, const double* est_pose7, const double* gt_pose7, const int* r0b, const int* r1b, int mode, double* out);
int msckf_hip_traj_rpe(msckf_hip_handle h, int n_rec, int n_traj, const double* est_pose7, const double* gt_pose7, const int* r0b, const int* r1b, const int* lags, int n_lags, double* out);
/* HIP-event stage timing: enable, run, sync, then read accumulated milliseconds and launch counts for
 * stages 0 propagate, 1 augment, 2 k_feature, 3 compression A (k_gram | TSQR stage 1), 4 compression B
 * (k_chol_mfma | TSQR merge), 5 kalman, 6 prune, 7 k_select (information form: k_select_diag, which also reduces the
 * block-diagonal part of the Gram matrix).  (While profiling, run_frames launches propagate and
 * augmentState separately; otherwise they share one launch.) */
int msckf_hip_profile_enable(msckf_hip_handle h, int on);
int msckf_hip_profile_read(msckf_hip_handle h, double* ms8, int* count8);
/* The same with the stages beyond the first eight (cap >= 8 entries are written, unknown ones as zero): 8 k_lit_pre, 9 k_lit_gamma,
 * 10 k_literal -- the three launches of the literal anisotropic compression (u_var' != v_var', msckf.h:423-431, 1343-1366;
 * kernels_literal.hip), which a profiled run brackets one by one (stage 3 is then k_gram alone); 11 k_replay_expand, the
 * expansion launches of msckf_hip_run_frames_replay; 12 k_replay_walk_scan, the one-off scan of the Q_imu model's walk table. */
int msckf_hip_profile_read_ex(msckf_hip_handle h, double* ms, int* count, int cap);
/* Milliseconds an event pair with nothing between its two records reads on the handle's stream (mean of 64 pairs): every
 * stage timer above brackets its launches with such a pair, so a single-kernel stage reads the kernel's duration plus
 * this.  (The reference's StageTiming message, asl_msckf.cpp:229-296, is host wall-clock and has no such term.) */
int msckf_hip_profile_event_overhead(msckf_hip_handle h, double* ms);
/* run_frames on n = 1..8 HIP streams: the batch is cut into n slices of independent trajectories that run the
 * same kernel sequence concurrently (latency-bound stages of one slice overlap chip-filling stages of another).
 * n is an upper bound: slices whose streams share a hardware queue run one after the other, slower than a single slice, so
 * the handle runs as many slices as the process has queues for (msckf_hip_set_hw_queues), and the process's default stream
 * holds one of those: with 4 queues a request for 4 slices runs 2; with 8, 4.  Results do not depend on the count. */
int msckf_hip_set_streams(msckf_hip_handle h, int n);
/* The hardware queues the HIP runtime gives this process, 1..32: GPU_MAX_HW_QUEUES as the process started with, 4 (the
 * runtime's default and the handle's) where it was not set.  The library reads no variable of the runtime's and sets none:
 * the caller says what its process has.  msckf_hip_parse_hw_queues turns the variable's text into that number (null, empty
 * or no number: 4; a number is clamped to 1..32). */
int msckf_hip_set_hw_queues(msckf_hip_handle h, int n);
int msckf_hip_parse_hw_queues(const char* text);
/* on != 0: the frame loops run exactly the slices msckf_hip_set_streams asked for, whatever the queues (A/B runs). */
int msckf_hip_set_slices_exact(msckf_hip_handle h, int on);
/* The slices msckf_hip_run_frames (streamed == 0) or msckf_hip_run_frames_streamed (streamed != 0) would run now. */
int msckf_hip_get_effective_streams(msckf_hip_handle h, int streamed, int* out);
/* Host cores for the threads of msckf_hip_run_frames / _streamed: cpus[0] for the calling thread while it uploads frames
 * (restored on return), cpus[1 + i] for the enqueue thread of slice i.  The hand-overs between them are spin waits; without
 * this the threads run wherever the scheduler puts them (n = 0 clears the list).  One core each, ideally on the GPU's NUMA
 * node. */
int msckf_hip_set_host_affinity(msckf_hip_handle h, const int* cpus, int n);
/* Exact early accept of the chi-square gate (gatingTest, msckf.h:1103-1124), OFF by default: S = H_o P H_o^T + sigma^2 I
 * >= sigma^2 I, so gamma <= |r_o|^2 / sigma^2; when that bound is below half the threshold the track passes without
 * forming S.  Same decisions as the reference; the reported gamma of such a track is the bound (status bit 32). */
int msckf_hip_set_gate_early_accept(msckf_hip_handle h, int on);
/* Compression of the stacked Jacobian (HouseholderQR + Q_1^T r_o of measurementUpdate, msckf.h:1338-1366):
 * -1 default for the window size, 0 Householder TSQR (kernels_qr.hip), 3 information form: [T | r_n] = chol(H_o^T H_o),
 * accumulated in f64 on the matrix cores (kernels_gram.hip) and factored by the blocked matrix-core Cholesky k_chol_mfma
 * (kernels_chol.hip; the default; two levels for windows of more than 31 cameras, 6 n_cap + 1 > 192).  1 and 2 selected the
 * register-resident factorizations of rounds 1-2, which are gone: they are accepted and mean 3.  The information form needs
 * 6 n_cap + 1 <= 384 and f_cap <= 1024 (-ENOTSUP otherwise).  Both routes give the reference's update (tests keep them
 * together). */
int msckf_hip_set_compression(msckf_hip_handle h, int route);
/* Covariance update of measurementUpdate (msckf.h:1368-1418): 0 (default) the square-root gain form -- S = L L^T,
 * W = P T_H^T L^-T, dx = W L^-1 r_n, P <- P - W W^T (= (I - K T_H) P, written symmetrically); 1 the reference's literal
 * Joseph sequence K, (I - K T_H) P (I - K T_H)^T + K R_n K^T, symmetrise; 2 the square-root gain form with the
 * register-resident solve of round 1 instead of the blocked matrix-core one.  Identical in exact arithmetic, equal to
 * rounding in the tests. */
int msckf_hip_set_covariance_update(msckf_hip_handle h, int form);
/* run_frames: launch a frame's per-track kernel on a side stream concurrently with the same frame's propagate + augmentState
 * whenever no track of the frame observes the camera that augmentState adds (it then depends only on what the previous
 * frame left behind).  Bit-identical results; OFF by default -- on MI355X at the benchmark configuration the per-track
 * kernel starves the latency-bound propagate/augment workgroups of CUs (100 k -> 82 k updates/s). */
int msckf_hip_set_feature_overlap(msckf_hip_handle h, int on);
/* run_frames (resident, streamed and replay inputs): the order of a frame's first launches.  1 (default): on a frame where
 * no track of the slice observes the camera state that augmentState adds, every window of the slice has room for it and no
 * cell is skipped, the per-track kernel runs FIRST, from what the previous frame's prune left, and the track selection shares
 * ONE launch with propagate + augmentState on the slice's own stream -- one launch less on the frame's latency chain.  Float
 * handles on the information-form route; never the first frame of a call, never while the stage profile is on; every other
 * frame, and every frame of a double handle, takes order 0: propagate + augmentState, per-track kernel, selection.
 * Bit-identical results either way.  -EINVAL for any other value.
 * msckf_hip_get_frame_order_count: how many frames took order 1 since the handle was created, counted once per slice
 * (msckf_hip_set_streams) and frame.
 * msckf_hip_set_frame_order_chol (on by default; it acts under order 1 only): "order 2".  Where a frame that takes order 1 runs
 * the kernel chain with a one-level Gram Cholesky (information form, windows up to 31 cameras; no trajectory of the slice in the
 * one-launch update of short windows, none of the batch on the literal anisotropic route) the selection keeps a launch of its own
 * and propagate + augmentState run inside the Gram Cholesky's launch, on compute units the factorization leaves idle -- off the
 * frame's latency chain altogether.  A frame that cannot takes order 1 as described above.  Bit-identical results either way.
 * (A switch of its own and not a value 2 of msckf_hip_set_frame_order, which keeps refusing every value but 0 and 1.)
 * msckf_hip_get_frame_order_chol_count: those of msckf_hip_get_frame_order_count's frames that took order 2. */
int msckf_hip_set_frame_order(msckf_hip_handle h, int order);
int msckf_hip_get_frame_order_count(msckf_hip_handle h, long long* count);
int msckf_hip_set_frame_order_chol(msckf_hip_handle h, int on);
int msckf_hip_get_frame_order_chol_count(msckf_hip_handle h, long long* count);
/* Anisotropic pixel noise, u_var_prime != v_var_prime (see the header comment): mode 0 (default) the reference's
 * R_o_j = A_j^T R_j A_j / HouseholderQR in column order / R_n = Q_1^T R_o Q_1 on the device (msckf.h:423-431, 1343-1366;
 * f64: the Householder sweep for its decisions, the result as a projection onto range(Q_1), kernels_literal.hip), handed to the
 * update as the information matrix [T_H | r_n]^T R_n^-1 [T_H | r_n]; mode 1 rows pre-whitened by 1/sigma (generalized least squares).  tail_tol: zero-tail tolerance of mode 0, < 0 = default (1e-10 double, 8e-4 float), 0 = the reference's
 * rule to the letter.  Applies to every trajectory of the handle, initialized or not.  -ENOMEM when the work space does not fit
 * (per trajectory about sixteen (6 n_cap)^2 matrices of doubles, the (2 * 6 n_cap + 16)^2 elimination matrix, and per TRACK six rows of
 * ldR doubles -- f_cap * 6 * ldR * 8 bytes, 1.8 MB at 200 tracks and a 30-camera window); -ENOTSUP on a device that does not grant
 * the route's kernels their 94 KB of LDS per workgroup (gfx950 does). */
int msckf_hip_set_anisotropic_noise(msckf_hip_handle h, int mode, double tail_tol);
/* last marginalize of trajectory b on the literal route: out[0..5] = stacked rows m, kept rows r of R (msckf.h:1347),
 * Householder steps that reflected, steps whose non-zero tail fell under tail_tol, route taken (3: the sequence of steps on
 * the compressed representation -- first 15 + 6N rows explicit, the rest through their Gram matrix; 2: the sweep over the
 * dense stack, environment MSCKF_HIP_LITERAL_ROUTE=1 at create time), leading steps that meet the zero IMU columns (15),
 * kept rows that a dependent column handed through in the middle of the sweep (route 3); out[7] reserved. */
int msckf_hip_literal_info(msckf_hip_handle h, int b, int* out8);

#ifdef __cplusplus
}
#endif
#endif
