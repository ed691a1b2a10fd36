"""ctypes binding of libmsckf_hip.so (the C-ABI declared in include/msckf_hip.h).

Product path: this module never imports anything from oracle/ and has no CPU fallback -- if the HIP
library cannot be loaded, or no GPU is visible, it raises.  `torch` (when installed) is imported first so
that the process ends up with ONE HIP runtime (torch bundles its own libamdhip64.so with the same soname).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MSCKF_HIP_LIB", os.path.join(_HERE, "libmsckf_hip.so"))   # override: A/B experiments only
_LIB = None

F32, F64, F16H = 0, 1, 2   # F16H: fp16 measurement Jacobian / f32 state + covariance (MSCKF_HIP_F16H_F32P)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_up = C.POINTER(C.c_uint64)

# every symbol include/msckf_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "msckf_hip_create", "msckf_hip_destroy", "msckf_hip_last_error", "msckf_hip_initialize", "msckf_hip_initialize_full", "msckf_hip_propagate",
    "msckf_hip_augment_state", "msckf_hip_update", "msckf_hip_add_features", "msckf_hip_marginalize",
    "msckf_hip_prune_empty_states", "msckf_hip_prune_redundant_states", "msckf_hip_finish",
    "msckf_hip_get_num_cam_states", "msckf_hip_get_imu_state", "msckf_hip_get_cam_states", "msckf_hip_get_map",
    "msckf_hip_get_pruned_state_ids", "msckf_hip_get_covariance", "msckf_hip_set_covariance", "msckf_hip_set_imu_state",
    "msckf_hip_set_cam_pose", "msckf_hip_get_num_residualized", "msckf_hip_set_num_residualized", "msckf_hip_last_stats",
    "msckf_hip_last_tracks", "msckf_hip_last_deltax", "msckf_hip_set_tracks", "msckf_hip_propagate_range",
    "msckf_hip_augment_range", "msckf_hip_marginalize_range", "msckf_hip_drop_oldest_range", "msckf_hip_scenario_alloc",
    "msckf_hip_scenario_set", "msckf_hip_scenario_commit", "msckf_hip_run_frames", "msckf_hip_run_frames_streamed", "msckf_hip_sync",
    "msckf_hip_profile_enable", "msckf_hip_profile_read", "msckf_hip_profile_read_ex", "msckf_hip_profile_event_overhead", "msckf_hip_set_streams", "msckf_hip_set_gate_early_accept",
    "msckf_hip_scenario_pin", "msckf_hip_set_upload_ring", "msckf_hip_clear_error_flags",
    "msckf_hip_set_compression", "msckf_hip_set_covariance_update", "msckf_hip_set_feature_overlap", "msckf_hip_get_pruned_states", "msckf_hip_get_cam_meta", "msckf_hip_get_tracked_feature_ids",
    "msckf_hip_set_anisotropic_noise", "msckf_hip_literal_info", "msckf_hip_get_error_flags", "msckf_hip_copy_state", "msckf_hip_set_host_affinity",
    "msckf_hip_image_cycle_range", "msckf_hip_get_effective_streams", "msckf_hip_set_hw_queues", "msckf_hip_parse_hw_queues", "msckf_hip_set_slices_exact",
    "msckf_hip_frame_log_enable", "msckf_hip_frame_log_reset", "msckf_hip_frame_log_count", "msckf_hip_frame_log_read", "msckf_hip_frame_log_metrics",
    "msckf_hip_scenario_set_cell", "msckf_hip_propagate_range_counts", "msckf_hip_frame_log_metrics_ranges",
    "msckf_hip_map_log_enable", "msckf_hip_map_log_reset", "msckf_hip_map_log_frames", "msckf_hip_map_log_counts", "msckf_hip_map_log_read", "msckf_hip_map_log_metrics",
    "msckf_hip_pruned_log_enable", "msckf_hip_pruned_log_reset", "msckf_hip_pruned_log_frames", "msckf_hip_pruned_log_counts", "msckf_hip_pruned_log_read", "msckf_hip_pruned_log_metrics",
    "msckf_hip_replay_alloc", "msckf_hip_replay_set_cell", "msckf_hip_replay_assign", "msckf_hip_replay_commit", "msckf_hip_run_frames_replay", "msckf_hip_replay_expand",
    "msckf_hip_replay_expand_ints", "msckf_hip_replay_assign_q", "msckf_hip_replay_walk", "msckf_hip_last_track_blocks",
    "msckf_hip_replay_set_faults", "msckf_hip_replay_expand_faults", "msckf_hip_replay_fault_counts", "msckf_hip_map_log_fault_metrics",
    "msckf_hip_replay_set_timing", "msckf_hip_replay_image_table", "msckf_hip_replay_expand_timing",
    "msckf_hip_set_frame_order", "msckf_hip_get_frame_order_count", "msckf_hip_set_frame_order_chol", "msckf_hip_get_frame_order_chol_count",
    "msckf_hip_truth_set", "msckf_hip_nees_log_enable", "msckf_hip_nees_log_reset", "msckf_hip_nees_log_count", "msckf_hip_nees_log_read", "msckf_hip_nees_log_ensemble",
    "msckf_hip_frame_log_align", "msckf_hip_frame_log_rpe", "msckf_hip_traj_align", "msckf_hip_traj_rpe",
    "msckf_hip_compile_create", "msckf_hip_compile_destroy", "msckf_hip_compile_image", "msckf_hip_compile_cell", "msckf_hip_replay_imu_sums",
    "msckf_hip_replay_set_imu_calib", "msckf_hip_replay_set_cam_calib", "msckf_hip_replay_expand_calib", "msckf_hip_replay_calib_counts",
]
CELL_SKIP = 1   # msckf_hip_scenario_set_cell's flag bit MSCKF_HIP_CELL_SKIP

# fields of a frame-log record (include/msckf_hip.h, "frame log record"): name -> slice of its 48 scalars
FRAME_LOG_STRIDE = 48
FRAME_LOG_FIELDS = {
    "q": slice(0, 4), "b_g": slice(4, 7), "v": slice(7, 10), "b_a": slice(10, 13), "p": slice(13, 16),
    "P_II_diag": slice(16, 31), "P_pp": slice(31, 37),          # P_pp: xx xy xz yy yz zz
    "n_cam": slice(37, 38), "n_tracks": slice(38, 39), "n_passed": slice(39, 40), "error_flags": slice(40, 41),
    "cam0": slice(41, 48),                                        # q_CG p_C_G of camera slot 0
}
# columns of frame_log_metrics' result
FRAME_LOG_METRICS = ("n", "sum_sq_err", "max_err", "final_err", "sum_nees", "n_flagged")
# fields of a map-log record (include/msckf_hip.h, "map log record"): name -> slice of its 8 scalars
MAP_LOG_STRIDE = 8
MAP_LOG_FIELDS = {"p": slice(0, 3), "gamma": slice(3, 4), "frame": slice(4, 5), "track": slice(5, 6), "flags": slice(6, 7), "M": slice(7, 8)}
MAP_FLAG_PASS, MAP_FLAG_INCLUDED, MAP_FLAG_BOUND = 1, 2, 4   # bits of "flags": gate passed, included in the update, gamma is the early-accept bound
# columns of map_log_metrics' result
MAP_LOG_METRICS = ("n", "n_matched", "sum_sq_err", "max_err", "n_gated", "sum_gamma", "sum_dof", "n_unmatched")
# columns of replay_fault_counts' and of map_log_fault_metrics' result, and replay_expand_faults' codes
REPLAY_FAULT_COUNTS = ("entries", "missed", "outliers", "tracks", "tracks_shortened", "tracks_contaminated")
MAP_LOG_FAULT_METRICS = ("n", "clean_passed", "clean_rejected", "contaminated_passed", "contaminated_rejected", "sum_gamma", "sum_dof", "n_unmatched")
FAULT_KEPT, FAULT_OUTLIER, FAULT_MISSED = 0, 1, 2
# fields of a pruned-state log record (include/msckf_hip.h, "pruned-state log record"): name -> slice of its 32 scalars
PRUNED_LOG_STRIDE = 32
PRUNED_LOG_FIELDS = {"q": slice(0, 4), "p": slice(4, 7), "frame": slice(7, 8), "cov": slice(8, 29),   # cov: upper triangle of the 6 x 6 block, row by row
                     "n_cam": slice(29, 30), "k": slice(30, 31), "pad": slice(31, 32)}
# columns of pruned_log_metrics' result
PRUNED_LOG_METRICS = ("n", "n_matched", "sum_sq_pos_err", "max_pos_err", "sum_sq_ang_err", "max_ang_err", "sum_nees", "n_nees", "n_bad_pivot", "n_unmatched")
# fields of a NEES log record (include/msckf_hip.h, "NEES log record"): name -> slice of its 8 doubles
NEES_LOG_STRIDE = 8
NEES_LOG_FIELDS = {"nees": slice(0, 1), "nees_theta": slice(1, 2), "nees_b_g": slice(2, 3), "nees_v": slice(3, 4), "nees_b_a": slice(4, 5),
                   "nees_p": slice(5, 6), "frame": slice(6, 7), "flags": slice(7, 8)}
NEES_FLAG_NOT_PD, NEES_FLAG_SKIPPED, NEES_FLAG_STAT_ERR = 1, 2, 4   # bits of "flags"
# columns of nees_log_ensemble's sums, per (record, group); the six of each run over NEES_LOG_FIELDS' first six
NEES_ENSEMBLE_STRIDE = 14
NEES_ENSEMBLE_FIELDS = {"n": slice(0, 1), "n_flagged": slice(1, 2), "sum": slice(2, 8), "sum_sq": slice(8, 14)}
# the aligned trajectory error (csrc/traj_plan.h): the modes, and the columns of an alignment row and of an RPE row
ALIGN_NONE, ALIGN_YAW, ALIGN_SE3 = 0, 1, 2
ALIGN_STRIDE = 20
ALIGN_FIELDS = {"n": slice(0, 1), "R": slice(1, 10), "t": slice(10, 13), "cond": slice(13, 14), "sum_sq_err": slice(14, 15), "max_err": slice(15, 16),
                "final_err": slice(16, 17), "sum_sq_ang_err": slice(17, 18), "max_ang_err": slice(18, 19), "sum_sq_err_unaligned": slice(19, 20)}
RPE_STRIDE = 4
RPE_MAX_LAGS = 8
RPE_FIELDS = {"n_pairs": slice(0, 1), "sum_sq_trans_err": slice(1, 2), "sum_sq_ang_err": slice(2, 3), "max_trans_err": slice(3, 4)}
# columns of replay_imu_sums' result (csrc/replay_plan.h, ImuSum)
IMU_SUM_STRIDE = 8
IMU_SUM_FIELDS = {"n": slice(0, 1), "omega": slice(1, 4), "a": slice(4, 7), "dT": slice(7, 8)}


def build():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(_HERE, "csrc")])


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libmsckf_hip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        try:
            import torch  # noqa: F401  (one HIP runtime per process)
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        L.msckf_hip_last_error.restype = C.c_char_p
        _LIB = L
    return _LIB


class HipError(RuntimeError):
    pass


def _chk(rc):
    if rc < 0:
        raise HipError("msckf_hip call failed (%d): %s" % (rc, lib().msckf_hip_last_error().decode()))
    return rc


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _i(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def pack_config(cfg):
    cam = np.array([cfg["c_u"], cfg["c_v"], cfg["f_u"], cfg["f_v"], cfg.get("b", 0.0)] + list(cfg["q_CI"]) + list(cfg["p_C_I"]), dtype=np.float64)
    noise = np.array([cfg["u_var_prime"], cfg["v_var_prime"]] + list(cfg["Q_imu_diag"]) + list(cfg["P0_diag"]), dtype=np.float64)
    params = np.array([cfg["max_gn_cost_norm"], cfg.get("min_rcond", 3e-12), cfg["translation_threshold"],
                       cfg.get("redundancy_angle_thresh", 0.005), cfg.get("redundancy_distance_thresh", 0.05),
                       cfg["min_track_length"], cfg["max_track_length"], cfg["max_cam_states"]], dtype=np.float64)
    return cam, noise, params


def full_noise(cfg):
    """(Q_imu 12 x 12, initial_imu_covar 15 x 15) of a config that carries "Q_imu" and/or "P0" (a missing one is the diagonal
    matrix of "Q_imu_diag" / "P0_diag"), or None for a config with neither: msckf_hip_initialize_full's matrices."""
    if "Q_imu" not in cfg and "P0" not in cfg:
        return None
    Q = np.asarray(cfg["Q_imu"], dtype=np.float64) if "Q_imu" in cfg else np.diag(np.asarray(cfg["Q_imu_diag"], dtype=np.float64))
    P0 = np.asarray(cfg["P0"], dtype=np.float64) if "P0" in cfg else np.diag(np.asarray(cfg["P0_diag"], dtype=np.float64))
    if Q.shape != (12, 12) or P0.shape != (15, 15):
        raise ValueError("Q_imu must be 12 x 12 and P0 15 x 15")
    return Q, P0


class Batch:
    """A batch of B independent filters resident on one GPU."""
    _replay_K = 0   # K of the last replay_alloc
    _replay_frames = 0   # its frames

    def __init__(self, B, n_cap, f_cap, m_cap, dtype=F32, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.B, self.n_cap, self.f_cap, self.m_cap, self.dtype = B, n_cap, f_cap, m_cap, dtype
        _chk(self.L.msckf_hip_create(B, n_cap, f_cap, m_cap, dtype, device, C.byref(self.h)))
        # the hardware queues of this process, for the slice policy (csrc/slice_policy.h): the native library reads no variable
        # of the runtime's, so its caller passes on what the runtime found when the process started
        # (a library from before the policy, given through MSCKF_HIP_LIB for an A/B run, has no such entry)
        if hasattr(self.L, "msckf_hip_set_hw_queues"):
            text = os.environ.get("GPU_MAX_HW_QUEUES")
            self.set_hw_queues(self.L.msckf_hip_parse_hw_queues(None if text is None else text.encode()))

    def close(self):
        if self.h:
            self.L.msckf_hip_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- reference API, per trajectory
    def initialize(self, b, cfg, imu29):
        """MSCKF::initialize; a config with "Q_imu" (12 x 12) and/or "P0" (15 x 15) goes through msckf_hip_initialize_full"""
        cam, noise, params = pack_config(cfg)
        a, pa = _d(cam); p, pp = _d(params); s, ps = _d(imu29)
        fn = full_noise(cfg)
        if fn is None:
            n, pn = _d(noise)
            _chk(self.L.msckf_hip_initialize(self.h, b, pa, pn, pp, ps))
            return
        uv, puv = _d(noise[:2])
        Q, pq = _d(np.asfortranarray(fn[0]).ravel(order="F")); P0, pp0 = _d(np.asfortranarray(fn[1]).ravel(order="F"))
        _chk(self.L.msckf_hip_initialize_full(self.h, b, pa, puv, pq, pp0, pp, ps))

    def propagate(self, b, readings):
        r, p = _d(np.asarray(readings).reshape(-1, 7))
        _chk(self.L.msckf_hip_propagate(self.h, b, p, r.shape[0]))

    def augment_state(self, b, state_id, time=0.0):
        _chk(self.L.msckf_hip_augment_state(self.h, b, int(state_id), C.c_double(time)))

    def update(self, b, meas, ids):
        m, pm = _d(np.asarray(meas).reshape(-1, 2)); i = np.ascontiguousarray(ids, dtype=np.uint64)
        _chk(self.L.msckf_hip_update(self.h, b, pm, i.ctypes.data_as(_up), len(i)))

    def add_features(self, b, meas, ids):
        m, pm = _d(np.asarray(meas).reshape(-1, 2)); i = np.ascontiguousarray(ids, dtype=np.uint64)
        _chk(self.L.msckf_hip_add_features(self.h, b, pm, i.ctypes.data_as(_up), len(i)))

    def marginalize(self, b):
        _chk(self.L.msckf_hip_marginalize(self.h, b))

    def prune_empty_states(self, b):
        _chk(self.L.msckf_hip_prune_empty_states(self.h, b))

    def prune_redundant_states(self, b):
        _chk(self.L.msckf_hip_prune_redundant_states(self.h, b))

    def finish(self, b):
        _chk(self.L.msckf_hip_finish(self.h, b))

    def num_cam_states(self, b):
        return _chk(self.L.msckf_hip_get_num_cam_states(self.h, b))

    def imu_state(self, b):
        o = np.zeros(29); _chk(self.L.msckf_hip_get_imu_state(self.h, b, o.ctypes.data_as(_dp))); return o

    def cam_states(self, b):
        o = np.zeros((self.n_cap, 7)); ids = np.zeros(self.n_cap, dtype=np.int32)
        n = _chk(self.L.msckf_hip_get_cam_states(self.h, b, o.ctypes.data_as(_dp), ids.ctypes.data_as(_ip), self.n_cap))
        return o[:n], ids[:n]

    def get_map(self, b):
        o = np.zeros((self.f_cap, 3)); n = _chk(self.L.msckf_hip_get_map(self.h, b, o.ctypes.data_as(_dp), self.f_cap)); return o[:n]

    def pruned_state_ids(self, b, cap=65536):
        o = np.zeros(cap, dtype=np.int32); n = _chk(self.L.msckf_hip_get_pruned_state_ids(self.h, b, o.ctypes.data_as(_ip), cap)); return o[:n]

    def pruned_states(self, b):
        """getPrunedStates() in full: rows of q_CG(4) p_C_G(3) time state_id last_correlated_id, sorted by state_id"""
        n = _chk(self.L.msckf_hip_get_pruned_states(self.h, b, None, None, None, None, 1 << 30))
        c = np.zeros((max(n, 1), 7)); t = np.zeros(max(n, 1)); ids = np.zeros(max(n, 1), dtype=np.int32); lc = np.zeros(max(n, 1), dtype=np.int32)
        n = _chk(self.L.msckf_hip_get_pruned_states(self.h, b, c.ctypes.data_as(_dp), t.ctypes.data_as(_dp), ids.ctypes.data_as(_ip), lc.ctypes.data_as(_ip), n))
        return np.concatenate([c[:n], t[:n, None], ids[:n, None].astype(np.float64), lc[:n, None].astype(np.float64)], 1)

    def cam_meta(self, b):
        """(time, len(tracked_feature_ids), last_correlated_id) per entry of getCamStates() (types.h:57-67)"""
        t = np.zeros(self.n_cap); k = np.zeros(self.n_cap, dtype=np.int32); lc = np.zeros(self.n_cap, dtype=np.int32)
        n = _chk(self.L.msckf_hip_get_cam_meta(self.h, b, t.ctypes.data_as(_dp), k.ctypes.data_as(_ip), lc.ctypes.data_as(_ip), self.n_cap))
        return t[:n], k[:n], lc[:n]

    def tracked_feature_ids(self, b, cam_index, cap=4096):
        o = np.zeros(cap, dtype=np.uint64)
        n = _chk(self.L.msckf_hip_get_tracked_feature_ids(self.h, b, int(cam_index), o.ctypes.data_as(_up), cap))
        return o[:n]

    # ---- additive accessors
    def covariance(self, b):
        D = 15 + 6 * self.num_cam_states(b)
        P = np.zeros((D, D), order="F")
        _chk(self.L.msckf_hip_get_covariance(self.h, b, P.ctypes.data_as(_dp), D))
        return np.array(P)

    def set_covariance(self, b, P):
        P = np.asfortranarray(P, dtype=np.float64)
        _chk(self.L.msckf_hip_set_covariance(self.h, b, P.ctypes.data_as(_dp), P.shape[0]))

    def set_imu_state(self, b, s):
        a, p = _d(s); _chk(self.L.msckf_hip_set_imu_state(self.h, b, p))

    def set_cam_pose(self, b, slot, qp):
        a, p = _d(qp); _chk(self.L.msckf_hip_set_cam_pose(self.h, b, int(slot), p))

    def num_residualized(self, b):
        n = C.c_longlong(0); _chk(self.L.msckf_hip_get_num_residualized(self.h, b, C.byref(n))); return n.value

    def set_num_residualized(self, b, n):
        _chk(self.L.msckf_hip_set_num_residualized(self.h, b, C.c_longlong(int(n))))

    def last_stats(self, b, strict=True):
        """strict: a sticky device-side error flag of the trajectory raises (msckf_hip_last_stats returns its code); otherwise the
        statistics come back either way with the flag bits under "error_flags" (a poll over many trajectories must not lose
        the numbers because one of them once clamped a pivot)"""
        o = np.zeros(7, dtype=np.int32)
        rc = self.L.msckf_hip_last_stats(self.h, b, o.ctypes.data_as(_ip))
        d = dict(zip(["n_tracks", "n_motion_rejected", "n_tri_rejected", "n_gate_rejected", "n_passed", "m_rows", "r_rows"], o.tolist()))
        if strict:
            _chk(rc)
            return d
        d["error_flags"] = self.error_flags(b)
        if rc < 0 and not d["error_flags"]:
            _chk(rc)
        return d

    def copy_state_from(self, other):
        _chk(self.L.msckf_hip_copy_state(self.h, other.h))

    def error_flags(self, b):
        """the trajectory's sticky device-side flags: bit 0 (1) camera-state capacity exceeded, bit 1 (2) a factorization of
        S = T_H P T_H^T + R_n met a non-positive pivot.  The pivot contract (include/msckf_hip.h, msckf_hip_last_stats): the flag is per
        trajectory, sticky until clear_error_flags, and raised by every covariance-update form, compression route and dtype; the
        other trajectories are unaffected bit for bit; the failed trajectory's state and covariance are undefined until they are
        overwritten or the trajectory is re-initialised; the handle is otherwise reusable after clear_error_flags."""
        f = C.c_int(0)
        _chk(self.L.msckf_hip_get_error_flags(self.h, int(b), C.byref(f)))
        return int(f.value)

    def last_tracks(self, b):
        o = np.zeros((self.f_cap, 8)); n = _chk(self.L.msckf_hip_last_tracks(self.h, b, o.ctypes.data_as(_dp), self.f_cap)); return o[:n]

    def last_track_blocks(self, b):
        """per track of the last marginalize, as the feature kernels stored it for the information form: dict of first [F], last [F]
        (camera slots), Hx [F][m_cap][2][6], rw [F][m_cap][2], B [F][3][6 n_cap + 1] (stale where a track has no observation / slot).
        On an F16H handle Hx is the stored fp16 blocks, widened: every entry is exactly a binary16 value.  -ENOTSUP only on handles
        without the information form."""
        F, m, nc = self.f_cap, self.m_cap, 6 * self.n_cap + 1
        first, Hx, rw, Bh = np.zeros(F, np.int32), np.zeros((F, m, 2, 6)), np.zeros((F, m, 2)), np.zeros((F, 3, nc))
        n = _chk(self.L.msckf_hip_last_track_blocks(self.h, int(b), first.ctypes.data_as(_ip), Hx.ctypes.data_as(_dp), rw.ctypes.data_as(_dp),
                                                    Bh.ctypes.data_as(_dp), F))
        return dict(first=first[:n] & 255, last=first[:n] >> 8, Hx=Hx[:n], rw=rw[:n], B=Bh[:n])

    def last_deltax(self, b):
        cap = 15 + 6 * self.n_cap
        o = np.zeros(cap); n = _chk(self.L.msckf_hip_last_deltax(self.h, b, o.ctypes.data_as(_dp), cap)); return o[:n]

    # ---- batched path
    def set_tracks(self, b, M, slots, obs):
        Ma, pM = _i(M); s, ps = _i(slots); o, po = _d(obs)
        _chk(self.L.msckf_hip_set_tracks(self.h, b, len(Ma), pM, ps, po))

    def propagate_range(self, b0, nb, readings):
        r, p = _d(np.asarray(readings).reshape(nb, -1, 7))
        _chk(self.L.msckf_hip_propagate_range(self.h, b0, nb, p, r.shape[1]))

    def propagate_range_counts(self, b0, nb, readings):
        """propagate_range with a sample count per trajectory: readings[i] is the [K_i][7] array of trajectory b0 + i (K_i = 0:
        the trajectory is not touched)"""
        rs = [np.asarray(r, dtype=np.float64).reshape(-1, 7) for r in readings]
        if len(rs) != nb:
            raise ValueError("one array of readings per trajectory of the range")
        K, pK = _i([len(r) for r in rs])
        r, p = _d(np.concatenate(rs) if nb else np.zeros((0, 7)))
        _chk(self.L.msckf_hip_propagate_range_counts(self.h, b0, nb, p, pK))

    def augment_range(self, b0, nb):
        _chk(self.L.msckf_hip_augment_range(self.h, b0, nb))

    def marginalize_range(self, b0, nb):
        _chk(self.L.msckf_hip_marginalize_range(self.h, b0, nb))

    def drop_oldest_range(self, b0, nb, n):
        _chk(self.L.msckf_hip_drop_oldest_range(self.h, b0, nb, int(n)))

    def image_cycle_range(self, b0, nb, state_ids, times, cur, new, prune_redundant=True, prune_empty=True):
        """The ASL runner's per-image cycle (asl_msckf.cpp:269-294) for trajectories b0 .. b0 + nb - 1 in lockstep:
        augmentState, update, addFeatures, marginalize, [pruneRedundantStates], [pruneEmptyStates].
        cur[i] / new[i] = (measurements [n][2], feature ids [n]) of trajectory b0 + i, as update() / addFeatures() take them."""
        self.image_cycle_range_packed(b0, nb, self.pack_image_inputs(nb, state_ids, times, cur, new), prune_redundant, prune_empty)

    @staticmethod
    def pack_image_inputs(nb, state_ids, times, cur, new):
        """the arguments of msckf_hip_image_cycle_range as contiguous arrays (a caller that replays images converts once, outside its loop)"""
        def cat(parts):
            n = np.array([len(p[1]) for p in parts], dtype=np.int32)
            m = np.concatenate([np.asarray(p[0], dtype=np.float64).reshape(-1, 2) for p in parts]) if n.sum() else np.zeros((0, 2))
            i = np.concatenate([np.asarray(p[1], dtype=np.uint64).reshape(-1) for p in parts]) if n.sum() else np.zeros(0, dtype=np.uint64)
            return np.ascontiguousarray(m, dtype=np.float64), np.ascontiguousarray(i, dtype=np.uint64), n
        return (np.ascontiguousarray(np.asarray(state_ids).reshape(nb), dtype=np.int32), np.ascontiguousarray(np.asarray(times, dtype=np.float64).reshape(nb))) + cat(cur) + cat(new)

    def image_cycle_range_packed(self, b0, nb, packed, prune_redundant=True, prune_empty=True):
        sid, tt, um, ui, un, nm, ni, nn = packed
        _chk(self.L.msckf_hip_image_cycle_range(self.h, b0, nb, sid.ctypes.data_as(_ip), tt.ctypes.data_as(_dp), um.ctypes.data_as(_dp), ui.ctypes.data_as(_up), un.ctypes.data_as(_ip),
                                                nm.ctypes.data_as(_dp), ni.ctypes.data_as(_up), nn.ctypes.data_as(_ip),
                                                (1 if prune_redundant else 0) | (2 if prune_empty else 0)))

    def scenario_alloc(self, n_frames, K):
        _chk(self.L.msckf_hip_scenario_alloc(self.h, n_frames, K))

    def scenario_set(self, frame, b, readings, M, slots, obs, n_drop, skip=False):
        """one (frame, trajectory) cell: its own len(readings) IMU samples (0 .. K of scenario_alloc), its work-list, its drop.
        skip: the trajectory's sequence has no image on this frame (no readings, tracks or drop) -- nothing of it changes"""
        r, pr = _d(np.asarray(readings, dtype=np.float64).reshape(-1, 7)); Ma, pM = _i(M); s, ps = _i(slots); o, po = _d(obs)
        _chk(self.L.msckf_hip_scenario_set_cell(self.h, frame, b, pr, r.shape[0], len(Ma), pM, ps, po, int(n_drop), CELL_SKIP if skip else 0))

    def scenario_commit(self):
        _chk(self.L.msckf_hip_scenario_commit(self.h))

    def run_frames(self, f0, f1):
        _chk(self.L.msckf_hip_run_frames(self.h, f0, f1))

    def run_frames_streamed(self, f0, f1):
        """run_frames with per-frame asynchronous H2D of the inputs (copy stream, ring of staging sets, compact work-lists)"""
        _chk(self.L.msckf_hip_run_frames_streamed(self.h, f0, f1))

    # ---- Monte-Carlo replay: shared noise-free sequences, per-trajectory seeded noise added on the device
    def replay_alloc(self, n_seq, n_frames, K):
        """n_seq sequences of n_frames cells with up to K IMU samples each (replaces a previous replay)"""
        _chk(self.L.msckf_hip_replay_alloc(self.h, int(n_seq), int(n_frames), int(K)))
        self._replay_K, self._replay_frames = int(K), int(n_frames)

    def replay_set_cell(self, frame, seq, readings, M, slots, obs, n_drop, skip=False):
        """one (frame, sequence) cell, noise-free: the arguments and rules of scenario_set"""
        r, pr = _d(np.asarray(readings, dtype=np.float64).reshape(-1, 7)); Ma, pM = _i(M); s, ps = _i(slots); o, po = _d(obs)
        _chk(self.L.msckf_hip_replay_set_cell(self.h, int(frame), int(seq), pr, r.shape[0], len(Ma), pM, ps, po, int(n_drop), CELL_SKIP if skip else 0))

    def replay_assign(self, seq_of, seeds, sigma4):
        """per trajectory its sequence, its 64-bit seed and (sigma_g, sigma_a, sigma_u, sigma_v); sigma4 [4] serves every
        trajectory.  May be called again between runs."""
        q, pq = _i(seq_of)
        sd = np.ascontiguousarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64)
        sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma4, dtype=np.float64), (self.B, 4)))
        if q.shape != (self.B,) or sd.shape != (self.B,):
            raise ValueError("seq_of and seeds must hold one value per trajectory")
        _chk(self.L.msckf_hip_replay_assign(self.h, pq, sd.ctypes.data_as(_up), sg.ctypes.data_as(_dp)))

    def replay_assign_q(self, seq_of, seeds, Q, scale, sigma_uv):
        """per trajectory its sequence, its 64-bit seed and the Q_imu noise model (include/msckf_hip.h): Q [12][12] (the
        filter's Q_imu, noise order n_g n_wg n_a n_wa), scale (Trajectory's imu_noise_scale) and (sigma_u, sigma_v); one Q, scale
        or sigma pair serves every trajectory.  A later replay_assign returns to the sigma4 model."""
        q, pq = _i(seq_of)
        sd = np.ascontiguousarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], dtype=np.uint64)
        if q.shape != (self.B,) or sd.shape != (self.B,):
            raise ValueError("seq_of and seeds must hold one value per trajectory")
        Qa = np.broadcast_to(np.asarray(Q, dtype=np.float64), (self.B, 12, 12))
        Qc = np.ascontiguousarray(np.swapaxes(Qa, 1, 2))                 # column-major, per trajectory
        sc_ = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (self.B,)))
        uv = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_uv, dtype=np.float64), (self.B, 2)))
        _chk(self.L.msckf_hip_replay_assign_q(self.h, pq, sd.ctypes.data_as(_up), Qc.ctypes.data_as(_dp), sc_.ctypes.data_as(_dp), uv.ctypes.data_as(_dp)))

    def replay_walk(self, f0=0, f1=None, b0=0, nb=None):
        """the model's bias walk at the start of the frames [f0, f1) (default: all frames + 1 rows) for the trajectories
        [b0, b0 + nb): [f1 - f0][nb][6], gyro then accelerometer bias offset; row f + 1 belongs to frame f's log record"""
        f1 = self._replay_frames + 1 if f1 is None else int(f1)
        nb = self.B - int(b0) if nb is None else int(nb)
        out = np.zeros((max(f1 - int(f0), 0), max(nb, 0), 6))
        _chk(self.L.msckf_hip_replay_walk(self.h, int(f0), f1, int(b0), nb, out.ctypes.data_as(_dp)))
        return out

    def replay_commit(self):
        _chk(self.L.msckf_hip_replay_commit(self.h))

    def run_frames_replay(self, f0, f1):
        """run_frames over the replay's frames [f0, f1): each frame's inputs are expanded from the sequences on the device"""
        _chk(self.L.msckf_hip_run_frames_replay(self.h, int(f0), int(f1)))

    def replay_expand(self, frame, b):
        """what the expansion kernel writes for trajectory b on `frame` (a launch of the same kernel into scratch memory): dict of
        rd [K][7], obs [entries][2] (the handle's scalars as doubles), n, drop, k, M [f_cap], off [f_cap], slots [entries]"""
        cap = self.f_cap * self.m_cap
        rd = np.zeros((self._replay_K, 7)); obs = np.zeros((cap, 2)); ints = np.zeros(3 + 2 * self.f_cap, dtype=np.int32); slots = np.zeros(cap, dtype=np.int32)
        n = _chk(self.L.msckf_hip_replay_expand(self.h, int(frame), int(b), rd.ctypes.data_as(_dp), obs.ctypes.data_as(_dp), cap))
        _chk(self.L.msckf_hip_replay_expand_ints(self.h, int(frame), int(b), ints.ctypes.data_as(_ip), slots.ctypes.data_as(_ip), cap))
        return dict(rd=rd, obs=obs[:n], n=int(ints[0]), drop=int(ints[1]), k=int(ints[2]), M=ints[3:3 + self.f_cap].copy(),
                    off=ints[3 + self.f_cap:].copy(), slots=slots[:n])

    def replay_set_faults(self, fault4):
        """seeded missed observations and outliers (include/msckf_hip.h): per trajectory (p_miss, p_out, rho_u, rho_v), one row
        serves every trajectory; None: no faults.  Stays through replay_assign, replay_assign_q and replay_commit."""
        if fault4 is None:
            _chk(self.L.msckf_hip_replay_set_faults(self.h, None))
            return
        ft = np.ascontiguousarray(np.broadcast_to(np.asarray(fault4, dtype=np.float64), (self.B, 4)))
        _chk(self.L.msckf_hip_replay_set_faults(self.h, ft.ctypes.data_as(_dp)))

    def replay_expand_faults(self, frame, b):
        """per sequence entry of trajectory b's cell on `frame`: FAULT_KEPT, FAULT_OUTLIER or FAULT_MISSED"""
        cap = self.f_cap * self.m_cap
        code = np.zeros(cap, dtype=np.int32)
        n = _chk(self.L.msckf_hip_replay_expand_faults(self.h, int(frame), int(b), code.ctypes.data_as(_ip), cap))
        return code[:n]

    def replay_set_timing(self, timing4):
        """the camera's clock (include/msckf_hip.h): per trajectory (t_d, r_y, y_0, sigma_j) -- time offset [s], readout slope
        [s per unit of normalised image y], the row exposed at the stamp, timestamp jitter [s]; one row serves every trajectory;
        None: no timing.  Stays through replay_assign, replay_assign_q, replay_set_faults and replay_commit."""
        if timing4 is None:
            _chk(self.L.msckf_hip_replay_set_timing(self.h, None))
            return
        tm = np.ascontiguousarray(np.broadcast_to(np.asarray(timing4, dtype=np.float64), (self.B, 4)))
        _chk(self.L.msckf_hip_replay_set_timing(self.h, tm.ctypes.data_as(_dp)))

    def replay_image_table(self, seq):
        """sequence seq's image table as the last replay_commit built it: (time [images], frame_of [images], base [frames])"""
        time = np.zeros(self._replay_frames); frame_of = np.zeros(self._replay_frames, dtype=np.int32); base = np.zeros(self._replay_frames, dtype=np.int32)
        n = _chk(self.L.msckf_hip_replay_image_table(self.h, int(seq), time.ctypes.data_as(_dp), frame_of.ctypes.data_as(_ip), base.ctypes.data_as(_ip)))
        return time[:n], frame_of[:n], base

    def replay_expand_timing(self, frame, b):
        """per sequence entry of trajectory b's cell on `frame`: its delta in seconds, from the expansion's own launch"""
        cap = self.f_cap * self.m_cap
        delta = np.zeros(cap)
        n = _chk(self.L.msckf_hip_replay_expand_timing(self.h, int(frame), int(b), delta.ctypes.data_as(_dp), cap))
        return delta[:n]

    def replay_fault_counts(self, f0=0, f1=None):
        """the faults of the frames [f0, f1) (default: all) per trajectory, counted on the device: int64 [B][6], columns
        REPLAY_FAULT_COUNTS"""
        f1 = self._replay_frames if f1 is None else int(f1)
        out = np.zeros((self.B, 6), dtype=np.int64)
        _chk(self.L.msckf_hip_replay_fault_counts(self.h, int(f0), f1, out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def replay_imu_sums(self, f0=0, f1=None):
        """per trajectory the IMU samples a run over the frames [f0, f1) (default: all) would hand its propagate, summed on the
        device as the expansion stores them: [B][8], columns IMU_SUM_FIELDS (sums and counts: ranges add)"""
        f1 = self._replay_frames if f1 is None else int(f1)
        out = np.zeros((self.B, IMU_SUM_STRIDE))
        _chk(self.L.msckf_hip_replay_imu_sums(self.h, int(f0), f1, out.ctypes.data_as(_dp)))
        return out

    def replay_set_imu_calib(self, imucal):
        """IMU calibration errors (include/msckf_hip.h): per trajectory the record [31] = T_g (9, row-major), T_a (9), G (9), sat_g,
        sat_a, lsb_g, lsb_a (scenario.imu_calib_record builds one); one row serves every trajectory; None: no record.  Stays
        through replay_assign, replay_assign_q, replay_set_faults, replay_set_timing and replay_commit."""
        if imucal is None:
            _chk(self.L.msckf_hip_replay_set_imu_calib(self.h, None))
            return
        ic = np.ascontiguousarray(np.broadcast_to(np.asarray(imucal, dtype=np.float64), (self.B, 31)))
        _chk(self.L.msckf_hip_replay_set_imu_calib(self.h, ic.ctypes.data_as(_dp)))

    def replay_set_cam_calib(self, camcal):
        """camera calibration errors (include/msckf_hip.h): per trajectory (e_u, e_v, d_u, d_v, k1, k2, p1, p2), the residual map
        in normalised coordinates (scenario.cam_calib_record / cam_calib_from_intrinsics build one); one row serves every
        trajectory; None: no record.  Lifetime as replay_set_imu_calib's."""
        if camcal is None:
            _chk(self.L.msckf_hip_replay_set_cam_calib(self.h, None))
            return
        cc = np.ascontiguousarray(np.broadcast_to(np.asarray(camcal, dtype=np.float64), (self.B, 8)))
        _chk(self.L.msckf_hip_replay_set_cam_calib(self.h, cc.ctypes.data_as(_dp)))

    def replay_expand_calib(self, frame, b):
        """from the expansion's own launch for trajectory b on `frame`: dict of rd_cal [K][6] (the noise-free calibrated samples, in
        double), clip [K] (6-bit masks of clipped components), obs_cal [entries][2] (the mapped noise-free coordinates per
        sequence entry)"""
        cap = self.f_cap * self.m_cap
        rd_cal = np.zeros((self._replay_K, 6)); clip = np.zeros(self._replay_K, dtype=np.int32); obs_cal = np.zeros((cap, 2))
        n = _chk(self.L.msckf_hip_replay_expand_calib(self.h, int(frame), int(b), rd_cal.ctypes.data_as(_dp), clip.ctypes.data_as(_ip), obs_cal.ctypes.data_as(_dp), cap))
        return dict(rd_cal=rd_cal, clip=clip, obs_cal=obs_cal[:n])

    def replay_calib_counts(self, f0=0, f1=None):
        """the saturation of the frames [f0, f1) (default: all) per trajectory, counted on the device without a run: int64 [B][8] =
        samples, gyro x y z clipped, accelerometer x y z clipped, samples with any component clipped"""
        f1 = self._replay_frames if f1 is None else int(f1)
        out = np.zeros((self.B, 8), dtype=np.int64)
        _chk(self.L.msckf_hip_replay_calib_counts(self.h, int(f0), f1, out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def replay_standstill(self, f0, f1):
        """the stand-still initialisation of the no-ground-truth runner, per seed: every trajectory's IMU state is set from the
        means of its own noisy samples over the frames [f0, f1) (replay_imu_sums -> asl.standstill_state -> set_imu_state).
        Returns the states [B][29]; the caller then runs run_frames_replay(f1, ...)."""
        from . import asl
        sums = self.replay_imu_sums(f0, f1)
        if not np.all(sums[:, 0] > 0):
            raise ValueError("no IMU samples inside the stand-still interval")
        states = np.stack([asl.standstill_state(r[1:4] / r[0], r[4:7] / r[0]) for r in sums])
        for b in range(self.B):
            self.set_imu_state(b, states[b])
        return states

    def scenario_pin(self, f0, f1):
        """page-lock the per-frame blocks of frames [f0, f1) ahead of a streamed run (outside any timed region)"""
        _chk(self.L.msckf_hip_scenario_pin(self.h, int(f0), int(f1)))

    def set_upload_ring(self, depth=6, mode=0):
        """staging sets of run_frames_streamed (2..8); mode 0 host hand-over (default), 1 device-side event waits"""
        _chk(self.L.msckf_hip_set_upload_ring(self.h, int(depth), int(mode)))

    def clear_error_flags(self, b):
        """clears trajectory b's sticky flags (error_flags has the contract); a state the failure left undefined stays as it is"""
        _chk(self.L.msckf_hip_clear_error_flags(self.h, int(b)))

    def sync(self):
        _chk(self.L.msckf_hip_sync(self.h))

    def set_host_affinity(self, cpus):
        """cpus[0]: the calling thread while it uploads frames; cpus[1 + i]: enqueue thread of slice i"""
        a = np.ascontiguousarray(list(cpus), dtype=np.int32)
        _chk(self.L.msckf_hip_set_host_affinity(self.h, a.ctypes.data_as(_ip), int(a.size)))

    def set_streams(self, n):
        _chk(self.L.msckf_hip_set_streams(self.h, int(n)))

    def set_hw_queues(self, n):
        """hardware queues the runtime gives this process (GPU_MAX_HW_QUEUES when it started, 4 by default): 1..32"""
        _chk(self.L.msckf_hip_set_hw_queues(self.h, int(n)))

    def set_slices_exact(self, on):
        """run exactly set_streams' slices whatever the hardware queues (A/B runs)"""
        _chk(self.L.msckf_hip_set_slices_exact(self.h, 1 if on else 0))

    def effective_streams(self, streamed=False):
        """the slices run_frames (or, streamed, run_frames_streamed) runs now: set_streams' count is an upper bound that the
        handle sizes to the process's hardware queues (csrc/slice_policy.h)"""
        n = C.c_int(0)
        _chk(self.L.msckf_hip_get_effective_streams(self.h, 1 if streamed else 0, C.byref(n)))
        return int(n.value)

    def set_compression(self, route):
        """-1 default for the window size; 0 Householder TSQR; 3 information form chol(H_o^T H_o) with the blocked matrix-core
        Cholesky k_chol_mfma (the default where it fits; 1 and 2 named retired factorizations and mean 3)"""
        _chk(self.L.msckf_hip_set_compression(self.h, int(route)))

    def set_covariance_update(self, form):
        """0 square-root gain form P - W W^T with the blocked matrix-core solve (default), 1 the reference's Joseph sequence,
        2 square-root gain form with the register-resident solve"""
        _chk(self.L.msckf_hip_set_covariance_update(self.h, int(form)))

    def set_feature_overlap(self, on):
        _chk(self.L.msckf_hip_set_feature_overlap(self.h, 1 if on else 0))

    def set_frame_order(self, order):
        """run_frames: 1 (default) feature kernel first and selection beside propagate + augmentState in one launch on the
        frames that allow it, 0 propagate first on every frame; same bits either way."""
        _chk(self.L.msckf_hip_set_frame_order(self.h, int(order)))

    def set_frame_order_chol(self, on):
        """under order 1 (on by default): propagate + augmentState inside the Gram Cholesky's launch on the frames that allow it,
        the selection in a launch of its own -- "order 2"; off: order 1 as it is described above; same bits either way."""
        _chk(self.L.msckf_hip_set_frame_order_chol(self.h, 1 if on else 0))

    def frame_order_count(self):
        """frames (one count per slice and frame) that took order 1 since the handle was created"""
        n = C.c_longlong(0)
        _chk(self.L.msckf_hip_get_frame_order_count(self.h, C.byref(n)))
        return n.value

    def frame_order_chol_count(self):
        """those of frame_order_count's frames that took order 2"""
        n = C.c_longlong(0)
        _chk(self.L.msckf_hip_get_frame_order_chol_count(self.h, C.byref(n)))
        return n.value

    def set_gate_early_accept(self, on):
        _chk(self.L.msckf_hip_set_gate_early_accept(self.h, 1 if on else 0))

    def set_anisotropic_noise(self, mode, tail_tol=-1.0):
        """u_var' != v_var': 0 (default) the reference's R_o_j = A_j^T R_j A_j / HouseholderQR / R_n = Q_1^T R_o Q_1 on the
        device (msckf.h:423-431, 1343-1366), 1 rows pre-whitened by 1/sigma.  tail_tol < 0: default, 0: the reference's
        zero-tail rule to the letter"""
        _chk(self.L.msckf_hip_set_anisotropic_noise(self.h, int(mode), C.c_double(float(tail_tol))))

    def literal_info(self, b):
        o = np.zeros(8, dtype=np.int32)
        _chk(self.L.msckf_hip_literal_info(self.h, int(b), o.ctypes.data_as(_ip)))
        return dict(zip(["m_rows", "kept_rows", "reflected", "skipped_by_tolerance", "route", "leading_rows_handed_through", "kept_handed_through_rows", "spare"], o.tolist()))

    # ---- per-frame device log of run_frames / run_frames_streamed
    def frame_log_enable(self, capacity_frames):
        """storage for capacity_frames records per trajectory (0: free the log and switch it off); drops the records written"""
        _chk(self.L.msckf_hip_frame_log_enable(self.h, int(capacity_frames)))

    def frame_log_reset(self):
        _chk(self.L.msckf_hip_frame_log_reset(self.h))

    def frame_log_count(self):
        return _chk(self.L.msckf_hip_frame_log_count(self.h))

    def frame_log_read(self, r0=0, n=None, b0=0, nb=None):
        """records [r0, r0 + n) (default: all written) of trajectories [b0, b0 + nb) (default: all): the array [n][nb][48] and
        a dict of views into it by field name (FRAME_LOG_FIELDS)"""
        n = self.frame_log_count() - r0 if n is None else int(n)
        nb = self.B - b0 if nb is None else int(nb)
        o = np.zeros((max(n, 0), max(nb, 0), FRAME_LOG_STRIDE))
        _chk(self.L.msckf_hip_frame_log_read(self.h, int(r0), n, int(b0), nb, o.ctypes.data_as(_dp)))
        return o, {k: o[:, :, s] for k, s in FRAME_LOG_FIELDS.items()}

    def frame_log_metrics(self, r0, r1, gt_p):
        """records [r0, r1) against ground-truth positions gt_p [r1 - r0][B][3], reduced on the device: [B][6], columns
        FRAME_LOG_METRICS (sums and counts: shard.ate_from_log_metrics turns them into ate_allreduce's accumulator)"""
        g = np.ascontiguousarray(gt_p, dtype=np.float64)
        if g.shape != (int(r1) - int(r0), self.B, 3):
            raise ValueError("gt_p must be [r1 - r0][B][3]")
        o = np.zeros((self.B, 6))
        _chk(self.L.msckf_hip_frame_log_metrics(self.h, int(r0), int(r1), g.ctypes.data_as(_dp), o.ctypes.data_as(_dp)))
        return o

    def frame_log_metrics_ranges(self, r0, r1, gt_p):
        """frame_log_metrics with a record range [r0[b], r1[b]) per trajectory (sequences of unequal length: r1[b] = the
        sequence's frame count); gt_p [max(r1) - min(r0)][B][3], indexed from min(r0)"""
        a0, p0 = _i(r0); a1, p1 = _i(r1)
        if a0.shape != (self.B,) or a1.shape != (self.B,):
            raise ValueError("r0 and r1 must hold one record index per trajectory")
        g = np.ascontiguousarray(gt_p, dtype=np.float64)
        if g.shape != (int(a1.max()) - int(a0.min()), self.B, 3):
            raise ValueError("gt_p must be [max(r1) - min(r0)][B][3]")
        o = np.zeros((self.B, 6))
        _chk(self.L.msckf_hip_frame_log_metrics_ranges(self.h, p0, p1, g.ctypes.data_as(_dp), o.ctypes.data_as(_dp)))
        return o

    # ---- the cursor logs' counts and read, stated once: prefix "map" or "pruned", the record's stride
    def _cursor_log_counts(self, prefix, b0, nb):
        nb = self.B - b0 if nb is None else int(nb)
        s = np.zeros(max(nb, 0), dtype=np.int32); f = np.zeros(max(nb, 0), dtype=np.int32)
        _chk(getattr(self.L, "msckf_hip_%s_log_counts" % prefix)(self.h, int(b0), nb, s.ctypes.data_as(_ip), f.ctypes.data_as(_ip)))
        return s, f

    def _cursor_log_read(self, prefix, stride, b, r0, n, aug=False):
        """([n][stride], augment ordinals [n] or None) of the stored records [r0, r0 + n) (default: all behind r0) of trajectory b"""
        n = int(self._cursor_log_counts(prefix, b, 1)[0][0]) - r0 if n is None else int(n)
        o = np.zeros((max(n, 0), stride)); a = np.full(max(n, 1), -1, dtype=np.int32) if aug else None
        _chk(getattr(self.L, "msckf_hip_%s_log_read" % prefix)(self.h, int(b), int(r0), n, o.ctypes.data_as(_dp), *([a.ctypes.data_as(_ip)] if aug else [])))
        return o, a

    # ---- per-track device log of run_frames / run_frames_streamed: the landmark map
    def map_log_enable(self, capacity_per_trajectory):
        """storage for capacity_per_trajectory records per trajectory (0: free the log and switch it off); drops the records held"""
        _chk(self.L.msckf_hip_map_log_enable(self.h, int(capacity_per_trajectory)))

    def map_log_reset(self):
        _chk(self.L.msckf_hip_map_log_reset(self.h))

    def map_log_frames(self):
        return _chk(self.L.msckf_hip_map_log_frames(self.h))

    def map_log_counts(self, b0=0, nb=None):
        """(stored, found) of trajectories [b0, b0 + nb) (default: all); found > stored: the trajectory's log overflowed"""
        return self._cursor_log_counts("map", b0, nb)

    def map_log_read(self, b, r0=0, n=None):
        """stored records [r0, r0 + n) (default: all behind r0) of trajectory b: the array [n][8] and a dict of views into it by
        field name (MAP_LOG_FIELDS)"""
        o = self._cursor_log_read("map", MAP_LOG_STRIDE, b, r0, n)[0]
        return o, {k: o[:, s] for k, s in MAP_LOG_FIELDS.items()}

    def map_log_metrics(self, q0, q1, gt=None):
        """the stored records with frame ordinal in [q0, q1), reduced on the device: [B][8], columns MAP_LOG_METRICS (sums and
        counts).  gt: (gt_xyz [.][3], gt_off [(q1 - q0) * B + 1]) as scenario.landmark_csr builds them, or None"""
        o = np.zeros((self.B, 8))
        if gt is None:
            _chk(self.L.msckf_hip_map_log_metrics(self.h, int(q0), int(q1), None, None, o.ctypes.data_as(_dp)))
            return o
        g = np.ascontiguousarray(gt[0], dtype=np.float64).reshape(-1, 3)
        off, po = _i(gt[1])
        if off.shape != ((int(q1) - int(q0)) * self.B + 1,) or (off.size and int(off[-1]) > len(g)):
            raise ValueError("gt_off must hold (q1 - q0) * B + 1 offsets into gt_xyz")
        _chk(self.L.msckf_hip_map_log_metrics(self.h, int(q0), int(q1), g.ctypes.data_as(_dp), po, o.ctypes.data_as(_dp)))
        return o

    def map_log_fault_metrics(self, q0, q1, f0):
        """the stored records with frame ordinal in [q0, q1) -- written by run_frames_replay contiguously from replay frame f0 --
        against the faults of their tracks, reduced on the device: [B][8], columns MAP_LOG_FAULT_METRICS"""
        o = np.zeros((self.B, 8))
        _chk(self.L.msckf_hip_map_log_fault_metrics(self.h, int(q0), int(q1), int(f0), o.ctypes.data_as(_dp)))
        return o

    # ---- pruned-state device log of run_frames / run_frames_streamed: the smoothed camera poses
    def pruned_log_enable(self, capacity_per_trajectory):
        """storage for capacity_per_trajectory records per trajectory (0: free the log, switch it off and give the prune on the
        downdate back); drops the records held"""
        _chk(self.L.msckf_hip_pruned_log_enable(self.h, int(capacity_per_trajectory)))

    def pruned_log_reset(self):
        _chk(self.L.msckf_hip_pruned_log_reset(self.h))

    def pruned_log_frames(self):
        return _chk(self.L.msckf_hip_pruned_log_frames(self.h))

    def pruned_log_counts(self, b0=0, nb=None):
        """(stored, found) of trajectories [b0, b0 + nb) (default: all); found > stored: the trajectory's log overflowed"""
        return self._cursor_log_counts("pruned", b0, nb)

    def pruned_log_read(self, b, r0=0, n=None):
        """stored records [r0, r0 + n) (default: all behind r0) of trajectory b: the array [n][32], a dict of views into it by
        field name (PRUNED_LOG_FIELDS) and the records' augment ordinals [n] (-1: the state's image is not known)"""
        o, a = self._cursor_log_read("pruned", PRUNED_LOG_STRIDE, b, r0, n, aug=True)
        return o, {k: o[:, s] for k, s in PRUNED_LOG_FIELDS.items()}, a[:o.shape[0]]

    def pruned_log_metrics(self, q0, q1, gt_pose=None):
        """the stored records with prune ordinal in [q0, q1) against ground-truth camera poses gt_pose [n_ord][B][7] (q_CG p_C_G
        of the camera of frame ordinal o; None: none, every record unmatched), reduced on the device: [B][10], columns
        PRUNED_LOG_METRICS (sums and counts: shard.ate_from_pruned_metrics turns them into ate_allreduce's accumulator)"""
        o = np.zeros((self.B, 10))
        if gt_pose is None:
            _chk(self.L.msckf_hip_pruned_log_metrics(self.h, int(q0), int(q1), None, 0, o.ctypes.data_as(_dp)))
            return o
        g = np.ascontiguousarray(gt_pose, dtype=np.float64)
        if g.ndim != 3 or g.shape[1:] != (self.B, 7):
            raise ValueError("gt_pose must be [n_ord][B][7]")
        _chk(self.L.msckf_hip_pruned_log_metrics(self.h, int(q0), int(q1), g.ctypes.data_as(_dp), int(g.shape[0]), o.ctypes.data_as(_dp)))
        return o

    # ---- aligned trajectory error on the device: yaw and SE(3) ATE, and the relative pose error
    def _traj_ranges(self, r0b, r1b, n_traj):
        """(keep-alive, pointer, pointer) of the per-trajectory ranges, or nulls when neither is given"""
        if r0b is None and r1b is None:
            return None, None, None
        if r0b is None or r1b is None:
            raise ValueError("r0b and r1b: both or neither")
        a0, p0 = _i(r0b); a1, p1 = _i(r1b)
        if a0.shape != (n_traj,) or a1.shape != (n_traj,):
            raise ValueError("r0b and r1b must hold one record index per trajectory")
        return (a0, a1), p0, p1

    @staticmethod
    def _traj_lags(lags):
        a, p = _i(np.atleast_1d(lags))
        if a.ndim != 1:
            raise ValueError("lags must be a list of record counts")
        return a, p

    def frame_log_align(self, r0, r1, gt_pose7, mode, r0b=None, r1b=None):
        """the frame log's records [r0, r1) against ground-truth poses gt_pose7 [r1 - r0][B][7] (trajeval.gt_pose7), after the
        alignment `mode` (ALIGN_NONE, ALIGN_YAW, ALIGN_SE3) of each trajectory, reduced on the device: [B][20], columns
        ALIGN_FIELDS (sums and counts).  r0b / r1b: a record range per trajectory inside [r0, r1)"""
        g = np.ascontiguousarray(gt_pose7, dtype=np.float64)
        if g.shape != (int(r1) - int(r0), self.B, 7):
            raise ValueError("gt_pose7 must be [r1 - r0][B][7]")
        keep, p0, p1 = self._traj_ranges(r0b, r1b, self.B)
        o = np.zeros((self.B, ALIGN_STRIDE))
        _chk(self.L.msckf_hip_frame_log_align(self.h, int(r0), int(r1), p0, p1, g.ctypes.data_as(_dp), int(mode), o.ctypes.data_as(_dp)))
        return o

    def frame_log_rpe(self, r0, r1, gt_pose7, lags, r0b=None, r1b=None):
        """the relative pose error of the frame log's records [r0, r1) over `lags` (at most RPE_MAX_LAGS, in records), reduced on
        the device: [B][len(lags)][4], columns RPE_FIELDS (sums and counts)"""
        g = np.ascontiguousarray(gt_pose7, dtype=np.float64)
        if g.shape != (int(r1) - int(r0), self.B, 7):
            raise ValueError("gt_pose7 must be [r1 - r0][B][7]")
        keep, p0, p1 = self._traj_ranges(r0b, r1b, self.B)
        la, pl = self._traj_lags(lags)
        o = np.zeros((self.B, max(len(la), 1), RPE_STRIDE))
        _chk(self.L.msckf_hip_frame_log_rpe(self.h, int(r0), int(r1), p0, p1, g.ctypes.data_as(_dp), pl, len(la), o.ctypes.data_as(_dp)))
        return o[:, :len(la)]

    @staticmethod
    def _traj_poses(est_pose7, gt_pose7):
        e = np.ascontiguousarray(est_pose7, dtype=np.float64); g = np.ascontiguousarray(gt_pose7, dtype=np.float64)
        if e.ndim != 3 or e.shape[1] < 1 or e.shape[2] != 7 or g.shape != e.shape:
            raise ValueError("est_pose7 and gt_pose7 must both be [n_rec][n_traj][7]")
        return e, g

    def traj_align(self, est_pose7, gt_pose7, mode, r0b=None, r1b=None):
        """frame_log_align on poses the caller hands over, est_pose7 and gt_pose7 [n_rec][n_traj][7] (q w x y z, then p; n_traj is
        free of B): [n_traj][20], columns ALIGN_FIELDS"""
        e, g = self._traj_poses(est_pose7, gt_pose7)
        keep, p0, p1 = self._traj_ranges(r0b, r1b, e.shape[1])
        o = np.zeros((e.shape[1], ALIGN_STRIDE))
        _chk(self.L.msckf_hip_traj_align(self.h, e.shape[0], e.shape[1], e.ctypes.data_as(_dp), g.ctypes.data_as(_dp), p0, p1, int(mode), o.ctypes.data_as(_dp)))
        return o

    def traj_rpe(self, est_pose7, gt_pose7, lags, r0b=None, r1b=None):
        """frame_log_rpe on poses the caller hands over: [n_traj][len(lags)][4], columns RPE_FIELDS"""
        e, g = self._traj_poses(est_pose7, gt_pose7)
        keep, p0, p1 = self._traj_ranges(r0b, r1b, e.shape[1])
        la, pl = self._traj_lags(lags)
        o = np.zeros((e.shape[1], max(len(la), 1), RPE_STRIDE))
        _chk(self.L.msckf_hip_traj_rpe(self.h, e.shape[0], e.shape[1], e.ctypes.data_as(_dp), g.ctypes.data_as(_dp), p0, p1, pl, len(la), o.ctypes.data_as(_dp)))
        return o[:, :len(la)]

    # ---- full-state NEES log of the frame loops, and its reduction per frame across trajectories
    def truth_set(self, truth16, row_of=None, add_walk=False):
        """the truth the NEES log is taken against: truth16 [n_frames][n_rows][16] (scenario.imu_state_gt), row_of [B] each
        trajectory's row (default: itself), add_walk: row f + 1 of the replay's walk table is added to the true biases of frame
        f (run_frames_replay under replay_assign_q only).  None frees the table."""
        if truth16 is None:
            _chk(self.L.msckf_hip_truth_set(self.h, 0, 0, None, None, 0))
            return
        t = np.ascontiguousarray(truth16, dtype=np.float64)
        if t.ndim != 3 or t.shape[2] != 16:
            raise ValueError("truth16 must be [n_frames][n_rows][16]")
        r, pr = _i(np.arange(self.B) if row_of is None else row_of)
        if r.shape != (self.B,):
            raise ValueError("row_of must hold one row per trajectory")
        _chk(self.L.msckf_hip_truth_set(self.h, int(t.shape[0]), int(t.shape[1]), t.ctypes.data_as(_dp), pr, 1 if add_walk else 0))

    def nees_log_enable(self, capacity_frames):
        """storage for capacity_frames records per trajectory (0: free the log and switch it off); drops the records written"""
        _chk(self.L.msckf_hip_nees_log_enable(self.h, int(capacity_frames)))

    def nees_log_reset(self):
        _chk(self.L.msckf_hip_nees_log_reset(self.h))

    def nees_log_count(self):
        return _chk(self.L.msckf_hip_nees_log_count(self.h))

    def nees_log_read(self, r0=0, n=None, b0=0, nb=None):
        """records [r0, r0 + n) (default: all written) of trajectories [b0, b0 + nb) (default: all): the array [n][nb][8] and
        a dict of views into it by field name (NEES_LOG_FIELDS)"""
        n = self.nees_log_count() - r0 if n is None else int(n)
        nb = self.B - b0 if nb is None else int(nb)
        o = np.zeros((max(n, 0), max(nb, 0), NEES_LOG_STRIDE))
        _chk(self.L.msckf_hip_nees_log_read(self.h, int(r0), n, int(b0), nb, o.ctypes.data_as(_dp)))
        return o, {k: o[:, :, s] for k, s in NEES_LOG_FIELDS.items()}

    def nees_log_ensemble(self, r0, r1, group_of, n_groups):
        """records [r0, r1) reduced on the device over the groups group_of [B] (-1: left out): (sums [r1 - r0][n_groups][14],
        columns NEES_ENSEMBLE_FIELDS -- sums and counts, ranks combine by addition -- and the ANEES curves [r1 - r0][n_groups][6]
        = sum / n over the unflagged members, NaN for a group without one)"""
        g, pg = _i(group_of)
        if g.shape != (self.B,):
            raise ValueError("group_of must hold one group per trajectory")
        o = np.zeros((max(int(r1) - int(r0), 0), max(int(n_groups), 0), NEES_ENSEMBLE_STRIDE))
        _chk(self.L.msckf_hip_nees_log_ensemble(self.h, int(r0), int(r1), pg, int(n_groups), o.ctypes.data_as(_dp)))
        with np.errstate(invalid="ignore", divide="ignore"):
            anees = np.where(o[:, :, 0:1] > 0, o[:, :, 2:8] / o[:, :, 0:1], np.nan)
        return o, anees

    def profile_enable(self, on=True):
        _chk(self.L.msckf_hip_profile_enable(self.h, 1 if on else 0))

    def profile_event_overhead(self):
        ms = C.c_double(0.0)
        _chk(self.L.msckf_hip_profile_event_overhead(self.h, C.byref(ms)))
        return float(ms.value)

    def profile_read(self):
        ms = np.zeros(16); cnt = np.zeros(16, dtype=np.int32)
        _chk(self.L.msckf_hip_profile_read_ex(self.h, ms.ctypes.data_as(_dp), cnt.ctypes.data_as(_ip), 16))
        names = ["propagate", "augment", "feature", "compress_stage1", "compress_merge", "kalman", "prune", "select", "lit_pre", "lit_gamma", "literal", "replay_expand", "replay_walk_scan"]
        return {n: (float(m), int(c)) for n, m, c in zip(names, ms, cnt)}


class TrackCompiler:
    """A recorded feature-id stream compiled into the cells of the frame loops (csrc/track_compile.h): host code alone, no GPU.
    One image at a time, in the order of the recording; `image` returns the cell the frame loop takes for it."""

    def __init__(self, max_cam_states, min_track_length, max_track_length):
        self.L = lib()
        self.c = C.c_void_p()
        _chk(self.L.msckf_hip_compile_create(int(max_cam_states), int(min_track_length), int(max_track_length), C.byref(self.c)))

    def close(self):
        if self.c:
            self.L.msckf_hip_compile_destroy(self.c)
            self.c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def image(self, cur, new):
        """cur / new = (measurements [n][2], feature ids [n]) as update() / addFeatures() take them.  Returns the image's cell:
        dict of M [F], slots [sum M], obs [sum M][2], ids [F] (the tracks' feature ids, in work-list order), n_drop, window
        (camera states after the augment, before the drop) and live (tracks still followed)"""
        um, pum = _d(np.asarray(cur[0], dtype=np.float64).reshape(-1, 2)); ui = np.ascontiguousarray(cur[1], dtype=np.uint64).reshape(-1)
        nm, pnm = _d(np.asarray(new[0], dtype=np.float64).reshape(-1, 2)); ni = np.ascontiguousarray(new[1], dtype=np.uint64).reshape(-1)
        if len(um) != len(ui) or len(nm) != len(ni):
            raise ValueError("one measurement per feature id")
        o5 = np.zeros(5, dtype=np.int32)
        _chk(self.L.msckf_hip_compile_image(self.c, pum, ui.ctypes.data_as(_up), len(ui), pnm, ni.ctypes.data_as(_up), len(ni), o5.ctypes.data_as(_ip)))
        F, E = int(o5[0]), int(o5[1])
        M = np.zeros(max(F, 1), dtype=np.int32); ids = np.zeros(max(F, 1), dtype=np.uint64)
        slots = np.zeros(max(E, 1), dtype=np.int32); obs = np.zeros((max(E, 1), 2))
        n = _chk(self.L.msckf_hip_compile_cell(self.c, M.ctypes.data_as(_ip), slots.ctypes.data_as(_ip), obs.ctypes.data_as(_dp), ids.ctypes.data_as(_up), F, E))
        assert n == F
        return dict(M=M[:F], slots=slots[:E], obs=obs[:E], ids=ids[:F], n_drop=int(o5[2]), window=int(o5[3]), live=int(o5[4]))


class MSCKF:
    """Host-side mirror of `msckf_mono::MSCKF<_S>` (msckf.h:66-848) over the C-ABI: same member names and
    call order as the reference so that the parity tests read like code written against the reference."""

    def __init__(self, dtype=F32, n_cap=32, f_cap=256, m_cap=32, device=0):
        self.batch = Batch(1, n_cap, f_cap, m_cap, dtype, device)
        self._device = device

    def copy(self):
        """value semantics of the reference object (msckf.h:31-67): a new filter with this one's state (msckf_hip_copy_state)"""
        c = MSCKF(self.batch.dtype, self.batch.n_cap, self.batch.f_cap, self.batch.m_cap, self._device)
        c.batch.copy_state_from(self.batch)
        return c

    def initialize(self, cfg, imu29):
        self.batch.initialize(0, cfg, imu29)

    def propagate(self, reading):
        self.batch.propagate(0, reading)

    def augmentState(self, state_id, time=0.0):
        self.batch.augment_state(0, state_id, time)

    def update(self, measurements, feature_ids):
        self.batch.update(0, measurements, feature_ids)

    def addFeatures(self, features, feature_ids):
        self.batch.add_features(0, features, feature_ids)

    def marginalize(self):
        self.batch.marginalize(0)

    def pruneRedundantStates(self):
        self.batch.prune_redundant_states(0)

    def sync(self):
        self.batch.sync()

    def pruneEmptyStates(self):
        self.batch.prune_empty_states(0)

    def finish(self):
        self.batch.finish(0)

    def getNumCamStates(self):
        return self.batch.num_cam_states(0)

    def getImuState(self):
        return self.batch.imu_state(0)

    def getCamStates(self):
        return self.batch.cam_states(0)

    def getMap(self):
        return self.batch.get_map(0)

    def getPrunedStates(self):
        return self.batch.pruned_state_ids(0)

    def getPrunedStatesFull(self):
        return self.batch.pruned_states(0)

    def getCamMeta(self):
        return self.batch.cam_meta(0)

    def getCovariance(self):
        return self.batch.covariance(0)
